// Splitter kernels, part 7 of 9: the Rabin-Karp batch kernel.
// The bit-reversed tables, the two-chain walk (rk_step64, rk_walk; cand_scan_rk_kernel of
// kcdc_split_long.h walks its segments with the same rk_walk) and split_batch_rk_kernel with its
// own copy of the visit protocol.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_feed.h"
#include "kcdc_split_queue.h"
#include "kcdc_split_visit.h"

namespace kcdc {
namespace dev {

// ================================================= Rabin-Karp pipelined kernel
// rabinkarp64 (splitter_rabinkarp64.go:26-67, rollinghash Roll):
//   u = v ^ out[leave];  v = (u << 8 | enter) ^ mod[u >> 45]
// Per byte the chain waits on one table read indexed by the hash itself (mod[]), so one
// chain per lane is LDS-latency bound (round 1: 4.07 ms on config 2).  Here each lane runs
// TWO independent chains, A over the first half of its lane segment and B over the second,
// interleaved byte by byte so two mod[] reads are in flight per lane (four per SIMD).
//
// Feeding keeps whole 128-byte lines (64-byte runs cap the DMA at 4.4 vs 6.6 TB/s,
// tools/membench.hip rk): the wave's one 8 KiB step slot receives, per lane, a line of
// chain A and a line of chain B alternately; a chain consumes 64 bytes per step, the
// first half of its line when it arrives and the second half (kept in VGPRs) one step
// later.  A tile (64 lanes x L bytes, L a multiple of 256) is:
//   W     the warm fill [A: 64 B before its half | B: 64 B before its half] (both chains
//         warm from a zero history);
//   2K    line fills (A line 0, B line 0, A line 1, ...), K = L/256 lines per chain;
//   D     drain: B's last 64 bytes (no fill: the slot takes the next tile's warm fill, or
//         the next stream's queue entry).
// (Round 3 tried two bytes per chain hop -- v2 = (v << 16 | c1 c2) ^ T_lo[b] ^ T_hi[a] ^ O16[l1] ^
// outx[l2], GF(2)-linear -- with conflict-free rotated tables: one LDS round trip per two bytes but
// 10.8 VALU per byte instead of 8.9, 2.94-2.97 vs 2.51-2.54 ms on config 2)
// Tables (96 KiB, conflict-free or nearly): out[] with 32 replicas at a 256-byte stride
// (lane l reads replica l % 32, bank pair 2(l % 32); address = one v_perm of the leaving
// byte), mod[] with 16 replicas at a 128-byte stride (lanes l and l+16 share a bank pair
// only for indices of equal parity).  8 waves x 8 KiB slots + 96 KiB = 160 KiB.
//
// Bit-reversed state (round 3).  The hash v (53 bits, deg P = 53) is kept as R = bitreverse64(v)
// in (hi, lo): v's bit j is R's bit 63 - j, so v's low bits -- the ones the cut test reads -- are
// the TOP bits of hi, and `(v & mask) == 0` is `hi < 2^(32 - log2(avg))`: the running test is one
// v_min3 per two bytes instead of a v_and + v_min per byte.  A roll v << 8 | c is R >> 8 with the
// bit-reversed entering byte on top: hi' = one v_perm of hi and the byte (the input dwords are
// bit-reversed once as they leave the step slot, so byte b of w sits bit-reversed in byte 3 - b),
// lo' = one v_alignbit.  The reduction index (v's bits 45..52) is lo's bits 11..18, bit-reversed:
// the tables are stored bit-reversed at bit-reversed rows.  8.9 -> ~7.9 VALU per byte.
// mod[] replicas: 16 = 2-way conflicts and a perm-addressed out[] (32 = conflict-free mod[] but a
// 2-op out[] address: 3.01 vs 2.80 ms on config 2, issue-bound); out[] gets the rest of 96 KiB.
constexpr int kRkModRep = 16;
constexpr int kRkOutRep = 48 - kRkModRep;
struct RkTables {
    uint64_t mod[256 * kRkModRep];  // row f (replicas at f*R + r): rev64(mod[rev8(f)]); first, so its
                                                    // addresses fit the 16-bit ds offset
    uint64_t out[256 * kRkOutRep];  // row f: rev64(outx[rev8(f)]) (outx[] pre-shifted and pre-reduced)
};
static_assert(sizeof(RkTables) + sizeof(RkSlots) <= 160 * 1024, "Rabin-Karp tables + step slots exceed LDS");
constexpr uint32_t kRkIdxBit = 11;  // the reduction index (v >> 45, bit-reversed) = lo bits 11..18

struct RkCtx {
    const char* modb;  // LDS byte address of RkTables::mod
    const char* outb;  // LDS byte address of RkTables::out
    uint32_t lane8o;   // (lane % out replicas) * 8
    uint32_t lane8m;   // (lane % mod replicas) * 8
    uint32_t thr;      // 2^(32 - log2(avg)): a position is a candidate iff hi < thr
};

// The RK kernels' view of a step slot: read_step128, then every dword bit-reversed.
__device__ __forceinline__ void rk_read_step128(const uint8_t* slot, int lane, int64_t c, int64_t off0,
                                                uint32_t (&dw)[32]) {
    read_step128(slot, lane, c, off0, dw);
#pragma unroll
    for (int i = 0; i < 32; i++) dw[i] = __builtin_bitreverse32(dw[i]);
}

// outx[] of the leaving byte b of a (bit-reversed) dword: its row is byte 3 - b.
__device__ __forceinline__ uint64_t rk_out(const RkCtx& k, uint32_t w, int b) {
    const int bb = 3 - b;
    uint32_t a;
    static_assert(kRkOutRep * 8 == 256, "out[]: 256-byte rows, the address in one v_perm");
    a = __builtin_amdgcn_perm(w, k.lane8o, 0x0c0c0000u | ((4u + bb) << 8));  // row << 8 | lane8o
    return *reinterpret_cast<const uint64_t*>(k.outb + a);
}
// v << 8 | c, high word: [hi.b1, hi.b2, hi.b3, the entering byte (byte 3 - b of the reversed dword)]
constexpr uint32_t rk_in_sel(int b) { return 0x00030201u | (static_cast<uint32_t>(7 - b) << 24); }
// mod[] address (16 replicas, 128-byte rows): ((lo >> 4) & 0x7F80) | lane8m as v_lshrrev + one
// v_bitop3 -- both issue every ~2.2-2.4 cycles at two waves per SIMD, where the v_bfe/v_lshl_or or
// v_and_or pairs the compiler picks take ~4.3 each (tools/valu_rate.hip; round 6: the hot loop
// alone 1.728 -> 1.586 ms, tools/rk_loop.hip).
__device__ __forceinline__ uint32_t rk_mod_addr(const RkCtx& k, uint32_t lo) {
    static_assert(kRkModRep == 16, "128-byte mod[] rows");
    return __builtin_amdgcn_bitop3_b32(lo >> (kRkIdxBit - 7), 0xFFu << 7, k.lane8m, 0xEA);  // (x & m) | lane8m
}
// out[] address of the leaving byte b of a (bit-reversed) dword, as rk_out, by one SDWA v_mov that
// writes the byte into byte 1 of `a` and keeps the rest: `a` holds lane8o in byte 0 for good.
__device__ __forceinline__ uint32_t rk_out_sdwa(uint32_t& a, uint32_t w, int b) {
    const int pos = 3 - b;
    if (pos == 0) asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0" : "+v"(a) : "v"(w));
    else if (pos == 1) asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1" : "+v"(a) : "v"(w));
    else if (pos == 2) asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2" : "+v"(a) : "v"(w));
    else asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3" : "+v"(a) : "v"(w));
    return a;
}
// One roll with the leaving byte's out[] value already read: updates (hi, lo).
// Linearity folds the leaving byte's removal into one table read that is off the chain:
// mod[] is GF(2)-linear in its index and idx(v ^ o) = idx(v) ^ idx(o), so
//   ((v ^ o) << 8 | c) ^ mod[idx(v ^ o)] = ((v << 8) | c) ^ mod[idx(v)] ^ outx[l],
//   outx[l] = (out[l] << 8) ^ mod[idx(out[l])]   (bits 53..60 cancel on both sides).
// The chain is lo -> address (2 VALU) -> mod[] read -> one v_bitop3.
__device__ __forceinline__ void rk_roll(const RkCtx& k, uint32_t& hi, uint32_t& lo, uint64_t ox, uint32_t w, int b) {
    const uint64_t m = *reinterpret_cast<const uint64_t*>(k.modb + rk_mod_addr(k, lo));
    const uint32_t th = __builtin_amdgcn_perm(w, hi, rk_in_sel(b));
    const uint32_t tl = __builtin_amdgcn_alignbit(hi, lo, 8);
    hi = __builtin_amdgcn_bitop3_b32(th, static_cast<uint32_t>(m >> 32), static_cast<uint32_t>(ox >> 32), 0x96);
    lo = __builtin_amdgcn_bitop3_b32(tl, static_cast<uint32_t>(m), static_cast<uint32_t>(ox), 0x96);
}
// Warm roll (leaving byte 0: out[0] = 0).
__device__ __forceinline__ void rk_roll0(const RkCtx& k, uint32_t& hi, uint32_t& lo, uint32_t w, int b) {
    const uint64_t m = *reinterpret_cast<const uint64_t*>(k.modb + rk_mod_addr(k, lo));
    const uint32_t th = __builtin_amdgcn_perm(w, hi, rk_in_sel(b));
    const uint32_t tl = __builtin_amdgcn_alignbit(hi, lo, 8);
    hi = th ^ static_cast<uint32_t>(m >> 32);
    lo = tl ^ static_cast<uint32_t>(m);
}

// 64 bytes of chain A (in a / leaving pa) and of chain B (in b / leaving pb), interleaved
// byte by byte; ma/mb: running min of hi over the piece's positions (a candidate iff < thr).
// Software-pipelined across the chains: a chain's next mod[] read issues right after its own
// roll, so it is in flight while the other chain rolls (one LDS latency + one roll per byte,
// not one latency + two rolls).  The outx[] reads of byte x + W follow each chain's mod[] read
// (the in-order LDS return then never queues a chain's read behind a prefetch).
// ACT_A/ACT_B: whether that chain's bytes are real (an idle chain is not rolled at all).
template <bool ACT_A, bool ACT_B>
__device__ __forceinline__ void rk_step64(const RkCtx& k, uint32_t& ha, uint32_t& la, const uint32_t (&a)[16],
                                          const uint32_t (&pa)[16], uint32_t& hb, uint32_t& lb,
                                          const uint32_t (&b)[16], const uint32_t (&pb)[16], uint32_t& ma,
                                          uint32_t& mb) {
    constexpr int W = 2;  // outx[] reads of both chains issued this many bytes ahead (2: 2.58 ms, 4: 2.65)
    uint64_t oa[64], ob[64];  // only W live at a time (unrolled: register renaming)
    uint32_t xa[W], xb[W];    // out[] address registers (rk_out_sdwa), one per read in flight
#pragma unroll
    for (int i = 0; i < W; i++) xa[i] = xb[i] = k.lane8o;
    auto ld_out = [&](uint32_t& x, uint32_t w, int b) {
        return *reinterpret_cast<const uint64_t*>(k.outb + rk_out_sdwa(x, w, b));
    };
    uint64_t mA = 0, mB = 0;
    if (ACT_A) mA = *reinterpret_cast<const uint64_t*>(k.modb + rk_mod_addr(k, la));
#pragma unroll
    for (int i = 0; i < W; i++)
        if (ACT_A) oa[i] = ld_out(xa[i], pa[i >> 2], i & 3);
    if (ACT_B) mB = *reinterpret_cast<const uint64_t*>(k.modb + rk_mod_addr(k, lb));
#pragma unroll
    for (int i = 0; i < W; i++)
        if (ACT_B) ob[i] = ld_out(xb[i], pb[i >> 2], i & 3);
    uint32_t pha = 0xFFFFFFFFu, phb = 0xFFFFFFFFu;  // the previous byte's hi (tested in pairs)
#pragma unroll
    for (int x = 0; x < 64; x++) {
        __builtin_amdgcn_sched_barrier(0);
        if (ACT_A) {
            const uint32_t th = __builtin_amdgcn_perm(a[x >> 2], ha, rk_in_sel(x & 3));
            const uint32_t tl = __builtin_amdgcn_alignbit(ha, la, 8);
            ha = __builtin_amdgcn_bitop3_b32(th, static_cast<uint32_t>(mA >> 32), static_cast<uint32_t>(oa[x] >> 32), 0x96);
            la = __builtin_amdgcn_bitop3_b32(tl, static_cast<uint32_t>(mA), static_cast<uint32_t>(oa[x]), 0x96);
            __builtin_amdgcn_sched_barrier(0);
            if (x + 1 < 64) mA = *reinterpret_cast<const uint64_t*>(k.modb + rk_mod_addr(k, la));
            if (x + W < 64) oa[x + W] = ld_out(xa[(x + W) % W], pa[(x + W) >> 2], (x + W) & 3);
            __builtin_amdgcn_sched_barrier(0);
            if (x & 1) asm("v_min3_u32 %0, %1, %2, %3" : "=v"(ma) : "v"(ma), "v"(pha), "v"(ha));  // one op per two bytes
            else pha = ha;
        }
        if (ACT_B) {
            const uint32_t th = __builtin_amdgcn_perm(b[x >> 2], hb, rk_in_sel(x & 3));
            const uint32_t tl = __builtin_amdgcn_alignbit(hb, lb, 8);
            hb = __builtin_amdgcn_bitop3_b32(th, static_cast<uint32_t>(mB >> 32), static_cast<uint32_t>(ob[x] >> 32), 0x96);
            lb = __builtin_amdgcn_bitop3_b32(tl, static_cast<uint32_t>(mB), static_cast<uint32_t>(ob[x]), 0x96);
            __builtin_amdgcn_sched_barrier(0);
            if (x + 1 < 64) mB = *reinterpret_cast<const uint64_t*>(k.modb + rk_mod_addr(k, lb));
            if (x + W < 64) ob[x + W] = ld_out(xb[(x + W) % W], pb[(x + W) >> 2], (x + W) & 3);
            __builtin_amdgcn_sched_barrier(0);
            if (x & 1) asm("v_min3_u32 %0, %1, %2, %3" : "=v"(mb) : "v"(mb), "v"(phb), "v"(hb));
            else phb = hb;
        }
    }
}

// Exact re-run of one chain's 64 bytes from (hi, lo) (rare): first index in [lo_i, hi_i]
// that is a candidate, else 64.
__device__ uint32_t rk_exact64(const RkCtx& k, uint32_t hi, uint32_t lo, const uint32_t (&in)[16],
                               const uint32_t (&prv)[16], int lo_i, int hi_i) {
    // 16-byte windows (the arrays shift by four dwords per window, not one per 4 bytes), done
    // once every lane running it has found its candidate
    uint32_t e[16], o[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        e[j] = in[j];
        o[j] = prv[j];
    }
    uint32_t first = 64;
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
#pragma unroll
        for (int b = 0; b < 16; b++) {
            rk_roll(k, hi, lo, rk_out(k, o[b >> 2], b & 3), e[b >> 2], b & 3);
            const int i = 16 * w + b;
            if (first == 64 && hi < k.thr && i >= lo_i && i <= hi_i) first = static_cast<uint32_t>(i);
        }
        if (__ballot(first == 64) == 0) break;
#pragma unroll
        for (int q = 0; q < 12; q++) {
            e[q] = e[q + 4];
            o[q] = o[q + 4];
        }
    }
    return first;
}

// Warm fill of a tile -> both chains' 64-byte histories (pa, pb) and states.
__device__ __forceinline__ void rk_warm(const RkCtx& kx, const uint32_t (&dw)[32], uint32_t& ha, uint32_t& la,
                                        uint32_t& hb, uint32_t& lb, uint32_t (&pa)[16], uint32_t (&pb)[16]) {
    ha = la = hb = lb = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        pa[i] = dw[i];
        pb[i] = dw[16 + i];
    }
#pragma unroll
    for (int x = 0; x < 64; x++) {
        if (x % 16 == 0) __builtin_amdgcn_sched_barrier(0);
        rk_roll0(kx, ha, la, pa[x >> 2], x & 3);
        rk_roll0(kx, hb, lb, pb[x >> 2], x & 3);
    }
}
__device__ __forceinline__ RkCtx rk_setup(RkTables& smt, const BatchArgs& a, int lane) {
    auto rev8 = [](uint32_t f) { return __builtin_bitreverse32(f) >> 24; };
    for (uint32_t i = threadIdx.x; i < 256u * kRkModRep; i += blockDim.x)
        smt.mod[i] = __builtin_bitreverse64(a.rk_mod[rev8(i / kRkModRep)]);
    for (uint32_t i = threadIdx.x; i < 256u * kRkOutRep; i += blockDim.x) {  // outx[] (rk_roll)
        const uint64_t o = a.rk_out[rev8(i / kRkOutRep)];
        smt.out[i] = __builtin_bitreverse64((o << 8) ^ a.rk_mod[(o >> 45) & 0xFFu]);
    }
    __syncthreads();
    RkCtx kx;
    kx.modb = reinterpret_cast<const char*>(smt.mod);
    kx.outb = reinterpret_cast<const char*>(smt.out);
    kx.lane8o = static_cast<uint32_t>(lane & (kRkOutRep - 1)) * 8u;
    kx.lane8m = static_cast<uint32_t>(lane & (kRkModRep - 1)) * 8u;
    kx.thr = 1u << (32 - __builtin_popcount(a.mask));  // mask = avg - 1, avg a power of two in [2, 2^31]
    return kx;
}
#define RK_STEP rk_step64
// The rare exact re-run of a 64-byte piece at coordinate c whose running test passed.
__device__ __forceinline__ uint32_t rk_exact(const RkCtx& k, uint32_t h0, uint32_t l0, const Loader& ld, int64_t c,
                                            const uint32_t (&in)[16], const uint32_t (&prv)[16], int lo_i, int hi_i) {
    (void)ld;
    (void)c;
    return rk_exact64(k, h0, l0, in, prv, lo_i, hi_i);
}

// Geometry of a Rabin-Karp tile at ct: L bytes per lane (a multiple of 256: two chains of
// whole 128-byte lines), K lines per chain.
struct RkGeom {
    int64_t L;
    int K;
    Loader ld;
};
__device__ __forceinline__ RkGeom rk_geom(int64_t ct, int64_t hi, const uint8_t* abase, int64_t off0,
                                          int64_t nbytes_coord, int64_t lane_cap = kLaneMax) {
    const int64_t rem = hi - ct + 1;
    int64_t per = (rem + kWave - 1) / kWave;
    per = (per + 255) & ~int64_t(255);
    RkGeom g;
    g.L = per < lane_cap ? per : lane_cap;  // lane_cap: a multiple of 256
    g.K = static_cast<int>(g.L / 256);
    g.ld = make_loader(abase, off0, nbytes_coord, ct >= 64 ? ct - 64 : 0);
    return g;
}
// Warm fill: lane l's slot line = [64 B before c0 | 64 B before c0 + L/2] (16-byte granule j
// of lane l at j ^ sw(l), as dma_step128).
__device__ __forceinline__ void rk_dma_warm(const Loader& ld, uint32_t slot, int64_t ct, int64_t L, int lane) {
    uint32_t sl = slot;  // opaque per call (as dma_step128)
    asm volatile("" : "+s"(sl));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int l = 8 * i + (lane >> 3);
        const int jj = (lane & 7) ^ ((l >> 1) & 7);
        const int64_t c0 = ct + l * L + (jj < 4 ? 0 : L / 2);
        const int64_t coord = c0 - 64 + 16 * (jj & 3);
        dma_lds16(ld.d, sl + 1024u * i, static_cast<int32_t>(coord - ld.tb));
    }
}
// Line fill f (1..2K): odd f = line (f-1)/2 of chain A, even f = line f/2 - 1 of chain B.
__device__ __forceinline__ void rk_dma_line(const Loader& ld, uint32_t slot, int64_t ct, int64_t L, int f, int lane) {
    const int64_t half = (f & 1) ? 0 : L / 2;
    const int64_t line = (f & 1) ? (f - 1) / 2 : f / 2 - 1;
    dma_step128(ld, ld.tb, slot, ct + half, L, line, lane);
}
__device__ __forceinline__ void rk_mask_head(uint32_t (&dw)[16], int64_t c, int64_t off0) {
    if (c == 0 && off0) {  // bytes before the stream start are virtual zeros
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int64_t keep_from = off0 - 4 * d;
            const uint32_t m = keep_from <= 0 ? 0xFFFFFFFFu : (keep_from >= 4 ? 0u : (0xFFFFFFFFu << (8 * keep_from)));
            dw[d] &= m;
        }
    }
}

// The line fills and drain of one tile (after its warm fill, which left both chains' states
// and histories in ha/la, hb/lb, pa, pb): refill(f) is called right after fill f has been
// read out of the slot (the slot is free), check(min, chain, offset from the chain's start,
// state before, bytes, history) after each chain's 64 bytes.  Coordinates stay out of the
// walk (64-bit per-lane values live across it spilled, and every reload's vmcnt wait drained
// the line DMA): `head` says whether lane 0's chain A starts at coordinate 0.
// KCDC_TRACE builds time every line fill's DMA wait (s_memtime, shader cycles) into `dmaw`.
#if KCDC_TRACE
#define RK_VMWAIT(acc)                                                  \
    do {                                                                \
        const uint64_t t0_ = __builtin_amdgcn_s_memtime();              \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                \
        acc += __builtin_amdgcn_s_memtime() - t0_;                      \
    } while (0)
#else
#define RK_VMWAIT(acc) asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif
template <class Refill, class Check>
__device__ __forceinline__ void rk_walk(const RkCtx& kx, const uint8_t* sl, int lane, bool head,
                                        int64_t off0, int K, uint32_t& ha, uint32_t& la, uint32_t& hb, uint32_t& lb,
                                        uint32_t (&pa)[16], uint32_t (&pb)[16], Refill&& refill, Check&& check,
                                        uint64_t& dmaw) {
    (void)dmaw;
    uint32_t bf[16];  // the second half of the line that arrived last step
#pragma unroll
    for (int i = 0; i < 16; i++) bf[i] = 0;
    for (int j = 0; j < K; j++) {
        // ---- odd fill 2j+1: A line j (A: its first half; B: the second half of its line j-1)
        {
            uint32_t dw[32], na[16];
            __builtin_amdgcn_sched_barrier(0);
            RK_VMWAIT(dmaw);
            rk_read_step128(sl, lane, head && j == 0 ? 0 : 1, off0, dw);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            refill(2 * j + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; i++) na[i] = dw[i];
            const uint32_t ha0 = ha, la0 = la, hb0 = hb, lb0 = lb;
            uint32_t ma = 0xFFFFFFFFu, mb = 0xFFFFFFFFu;
            if (j == 0) {
                RK_STEP<true, false>(kx, ha, la, na, pa, hb, lb, bf, pb, ma, mb);
            } else {
                RK_STEP<true, true>(kx, ha, la, na, pa, hb, lb, bf, pb, ma, mb);
                check(mb, 1, 128 * (j - 1) + 64, hb0, lb0, bf, pb);
#pragma unroll
                for (int i = 0; i < 16; i++) pb[i] = bf[i];
            }
            check(ma, 0, 128 * j, ha0, la0, na, pa);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                pa[i] = na[i];
                bf[i] = dw[16 + i];  // A's second half, next step
            }
        }
        // ---- even fill 2j+2: B line j (A: the second half of its line j; B: its first half)
        {
            uint32_t dw[32], nb[16];
            __builtin_amdgcn_sched_barrier(0);
            RK_VMWAIT(dmaw);
            rk_read_step128(sl, lane, 1, off0, dw);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            refill(2 * j + 2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; i++) nb[i] = dw[i];
            const uint32_t ha0 = ha, la0 = la, hb0 = hb, lb0 = lb;
            uint32_t ma = 0xFFFFFFFFu, mb = 0xFFFFFFFFu;
            RK_STEP<true, true>(kx, ha, la, bf, pa, hb, lb, nb, pb, ma, mb);
            check(ma, 0, 128 * j + 64, ha0, la0, bf, pa);
            check(mb, 1, 128 * j, hb0, lb0, nb, pb);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                pa[i] = bf[i];
                pb[i] = nb[i];
                bf[i] = dw[16 + i];  // B's second half, next step
            }
        }
    }
    // ---- D: B's last 64 bytes (the slot meanwhile takes the next warm fill / entry)
    {
        const uint32_t hb0 = hb, lb0 = lb;
        uint32_t ma = 0xFFFFFFFFu, mb = 0xFFFFFFFFu;
        RK_STEP<false, true>(kx, ha, la, bf, pa, hb, lb, bf, pb, ma, mb);
        check(mb, 1, 128 * (K - 1) + 64, hb0, lb0, bf, pb);
    }
}
#undef RK_STEP  // rk_walk was their only user (the long path's scan calls rk_walk, not the macros)
#undef RK_VMWAIT

// Rabin-Karp lane segments: twice the buzhash cap (warm-up vs tile overshoot; 2 vs 1: 4M 2.542 vs
// 2.554 ms, 128K 5.536 vs 5.643 ms, profiles/r03/rk/kbench_lmul_*.log)
constexpr int64_t kRkLaneMul = 2;
// Intra-region help as in split_batch_pipe_kernel (the same help slots, claim words and rows; hep,
// hs and the kHs* flags mean the same).  An own tile is T = 64 x rk_cap bytes; a help task scans
// one in two sub-tiles of rk_cap / 2 bytes per lane.
// This kernel spells the visit protocol out itself, statement for statement what Visit, Tile and
// the visit_* functions above do for the buzhash kernel: on the shared functions it measured
// slower (same-process A/B against the kernel as it stands, 4M: 4096 x 4 MiB 2.221 vs 2.205 ms,
// 1024 x 16 MiB 4.092 vs 4.031, 512 x 32 MiB 6.512 vs 6.381; with only the take and the adoption
// shared, 512 x 32 MiB 6.406 and 128K 64 x 64 MiB 29.66 vs 29.42).  The statements are the same;
// the register allocation around the walk is not (200 vs 185 SGPR spills, 50 vs 35 spill reloads
// in the walk's blocks).  A change to the protocol is made in both places.
__global__ __launch_bounds__(kRkWaves * kWave, kRkWaves / 4) void split_batch_rk_kernel(BatchArgs a) {
    __shared__ RkTables smt;
    __shared__ RkSlots smslots;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const RkCtx kx = rk_setup(smt, a, lane);
    uint8_t* sl = smslots.b[wave][0];
    const uint32_t sl32 = lds_addr(sl);
    const int64_t mx = static_cast<int64_t>(a.max_size);
    const uint32_t me = blockIdx.x * kRkWaves + wave;  // this wave's help slot
    const int64_t rk_cap = kRkLaneMul * static_cast<int64_t>(a.lane_cap);  // lane bytes of an own tile (>= 512)

#if KCDC_TRACE  // per wave at trace[8 * global wave]: start, end, ticks in blocking takes, the last take's
                // start (s_memrealtime); help tiles | own tiles << 32; shader cycles in line-fill DMA
                // waits, in the walks, in the warm fills (s_memtime)
    const uint32_t gw = blockIdx.x * kRkWaves + wave;
    uint64_t tr_block = 0, tr_last = 0, tr_tiles = 0, tr_dma = 0, tr_walk = 0, tr_warm = 0;
    const uint64_t tr_mt0 = __builtin_amdgcn_s_memtime();  // span in shader cycles after the records
    if (lane == 0) a.trace[8 * gw] = __builtin_amdgcn_s_memrealtime();
#define KCDC_RKRET                                                                \
    do {                                                                          \
        if (lane == 0) {                                                          \
            a.trace[8 * gw + 1] = __builtin_amdgcn_s_memrealtime();                \
            a.trace[8 * gw + 2] = tr_block;                                       \
            a.trace[8 * gw + 3] = tr_last;                                        \
            a.trace[8 * gw + 4] = tr_tiles;                                       \
            a.trace[8 * gw + 5] = tr_dma;                                         \
            a.trace[8 * gw + 6] = tr_walk;                                        \
            a.trace[8 * gw + 7] = tr_warm;                                        \
            a.trace[8ull * gridDim.x * kRkWaves + gw] = __builtin_amdgcn_s_memtime() - tr_mt0; \
        }                                                                         \
        return;                                                                   \
    } while (0)
#else
    uint64_t tr_dma = 0;
#define KCDC_RKRET return
#endif
    PStream cur;
    int64_t budget = kNoYield;
    uint32_t hep = 0, hs = 0;
    hs = kHsNeedPub;
    auto hK = [&] { return hs & 0xFFu; };
    auto htile = [&] { return (hs >> 8) & 0xFFu; };
    auto take_blocking = [&](uint32_t t, int64_t backlog_hint, uint32_t claim) -> bool {
#if KCDC_TRACE
        const uint64_t tb0 = __builtin_amdgcn_s_memrealtime();
        tr_last = tb0;
        struct Acc {
            uint64_t t0, &sum;
            __device__ ~Acc() { sum += __builtin_amdgcn_s_memrealtime() - t0; }
        } acc{tb0, tr_block};
#endif
        for (;;) {
            int64_t backlog = backlog_hint;
            if (t == 0xFFFFFFFFu) {
                const uint64_t ht = qht_take(a, lane, 1);
                t = static_cast<uint32_t>(ht);
                backlog = static_cast<int64_t>(ht >> 32) - static_cast<int64_t>(t) - 1;
            }
            const uint32_t held = t;
            const int r = presolve(a, lane, held, cur, kRkWaves, me, a.help != nullptr && claim == 0xFFFFFFFFu);
            if (r == 0) return false;
            if (r == 3) {  // a help task; the ticket stays held (in cap, unused by help tasks, and in memory)
                held_put(a, lane, me, held);
                cur.cap = held;
                uniformize(cur);
                return true;
            }
            t = 0xFFFFFFFFu;
            if (claim != 0xFFFFFFFFu) {
                const bool requeued = bcast(claim) == 2u;
                claim = 0xFFFFFFFFu;
                if (requeued) continue;
            }
            if (r == 2) continue;  // tombstone
            uniformize(cur);
            if (!pcheck(a, lane, cur, held, 1)) return false;
            budget = pipe_quantum(backlog);
            if (pstream_region(a, cur, lane)) return true;
            if (lane == 0) {
                a.counts[cur.sid] = cur.cnt;
                add_agent(a.queue + kQDone, 1u);
            }
        }
    };
    bool need_take = true;
    uint32_t take_t = 0xFFFFFFFFu, take_claim = 0xFFFFFFFFu;
    int64_t take_backlog = 0;
    {
        uint32_t claim = 1u;
        if (lane == 0) {
            claim = 0u;
            __hip_atomic_compare_exchange_strong((gu32*)(a.queue + kQFlags + blockIdx.x), &claim, 1u,
                                                 __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t t0 = first_ticket(blockIdx.x, wave);
        const int64_t nw = static_cast<int64_t>(gridDim.x) * kRkWaves;
        take_t = t0 < a.nstreams ? t0 : 0xFFFFFFFFu;
        take_backlog = static_cast<int64_t>(a.nstreams) - nw;
        take_claim = t0 < a.nstreams ? (claim & 3u) : 0xFFFFFFFFu;
    }
    bool issued = false;  // this tile's warm fill is in flight
    for (;;) {
#if KCDC_HELP_DIAG
        diag_record(a, lane, divergent_bit(need_take, 0) | divergent_bit(take_t, 1) | divergent_bit(issued, 2));
#endif
        if (need_take) {
            if (!take_blocking(take_t, take_backlog, take_claim)) KCDC_RKRET;
            need_take = false;
            issued = false;
            hs |= kHsNeedPub;
        }
#if KCDC_HELP_DIAG
        diag_record(a, lane, divergent_bit(hs, 3) | divergent_bit(hep, 4) | divergent_bit(cur.sid, 5) |
                                 divergent_bit(static_cast<uint32_t>(cur.cap), 6) |
                                 divergent_bit(static_cast<uint32_t>(cur.ct), 7) |
                                 divergent_bit(static_cast<uint32_t>(budget), 8));
#endif
        uniformize(cur);
        if (!pcheck(a, lane, cur, 0xFFFFFFFFu, 5)) KCDC_RKRET;
        const bool is_help = (cur.sid & kHelpBit) != 0;
#if KCDC_TRACE
        tr_tiles += is_help ? 1ull : (1ull << 32);
        const uint64_t tr_t0 = __builtin_amdgcn_s_memtime();
#endif
        int64_t lo, hi;
        pregion(a, cur, lo, hi);
        const int64_t lcap = is_help ? rk_cap / 2 : rk_cap;
        const RkGeom g = rk_geom(cur.ct, hi, cur.abase, cur.off0, cur.off0 + cur.n, lcap);
        const int64_t ct = cur.ct, ct_next = ct + kWave * g.L;
        const bool last_of_region = ct_next > hi;
        // A region new to this wave: publish it when it is long enough to share.
        if ((hs & kHsNeedPub) && !is_help) {
            const int64_t T = kWave * rk_cap;
            const uint32_t K = static_cast<uint32_t>((hi - ct + T) / T);
            hs = 0;
            if (a.help && K >= kHelpMinTiles && K <= static_cast<uint32_t>(kHelpTiles)) {
                const uint32_t Kw = a.help_window && K > a.help_window ? a.help_window : K;  // a window
                hep++;
                hs = kHsPub | Kw;
                help_publish(a, lane, me, hep, cur, ct, Kw < K ? ct + static_cast<int64_t>(Kw) * T - 1 : hi, Kw, T);
            }
        }
        // The owner's claim on its next tile: an atomic add on its slot's bottom after fill 1's
        // DMA, its value consumed at fill 2 (after that fill's vmcnt wait, before its DMA), so
        // no compiler-visible load is in flight across a DMA.
        const bool claim_next_r = (hs & kHsPub) && !is_help && !last_of_region && htile() + 1u < hK();
        const bool budget_out = !is_help && !(hs & kHsHelped) && budget - kWave * g.L <= 0;
        bool ends_nocand = false;
        if (!is_help && last_of_region) {
            const int64_t s2 = cur.s + mx - 1 <= cur.n - 1 ? cur.s + mx : cur.n;
            ends_nocand = s2 >= cur.n || s2 + static_cast<int64_t>(a.min_size) - 1 >= cur.n;
        }
        const bool switching = !is_help && (budget_out || ends_nocand);
        const bool reserve = budget_out && !ends_nocand;
        const bool claim_next = claim_next_r && !switching;
        uint64_t ht_raw = 0;
        if (switching) ht_raw = qht_add(a, lane, 1);  // the next stream's ticket
        uint32_t ht_lo = static_cast<uint32_t>(ht_raw), ht_hi = static_cast<uint32_t>(ht_raw >> 32);
        if (!issued) rk_dma_warm(g.ld, sl32, ct, g.L, lane);
        uint32_t ha = 0, la = 0, hb = 0, lb = 0;
        uint32_t pa[16], pb[16];
        // ---- W: warm fill -> both chains' 64-byte histories; line 1 (A line 0) goes out
        {
            uint32_t dw[32];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(ht_lo), "+v"(ht_hi)::"memory");
            rk_read_step128(sl, lane, -1, cur.off0, dw);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            rk_dma_line(g.ld, sl32, ct, g.L, 1, lane);
            __builtin_amdgcn_sched_barrier(0);
            rk_warm(kx, dw, ha, la, hb, lb, pa, pb);
        }
#if KCDC_TRACE
        const uint64_t tr_t1 = __builtin_amdgcn_s_memtime();
        tr_warm += tr_t1 - tr_t0;
#endif
        uint32_t tk = 0;
        int64_t nbacklog = 0;
        if (switching) {
            const uint64_t ht = qht_value(ht_lo, ht_hi);
            tk = static_cast<uint32_t>(ht);
            nbacklog = static_cast<int64_t>(ht >> 32) + (reserve ? 1 : 0) - static_cast<int64_t>(tk) - 1;
        }
        uint64_t pe_raw = 0;
        bool res_issued = false, next_issued = false, entry_issued = false;
        bool claim_ok = false, claim_known = !claim_next;
        uint64_t claim_raw = 0;
        auto claim_decode = [&]() {  // the claim word before this tile's add (+1 = after it)
            const uint64_t cw = qht_value(static_cast<uint32_t>(claim_raw), static_cast<uint32_t>(claim_raw >> 32)) + 1ull;
            const uint32_t top = static_cast<uint32_t>(cw >> 20) & 0xFFFFFu, bot = static_cast<uint32_t>(cw) & 0xFFFFFu;
            claim_ok = static_cast<uint32_t>(cw >> 40) == hep && bot <= top;
            if (top < hK()) hs |= kHsHelped;
            claim_known = true;
        };
        // After the tile's last fill: the next tile's warm fill, or the next stream's entry.
        auto refill_last = [&]() {
            if (reserve && !res_issued) {  // this stream's ring entry, reserved late
                pe_raw = qht_add(a, lane, 1ull << 32);
                res_issued = true;
            }
            if (switching) {
                pentry_dma(a, lane, tk, sl32);
                entry_issued = true;
            } else if (!last_of_region && (!claim_next || claim_ok)) {  // the next tile has its own geometry
                const RkGeom gn = rk_geom(ct_next, hi, cur.abase, cur.off0, cur.off0 + cur.n, lcap);
                rk_dma_warm(gn.ld, sl32, ct_next, gn.L, lane);
                next_issued = true;
            }
        };
        int32_t found_a = -1, found_b = -1;  // offsets from the chain's start
        // After line fill f is read: issue what the slot takes next (fill f+1, or after the
        // last fill the next tile's warm fill / the next stream's queue entry).
        auto refill = [&](int f) {
            if (claim_next && f == 2) claim_decode();
            if (f < 2 * g.K)
                rk_dma_line(g.ld, sl32, ct, g.L, f + 1, lane);
            else
                refill_last();
            if (claim_next && f == 1 && lane == 0)
                claim_raw = __hip_atomic_fetch_add((gu64*)help_claim(a, me), 1ull, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        };
        // Hit check of one chain's 64 bytes at `rel` from its start (state before: h0/l0):
        // the chain's first candidate in [lo, hi].  The coordinate is formed only here, from
        // wave-uniform values and an opaque lane id (nothing 64-bit per lane lives across the walk).
        auto check = [&](uint32_t mm, int chain, int rel, uint32_t h0, uint32_t l0, const uint32_t (&in)[16],
                         const uint32_t (&prv)[16]) {
            if (mm < kx.thr && (chain ? found_b : found_a) < 0) {
                int ln = lane;
                asm volatile("" : "+v"(ln));
                const int64_t c = ct + ln * g.L + (chain ? g.L / 2 : 0) + rel;
                if (c <= hi) {
                    const int64_t blo = lo - c, bhi = hi - c;
                    const uint32_t idx = rk_exact(kx, h0, l0, g.ld, c, in, prv, blo < 0 ? 0 : static_cast<int>(blo),
                                                  bhi > 63 ? 63 : static_cast<int>(bhi));
                    if (idx < 64u) {
                        if (chain)
                            found_b = rel + static_cast<int32_t>(idx);
                        else
                            found_a = rel + static_cast<int32_t>(idx);
                    }
                }
            }
        };
        rk_walk(kx, sl, lane, ct == 0 && lane == 0, cur.off0, g.K, ha, la, hb, lb, pa, pb, refill, check, tr_dma);
#if KCDC_TRACE
        tr_walk += __builtin_amdgcn_s_memtime() - tr_t1;
#endif
        const int64_t c0 = ct + lane * g.L;
        const int64_t found = found_a >= 0 ? c0 + found_a : found_b >= 0 ? c0 + g.L / 2 + found_b : -1;
        // ---- end of tile
        if (!claim_known) {  // one-line tiles (K = 1) consume the claim here
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            claim_decode();
        }
        if (reserve && !res_issued) {
            pe_raw = qht_add(a, lane, 1ull << 32);
            res_issued = true;
        }
        const uint64_t hit = __ballot(found >= 0);
        if (is_help) {
            bool done = true;
            if (hit || last_of_region) {  // post the tile's first candidate to its owner's row
                int64_t f = -1;
                if (hit) f = static_cast<int64_t>(uni64(static_cast<uint64_t>(__shfl(found, __builtin_ctzll(hit)))));
                help_post(a, lane, static_cast<uint32_t>(cur.cb), cur.epoch, static_cast<uint32_t>(cur.cnt), cur.s, f);
            } else {  // the next sub-tile (prefetched), unless the owner has closed the region
                const uint64_t w = ld_agent64(help_claim(a, static_cast<uint32_t>(cur.cb)));
                done = static_cast<uint32_t>(qht_value(static_cast<uint32_t>(w), static_cast<uint32_t>(w >> 32)) >> 40) !=
                       cur.epoch;
            }
            if (!done) {
                cur.ct = ct_next;
                issued = next_issued;
                continue;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the post, or a dropped prefetch
            need_take = true;
            take_t = held_get(a, lane, me, static_cast<uint32_t>(cur.cap));
            take_backlog = 0;
            take_claim = 0xFFFFFFFFu;
            continue;
        }
        bool region_changed = true;
        const int64_t forced = cur.s + mx - 1 <= cur.n - 1 ? cur.s + mx : cur.n;
        int64_t cut = -1;  // this region's cut, once known
        if (hit) {
            const int first = __builtin_ctzll(hit);
            const int64_t f = static_cast<int64_t>(uni64(static_cast<uint64_t>(__shfl(found, first))));
            cut = f - cur.off0 + 1;
        } else if (last_of_region) {  // forced cut at max size (splitter_rabinkarp64.go:60-64) or the end
            cut = forced;
        } else if (claim_next && !claim_ok) {  // the helpers hold the rest of the region
            const int64_t T = kWave * rk_cap;
            const int64_t ct0 = ct - static_cast<int64_t>(htile()) * T;  // the published tile 0
            const int64_t r = help_wait(a, lane, me, hep, htile() + 1u, hK(), ct0);
            const int64_t wend = ct0 + static_cast<int64_t>(hK()) * T;  // past the published window
            if (r >= 0) {
                cut = r - cur.off0 + 1;
            } else if (r == -1 && wend <= hi) {  // no candidate in the window: publish the next one
                cur.ct = wend;
                help_close(a, lane, me, hep);
                hs = kHsNeedPub;
                region_changed = false;
            } else if (r == -1) {
                cut = forced;
            } else {  // a tile still pending: scan on from it, unshared
                cur.ct = ct0 + (-2 - r) * T;
                help_close(a, lane, me, hep);
                hs = 0;
                region_changed = false;
            }
        } else {
            cur.ct = ct_next;
            hs += 1u << 8;  // htile++
            budget -= kWave * g.L;
            region_changed = false;
            if ((hs & kHsPub) && htile() >= hK()) {  // past its published window: the next one
                help_close(a, lane, me, hep);
                hs = kHsNeedPub;
            }
        }
        if (cut >= 0) {
            emit_cut(a, cur, lane, cut);
            cur.s = cut;
            cur.ct = -1;
        }
        if (region_changed) {
            if (hs & kHsPub) help_close(a, lane, me, hep);
            hs = kHsNeedPub;
        }
        const bool live = pstream_region(a, cur, lane);
        if (!live && lane == 0) {
            a.counts[cur.sid] = cur.cnt;
            add_agent(a.queue + kQDone, 1u);
        }
        if (!switching && live) {  // same stream, next tile
            issued = next_issued && !region_changed;
            if (next_issued && region_changed) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stale prefetch
            continue;
        }
        if (hs & kHsPub) help_close(a, lane, me, hep);  // a yielded region is not ours to share any more
        hs = kHsNeedPub;
        if (reserve) {
            const uint32_t pe = static_cast<uint32_t>(
                qht_value(static_cast<uint32_t>(pe_raw), static_cast<uint32_t>(pe_raw >> 32)) >> 32);
            pwrite(a, lane, pe, cur, !live);
        } else if (live) {  // a candidate kept the stream alive past its predicted last tile
            const uint64_t ht = qht_take(a, lane, 1ull << 32);
            pwrite(a, lane, static_cast<uint32_t>(ht >> 32), cur, false);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the entry DMA (or a stale prefetch) has landed
        bool took = false;
        if (switching && entry_issued) {
            const u32x4 ev = *reinterpret_cast<const u32x4*>(sl + 16 * (lane & 7));
            if (pentry_ok(ev, lane, tk) && static_cast<uint32_t>(__builtin_amdgcn_readlane(ev.w, 0)) != kTombstone) {
                PStream nx;
                pentry_decode(nx, ev);
                uniformize(nx);
                if (!pcheck(a, lane, nx, tk, 2)) KCDC_RKRET;
                cur = nx;
                budget = pipe_quantum(nbacklog);
                took = true;
                issued = false;
                if (!pstream_region(a, cur, lane)) {
                    if (lane == 0) {
                        a.counts[cur.sid] = cur.cnt;
                        add_agent(a.queue + kQDone, 1u);
                    }
                    need_take = true;
                    take_t = 0xFFFFFFFFu;
                    take_backlog = 0;
                    take_claim = 0xFFFFFFFFu;
                }
                continue;
            }
        }
        if (!took) {
            need_take = true;
            take_t = switching ? tk : 0xFFFFFFFFu;
            take_backlog = nbacklog;
            take_claim = 0xFFFFFFFFu;
        }
    }
}
#undef KCDC_RKRET

}  // namespace dev
}  // namespace kcdc
