// Splitter kernels, part 9 of 9: the long-stream path (intra-stream parallel).
// LongStream / LongArgs / Seg, the two candidate scans (cand_scan_dma_kernel buzhash,
// cand_scan_rk_kernel Rabin-Karp), seg_prefix, compact, the serial and the parallel resolver,
// and occupy_kernel (test support).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_hash.h"
#include "kcdc_split_feed.h"
#include "kcdc_split_queue.h"
#include "kcdc_split_rk.h"

namespace kcdc {
namespace dev {

// ------------------------------------------- long single stream (config 3)
// Phase 1: every 128 KiB segment (in coordinates) is scanned by one wave (lane
// l: a 2 KiB sub-range with a 64-byte warm-up), which stores the segment's first
// kSegK candidate positions and whether it had more ("truncated").  Phase 2:
// exclusive prefix sum of the stored counts.  Phase 3: compaction into one
// sorted candidate list.  Phase 4: one wave walks the chunk rule over that list
// from LDS windows; where a truncated (candidate-dense) segment may hide the
// candidate it needs, it rescans that range with the same scan_region() the
// batch kernel uses.  The cut set is therefore exactly the sequential one.
constexpr int64_t kSegBytes = kWave * kLaneMax;  // 128 KiB
constexpr int kSegK = 8;
constexpr uint64_t kTruncBit = 1ull << 63;

// One stream of a long-path launch (several streams share one launch: their segments are
// numbered consecutively, stream j owning global segments [seg0, seg0 + its segment count)).
struct LongStream {
    const uint8_t* abase;
    int64_t off0;
    int64_t n;
    int64_t seg0;
    uint64_t* cuts;
    uint64_t cuts_cap;
    uint64_t* count;
    uint64_t pad;
};
struct LongArgs {
    const LongStream* streams;
    uint32_t nstreams;
    int64_t nseg;        // all streams
    uint32_t* seg_cnt;   // stored count | (truncated << 31)
    uint64_t* seg_cand;  // [nseg][kSegK] positions (relative to the segment's stream)
    uint64_t* seg_off;   // exclusive prefix of stored counts
    uint64_t* list;      // compacted candidates (kTruncBit marks the last stored of a truncated segment)
    uint64_t* total;     // [1] number of list entries
    // parallel resolver (resolve_par_kernel); serial == nullptr: every stream resolves serially
    uint32_t* serial;    // [nstreams] 1: this stream needs the serial resolver
    uint32_t* jump;      // [levels][node_cap] successor tables, node k of stream j at lbeg + 2j + k
    uint32_t* forced;    // [node_cap] non-candidate cuts between a node's cut and its successor's
    uint64_t node_cap;
    uint32_t levels;
};

// The stream owning global segment `seg`: the last j with seg0 <= seg (wave-uniform).
__device__ __forceinline__ uint32_t long_stream_of(const LongArgs& g, int64_t seg) {
    uint32_t lo = 0, hi = g.nstreams - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        const int64_t s0 = static_cast<int64_t>(uni64(static_cast<uint64_t>(g.streams[mid].seg0)));
        if (s0 <= seg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Global segment `seg` as its scanning wave sees it (wave-uniform): its stream, the segment's
// first coordinate cs and the stream's coordinates [lo, hi] inside it.
struct Seg {
    const uint8_t* abase;
    int64_t off0, n, cs, lo, hi;
};
__device__ __forceinline__ Seg long_seg_of(const LongArgs& g, int64_t seg) {
    const LongStream& S = g.streams[long_stream_of(g, seg)];
    Seg q;
    q.off0 = static_cast<int64_t>(uni64(static_cast<uint64_t>(S.off0)));
    q.n = static_cast<int64_t>(uni64(static_cast<uint64_t>(S.n)));
    q.abase = reinterpret_cast<const uint8_t*>(uni64(reinterpret_cast<uint64_t>(S.abase)));
    q.cs = (seg - static_cast<int64_t>(uni64(static_cast<uint64_t>(S.seg0)))) * kSegBytes;
    q.lo = q.cs > q.off0 ? q.cs : q.off0;
    q.hi = (q.cs + kSegBytes < q.off0 + q.n ? q.cs + kSegBytes : q.off0 + q.n) - 1;
    return q;
}

// Record segment `seg`: lane l found nf candidates (kSegK + 1: more than kSegK) at offsets
// found[] from the segment start, lanes in position order.  Stores the segment's first kSegK
// candidates (positions from the stream start) and its count with the truncation flag.
__device__ __forceinline__ void long_seg_record(const LongArgs& g, int64_t seg, const Seg& q, int lane, int nf,
                                                const uint32_t (&found)[kSegK]) {
    // exclusive prefix of per-lane counts (lane segments are in position order)
    int incl = nf;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    const int tot = __shfl(incl, kWave - 1);
    const int pre = incl - nf;
    for (int j = 0; j < nf && j < kSegK; j++)
        if (pre + j < kSegK) g.seg_cand[seg * kSegK + pre + j] = static_cast<uint64_t>(q.cs - q.off0) + found[j];
    if (lane == 0)
        g.seg_cnt[seg] = (tot > kSegK ? 0x80000000u : 0u) | static_cast<uint32_t>(tot < kSegK ? tot : kSegK);
}

// Rabin-Karp candidate scan of the long path on split_batch_rk_kernel's tile walk (two
// chains per lane, alternating 128-byte line fills, outx[] folding): one 128 KiB segment per
// tile, persistent grid-stride over the segments of every stream of the launch, the next
// segment's warm fill issued during the drain step.  Records what cand_scan_dma_kernel records.
__global__ __launch_bounds__(kRkWaves * kWave, kRkWaves / 4) void cand_scan_rk_kernel(BatchArgs a, LongArgs g) {
    __shared__ RkTables smt;
    __shared__ RkSlots smslots;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const RkCtx kx = rk_setup(smt, a, lane);
    uint8_t* sl = smslots.b[wave][0];
    const uint32_t sl32 = lds_addr(sl);
    const int64_t nw = static_cast<int64_t>(gridDim.x) * kRkWaves;
    auto issue = [&](const Seg& q) {
        const RkGeom t = rk_geom(q.cs, q.hi, q.abase, q.off0, q.off0 + q.n);
        rk_dma_warm(t.ld, sl32, q.cs, t.L, lane);
    };
    int64_t seg = static_cast<int64_t>(blockIdx.x) * kRkWaves + wave;
    if (seg >= g.nseg) return;
    Seg q = long_seg_of(g, seg);
    issue(q);
    for (;;) {
        const int64_t nseg_next = seg + nw;
        const bool has_next = nseg_next < g.nseg;
        Seg qn = q;
        if (has_next) qn = long_seg_of(g, nseg_next);
        const RkGeom t = rk_geom(q.cs, q.hi, q.abase, q.off0, q.off0 + q.n);
        uint32_t ha, la, hb, lb, pa[16], pb[16];
        {
            uint32_t dw[32];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            rk_read_step128(sl, lane, -1, q.off0, dw);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            rk_dma_line(t.ld, sl32, q.cs, t.L, 1, lane);
            __builtin_amdgcn_sched_barrier(0);
            rk_warm(kx, dw, ha, la, hb, lb, pa, pb);
        }
        // candidates per chain, two per register: 16-bit offsets from the chain's start (a lane
        // covers at most 2 KiB of a 128 KiB segment tile); halves state live across the walk
        uint32_t fa[kSegK / 2], fb[kSegK / 2];
#pragma unroll
        for (int k = 0; k < kSegK / 2; k++) fa[k] = fb[k] = 0;
        int na = 0, nb = 0;  // candidates per chain (kSegK + 1: more than kSegK)
        auto refill = [&](int f) {
            if (f < 2 * t.K)
                rk_dma_line(t.ld, sl32, q.cs, t.L, f + 1, lane);
            else if (has_next)
                issue(qn);
        };
        auto check = [&](uint32_t mm, int chain, int crel, uint32_t h0, uint32_t l0, const uint32_t (&in)[16],
                         const uint32_t (&prv)[16]) {
            int& nf = chain ? nb : na;
            uint32_t(&fnd)[kSegK / 2] = chain ? fb : fa;
            if (mm < kx.thr && nf <= kSegK) {  // rare: enumerate the piece's candidates exactly
                int ln = lane;
                asm volatile("" : "+v"(ln));  // the coordinate is formed here only (rk_walk)
                const int64_t c = q.cs + ln * t.L + (chain ? t.L / 2 : 0) + crel;
                const int64_t blo = q.lo - c, bhi = q.hi - c;
                int from = blo < 0 ? 0 : static_cast<int>(blo);
                const int to = bhi > 63 ? 63 : static_cast<int>(bhi);
                while (from <= to && nf <= kSegK) {
                    const uint32_t idx = rk_exact(kx, h0, l0, t.ld, c, in, prv, from, to);
                    if (idx >= 64u) break;
                    const uint32_t rel = static_cast<uint32_t>(crel) + idx;  // < 2^16
#pragma unroll
                    for (int k = 0; k < kSegK; k++)  // entry nf = rel, kept in registers (no scratch)
                        if (k == nf) fnd[k >> 1] |= rel << (16 * (k & 1));
                    nf++;
                    from = static_cast<int>(idx) + 1;
                }
            }
        };
        uint64_t dmaw = 0;
        rk_walk(kx, sl, lane, q.cs == 0 && lane == 0, q.off0, t.K, ha, la, hb, lb, pa, pb, refill, check, dmaw);
        const int64_t c0 = q.cs + lane * t.L, c0b = c0 + t.L / 2;
        // this lane's candidates in position order: chain A's, then chain B's
        const int nas = na < kSegK ? na : kSegK;
        const int nf = na + nb > kSegK ? kSegK + 1 : na + nb;
        uint32_t found[kSegK];  // offsets from the segment start
        const uint32_t base_a = static_cast<uint32_t>(c0 - q.cs), base_b = static_cast<uint32_t>(c0b - q.cs);
#pragma unroll
        for (int j = 0; j < kSegK; j++) {
            uint32_t v = base_a + ((fa[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
#pragma unroll
            for (int k = 0; k < kSegK; k++)
                if (j >= nas && k == j - nas) v = base_b + ((fb[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
            found[j] = v;
        }
        long_seg_record(g, seg, q, lane, nf, found);
        if (!has_next) break;
        seg = nseg_next;
        q = qn;
    }
}

// Buzhash candidate scan of the long path on the batch kernel's feeding scheme: a segment
// (128 KiB of coordinates) is exactly one tile of 64 lane segments, streamed by LDS-DMA in
// 128-byte steps with the next segment's warm piece and first step prefetched during the
// last step; persistent grid (one workgroup of kDmaWaves waves per CU), grid-stride over
// the segments of every stream of the launch.  Per segment it records the first kSegK
// candidates (positions from the stream start) and a truncation flag.
template <bool TOP>
__global__ __launch_bounds__(kDmaWaves * kWave, kDmaWaves / 4) void cand_scan_dma_kernel(BatchArgs a, LongArgs g) {
    __shared__ BuzShared smtab;
    __shared__ DmaSlots smslots;
    __shared__ WarmSlots smwarm;
    fill_buz_table(smtab, a.buz, a.buz_rot);
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    BuzRing hash;
    hash.tab = reinterpret_cast<const char*>(smtab.tab);
    hash.lane4 = static_cast<uint32_t>(lane) * 4u;
    hash.mask = a.mask;
    hash.h = 0;
    uint8_t* sl = smslots.b[wave][0];
    uint8_t* wl = smwarm.b[wave];
    const uint32_t sl32 = lds_addr(sl), wl32 = lds_addr(wl);
    const uint32_t lim = TOP ? a.buz_lim : 0u;
    const int64_t nw = static_cast<int64_t>(gridDim.x) * kDmaWaves;
    auto issue = [&](const Seg& q) {
        const TileGeom t = tile_geom(q.cs, q.hi, q.abase, q.off0, q.off0 + q.n);
        dma_piece(t.ld, t.ld.tb, wl32, q.cs, t.L, -1, lane);
        dma_step128(t.ld, t.ld.tb, sl32, q.cs, t.L, 0, lane);
    };
    int64_t seg = static_cast<int64_t>(blockIdx.x) * kDmaWaves + wave;
    if (seg >= g.nseg) return;
    Seg q = long_seg_of(g, seg);
    issue(q);
    for (;;) {
        const int64_t nseg_next = seg + nw;
        const bool has_next = nseg_next < g.nseg;
        Seg qn = q;
        if (has_next) qn = long_seg_of(g, nseg_next);
        const TileGeom t = tile_geom(q.cs, q.hi, q.abase, q.off0, q.off0 + q.n);
        const int64_t c0 = q.cs + lane * t.L;
        {
            uint32_t w16[16];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            read_piece(wl, lane, c0 - 64, q.off0, w16);
            hash.clear();
            hash.template block<kWarm>(w16);
        }
        uint32_t found[kSegK];
        int nf = 0;  // candidates of this lane (kSegK + 1: more than kSegK)
        for (int nb = 0; nb < t.nb; nb++) {
            const int64_t c = c0 + 128 * nb;
            const typename BuzRing::State st0 = hash.save();
            uint32_t dw[32];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            read_step128(sl, lane, c, q.off0, dw);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot free: refill it
            __builtin_amdgcn_sched_barrier(0);
            if (nb + 1 < t.nb)
                dma_step128(t.ld, t.ld.tb, sl32, q.cs, t.L, nb + 1, lane);
            else if (has_next)
                issue(qn);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t m = hash.template step128<TOP>(dw, 0u);
            __builtin_amdgcn_sched_barrier(0);
            if (m <= lim && c <= q.hi && nf <= kSegK) {  // rare: exact re-run from global memory
                uint32_t prv[16], cur32[32];
                t.ld.load(c - 64, prv);
                t.ld.load(c, cur32);
                const int64_t blo = q.lo - c, bhi = q.hi - c;
                int from = blo < 0 ? 0 : static_cast<int>(blo);
                const int to = bhi > 127 ? 127 : static_cast<int>(bhi);
                while (from <= to && nf <= kSegK) {
                    const uint32_t idx = hash.exact(st0, prv, cur32, from, to);
                    if (idx >= 128u) break;
                    if (nf < kSegK) found[nf] = static_cast<uint32_t>(c - q.cs) + idx;
                    nf++;
                    from = static_cast<int>(idx) + 1;
                }
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the waitcnt pass
            }
        }
        long_seg_record(g, seg, q, lane, nf, found);
        if (!has_next) break;
        seg = nseg_next;
        q = qn;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Exclusive prefix sum of the stored counts over all segments, in three launches:
// per-block sums of kPrefixItems segments, a scan of the block sums (one thread: a few
// hundred blocks at most), then every block scans its items from its offset.
constexpr int kPrefixItems = 1024 * 8;
__global__ __launch_bounds__(1024) void seg_blocksum_kernel(LongArgs g, uint64_t* block_sum) {
    __shared__ uint32_t wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kPrefixItems;
    uint32_t sum = 0;
    for (int j = 0; j < 8; j++) {
        const int64_t i = base + static_cast<int64_t>(t) * 8 + j;
        sum += i < g.nseg ? (g.seg_cnt[i] & 0x7FFFFFFFu) : 0u;
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d);
    if (lane == 0) wsum[w] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t tot = 0;
        for (int k = 0; k < 16; k++) tot += wsum[k];
        block_sum[blockIdx.x] = tot;
    }
}

__global__ void block_offsets_kernel(LongArgs g, uint64_t* block_sum, uint32_t nblocks) {
    if (threadIdx.x != 0) return;
    uint64_t run = 0;
    for (uint32_t b = 0; b < nblocks; b++) {  // in place: block_sum[b] becomes its exclusive offset
        const uint64_t v = block_sum[b];
        block_sum[b] = run;
        run += v;
    }
    g.total[0] = run;
}

__global__ __launch_bounds__(1024) void seg_prefix_kernel(LongArgs g, const uint64_t* block_off) {
    __shared__ uint64_t wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    constexpr int kItems = 8;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kPrefixItems;
    uint32_t v[kItems];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kItems; j++) {
        const int64_t i = base + static_cast<int64_t>(t) * kItems + j;
        v[j] = i < g.nseg ? (g.seg_cnt[i] & 0x7FFFFFFFu) : 0u;
        sum += v[j];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(incl, d);
        if (lane >= d) incl += x;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t run = block_off[blockIdx.x];
    for (int k = 0; k < w; k++) run += wsum[k];
    run += incl - sum;
#pragma unroll
    for (int j = 0; j < kItems; j++) {
        const int64_t i = base + static_cast<int64_t>(t) * kItems + j;
        if (i < g.nseg) g.seg_off[i] = run;
        run += v[j];
    }
}

__global__ void compact_kernel(LongArgs g) {
    const int64_t seg = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (seg >= g.nseg) return;
    const uint32_t c = g.seg_cnt[seg];
    const uint32_t k = c & 0x7FFFFFFFu;
    const uint64_t o = g.seg_off[seg];
    for (uint32_t j = 0; j < k; j++) {
        uint64_t v = g.seg_cand[seg * kSegK + j];
        if ((c >> 31) && j + 1 == k) v |= kTruncBit;
        g.list[o + j] = v;
    }
}

constexpr int kResolveWin = 4096;  // candidate-list entries staged in LDS

// One wave per stream (blockIdx.x): walks the chunk rule over the stream's candidate list.
template <int KIND>
__global__ __launch_bounds__(kWave) void resolve_kernel(BatchArgs a, LongArgs g, int64_t mn, int64_t mx) {
    if (g.serial && g.serial[blockIdx.x] == 0) return;  // resolved by resolve_par_kernel
    __shared__ HashSmem<KIND> sm;
    __shared__ uint64_t win[kResolveWin];
    fill_tables<KIND>(sm, a);
    const int lane = threadIdx.x;
    const auto hash = make_hash<KIND>(sm, a, lane);
    const LongStream& S = g.streams[blockIdx.x];
    const int64_t n = static_cast<int64_t>(uni64(static_cast<uint64_t>(S.n)));
    const int64_t off0 = static_cast<int64_t>(uni64(static_cast<uint64_t>(S.off0)));
    const uint8_t* abase = reinterpret_cast<const uint8_t*>(uni64(reinterpret_cast<uint64_t>(S.abase)));
    const int64_t seg0 = static_cast<int64_t>(uni64(static_cast<uint64_t>(S.seg0)));
    const uint64_t cuts_cap = uni64(S.cuts_cap);
    uint64_t* const cuts = reinterpret_cast<uint64_t*>(uni64(reinterpret_cast<uint64_t>(S.cuts)));
    // this stream's slice of the compacted list
    const int64_t lbeg = seg0 < g.nseg ? static_cast<int64_t>(uni64(g.seg_off[seg0])) : 0;
    const int64_t lend = blockIdx.x + 1 < g.nstreams && uni64(static_cast<uint64_t>(g.streams[blockIdx.x + 1].seg0)) <
                                                            static_cast<uint64_t>(g.nseg)
                             ? static_cast<int64_t>(uni64(g.seg_off[g.streams[blockIdx.x + 1].seg0]))
                             : static_cast<int64_t>(uni64(g.total[0]));
    const uint64_t* const list = g.list + lbeg;
    const int64_t total = n > 0 ? lend - lbeg : 0;
    int64_t wbase = 0;  // list index of win[0]
    auto load_win = [&](int64_t at) {
        __syncthreads();
        for (int j = lane; j < kResolveWin; j += kWave) win[j] = at + j < total ? list[at + j] : ~0ull >> 1;
        __syncthreads();
        wbase = at;
    };
    auto entry = [&](int64_t i) -> uint64_t {  // wave-uniform
        if (i < wbase || i >= wbase + kResolveWin) load_win(i > 64 ? i - 64 : 0);
        return win[i - wbase];
    };
    load_win(0);
    int64_t s = 0, i = 0;
    uint64_t cnt = 0;
    while (s < n) {
        const int64_t lo = s + mn - 1;
        int64_t next;
        if (lo >= n) {
            next = n;
        } else {
            const int64_t hi = s + mx - 1 < n - 1 ? s + mx - 1 : n - 1;
            // advance i to the first entry >= lo, 64 entries per step
            for (;;) {
                if (i >= total) break;
                if (i < wbase || i + kWave > wbase + kResolveWin) load_win(i > 64 ? i - 64 : 0);
                const int64_t j = i + lane;
                const bool ge = j >= total || static_cast<int64_t>(win[j - wbase] & ~kTruncBit) >= lo;
                const uint64_t bal = __ballot(ge);
                if (bal) {
                    i += __builtin_ctzll(bal);
                    break;
                }
                i += kWave;
            }
            if (i > total) i = total;
            int64_t c = -1;
            if (i > 0) {
                const uint64_t e = entry(i - 1);
                if (e & kTruncBit) {  // its segment may hold unlisted candidates >= lo
                    // end (exclusive, in positions) of the coordinate segment holding entry e
                    const int64_t seg_end =
                        ((static_cast<int64_t>(e & ~kTruncBit) + off0) / kSegBytes + 1) * kSegBytes - off0;
                    if (seg_end > lo) {
                        const int64_t rh = seg_end - 1 < hi ? seg_end - 1 : hi;
                        const int64_t f = scan_region(hash, abase, off0, off0 + n, lo + off0, rh + off0, lane);
                        if (f >= 0) c = f - off0;
                    }
                }
            }
            if (c < 0 && i < total) {
                const int64_t p = static_cast<int64_t>(entry(i) & ~kTruncBit);
                if (p <= hi) c = p;
            }
            if (c >= 0)
                next = c + 1;
            else if (s + mx - 1 <= n - 1)
                next = s + mx;
            else
                next = n;
        }
        if (lane == 0 && cnt < cuts_cap) cuts[cnt] = static_cast<uint64_t>(next);
        cnt++;
        s = next;
    }
    if (lane == 0) S.count[0] = cnt;
}

// Parallel chunk resolution of one stream per workgroup (1024 threads), for streams whose
// candidate list is complete (no truncated segment) and fits the node tables.  Nodes: the
// list entries 0..M-1 ("a chunk ends after p_k"), START = M (the stream start) and END.
//  A. succ(k): the node whose candidate ends the chunk after node k's cut, walking the
//     chunk rule from s = p_k + 1 (forced cuts at max size / the stream end in between are
//     counted in forced[k]; they are arithmetic in s).  Candidates are sorted: binary search.
//  B. jump tables: jump_t(k) = succ^(2^t)(k).
//  C. the chain START -> ... -> END: node d of the chain by binary lifting on d, its cut
//     index by a block prefix sum of (1 + forced), then every node writes its own cuts.
// The cut list equals the serial walk's (resolve_kernel) cut for cut.
__device__ __forceinline__ uint32_t lower_bound_pos(const uint64_t* list, uint32_t m, int64_t v) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (static_cast<int64_t>(list[mid]) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(1024) void resolve_par_kernel(LongArgs g, int64_t mn, int64_t mx) {
    __shared__ uint32_t s_flag;
    __shared__ uint64_t s_wsum[16];
    __shared__ uint64_t s_carry;
    __shared__ uint64_t s_depth;
    const uint32_t j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const LongStream& S = g.streams[j];
    const int64_t n = S.n;
    const int64_t seg0 = S.seg0;
    const int64_t lbeg = seg0 < g.nseg ? static_cast<int64_t>(g.seg_off[seg0]) : 0;
    const int64_t lend = j + 1 < g.nstreams && static_cast<uint64_t>(g.streams[j + 1].seg0) < static_cast<uint64_t>(g.nseg)
                             ? static_cast<int64_t>(g.seg_off[g.streams[j + 1].seg0])
                             : static_cast<int64_t>(g.total[0]);
    const uint32_t M = n > 0 ? static_cast<uint32_t>(lend - lbeg) : 0u;
    const uint64_t nb = static_cast<uint64_t>(lbeg) + 2ull * j;  // this stream's node base
    const uint64_t* list = g.list + lbeg;
    if (tid == 0) s_flag = nb + M + 2 > g.node_cap ? 1u : 0u;
    __syncthreads();
    for (uint32_t k = tid; k < M && !s_flag; k += 1024)
        if (list[k] & kTruncBit) s_flag = 1u;  // benign race: any writer stores 1
    __syncthreads();
    if (s_flag) {
        if (tid == 0) g.serial[j] = 1u;
        return;
    }
    if (tid == 0) g.serial[j] = 0u;
    const uint32_t START = M, END = M + 1;
    uint32_t* J0 = g.jump + nb;
    uint32_t* F = g.forced + nb;
    for (uint32_t k = tid; k <= END; k += 1024) {  // A
        uint32_t sc = END, f = 0;
        if (k != END) {
            int64_t s = k == START ? 0 : static_cast<int64_t>(list[k]) + 1;
            while (s < n) {
                const int64_t lo = s + mn - 1;
                if (lo >= n) {  // the last chunk [s, n)
                    f++;
                    break;
                }
                const int64_t hi = s + mx - 1 < n - 1 ? s + mx - 1 : n - 1;
                const uint32_t q = lower_bound_pos(list, M, lo);
                if (q < M && static_cast<int64_t>(list[q]) <= hi) {
                    sc = q;
                    break;
                }
                f++;  // forced cut at s + mx, or at the stream end
                if (s + mx - 1 <= n - 1) s += mx;
                else break;
            }
        }
        J0[k] = sc;
        F[k] = f;
    }
    __syncthreads();
    const uint64_t stride = g.node_cap;
    for (uint32_t t = 1; t < g.levels; t++) {  // B
        const uint32_t* Jp = g.jump + (t - 1) * stride + nb;
        uint32_t* Jt = g.jump + t * stride + nb;
        for (uint32_t k = tid; k <= END; k += 1024) Jt[k] = Jp[Jp[k]];
        __syncthreads();
    }
    if (tid == 0) {  // chain length: START's depth (number of candidate nodes on the chain)
        uint32_t cur = START;
        uint64_t d = 0;
        for (int t = static_cast<int>(g.levels) - 1; t >= 0; t--) {
            const uint32_t nx = g.jump[static_cast<uint64_t>(t) * stride + nb + cur];
            if (nx != END) {
                cur = nx;
                d += 1ull << t;
            }
        }
        s_depth = d;
        s_carry = 0;
    }
    __syncthreads();
    const uint64_t D = s_depth;  // chain nodes d = 0 (START) .. D
    uint64_t* const cuts = S.cuts;
    const uint64_t cap = S.cuts_cap;
    for (uint64_t base = 0; base <= D; base += 1024) {  // C
        const uint64_t d = base + static_cast<uint64_t>(tid);
        const bool valid = d <= D;
        uint32_t node = START;
        if (valid)
            for (uint32_t t = 0; t < g.levels; t++)
                if ((d >> t) & 1) node = g.jump[static_cast<uint64_t>(t) * stride + nb + node];
        const uint64_t wgt = valid ? F[node] + (d > 0 ? 1u : 0u) : 0u;
        uint64_t incl = wgt;
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wsum[w] = incl;
        __syncthreads();
        uint64_t pre = s_carry;
        for (int k = 0; k < w; k++) pre += s_wsum[k];
        uint64_t idx = pre + incl - wgt;
        if (valid) {
            int64_t s = 0;
            if (d > 0) {
                s = static_cast<int64_t>(list[node]) + 1;
                if (idx < cap) cuts[idx] = static_cast<uint64_t>(s);
                idx++;
            }
            for (uint32_t r = 0; r < F[node]; r++) {
                const int64_t next = s + mn - 1 >= n ? n : (s + mx - 1 <= n - 1 ? s + mx : n);
                if (idx < cap) cuts[idx] = static_cast<uint64_t>(next);
                idx++;
                s = next;
            }
        }
        __syncthreads();
        if (tid == 1023) {
            uint64_t tot = s_carry;
            for (int k = 0; k < 16; k++) tot += s_wsum[k];
            s_carry = tot;
        }
        __syncthreads();
    }
    if (tid == 0) S.count[0] = s_carry;
}

// Test support (kcdc_test_occupy): hold `nwg` CUs -- one workgroup each, all of the CU's
// LDS -- for `us` microseconds of the 100 MHz constant clock, then exit (bounded).
__global__ __launch_bounds__(64) void occupy_kernel(uint64_t ticks, uint32_t* sink) {
    extern __shared__ uint32_t hold[];
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t x = threadIdx.x;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) {
        __builtin_amdgcn_s_sleep(127);
        x = x * 1664525u + 1013904223u;
    }
    hold[threadIdx.x] = x;
    __syncthreads();
    if (hold[(threadIdx.x + 1) & 63] == 0x12345678u) sink[0] = x;  // keeps the loop and the LDS live
}

}  // namespace dev
}  // namespace kcdc
