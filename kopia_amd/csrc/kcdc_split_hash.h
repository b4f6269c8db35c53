// Splitter kernels, part 2 of 9: the two rolling hashes and the region scanner.
// Reference semantics (bit-exact):
//   buzhash32Splitter.NextSplitPoint   repo/splitter/splitter_buzhash32.go:26-67
//   rabinKarp64Splitter.NextSplitPoint repo/splitter/splitter_rabinkarp64.go:26-67
// BuzShared / BuzRing (the 64x replicated table in LDS, a T-ring register for the leaving
// byte), RabinShared / Rabin (one chain per lane; the batch kernel's two-chain walk is in
// kcdc_split_rk.h) and scan_region(): 64 lanes x L bytes with per-lane 16-byte loads, used by
// the streaming scans and the long path's rescans.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"

namespace kcdc {
namespace dev {

// ------------------------------------------------------------------ hashes
// Both hashes keep `prev`: the 64 bytes before the current step (the bytes that
// leave the window while the step's bytes enter it).  block<MODE, N>(dw) rolls
// the 4N bytes of dw; byte i leaves-byte is (prev ++ dw)[i].

// buzhash32: h(p) = rotl(h(p-1),1) ^ T[b[p-64]] ^ T[b[p]]  (rollinghash Roll with
// window 64: rotl(T[leave], 64 % 32 = 0)).
struct BuzShared {
    __attribute__((aligned(16))) uint32_t tab[256 * 64];  // tab[v*64 + r] = T[v]  (64 KiB, replica r read by lane r)
};
// Fill the replicated table at kernel start: one global load per thread (two threads per
// entry, 32 replicas each, as four-dword stores rotated by entry so a store instruction's
// lanes spread over the banks).  The loop of one load per replica took 4 dependent rounds of
// L2 loads at every workgroup's start.
__device__ __forceinline__ void fill_buz_table(BuzShared& sm, const uint32_t* buz, uint32_t rot) {
    static_assert(sizeof(BuzShared) == 256 * 64 * 4, "table layout");
    for (uint32_t t = threadIdx.x; t < 512u; t += blockDim.x) {
        const uint32_t e = t & 255u, h = t >> 8;
        const uint32_t v = rotl_n(buz[e], rot);
        const u32x4 q = {v, v, v, v};
        u32x4* row = reinterpret_cast<u32x4*>(sm.tab + e * 64u + h * 32u);
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) row[(k + e) & 7u] = q;
    }
}

// buzhash32 with a register T-ring: ring[j] holds T[b] of the j-th of the 64 bytes
// before the current step, so each byte costs ONE table read (the entering byte);
// the leaving byte's value comes from the ring (first half of a 128-byte step) or
// from the step's own first half (second half), and the second half refills the
// ring in place.  No register rotation at the step boundary: ring[j] dies at byte
// j and is reborn at byte 64+j.
struct BuzRing {
    const char* tab;
    uint32_t lane4;
    uint32_t mask;
    uint32_t h;
    uint32_t ring[64];
    using State = uint32_t;
    __device__ __forceinline__ State save() const { return h; }
    __device__ __forceinline__ uint32_t look(uint32_t dwv, int k) const {
        const uint32_t a = __builtin_amdgcn_perm(dwv, lane4, 0x0c0c0000u | ((4u + k) << 8));
        return *reinterpret_cast<const uint32_t*>(tab + a);
    }
    __device__ __forceinline__ void clear() {
        h = 0;
#pragma unroll
        for (int i = 0; i < 64; i++) ring[i] = 0;
    }
    template <int MODE, int N>
    __device__ __forceinline__ uint32_t block(const uint32_t (&dw)[N]) {
        static_assert(N == 16 || N == 32, "T-ring steps are 64 or 128 bytes");
        uint32_t m = 0xFFFFFFFFu;
        if constexpr (MODE == kWarm) {  // 64 bytes on a zero history: G-recurrence warm-up
#pragma unroll
            for (int i = 0; i < 64; i++) {
                if (kSchedWindow && i % kSchedWindow == 0) __builtin_amdgcn_sched_barrier(0);
                const uint32_t t = look(dw[i >> 2], i & 3);
                h = rotl1(h) ^ t;
                ring[i] = t;
            }
            return m;
        } else if constexpr (N == 16) {
#pragma unroll
            for (int i = 0; i < 64; i++) {
                if (kSchedWindow && i % kSchedWindow == 0) __builtin_amdgcn_sched_barrier(0);
                const uint32_t t = look(dw[i >> 2], i & 3);
                h = roll3(h, ring[i], t);
                ring[i] = t;
                m = min(m, h & mask);
                if ((i & 3) == 3) asm volatile("" : "+v"(m));
            }
            return m;
        } else {
            uint32_t loc[64];
#pragma unroll
            for (int i = 0; i < 64; i++) {
                if (kSchedWindow && i % kSchedWindow == 0) __builtin_amdgcn_sched_barrier(0);
                const uint32_t t = look(dw[i >> 2], i & 3);
                h = roll3(h, ring[i], t);
                loc[i] = t;
                m = min(m, h & mask);
                if ((i & 3) == 3) asm volatile("" : "+v"(m));
            }
#pragma unroll
            for (int i = 64; i < 128; i++) {
                if (kSchedWindow && i % kSchedWindow == 0) __builtin_amdgcn_sched_barrier(0);
                const uint32_t t = look(dw[i >> 2], i & 3);
                h = roll3(h, loc[i - 64], t);
                ring[i - 64] = t;
                m = min(m, h & mask);
                if ((i & 3) == 3) asm volatile("" : "+v"(m));
            }
            return m;
        }
    }
    // A whole 128-byte step (the 128-byte-run DMA path): bytes 0..63 consume the ring and
    // fill loc, bytes 64..127 consume loc and refill the ring (loc[b] can take ring[b]'s
    // register).  Table reads run one 16-byte window ahead of the arithmetic.
    // Positions 0..62 keep their own running min m0, or-ed with hmask at the end.
    template <bool TOP>
    __device__ __forceinline__ uint32_t step128(const uint32_t (&dw)[32], uint32_t hmask) {
        constexpr int W = kLookahead;  // bytes per lookahead window
        uint32_t loc[64];
        uint32_t m = 0xFFFFFFFFu, m0 = 0xFFFFFFFFu;
        uint32_t tw[W], tn[W];
#pragma unroll
        for (int i = 0; i < W; i++) tw[i] = look(dw[i >> 2], i & 3);
#pragma unroll
        for (int w = 0; w < 128 / W; w++) {
            __builtin_amdgcn_sched_barrier(0);
            if (w < 128 / W - 1) {
#pragma unroll
                for (int i = 0; i < W; i++) tn[i] = look(dw[(W * (w + 1) + i) >> 2], i & 3);
            }
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int b = W * w + i;
                if (b < 64) {
                    h = roll3(h, ring[b], tw[i]);
                    loc[b] = tw[i];
                } else {
                    h = roll3(h, loc[b - 64], tw[i]);
                    ring[b - 64] = tw[i];
                }
                const uint32_t t = TOP ? h : h & mask;
                if (b < 63) {
                    m0 = min(m0, t);
                    if ((b & 3) == 3) asm volatile("" : "+v"(m0));
                } else {
                    m = min(m, t);
                    if ((b & 3) == 3) asm volatile("" : "+v"(m));
                }
            }
#pragma unroll
            for (int i = 0; i < W; i++) tw[i] = tn[i];
        }
        return min(m, m0 | hmask);
    }
    // The rare exact re-run of a step whose running test passed: the first position in [lo, hi]
    // that is a candidate, else 4N.  16-byte windows (the arrays shift by four dwords per window),
    // done as soon as every lane running it has found its candidate.  (Round 5: the arrays shifted
    // by one dword every 4 bytes, ~3,800 VALU per re-run, and at 128K averages 6 % of wave-steps
    // re-run.  Fully unrolled instead, the long-path scan kernel spilled.)
    template <int N>
    __device__ __forceinline__ uint32_t exact(State st0, const uint32_t (&prv)[16], const uint32_t (&dw)[N], int lo,
                                              int hi) const {
        static_assert(N % 4 == 0, "16-byte windows");
        uint32_t e[N], o[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            e[j] = dw[j];
            o[j] = j < 16 ? prv[j] : dw[j - 16];
        }
        uint32_t hh = st0, first = 4 * N;
#pragma unroll 1
        for (int w = 0; w < N / 4; w++) {
#pragma unroll
            for (int b = 0; b < 16; b++) {
                hh = rotl1(hh) ^ look(o[b >> 2], b & 3) ^ look(e[b >> 2], b & 3);
                const int i = 16 * w + b;
                if (first == 4 * N && (hh & mask) == 0 && i >= lo && i <= hi) first = static_cast<uint32_t>(i);
            }
            if (__ballot(first == 4 * N) == 0) break;
#pragma unroll
            for (int k = 0; k < N - 4; k++) {
                e[k] = e[k + 4];
                o[k] = o[k + 4];
            }
        }
        return first;
    }
};

// rabinkarp64: v ^= out[b[p-64]]; idx = v >> shift; v = (v << 8 | b[p]) ^ mod[idx].
struct RabinShared {
    uint64_t out[256];
    uint64_t mod[256];
};

struct Rabin {
    const RabinShared* tab;
    uint32_t mask;
    uint32_t shift;
    uint64_t v;
    uint32_t prev[16];
    using State = uint64_t;
    __device__ __forceinline__ State save() const { return v; }

    __device__ __forceinline__ void clear() {
        v = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) prev[i] = 0;
    }
    __device__ __forceinline__ uint64_t roll(uint64_t x, uint32_t bo, uint32_t bi) const {
        x ^= tab->out[bo];
        const uint32_t idx = static_cast<uint32_t>(x >> shift) & 0xFFu;
        return ((x << 8) | bi) ^ tab->mod[idx];
    }
    template <int MODE, int N>
    __device__ __forceinline__ uint32_t block(const uint32_t (&dw)[N]) {
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 4 * N; i++) {
            const uint32_t bo = MODE == kWarm ? 0u : (i < 64 ? byte_at(prev, i) : byte_at(dw, i - 64));
            v = roll(v, bo, byte_at(dw, i));
            if (MODE == kFast) {
                m = min(m, static_cast<uint32_t>(v) & mask);
                if ((i & 3) == 3) asm volatile("" : "+v"(m));
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) prev[i] = dw[N - 16 + i];
        return m;
    }
    template <int N>
    __device__ __forceinline__ uint32_t exact(State st0, const uint32_t (&prv)[16], const uint32_t (&dw)[N], int lo,
                                              int hi) const {
        uint32_t e[N], o[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            e[j] = dw[j];
            o[j] = j < 16 ? prv[j] : dw[j - 16];
        }
        uint64_t vv = st0;
        uint32_t first = 4 * N;
#pragma unroll 1
        for (int j = 0; j < N; j++) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                vv = roll(vv, (o[0] >> (8 * b)) & 0xFFu, (e[0] >> (8 * b)) & 0xFFu);
                const int i = 4 * j + b;
                if (first == 4 * N && (static_cast<uint32_t>(vv) & mask) == 0 && i >= lo && i <= hi)
                    first = static_cast<uint32_t>(i);
            }
#pragma unroll
            for (int k = 0; k < N - 1; k++) {
                e[k] = e[k + 1];
                o[k] = o[k + 1];
            }
        }
        return first;
    }
};

// --------------------------------------------------------- region scanner
// First candidate coordinate in [lo, hi] (inclusive, lo <= hi), or -1.
// Wave-uniform in and out.  `H` is a prepared hash (tables + mask).
template <class H>
__device__ int64_t scan_region(H hash, const uint8_t* abase, int64_t off0, int64_t nbytes_coord, int64_t lo,
                               int64_t hi, int lane) {
    int64_t ct = lo & ~int64_t(63);
    while (ct <= hi) {
        const int64_t rem = hi - ct + 1;
        int64_t per = (rem + kWave - 1) / kWave;
        per = (per + kBlk - 1) / kBlk * kBlk;
        const int64_t L = per < kLaneMax ? per : kLaneMax;
        const int64_t tb = ct >= 64 ? ct - 64 : 0;
        const Loader ld = make_loader(abase, off0, nbytes_coord, tb);

        const int64_t c0 = ct + lane * L;
        const int nb = static_cast<int>(L / kBlk);
        int64_t found = -1;
        if (c0 <= hi) {
            uint32_t cur[kNdw], nxt[kNdw];
            {
                uint32_t w[16];
                hash.clear();
                ld.load(c0 - 64, w);
                hash.template block<kWarm>(w);  // h = hash of the 64-byte window before c0
            }
            ld.load(c0, cur);
            int k = 0;
            for (;;) {
                bool hit = false;
                typename H::State st0 = hash.save();
                for (; k < nb; k++) {
                    if (c0 + kBlk * k > hi) break;
                    if (k + 1 < nb) ld.load(c0 + kBlk * (k + 1), nxt);
                    st0 = hash.save();
                    if (hash.template block<kFast>(cur) == 0) {
                        hit = true;
                        break;
                    }
#pragma unroll
                    for (int i = 0; i < kNdw; i++) cur[i] = nxt[i];
                }
                if (!hit) break;
                // rare: re-run step k exactly (the fast pass already left the end state)
                const int64_t c = c0 + kBlk * k;
                uint32_t prv[16];
                ld.load(c - 64, prv);
                const int64_t blo = lo - c, bhi = hi - c;
                const uint32_t idx = hash.exact(st0, prv, cur, blo < 0 ? 0 : static_cast<int>(blo),
                                                bhi > kBlk - 1 ? kBlk - 1 : static_cast<int>(bhi));
                if (idx < static_cast<uint32_t>(kBlk)) {
                    found = c + idx;
                    break;
                }
                if (++k >= nb) break;
                ld.load(c0 + kBlk * k, cur);
            }
        }
        const uint64_t hit = __ballot(found >= 0);
        if (hit) {
            const int first = __builtin_ctzll(hit);
            return static_cast<int64_t>(uni64(static_cast<uint64_t>(__shfl(found, first))));
        }
        ct += kWave * L;
    }
    return -1;
}

}  // namespace dev
}  // namespace kcdc
