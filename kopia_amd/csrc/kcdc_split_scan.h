// Splitter kernels, part 8 of 9: the small kernels around the batch launches and the streaming
// scans.  init_ring_kernel and poison_counts_kernel (before / after a pipelined launch),
// split_fixed_kernel (FIXED names: fixedSplitter.NextSplitPoint, repo/splitter/splitter_fixed.go:
// 15-26; reads no data), scan_first_cp_kernel / scan_first_batch_cp_kernel (a slice's first
// candidate, streaming handles), ServerMbox and scan_server_kernel (the resident scan server)
// and fill_prng_kernel (synthetic streams).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_hash.h"
#include "kcdc_split_feed.h"
#include "kcdc_split_queue.h"

namespace kcdc {
namespace dev {

// Before each pipelined launch: zero the queue header (tail := n) and write ring entries
// 0..n-1 = every stream's initial state; later entries get tag 0 (never a valid tag).
// Head starts at min(n, launch waves): every wave's first ticket is preassigned
// (first_ticket: w * grid + b), taken without an atomic (2048 waves hitting one counter at
// launch serialised for ~100 us).  The help slots' claim words start at zero (nothing published).
__global__ void init_ring_kernel(BatchArgs a, uint32_t nslots, uint32_t nwaves, uint32_t spin_cap,
                                 uint32_t steal_spins) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (a.help && i < a.help_waves) *help_claim(a, i) = 0ull;  // help slot i: nothing published
    if (a.help && i < (a.help_waves + 31u) / 32u) help_bits(a)[i] = 0u;
    if (i < kQHeaderBytes / 4)  // (workgroup flags kQFlags.. start at 0: none has started)
        a.queue[i] = i == static_cast<uint32_t>(kQHT) + 1u ? a.nstreams  // tail = n
                   : i == static_cast<uint32_t>(kQHT) ? (nwaves < a.nstreams ? nwaves : a.nstreams)
                   : i == static_cast<uint32_t>(kQCfg) ? spin_cap
                   : i == static_cast<uint32_t>(kQCfg) + 1u ? steal_spins
                                                      : 0u;
    // Every count starts as KCDC_COUNT_FAILED and is overwritten when its stream finishes: a
    // launch that loses a stream (a wave gave up waiting) can never report it as split.
    if (i < a.nstreams) a.counts[i] = ~0ull;
    if (i >= nslots * 8u) return;
    const uint32_t e = i >> 3, g = i & 7u;
    u32x4 v = {0, 0, 0, 0};
    if (e < a.nstreams && g < static_cast<uint32_t>(kPEntryLanes)) {
        const uint64_t p = reinterpret_cast<uint64_t>(a.ptrs[e]);
        const uint64_t cb = a.cut_base[e];
        const uint64_t cend = cut_end_of(a, e);
        const uint64_t w = g == 0 ? 0ull                           // cnt
                         : g == 1 ? (a.starts ? a.starts[e] : 0ull)  // s
                         : g == 2 ? static_cast<uint64_t>(resume_ct(a, e, a.starts ? static_cast<int64_t>(a.starts[e]) : 0,
                                                                     static_cast<int64_t>(a.lens[e]),
                                                                     static_cast<int64_t>(p & 15u)))  // ct (-1: not set up)
                         : g == 3 ? p
                         : g == 4 ? a.lens[e]
                         : g == 5 ? cb
                         : g == 6 ? (cend > cb ? cend - cb : 0ull)
                                  : 0ull;                          // aux 0, epoch 0
        v = pgranule(e + 1u, w, g == 0 ? e : 0u);
    }
    *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(a.ring) + static_cast<size_t>(e) * kPEntryStride + 16 * g) = v;
}

// Test hook (KCDC_TEST_FORCE_ERROR): mark a finished launch as failed.
__global__ void poison_counts_kernel(BatchArgs a) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nstreams; i += gridDim.x * blockDim.x)
        a.counts[i] = ~0ull;
}

// FIXED-*: cuts every chunk length (splitter_fixed.go:15-26); reads no data.
__global__ void split_fixed_kernel(BatchArgs a) {
    const uint32_t sid = blockIdx.x;
    if (sid >= a.nstreams) return;
    const uint64_t n = a.lens[sid];
    const uint64_t cb = a.cut_base[sid];
    const uint64_t cend = cut_end_of(a, sid);
    const uint64_t cap = cend > cb ? cend - cb : 0;
    const uint64_t L = a.min_size;
    const uint64_t full = n / L;
    const uint64_t cnt = full + (n % L ? 1 : 0);
    for (uint64_t k = threadIdx.x; k < cnt && k < cap; k += blockDim.x) a.cuts[cb + k] = k < full ? (k + 1) * L : n;
    if (threadIdx.x == 0) a.counts[sid] = cnt;
}

// Streaming-handle scans: the first candidate in [lo, hi] of one request, a slice of `len` bytes
// (64 bytes of history first) in mapped host staging.  Copy, then scan, one 8-wave workgroup per
// request: the bytes are copied into device scratch with 8 16-byte PCIe reads in flight per
// thread (a load-store loop left one read per thread outstanding and cost ~2 us per 8 KiB), then
// 8 waves scan 8 sub-ranges of [lo, hi] and the smallest first candidate wins.  One wave reading
// 64 KiB of host memory itself was PCIe-latency bound (41 us per private scan, 54 us per group
// launch).  Called by every thread of the workgroup; between two calls in one kernel the caller
// puts a barrier (the per-wave results are rewritten).
constexpr int kScanWaves = 8;  // 64 KiB of PCIe reads in flight; 2 waves per SIMD: its kernels need up to 253
                               // VGPRs (`make asm`, build/asm/resource.txt), so 1,024 threads would spill
template <int KIND>
__device__ __forceinline__ int64_t scan_request_cp(HashSmem<KIND>& sm, const BatchArgs& a, const uint8_t* src,
                                                   uint8_t* scr, int64_t len, int64_t lo, int64_t hi) {
    __shared__ int64_t wf[kScanWaves];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    constexpr int kIn = 8;
    constexpr int64_t kT = kScanWaves * kWave;
    const int64_t n16 = len >> 4;
    const u32x4* s16 = reinterpret_cast<const u32x4*>(src);
    u32x4* d16 = reinterpret_cast<u32x4*>(scr);
    for (int64_t b = 0; b < n16; b += kIn * kT) {
        u32x4 v[kIn];
#pragma unroll
        for (int k = 0; k < kIn; k++) {
            const int64_t i = b + k * kT + threadIdx.x;
            if (i < n16) v[k] = __builtin_nontemporal_load(s16 + i);
        }
#pragma unroll
        for (int k = 0; k < kIn; k++) {
            const int64_t i = b + k * kT + threadIdx.x;
            if (i < n16) d16[i] = v[k];
        }
    }
    for (int64_t i = (n16 << 4) + threadIdx.x; i < len; i += kT) scr[i] = src[i];
    __syncthreads();
    asm volatile("buffer_inv sc0" ::: "memory");  // this CU's L1 may hold an earlier request's lines
    const auto hash = make_hash<KIND>(sm, a, lane);
    const int64_t span = hi - lo + 1, per = ((span + kScanWaves - 1) / kScanWaves + 63) & ~int64_t(63);
    const int64_t mlo = lo + per * w, mhi = mlo + per - 1 < hi ? mlo + per - 1 : hi;
    const int64_t f = mlo <= mhi ? scan_region(hash, scr, 0, len, mlo, mhi, lane) : -1;
    if (lane == 0) wf[w] = f;
    __syncthreads();
    int64_t best = -1;
    for (int k = 0; k < kScanWaves; k++)
        if (wf[k] >= 0 && (best < 0 || wf[k] < best)) best = wf[k];
    return best;
}

template <int KIND>
__global__ __launch_bounds__(kScanWaves * kWave) void scan_first_cp_kernel(BatchArgs a, const uint8_t* buf, int64_t len,
                                                                           int64_t lo, int64_t hi, int64_t* out,
                                                                           uint8_t* scratch) {
    __shared__ HashSmem<KIND> sm;
    fill_tables<KIND>(sm, a);
    const int64_t f = scan_request_cp<KIND>(sm, a, buf, scratch, len, lo, hi);
    if (threadIdx.x == 0) out[0] = f;
}

template <int KIND>
__global__ __launch_bounds__(kScanWaves * kWave) void scan_first_batch_cp_kernel(BatchArgs a, const uint8_t* base,
                                                                                 const ScanReq* reqs, int64_t* out,
                                                                                 uint8_t* scratch) {
    __shared__ HashSmem<KIND> sm;
    fill_tables<KIND>(sm, a);
    const ScanReq& r = reqs[blockIdx.x];
    const uint64_t off = uni64(r.off);
    const int64_t len = static_cast<int64_t>(uni64(static_cast<uint64_t>(r.len)));
    const int64_t lo = static_cast<int64_t>(uni64(static_cast<uint64_t>(r.lo)));
    const int64_t hi = static_cast<int64_t>(uni64(static_cast<uint64_t>(r.hi)));
    const int64_t f = scan_request_cp<KIND>(sm, a, base + off, scratch + off, len, lo, hi);
    if (threadIdx.x == 0) out[blockIdx.x] = f;
}

// Resident scan server for private streaming handles (kcdc_splitter_next): one workgroup
// stays on the GPU while handles are busy and takes requests from a mailbox in fine-grained
// (coherent) host memory, so a NextSplitPoint pays no kernel launch and no table fill.
// Each request is one scan_request_cp.  The kernel exits after kSrvIdle ticks without a
// request or kSrvLife ticks in total (s_memrealtime, 100 MHz); the host relaunches it when
// needed.
struct ServerMbox {
    uint64_t req_seq;  // host: incremented after the fields below are written
    uint64_t pad0[7];
    uint64_t src;      // device-visible address of the slice (history || bytes)
    int64_t len, lo, hi;
    uint64_t pad1[4];
    uint64_t done_seq;  // device: the request served, after `result`
    int64_t result;
    uint64_t pad2[6];
};
constexpr uint64_t kSrvIdle = 200000;     // 2 ms
constexpr uint64_t kSrvLife = 20000000;   // 200 ms: every server kernel is bounded

template <int KIND>
__global__ __launch_bounds__(kScanWaves * kWave) void scan_server_kernel(BatchArgs a, ServerMbox* mb, uint8_t* scratch,
                                                                         uint64_t served) {
    __shared__ HashSmem<KIND> sm;
    __shared__ uint64_t cmd[5];
    fill_tables<KIND>(sm, a);
    const uint64_t t0 = wall_clock64();
    uint64_t last = t0;
    for (;;) {
        if (threadIdx.x == 0) {
            uint64_t sq = served;
            for (;;) {
                // relaxed: an acquire at system scope invalidates the L2 on every poll.  The
                // mailbox and the staging are fine-grained host memory (never cached), and the
                // loads below issue only after this loop has exited.
                sq = __hip_atomic_load(&mb->req_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (sq != served) break;
                const uint64_t now = wall_clock64();
                if (now - last > kSrvIdle || now - t0 > kSrvLife) break;
                __builtin_amdgcn_s_sleep(1);
            }
            cmd[0] = sq;
            if (sq != served) {
                cmd[1] = __hip_atomic_load(&mb->src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                cmd[2] = static_cast<uint64_t>(__hip_atomic_load(&mb->len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
                cmd[3] = static_cast<uint64_t>(__hip_atomic_load(&mb->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
                cmd[4] = static_cast<uint64_t>(__hip_atomic_load(&mb->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
            }
        }
        __syncthreads();
        const uint64_t sq = cmd[0];
        if (sq == served) break;  // idle or lifetime: every thread leaves together
        const uint8_t* src = reinterpret_cast<const uint8_t*>(cmd[1]);
        const int64_t len = static_cast<int64_t>(cmd[2]), lo = static_cast<int64_t>(cmd[3]),
                      hi = static_cast<int64_t>(cmd[4]);
        // One system-scope acquire per request (not per poll): no line of the staging, which
        // the host rewrites between requests, may be served from a cache.  (The staging is
        // 256-byte aligned; len <= the scratch.)
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        // Every reader of the scratch is a wave of this workgroup: scan_request_cp invalidates
        // just this CU's vector L1 after its copy (an agent-scope fence would also write back
        // and invalidate the L2 on every request).
        const int64_t best = scan_request_cp<KIND>(sm, a, src, scratch, len, lo, hi);
        if (threadIdx.x == 0) {
            // result, then (after it has completed) the sequence number the host waits for; a
            // release at system scope would write back the whole L2 first
            __hip_atomic_store(&mb->result, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(&mb->done_seq, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        served = sq;
        last = wall_clock64();
        __syncthreads();  // thread 0 rewrites cmd[], and the next request the per-wave results
    }
}

// ------------------------------------------------------ synthetic streams
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void fill_prng_kernel(uint8_t* data, uint64_t stride, uint64_t len, uint32_t nstreams, uint64_t seed,
                                 uint64_t first_sid) {
    const uint64_t words = len >> 3;
    const uint64_t total = words * nstreams;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < total; g += step) {
        const uint64_t i = g / words, j = g - i * words;
        const uint64_t key = mix64(seed ^ mix64(first_sid + i + 0x632BE59BD9B4E019ull));
        reinterpret_cast<uint64_t*>(data + i * stride)[j] = mix64(key + (j + 1) * 0x9E3779B97F4A7C15ull);
    }
    if (len & 7) {  // tail bytes of each stream
        for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nstreams; i += step) {
            const uint64_t key = mix64(seed ^ mix64(first_sid + i + 0x632BE59BD9B4E019ull));
            const uint64_t w = mix64(key + (words + 1) * 0x9E3779B97F4A7C15ull);
            for (uint64_t b = 0; b < (len & 7); b++) data[i * stride + words * 8 + b] = static_cast<uint8_t>(w >> (8 * b));
        }
    }
}

}  // namespace dev
}  // namespace kcdc
