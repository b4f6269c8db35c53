// The content-ID set: WriteContent's dedup decision (repo/content/content_manager.go:812-842) on the
// device, between kcdc_hash_chunks_device and kcdc_pack_chunks_device.  Every decision is a function
// of kcdc_dedup_format.h; this file holds the kernels that run them and their launchers.
//
// A claim (or insert, or grow) of n IDs is five steps, each published to the next by the kernel
// boundary; no kernel polls a word another lane will write:
//   probe    one lane per ID walks its probe chain: an empty slot is taken with a CAS of a
//            reference to the caller's ID; a slot whose key equals the lane's gets atomicMin of that
//            reference, so every racing duplicate converges on the lowest index and a stored key
//            (a smaller word) beats them all.  Slot words are touched by agent-scope atomics only;
//            the keys they refer to (the caller's IDs, the key store) were complete before the
//            kernel started.
//   outcome  reads each ID's slot: d_first, d_keep, and the keep flags for the prefix sum
//   scan     exclusive prefix sums of the keep flags (tile sums, their scan, the tiles)
//   commit   a kept ID is copied to place stored + prefix of the key store and its slot rewritten
//            with the reference to that place
//   finish   the count and d_totals
// A refused call (dedupfmt::refused, from the count on the device) runs the same launches: probe,
// scan and commit return at once, outcome writes the refusal, finish leaves the count.
// probe, outcome and commit are persistent waves that draw batched tickets of 64 IDs.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/kcdc.h"
#include "kcdc_dedup_format.h"
#include "kcdc_internal.h"

namespace kcdc {
namespace dedupdev {
using namespace dedupfmt;

static_assert(kKnown == KCDC_DEDUP_KNOWN && kEnospc == KCDC_ENOSPC, "ABI constants");

struct DevWords {  // slot words on the device: agent scope, relaxed (the kernel boundaries order the rest)
    static __device__ __forceinline__ uint64_t load(const uint64_t* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
    static __device__ __forceinline__ void min(uint64_t* p, uint64_t v) {
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void store(uint64_t* p, uint64_t v) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

struct Args {
    Table t;
    Keys call;
    uint32_t n;
    const uint64_t* n_src;  // grow: the source set's count (device); else nullptr
    uint64_t max_keys;
    unsigned long long* tickets;
    uint64_t* scal;
    uint32_t *slot_of, *pos, *tile_sums;
    uint32_t ntiles;  // workgroups of the scan's tile kernels
    uint8_t* keep;
    uint32_t* first;
    uint64_t* totals;
};

__device__ __forceinline__ uint32_t ids_of(const Args& a) { return a.n_src ? static_cast<uint32_t>(*a.n_src) : a.n; }

// Persistent waves; a ticket is 64 consecutive IDs, one per lane, and a wave takes `batch` consecutive
// tickets at a time: its share of the call, up to 64.  A wave's first batch is the one of its own
// number and costs no atomic; the batches after those are drawn from the counter.  One counter word
// serves some 90 draws per microsecond, which at a ticket per draw bounded a claim of 2^20 IDs: with
// these batches a call of up to 64 tickets per wave draws nothing, and a longer one draws once per
// 4,096 IDs.
template <class F>
__device__ __forceinline__ void for_tickets(uint64_t n, unsigned long long* ticket, F f) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t total = (n + 63u) / 64u;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
    const uint64_t per = (total + waves - 1u) / waves, batch = per < 1u ? 1u : per > 64u ? 64u : per;
    const uint64_t first = waves * batch;  // tickets below this are taken by wave number
    const bool draws = first < total;
    uint64_t t = (static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * batch;
    for (;;) {
        if (t >= total) return;
        const uint64_t end = t + batch < total ? t + batch : total;
        for (; t < end; t++) {
            const uint64_t i = t * 64u + lane;
            if (i < n) f(static_cast<uint32_t>(i));
        }
        if (!draws) return;
        unsigned long long d = 0;
        if (lane == 0) d = atomicAdd(ticket, static_cast<unsigned long long>(batch));
        t = first + __shfl(d, 0, 64);
    }
}

__global__ __launch_bounds__(256) void probe_kernel(Args a) {
    const uint32_t n = ids_of(a);
    if (refused(a.scal[kStored], n, a.max_keys)) return;
    for_tickets(n, a.tickets + kTicketProbe, [&](uint32_t i) {
        a.slot_of[i] = static_cast<uint32_t>(probe_claim<DevWords>(a.t, a.call, i));
    });
}

__global__ __launch_bounds__(256) void outcome_kernel(Args a) {
    const uint32_t n = ids_of(a);
    const bool refuse = refused(a.scal[kStored], n, a.max_keys);
    for_tickets(n, a.tickets + kTicketOutcome, [&](uint32_t i) {
        const uint32_t first = refuse ? kKnown : outcome_first<DevWords>(a.t, a.slot_of[i]);
        const uint32_t keep = first == i ? 1u : 0u;
        if (!refuse) a.pos[i] = keep;
        if (a.keep) a.keep[i] = static_cast<uint8_t>(keep);
        if (a.first) a.first[i] = first;
    });
}

// ---- the prefix sum of pos[0..n): tiles of kScanTile flags, 16 per thread
constexpr uint32_t kPerThread = kScanTile / 256u;

__device__ __forceinline__ uint32_t thread_sum(const uint32_t* pos, uint64_t at, uint32_t n) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) s += at + k < n ? pos[at + k] : 0u;
    return s;
}

__global__ __launch_bounds__(256) void scan_tile_sums_kernel(Args a) {
    __shared__ uint32_t part[4];
    const uint32_t n = ids_of(a);
    if (refused(a.scal[kStored], n, a.max_keys)) return;
    uint32_t s = thread_sum(a.pos, uint64_t(blockIdx.x) * kScanTile + threadIdx.x * kPerThread, n);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.tile_sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Exclusive prefix sums of v[0..m) in place; v[m] = the total.  One workgroup.
__global__ __launch_bounds__(1024) void scan_sums_kernel(Args a) {
    __shared__ uint32_t part[1024];
    if (refused(a.scal[kStored], ids_of(a), a.max_keys)) return;
    uint32_t* v = a.tile_sums;
    const uint32_t m = a.ntiles, t = threadIdx.x;
    const uint64_t b = uint64_t(m) * t / 1024u, e = uint64_t(m) * (t + 1u) / 1024u;
    uint32_t s = 0;
    for (uint64_t i = b; i < e; i++) s += v[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
        const uint32_t x = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint64_t i = b; i < e; i++) {
        const uint32_t x = v[i];
        v[i] = run;
        run += x;
    }
    if (t == 1023u) v[m] = run;
}

__global__ __launch_bounds__(256) void scan_tiles_kernel(Args a) {
    __shared__ uint32_t part[4];
    const uint32_t n = ids_of(a);
    if (refused(a.scal[kStored], n, a.max_keys)) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t at = uint64_t(blockIdx.x) * kScanTile + threadIdx.x * kPerThread;
    const uint32_t s = thread_sum(a.pos, at, n);
    uint32_t inc = s;  // inclusive over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t x = __shfl_up(inc, off, 64);
        if (lane >= static_cast<uint32_t>(off)) inc += x;
    }
    if (lane == 63u) part[wave] = inc;
    __syncthreads();
    uint32_t run = a.tile_sums[blockIdx.x] + inc - s;
    for (uint32_t w = 0; w < wave; w++) run += part[w];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++)
        if (at + k < n) {
            const uint32_t x = a.pos[at + k];
            a.pos[at + k] = run;
            run += x;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.pos[n] = a.tile_sums[a.ntiles];
}

__global__ __launch_bounds__(256) void commit_kernel(Args a) {
    const uint32_t n = ids_of(a);
    const uint64_t stored = a.scal[kStored];
    if (refused(stored, n, a.max_keys)) return;
    for_tickets(n, a.tickets + kTicketCommit, [&](uint32_t i) {
        commit_key<DevWords>(a.t, a.call, i, a.slot_of[i], static_cast<uint32_t>(stored) + a.pos[i]);
    });
}

__global__ void finish_kernel(Args a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t n = ids_of(a);
    const uint64_t stored = a.scal[kStored];
    const bool refuse = refused(stored, n, a.max_keys);
    const uint64_t added = refuse || n == 0 ? 0u : a.pos[n];
    a.totals[0] = refuse ? static_cast<uint64_t>(static_cast<int64_t>(kEnospc)) : 0u;
    a.totals[1] = added;
    a.totals[2] = stored + added;
    a.scal[kStored] = stored + added;
}

__global__ __launch_bounds__(256) void lookup_kernel(Args a) {
    for_tickets(a.n, a.tickets + kTicketProbe, [&](uint32_t i) {
        a.keep[i] = probe_lookup<DevWords>(a.t, a.call, i) ? 1 : 0;
    });
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// slots: nslots * 8 bytes, a multiple of 16, 256-byte aligned
__global__ __launch_bounds__(256) void clear_kernel(u32x4* slots, uint64_t granules, uint64_t* scal) {
    const u32x4 ones = {~0u, ~0u, ~0u, ~0u};
    for (uint64_t g = uint64_t(blockIdx.x) * 256u + threadIdx.x; g < granules; g += uint64_t(gridDim.x) * 256u)
        slots[g] = ones;
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[kStored] = 0;
}

}  // namespace dedupdev

namespace {
using namespace dedupfmt;

dedupdev::Args set_args(const DedupSet& s) {
    const Layout l = layout(s.id_len, s.max_keys);
    dedupdev::Args a{};
    a.t = Table{reinterpret_cast<uint64_t*>(s.base + l.slots), slot_count(s.max_keys), s.base + l.store, s.id_len};
    a.max_keys = s.max_keys;
    a.tickets = reinterpret_cast<unsigned long long*>(s.base + l.tickets);
    a.scal = reinterpret_cast<uint64_t*>(s.base + l.scal);
    a.slot_of = reinterpret_cast<uint32_t*>(s.base + l.slot_of);
    a.pos = reinterpret_cast<uint32_t*>(s.base + l.pos);
    a.tile_sums = reinterpret_cast<uint32_t*>(s.base + l.tile_sums);
    return a;
}

// Workgroups of a persistent kernel over at most n IDs: no more than one ticket each would feed.
uint32_t persistent_grid(const DedupSet& s, uint64_t n) {
    const uint64_t want = (n + 255u) / 256u;
    const uint32_t g = static_cast<uint32_t>(want < s.grid ? (want ? want : 1u) : s.grid);
    return cap_chunk_grid(g);  // KCDC_TEST_CHUNK_GRID
}

int launched(hipError_t memset_rc, const char* what) {
    const hipError_t e = memset_rc != hipSuccess ? memset_rc : hipGetLastError();
    return e == hipSuccess ? 0 : set_error(-5, std::string(what) + hipGetErrorString(e));
}
}  // namespace

int dedup_launch_clear(const DedupSet& s, void* stream) {
    const dedupdev::Args a = set_args(s);
    const uint64_t granules = a.t.nslots / 2u;
    const uint64_t want = (granules + 255u) / 256u;
    hipLaunchKernelGGL(dedupdev::clear_kernel, dim3(static_cast<uint32_t>(want < s.grid ? want : s.grid)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<dedupdev::u32x4*>(a.t.slots), granules, a.scal);
    return launched(hipSuccess, "dedup clear launch: ");
}

int dedup_launch_claim(const DedupSet& s, const DedupSet* from, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride,
                       uint32_t n, uint8_t* d_keep, uint32_t* d_first, uint64_t* d_totals, void* stream) {
    using namespace dedupdev;
    Args a = set_args(s);
    uint64_t bound = n;  // the most IDs the call can have
    if (from) {
        const Args f = set_args(*from);
        a.call = store_keys(f.t);
        a.n_src = f.scal + kStored;
        bound = from->max_keys;
    } else {
        a.call = Keys{d_ids, id_stride, s.id_len, prefix, 0};
        a.n = n;
    }
    a.keep = d_keep;
    a.first = d_first;
    a.totals = d_totals;
    // the scan runs only in a call that is not refused, which has at most max_keys IDs
    a.ntiles = static_cast<uint32_t>(scan_tiles(bound < s.max_keys ? bound : s.max_keys));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t m = hipMemsetAsync(a.tickets, 0, kTickets * 8u, st);
    const dim3 grid(persistent_grid(s, bound)), b256(256);
    hipLaunchKernelGGL(probe_kernel, grid, b256, 0, st, a);
    hipLaunchKernelGGL(outcome_kernel, grid, b256, 0, st, a);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(a.ntiles), b256, 0, st, a);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(a.ntiles), b256, 0, st, a);
    hipLaunchKernelGGL(commit_kernel, grid, b256, 0, st, a);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, st, a);
    return launched(m, "dedup claim launch: ");
}

int dedup_launch_lookup(const DedupSet& s, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride, uint32_t n,
                        uint8_t* d_known, void* stream) {
    using namespace dedupdev;
    Args a = set_args(s);
    a.call = Keys{d_ids, id_stride, s.id_len, prefix, 0};
    a.n = n;
    a.keep = d_known;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t m = hipMemsetAsync(a.tickets, 0, kTickets * 8u, st);
    hipLaunchKernelGGL(lookup_kernel, dim3(persistent_grid(s, n)), dim3(256), 0, st, a);
    return launched(m, "dedup lookup launch: ");
}

}  // namespace kcdc
