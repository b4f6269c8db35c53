// kcdc_pack_chunks_device: compress, seal, (ECC) and place many chunks in packs in one
// asynchronous call (maybeCompressAndEncryptDataForPacking, content_manager_lock_free.go:30-89, and
// the append of addToPackUnlocked, content_manager.go:257-353).  The byte work is the existing
// stages' (kcdc_compress.hip, kcdc_crypt.hip, kcdc_ecc.hip); this file holds the plan kernels that
// connect them on the device and the gather that moves sealed contents from their aligned staging
// slots to their dense places.  Every decision is a function of kcdc_pack_format.h.
//
//   plan0    working lengths (0 for a chunk that takes no room), the max_total_bytes check,
//            compress and staging slot offsets
//   compress into the workspace slots (skipped without a compressor)
//   plan1    keep-or-drop, the seal's source table, stored sizes, their prefix sums, the chain of
//            packs (one thread, one bisection per pack), entries and destinations
//   seal     into the staging slots; a kept content is read from its compress slot and a dropped
//            one from the caller's buffer, through offsets relative to d_data (the seal kernels
//            form d_data + offset in 64 bits and load from the sum)
//   place    ECC encode from the staging slots straight to the pack, or the gather kernel
//
// A chunk that takes no room (skipped, too long, or a refused call) runs through the stages with
// working length 0: it compresses and seals to a few bytes in its own workspace slots, the ECC
// encode gets a length at its documented limit (KCDC_EFBIG, nothing written) and the gather gets
// no part, so nothing of it reaches d_pack.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/kcdc.h"
#include "kcdc_internal.h"
#include "kcdc_pack_format.h"

namespace kcdc {
namespace packdev {
using namespace packfmt;

static_assert(sizeof(Row) == sizeof(kcdc_pack_info) && sizeof(Entry) == sizeof(kcdc_pack_entry), "ABI rows");

constexpr uint32_t kPart = 65536;  // bytes of one gather ticket

struct PlanArgs {
    uint32_t n, has_comp;
    Rule rule;
    uint64_t max_total;
    const uint8_t* data;
    const uint64_t* offs;
    const uint64_t* lens;
    const uint8_t* keep;
    uint64_t *scal, *wlen, *comp_off, *comp_len, *stage_off, *seal_off, *seal_len, *E, *C, *dst_off, *aux;
    uint32_t* comp_ids;
    const uint8_t* comp_area;
    const uint8_t* stage_area;
    uint8_t* pack;
    uint64_t pack_cap;
    Entry* entries;
    Row* rows;
    uint64_t rows_cap;
    uint64_t* totals;
};

__device__ __forceinline__ int32_t status_of(const PlanArgs& a, uint32_t i) {
    return chunk_status(a.lens[i], a.keep ? a.keep[i] != 0 : true);
}

__global__ void init_kernel(uint64_t* scal) {
    if (threadIdx.x < kScalars) scal[threadIdx.x] = 0;
}

// working lengths and their sum
__global__ __launch_bounds__(256) void plan0_lens_kernel(PlanArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint64_t w = 0;
    if (i < a.n) {
        w = status_of(a, i) == kPacked ? a.lens[i] : 0;
        a.wlen[i] = w;
    }
    unsigned long long s = w;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63u) == 0 && s) atomicAdd(reinterpret_cast<unsigned long long*>(a.scal), s);
}

// the max_total_bytes check; slot sizes (scanned in place afterwards)
__global__ __launch_bounds__(256) void plan0_slots_kernel(PlanArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool refuse = a.scal[0] > a.max_total;
    if (i == 0 && refuse) a.scal[1] = static_cast<uint64_t>(static_cast<int64_t>(kEnomem));
    if (i >= a.n) return;
    uint64_t w = a.wlen[i];
    if (refuse) a.wlen[i] = w = 0;
    a.comp_off[i] = compress_bound(w);
    a.stage_off[i] = align_up(w + kSealOverhead, 4);
}

// Exclusive prefix sums of v[0..n) in place; v[n] = the total.  One workgroup.
__global__ __launch_bounds__(1024) void scan_kernel(uint32_t n, uint64_t* v) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t b = static_cast<uint64_t>(n) * t / 1024u, e = static_cast<uint64_t>(n) * (t + 1) / 1024u;
    uint64_t s = 0;
    for (uint64_t i = b; i < e; i++) s += v[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
        const uint64_t x = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint64_t i = b; i < e; i++) {
        const uint64_t x = v[i];
        v[i] = run;
        run += x;
    }
    if (t == 1023u) v[n] = run;
}

// keep-or-drop, the seal's source and length, the stored size
__global__ __launch_bounds__(256) void plan1_sizes_kernel(PlanArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const bool room = status_of(a, i) == kPacked && a.scal[1] == 0;
    const uint64_t w = a.wlen[i];
    const uint64_t base = reinterpret_cast<uint64_t>(a.data);
    bool kept = false;
    uint64_t plain = w;
    if (room && a.has_comp) {
        const uint64_t cl = a.comp_len[i];
        kept = a.comp_ids[i] != 0 && cl != 0 && keep_compressed(cl, w);
        if (kept) plain = cl;
    }
    // offsets relative to d_data, modulo 2^64: the seal adds d_data back
    a.seal_off[i] = kept   ? reinterpret_cast<uint64_t>(a.comp_area) + a.comp_off[i] - base
                    : room ? a.offs[i]
                           : reinterpret_cast<uint64_t>(a.stage_area) - base;
    a.seal_len[i] = room ? plain : 0;
    a.E[i] = room ? stored_size(a.rule, plain) : 0;
    a.C[i] = room ? 1u : 0u;
    a.entries[i].header_id = kept ? a.comp_ids[i] : 0u;
}

__global__ void plan1_chain_kernel(PlanArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const Totals t = place_chain(a.rule, a.E, a.C, a.n, a.rows, a.rows_cap, a.pack_cap);
    if (t.refuse) a.scal[1] = static_cast<uint64_t>(static_cast<int64_t>(t.refuse));
    a.scal[2] = t.packs;
    a.totals[0] = t.packs;
    a.totals[1] = t.bytes;
}

// entries, destinations, and what the placing stage is given per chunk: the ECC input length, or
// the number of gather parts
__global__ __launch_bounds__(256) void plan1_entries_kernel(PlanArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const int32_t refuse = static_cast<int32_t>(static_cast<int64_t>(a.scal[1]));
    const Entry e = place_entry(a.rule, a.E, a.rows, static_cast<uint32_t>(a.scal[2]), i, a.lens[i], status_of(a, i),
                                a.entries[i].header_id, refuse);
    a.entries[i] = e;
    const bool placed = e.status == kPacked;
    const uint64_t sealed = a.seal_len[i] + kSealOverhead;
    a.dst_off[i] = placed ? a.rows[e.pack].start + e.pack_offset : 0;
    a.aux[i] = a.rule.ecc ? (placed ? sealed : kEccNoWrite) : (placed ? (sealed + kPart - 1u) / kPart : 0u);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// n bytes from src (a multiple of 4) to dst (any alignment) by one wave: byte stores up to dst's
// first 16-byte line and after its last, 16-byte stores between, each from the four or five
// aligned source words that hold its bytes.  Only aligned source words holding a byte of
// [src, src + n) are read.
__device__ __forceinline__ void copy_part(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
    const uint32_t head = min(n, static_cast<uint32_t>((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
    if (lane < head) dst[lane] = src[lane];
    const uint32_t m = (n - head) >> 4;
    u32x4* __restrict__ dq = reinterpret_cast<u32x4*>(dst + head);
    const uint8_t* s0 = src + head;
    const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(s0) & 3u);
    const uint32_t* __restrict__ sw = reinterpret_cast<const uint32_t*>(s0 - sh);
    auto load = [&](uint32_t g, u32x4& v, uint32_t& w4) {
        const uint32_t* p = sw + 4u * g;
        __builtin_memcpy(&v, p, 16);  // 4-byte aligned: one 16-byte load
        w4 = sh ? p[4] : 0u;
    };
    auto store = [&](uint32_t g, const u32x4& v, uint32_t w4) {
        u32x4 o;
        o.x = __builtin_amdgcn_alignbit(v.y, v.x, 8u * sh);
        o.y = __builtin_amdgcn_alignbit(v.z, v.y, 8u * sh);
        o.z = __builtin_amdgcn_alignbit(v.w, v.z, 8u * sh);
        o.w = __builtin_amdgcn_alignbit(w4, v.w, 8u * sh);
        dq[g] = o;
    };
    constexpr uint32_t kU = 4;  // granules per lane in flight
    uint32_t g = lane;
    for (; g + 64u * (kU - 1u) < m; g += 64u * kU) {
        u32x4 v[kU];
        uint32_t w4[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) load(g + 64u * u, v[u], w4[u]);
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) store(g + 64u * u, v[u], w4[u]);
    }
    for (; g < m; g += 64u) {
        u32x4 v;
        uint32_t w4;
        load(g, v, w4);
        store(g, v, w4);
    }
    const uint32_t done = head + 16u * m;
    if (lane < n - done) dst[done + lane] = src[done + lane];
}

// Persistent waves; a ticket is one part (up to kPart bytes) of one sealed content.
// parts[0..n]: exclusive prefix of the contents' part counts.
__global__ __launch_bounds__(256) void gather_kernel(uint32_t n, const uint64_t* __restrict__ parts,
                                                     const uint64_t* __restrict__ seal_len,
                                                     const uint64_t* __restrict__ stage_off,
                                                     const uint64_t* __restrict__ dst_off, const uint8_t* stage,
                                                     uint8_t* pack, unsigned long long* ticket) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t total = parts[n];
    // A wave draws `batch` consecutive tickets per atomic: one while there are few parts per wave
    // (large contents: the tail stays short), up to 64 when a call holds many small contents and
    // the one ticket counter would otherwise bound the kernel.
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
    const uint64_t per = total / (waves * 8u), batch = per < 1u ? 1u : per > 64u ? 64u : per;
    for (;;) {
        unsigned long long t = 0;
        if (lane == 0) t = atomicAdd(ticket, static_cast<unsigned long long>(batch));
        t = __shfl(t, 0, 64);
        if (t >= total) return;
        const uint64_t end = t + batch < total ? t + batch : total;
        uint32_t lo = 0, hi = n;  // parts[lo] <= t < parts[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (parts[mid] <= t) lo = mid;
            else hi = mid;
        }
        for (; t < end; t++) {
            while (parts[lo + 1u] <= t) lo++;  // parts[n] = total > t
            const uint64_t piece = seal_len[lo] + kSealOverhead, off = (t - parts[lo]) * kPart;
            const uint32_t nb = static_cast<uint32_t>(piece - off < kPart ? piece - off : kPart);
            copy_part(pack + dst_off[lo] + off, stage + stage_off[lo] + off, nb, lane);
        }
    }
}

}  // namespace packdev

namespace {
int gather_grid(int* err) {
    static thread_local int cached_dev = -1, cached_grid = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return *err = set_error(-5, "hipGetDevice failed"), 0;
    if (dev != cached_dev) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            return *err = set_error(-5, "device attribute query failed"), 0;
        cached_grid = cus * 4;  // 16 waves per CU
        cached_dev = dev;
    }
    return cached_grid;
}
}  // namespace

uint64_t pack_workspace_size(const PackRun& r, uint32_t n) {
    return packfmt::ws_layout(n, r.max_total, r.compression != nullptr,
                              r.compression ? kcdc_compress_workspace_size(r.max_total, n) : 0,
                              kcdc_crypt_workspace_size(n))
        .total;
}

int launch_pack(const PackRun& r, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_lens,
                const uint8_t* d_keep, uint32_t n, const uint8_t* d_ids, uint32_t id_len, uint32_t id_stride,
                const uint8_t* d_nonces, uint8_t* d_pack, uint64_t pack_cap, void* d_entries, void* d_packs,
                uint32_t packs_cap, uint64_t* d_totals, void* d_work, uint64_t work_bytes, void* stream) {
    using namespace packdev;
    const bool comp = r.compression != nullptr;
    const uint64_t comp_ws = comp ? kcdc_compress_workspace_size(r.max_total, n) : 0;
    const uint64_t crypt_ws = kcdc_crypt_workspace_size(n);
    const Ws l = ws_layout(n, r.max_total, comp, comp_ws, crypt_ws);
    if (work_bytes < l.total) return set_error(-22, "workspace too small (kcdc_pack_bounds)");
    int err = 0;
    int grid = gather_grid(&err);
    if (err) return err;
    grid = static_cast<int>(cap_chunk_grid(static_cast<uint32_t>(grid)));  // KCDC_TEST_CHUNK_GRID

    uint8_t* w = static_cast<uint8_t*>(d_work);
    auto u64 = [&](uint64_t off) { return reinterpret_cast<uint64_t*>(w + off); };
    PlanArgs a{};
    a.n = n;
    a.has_comp = comp;
    a.rule = r.rule;
    a.max_total = r.max_total;
    a.data = d_data;
    a.offs = d_offsets;
    a.lens = d_lens;
    a.keep = d_keep;
    a.scal = u64(l.scal);
    a.wlen = u64(l.wlen);
    a.comp_off = u64(l.comp_off);
    a.comp_len = u64(l.comp_len);
    a.stage_off = u64(l.stage_off);
    a.seal_off = u64(l.seal_off);
    a.seal_len = u64(l.seal_len);
    a.E = u64(l.E);
    a.C = u64(l.C);
    a.dst_off = u64(l.dst_off);
    a.aux = u64(l.aux);
    a.comp_ids = reinterpret_cast<uint32_t*>(w + l.comp_ids);
    a.comp_area = w + l.comp_area;
    a.stage_area = w + l.stage_area;
    a.pack = d_pack;
    a.pack_cap = pack_cap;
    a.entries = static_cast<Entry*>(d_entries);
    a.rows = static_cast<Row*>(d_packs);
    a.rows_cap = packs_cap;
    a.totals = d_totals;
    int32_t* seal_st = reinterpret_cast<int32_t*>(w + l.seal_st);
    int32_t* ecc_st = reinterpret_cast<int32_t*>(w + l.ecc_st);

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 per_chunk((n + 255u) / 256u), b256(256);
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(64), 0, st, a.scal);
    hipLaunchKernelGGL(plan0_lens_kernel, per_chunk, b256, 0, st, a);
    hipLaunchKernelGGL(plan0_slots_kernel, per_chunk, b256, 0, st, a);
    if (comp) hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, n, a.comp_off);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, n, a.stage_off);
    if (comp) {
        const int rc = kcdc_compress_chunks_device(r.compression, d_data, d_offsets, a.wlen, n, w + l.comp_area,
                                                   a.comp_off, a.comp_len, a.comp_ids, w + l.comp_ws, comp_ws, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(plan1_sizes_kernel, per_chunk, b256, 0, st, a);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, n, a.E);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, n, a.C);
    hipLaunchKernelGGL(plan1_chain_kernel, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(plan1_entries_kernel, per_chunk, b256, 0, st, a);
    {
        const int rc = kcdc_encrypt_chunks_device(r.encryption, r.secret, r.secret_len, d_data, a.seal_off, a.seal_len, n,
                                                  d_ids, id_len, id_stride, d_nonces, w + l.stage_area, a.stage_off,
                                                  seal_st, w + l.crypt_ws, crypt_ws, stream);
        if (rc) return rc;
    }
    if (r.rule.ecc) {
        const int rc = kcdc_ecc_encode_chunks_device(r.ecc, r.ecc_overhead, r.ecc_max_shard, w + l.stage_area, a.stage_off,
                                                     a.aux, n, d_pack, a.dst_off, ecc_st, stream);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, n, a.aux);
        hipLaunchKernelGGL(gather_kernel, dim3(grid), b256, 0, st, n, a.aux, a.seal_len, a.stage_off, a.dst_off,
                           a.stage_area, d_pack, reinterpret_cast<unsigned long long*>(a.scal + 3));
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error(-5, std::string("pack kernel launch: ") + hipGetErrorString(e));
}

}  // namespace kcdc
