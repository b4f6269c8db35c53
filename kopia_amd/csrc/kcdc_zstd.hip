// zstd decoding on the device: the read path's Decompress for the four zstd* compressors
// (compressor_zstd.go:73-91: verifyCompressionHeader, then zstd.NewReader; called per content by
// committed_read_manager.go:336).
//
// A zstd frame can be indexed: every block header carries the block's size, a block's literals and
// sequences decode without looking at the window, and only the execution of the sequences is
// ordered within a content.  So the passes are
//   scan      one workgroup: each content's literal room, sequence room and descriptor room by
//             prefix over the caps, the regions' places and the extra descriptors' equal share
//             (zstd_scan_kernel<kScanRooms>)
//   index     a thread per content: header ID, frame headers, the hop over the block headers; a
//             32-byte descriptor per block and per frame, the carriers of Treeless and Repeat_Mode
//             tables, the stored checksums, the content's status (zstd_index_kernel over
//             zsf::index_content)
//   prefix    descriptors per content -> the global block list (zstd_scan_kernel<kScanBlocks>)
//   entropy   persistent waves, a compressed block at a time by ticket over the global list: the
//             Huffman and FSE tables in LDS (from the carrier's description where the mode says
//             so), the literals into the literal room with the streams of a block on lanes 0..3,
//             the sequences into 12-byte records (zstd_entropy_kernel over zsf::entropy_block)
//   execute   persistent waves, a content at a time by ticket: raw blocks copied, RLE blocks
//             filled, sequences executed in batches of kZstdBatch with lanes mapped to the batch's
//             output bytes (zstd_execute_kernel over zsf::execute_content)
//   checksum  a wave per content: XXH64 of every flagged frame, the four accumulators on lanes 0..3
//             (zstd_checksum_kernel)
//   final     d_out_lens (zstd_final_kernel)
// No wave waits for another: the passes are ordered by kernel boundaries and work is handed out by
// tickets alone.  LDS: the entropy wave's context and its held arguments, 10,232 bytes: 16 single-wave
// workgroups per CU.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kcdc_internal.h"
#include "kcdc_wave.h"
#include "kcdc_zstd_format.h"

namespace kcdc {
namespace zsdev {

using zsf::Desc;
using zsf::SeqRec;

constexpr uint32_t kWaves = 256u * 16u;  // the persistent grids: 16 waves for each of 256 CUs

struct Info {  // at the workspace's start; written by the scan pass
    uint32_t ticket_entropy, ticket_execute;
    uint32_t fits, pad;
    uint64_t seq_off, lit_off, desc_off;  // the regions' places in the workspace
    uint64_t max_desc, extra;             // descriptors the workspace holds; the extra ones per content
};

struct ZsArgs {
    const uint8_t* in;
    const uint64_t* in_offs;
    const uint64_t* in_lens;
    uint8_t* out;
    const uint64_t* out_offs;
    const uint64_t* out_caps;
    uint64_t* out_lens;
    int32_t* status;
    uint8_t* work;
    uint64_t work_bytes;
    Info* info;
    uint64_t* litb;   // [n + 1]: literal room prefix (bytes)
    uint64_t* seqb;   // [n + 1]: sequence room prefix (records)
    uint64_t* qb;     // [n + 1]: descriptor quota prefix
    uint64_t* gb;     // [n + 1]: descriptors per content, then their exclusive prefix; [n] the total
    uint32_t* total;  // [n]: decoded bytes
    uint64_t fixed;   // bytes of the workspace before the regions
    uint32_t n;
    uint32_t header_id;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t cap32(uint64_t cap) { return cap > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(cap); }

constexpr int kScanRooms = 0, kScanBlocks = 1;
// Exclusive prefixes over the contents by one workgroup (the shape of decode_scan_kernel): thread t
// sums a run of contents, the runs' sums are scanned in LDS.  kScanRooms: cap bytes of literal
// room, cap / 3 + 1 sequence records and 4 + cap / 1 KiB descriptors per content, then the regions
// and the tickets' zeros; kScanBlocks: gb in place.
template <int Mode>
__global__ __launch_bounds__(1024) void zstd_scan_kernel(ZsArgs a) {
    __shared__ uint64_t part[3][1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (a.n + 1023u) / 1024u;
    const uint32_t lo = min(a.n, t * per), hi = min(a.n, lo + per);
    constexpr int kSums = Mode == kScanRooms ? 3 : 1;
    auto value = [&](uint32_t c, int k) -> uint64_t {
        if (Mode == kScanBlocks) return a.gb[c];
        const uint64_t cap = cap32(a.out_caps[c]);
        return k == 0 ? cap : k == 1 ? cap / 3u + 1u : zsf::kQuotaBase + (cap >> zsf::kQuotaShift);
    };
    uint64_t sum[3] = {0, 0, 0};
    for (uint32_t c = lo; c < hi; c++)
        for (int k = 0; k < kSums; k++) sum[k] += value(c, k);
    for (int k = 0; k < kSums; k++) part[k][t] = sum[k];
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        uint64_t v[3];
        for (int k = 0; k < kSums; k++) v[k] = t >= d ? part[k][t - d] : 0u;
        __syncthreads();
        for (int k = 0; k < kSums; k++) part[k][t] += v[k];
        __syncthreads();
    }
    uint64_t run[3];
    for (int k = 0; k < kSums; k++) run[k] = part[k][t] - sum[k];
    for (uint32_t c = lo; c < hi; c++) {
        if (Mode == kScanBlocks) {
            const uint64_t v = a.gb[c];
            a.gb[c] = run[0];
            run[0] += v;
        } else {
            a.litb[c] = run[0];
            a.seqb[c] = run[1];
            a.qb[c] = run[2];
            for (int k = 0; k < 3; k++) run[k] += value(c, k);
        }
    }
    if (t == 1023u) {
        if (Mode == kScanBlocks) {
            a.gb[a.n] = part[0][1023];
        } else {
            const uint64_t lits = part[0][1023], seqs = part[1][1023], quota = part[2][1023];
            a.litb[a.n] = lits;
            a.seqb[a.n] = seqs;
            a.qb[a.n] = quota;
            Info f{};
            // every cap is below 2^32 and there are fewer than 2^32 of them: no sum wraps
            f.seq_off = a.fixed;
            f.lit_off = f.seq_off + seqs * sizeof(SeqRec);
            f.desc_off = (f.lit_off + lits + 31u) & ~uint64_t(31);
            const bool fits = f.desc_off <= a.work_bytes && quota <= (a.work_bytes - f.desc_off) / sizeof(Desc) &&
                              quota <= 0x7fffffffull;
            f.fits = fits ? 1u : 0u;
            f.max_desc = fits ? (a.work_bytes - f.desc_off) / sizeof(Desc) : 0u;
            if (f.max_desc > 0x7fffffffull) f.max_desc = 0x7fffffffull;  // the entropy ticket is 32 bits
            f.extra = fits && f.max_desc > quota ? (f.max_desc - quota) / a.n : 0u;
            *a.info = f;
        }
    }
}

__device__ __forceinline__ Desc* content_desc(const ZsArgs& a, const Info& f, uint32_t c) {
    return reinterpret_cast<Desc*>(a.work + f.desc_off) + a.qb[c] + f.extra * c;
}

__global__ __launch_bounds__(64) void zstd_index_kernel(ZsArgs a) {
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.n) return;
    const Info f = *a.info;
    uint32_t count = 0;
    int32_t st = zsf::kNoMem;  // a workspace below the rule's size for these caps holds no content's rooms
    if (f.fits)
        st = zsf::index_content(a.in + a.in_offs[c], a.in_lens[c], a.header_id, cap32(a.out_caps[c]), content_desc(a, f, c),
                                a.qb[c + 1] - a.qb[c] + f.extra, &count);
    a.status[c] = st;
    a.gb[c] = st == 0 ? count : 0u;
    a.total[c] = 0;
}

// The Io of zsf::entropy_block and zsf::execute_content: one wave.
struct WaveIo {
    uint32_t l;
    __device__ uint32_t lane() const { return l; }
    __device__ uint32_t lanes() const { return 64u; }
    __device__ bool leader() const { return l == 0; }
    __device__ void sync() const {  // LDS writes of a lane before the other lanes' reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // The source of a copy may be what other lanes of this wave stored: order them before the loads
    // at workgroup scope (one CU, one vector L1), as the S2 decoder does.
    __device__ void fence() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }
    __device__ int32_t all(int32_t st) const { return __ballot(st != 0) ? zsf::kBadMsg : 0; }
    __device__ void copy(uint8_t* dst, const uint8_t* src, uint32_t len) const { compdev::wave_copy(dst, src, len, l); }
    __device__ void fill(uint8_t* dst, uint8_t v, uint32_t len) const {
        for (uint32_t k = l; k < len; k += 64u) dst[k] = v;
    }
    __device__ void match(uint8_t* dst, uint32_t len, uint32_t dist) const {  // dist bytes exist before dst
        const uint8_t* src = dst - dist;
        if (dist >= len) {
            for (uint32_t k = l; k < len; k += 64u) dst[k] = src[k];
        } else {  // periodic extension: only bytes written before this match are read
            for (uint32_t k = l; k < len; k += 64u) dst[k] = src[k % dist];
        }
    }
};

// What the two persistent kernels need of the arguments and the Info, held in LDS: read from there,
// they occupy no SGPRs between uses.
struct Held {
    const uint8_t* in;
    const uint64_t* in_offs;
    uint8_t* out;
    const uint64_t* out_offs;
    const uint64_t* out_caps;
    int32_t* status;
    uint32_t* total;
    uint8_t* work;
    uint32_t* ticket;
    const uint64_t *litb, *seqb, *qb, *gb;
    uint64_t seq_off, lit_off, desc_off, extra;
    uint32_t n;
};
__device__ __forceinline__ void hold(Held* h, const ZsArgs& a, uint32_t* ticket, uint32_t lane) {
    if (lane == 0) {
        const Info f = *a.info;
        *h = Held{a.in, a.in_offs, a.out, a.out_offs, a.out_caps, a.status, a.total, a.work, ticket, a.litb, a.seqb,
                  a.qb, a.gb, f.seq_off, f.lit_off, f.desc_off, f.extra, a.n};
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ Desc* held_desc(const Held& h, uint32_t c) {
    return reinterpret_cast<Desc*>(h.work + h.desc_off) + h.qb[c] + h.extra * c;
}

__global__ __launch_bounds__(64) void zstd_entropy_kernel(ZsArgs a) {
    __shared__ zsf::Ctx ctx;
    __shared__ Held h;
    const uint32_t lane = threadIdx.x;
    WaveIo io{lane};
    hold(&h, a, &a.info->ticket_entropy, lane);
    for (;;) {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(h.ticket, 1u);
        b = uni(b);
        if (b >= h.gb[h.n]) return;
        uint32_t lo = 0, hi = h.n;  // the block's content, by bisection of the prefix
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (h.gb[mid] <= b) lo = mid; else hi = mid;
        }
        const uint32_t c = uni(lo);
        const Desc* desc = held_desc(h, c);
        const uint32_t bi = uni(static_cast<uint32_t>(b - h.gb[c]));
        if (zsf::dget(desc[bi], zsf::kFType) != zsf::kTypeComp) continue;
        uint8_t* lit_room = h.work + h.lit_off + h.litb[c];
        SeqRec* seq_room = reinterpret_cast<SeqRec*>(h.work + h.seq_off) + h.seqb[c];
        const int32_t st = zsf::entropy_block(io, &ctx, h.in + h.in_offs[c], desc, bi, lit_room, seq_room);
        if (st != 0 && lane == 0) atomicCAS(&h.status[c], 0, st);  // a bad block marks its content
    }
}

__global__ __launch_bounds__(64) void zstd_execute_kernel(ZsArgs a) {
    __shared__ zsf::Plan plan;
    __shared__ Held h;
    const uint32_t lane = threadIdx.x;
    WaveIo io{lane};
    hold(&h, a, &a.info->ticket_execute, lane);
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(h.ticket, 1u);
        c = uni(c);
        if (c >= h.n) return;
        if (h.status[c] != 0) continue;
        const uint32_t ndesc = uni(static_cast<uint32_t>(h.gb[c + 1] - h.gb[c]));
        uint32_t total = 0;
        const int32_t st = zsf::execute_content(io, &plan, h.in + h.in_offs[c], held_desc(h, c), ndesc,
                                                h.work + h.lit_off + h.litb[c],
                                                reinterpret_cast<const SeqRec*>(h.work + h.seq_off) + h.seqb[c],
                                                h.out + h.out_offs[c], cap32(h.out_caps[c]), &total);
        if (lane == 0) {
            h.status[c] = st;
            h.total[c] = st == 0 ? total : 0u;
        }
    }
}

// XXH64 (seed 0) of p[0..len), its low 32 bits, by one wave: the four accumulators are lanes 0..3,
// each with the loads of four stripes in flight; lane 0 merges them and takes the tail.
__device__ uint32_t wave_xxh64_low(const uint8_t* p, uint32_t len, uint32_t lane) {
    const uint32_t stripes = len >> 5;
    uint64_t v = zsf::xxh_init(lane & 3u);
    if (lane < 4u) {
        const uint8_t* q = p + 8u * lane;
        uint32_t s = 0;
        for (; s + 4u <= stripes; s += 4u) {
            uint64_t w[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) w[u] = zsf::le64(q + 32u * (s + u));
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) v = zsf::xxh_round(v, w[u]);
        }
        for (; s < stripes; s++) v = zsf::xxh_round(v, zsf::le64(q + 32u * s));
    }
    const uint32_t vl = static_cast<uint32_t>(v), vh = static_cast<uint32_t>(v >> 32);
    const uint64_t v0 = (uint64_t(__shfl(vh, 0, 64)) << 32) | __shfl(vl, 0, 64);
    const uint64_t v1 = (uint64_t(__shfl(vh, 1, 64)) << 32) | __shfl(vl, 1, 64);
    const uint64_t v2 = (uint64_t(__shfl(vh, 2, 64)) << 32) | __shfl(vl, 2, 64);
    const uint64_t v3 = (uint64_t(__shfl(vh, 3, 64)) << 32) | __shfl(vl, 3, 64);
    uint32_t low = 0;
    if (lane == 0) {
        const uint64_t vs[4] = {v0, v1, v2, v3};
        low = static_cast<uint32_t>(zsf::xxh_finish(vs, p + 32u * stripes, len));
    }
    return uni(low);
}

__global__ __launch_bounds__(64) void zstd_checksum_kernel(ZsArgs a) {
    const uint32_t lane = threadIdx.x;
    const Info f = *a.info;
    for (uint32_t c = blockIdx.x; c < a.n; c += gridDim.x) {
        if (a.status[c] != 0) continue;
        const Desc* desc = content_desc(a, f, c);
        const uint32_t ndesc = uni(static_cast<uint32_t>(a.gb[c + 1] - a.gb[c]));
        const uint8_t* out = a.out + a.out_offs[c];
        bool ok = true;
        for (uint32_t base = 0; base < ndesc; base += 64u) {  // 64 descriptors at a look
            bool mine = false;
            if (base + lane < ndesc) {
                const Desc d = desc[base + lane];
                mine = zsf::dget(d, zsf::kFType) == zsf::kTypeFrame && (zsf::dget(d, zsf::kFInOff) & zsf::kFrameHasSum);
            }
            for (uint64_t m = __ballot(mine); m; m &= m - 1u) {
                const Desc d = desc[base + static_cast<uint32_t>(__builtin_ctzll(m))];
                const uint32_t at = uni(static_cast<uint32_t>(d.q[2] >> 32)), len = uni(static_cast<uint32_t>(d.q[3]));
                if (wave_xxh64_low(out + at, len, lane) != uni(static_cast<uint32_t>(d.q[1] >> 32))) ok = false;
            }
        }
        if (!ok && lane == 0) a.status[c] = zsf::kBadMsg;
    }
}

__global__ __launch_bounds__(256) void zstd_final_kernel(ZsArgs a) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < a.n) a.out_lens[c] = a.status[c] == 0 ? a.total[c] : 0u;
}

}  // namespace zsdev

namespace {
uint64_t align256z(uint64_t v) { return (v + 255u) & ~uint64_t(255); }
struct ZsWs {
    uint64_t litb, seqb, qb, gb, total, fixed;
};
ZsWs zs_ws(uint32_t n) {
    ZsWs l;
    const uint64_t arr = (uint64_t(n) + 1u) * 8u;
    l.litb = 256;  // the Info
    l.seqb = align256z(l.litb + arr);
    l.qb = align256z(l.seqb + arr);
    l.gb = align256z(l.qb + arr);
    l.total = align256z(l.gb + arr);
    l.fixed = align256z(l.total + uint64_t(n) * 4u);
    return l;
}
}  // namespace

// The fixed part, then 12 bytes per sequence record (cap / 3 + 1 per content), the literal rooms
// (cap bytes per content), and 32 bytes per descriptor (4 + cap / 1 KiB per content).
uint64_t zstd_decode_workspace_size(uint64_t total_out_cap_bytes, uint32_t nchunks) {
    const uint64_t n = nchunks;
    return zs_ws(nchunks).fixed + (total_out_cap_bytes / 3u + n) * sizeof(zsf::SeqRec) + total_out_cap_bytes + 32u +
           (zsf::kQuotaBase * n + (total_out_cap_bytes >> zsf::kQuotaShift)) * sizeof(zsf::Desc);
}

int launch_zstd_decode(uint32_t header_id, const uint8_t* d_comp, const uint64_t* d_offsets, const uint64_t* d_comp_lens,
                       uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets, const uint64_t* d_out_caps,
                       uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes, void* stream) {
    const ZsWs l = zs_ws(nchunks);
    if (work_bytes < zstd_decode_workspace_size(0, nchunks) || (reinterpret_cast<uintptr_t>(d_work) & 7u))
        return set_error(-22, "workspace too small or not 8-byte aligned (kcdc_zstd_decode_workspace_size)");
    zsdev::ZsArgs a{};
    a.in = d_comp;
    a.in_offs = d_offsets;
    a.in_lens = d_comp_lens;
    a.out = d_out;
    a.out_offs = d_out_offsets;
    a.out_caps = d_out_caps;
    a.out_lens = d_out_lens;
    a.status = d_status;
    uint8_t* w = static_cast<uint8_t*>(d_work);
    a.work = w;
    a.work_bytes = work_bytes;
    a.info = reinterpret_cast<zsdev::Info*>(w);
    a.litb = reinterpret_cast<uint64_t*>(w + l.litb);
    a.seqb = reinterpret_cast<uint64_t*>(w + l.seqb);
    a.qb = reinterpret_cast<uint64_t*>(w + l.qb);
    a.gb = reinterpret_cast<uint64_t*>(w + l.gb);
    a.total = reinterpret_cast<uint32_t*>(w + l.total);
    a.fixed = l.fixed;
    a.n = nchunks;
    a.header_id = header_id;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(zsdev::zstd_scan_kernel<zsdev::kScanRooms>, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(zsdev::zstd_index_kernel, dim3((nchunks + 63u) / 64u), dim3(64), 0, st, a);
    hipLaunchKernelGGL(zsdev::zstd_scan_kernel<zsdev::kScanBlocks>, dim3(1), dim3(1024), 0, st, a);
    // KCDC_TEST_CHUNK_GRID caps the entropy and the execute grids (the checksum grid follows the latter)
    const uint64_t descs = (work_bytes - l.fixed) / sizeof(zsf::Desc);  // no more blocks than this
    const uint32_t ewaves = cap_chunk_grid(static_cast<uint32_t>(descs < zsdev::kWaves ? (descs ? descs : 1u) : zsdev::kWaves));
    const uint32_t xwaves = cap_chunk_grid(nchunks < zsdev::kWaves ? nchunks : zsdev::kWaves);
    hipLaunchKernelGGL(zsdev::zstd_entropy_kernel, dim3(ewaves), dim3(64), 0, st, a);
    hipLaunchKernelGGL(zsdev::zstd_execute_kernel, dim3(xwaves), dim3(64), 0, st, a);
    hipLaunchKernelGGL(zsdev::zstd_checksum_kernel, dim3(xwaves), dim3(64), 0, st, a);
    hipLaunchKernelGGL(zsdev::zstd_final_kernel, dim3((nchunks + 255u) / 256u), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error(-5, std::string("zstd decode kernel launch: ") + hipGetErrorString(e));
}

}  // namespace kcdc
