// Content decompression on the device: the read path's counterpart of kcdc_compress.hip for the
// s2-* compressors (compressor_s2.go:73-90: Decompress = verifyCompressionHeader, then
// s2.NewReader; called per content by committed_read_manager.go:336).
//
// Every data chunk of the S2 framing is an independent, CRC-checked block, so a batch of contents
// is a list of independent block decodes:
//   quota   descriptor room per content: 1 + cap / 16 KiB, their prefix, and an equal share of
//           whatever the workspace holds beyond that (decode_scan_kernel<kScanQuota>)
//   index   one thread per content: header ID, stream identifier, the hop over the framing chunks;
//           a descriptor per data chunk, the content's status and decoded length
//           (decode_index_kernel; the walk itself is s2f::index_content)
//   prefix  blocks per content -> the global block list (decode_scan_kernel<kScanBlocks>); the
//           total stays on the device
//   decode  persistent waves, one block at a time by ticket: a wave-uniform element walk over a
//           256-byte register window of the input, literals copied input -> output, matches
//           output -> output by the whole wave (decode_blocks_kernel)
//   crc     CRC-32C of every decoded block against its stored masked value, in 32 KiB pieces
//           counted back from the block's end and combined by shifts (decode_crc_kernel)
//   final   d_out_lens (decode_final_kernel)
// A block that fails marks its content's status with an atomic; nothing is written outside a
// block's own output range, which the index pass has placed inside the content's slot.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kcdc_internal.h"
#include "kcdc_s2_format.h"
#include "kcdc_wave.h"

namespace kcdc {
namespace decdev {

using compdev::kCrc32cPoly;
using compdev::multmodp;
using s2f::Desc;

using compdev::kPiece;
using compdev::piece_crc;
constexpr uint32_t kCrcWaves = 4;
constexpr uint32_t kDecodeWaves = 256u * 16u;  // the persistent grid: 16 waves for each of 256 CUs

struct DecArgs {
    const uint8_t* in;
    const uint64_t* in_offs;
    const uint64_t* in_lens;
    uint8_t* out;
    const uint64_t* out_offs;
    const uint64_t* out_caps;
    uint64_t* out_lens;
    int32_t* status;
    uint64_t* qbase;    // [n + 2]: descriptor quota prefix; [n] their sum, [n + 1] the extra share per content
    uint64_t* gbase;    // [n + 1]: blocks per content, then their exclusive prefix; [n] the block total
    uint64_t* total;    // [n]: decoded bytes per content
    uint32_t* ticket;   // [1]: next block of the decode pass
    Desc* desc;         // [max_desc]
    uint64_t max_desc;
    uint32_t n;
    uint32_t header_id;
    uint32_t x2nc[32];  // x^(2^k) mod the CRC-32C polynomial
};

constexpr int kScanQuota = 0, kScanBlocks = 1;
// Exclusive prefix over the contents by one workgroup: thread t sums a run of contents, the runs'
// sums are scanned in LDS.  kScanQuota: 1 + cap / 16 KiB into qbase (and the extra share, and the
// decode ticket's zero); kScanBlocks: gbase in place.
template <int Mode>
__global__ __launch_bounds__(1024) void decode_scan_kernel(DecArgs a) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (a.n + 1023u) / 1024u;
    const uint32_t lo = min(a.n, t * per), hi = min(a.n, lo + per);
    auto value = [&](uint32_t c) -> uint64_t {
        return Mode == kScanQuota ? 1u + (a.out_caps[c] >> s2f::kQuotaShift) : a.gbase[c];
    };
    uint64_t sum = 0;
    for (uint32_t c = lo; c < hi; c++) sum += value(c);
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    uint64_t* dst = Mode == kScanQuota ? a.qbase : a.gbase;
    for (uint32_t c = lo; c < hi; c++) {
        const uint64_t v = value(c);
        dst[c] = run;
        run += v;
    }
    if (t == 1023u) {
        const uint64_t all = part[1023];
        dst[a.n] = all;
        if (Mode == kScanQuota) {
            a.qbase[a.n + 1] = a.max_desc > all ? (a.max_desc - all) / a.n : 0u;
            *a.ticket = 0;
        }
    }
}

__global__ __launch_bounds__(64) void decode_index_kernel(DecArgs a) {
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.n) return;
    // the content's descriptors: [lo, lo + quota) of the list, cut off at the list's end
    const uint64_t extra = a.qbase[a.n + 1];
    uint64_t lo = a.qbase[c] + extra * c;
    uint64_t quota = a.qbase[c + 1] - a.qbase[c] + extra;
    if (lo > a.max_desc) lo = a.max_desc;
    if (quota > a.max_desc - lo) quota = a.max_desc - lo;
    uint32_t count = 0;
    uint64_t total = 0;
    const int32_t st = s2f::index_content(a.in + a.in_offs[c], a.in_lens[c], a.header_id, a.out_caps[c], c,
                                          a.in_offs[c], a.out_offs[c], a.desc + lo, quota, &count, &total);
    a.status[c] = st;
    a.gbase[c] = st == 0 ? count : 0u;
    a.total[c] = total;
}

// Block b of the global list: its content by bisection of the prefix, its descriptor in the
// content's own range of the list.
__device__ __forceinline__ const Desc* block_desc(const DecArgs& a, uint64_t b) {
    uint32_t lo = 0, hi = a.n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.gbase[mid] <= b) lo = mid; else hi = mid;
    }
    return a.desc + a.qbase[lo] + a.qbase[a.n + 1] * lo + (b - a.gbase[lo]);
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// One block by one wave.  The walk is wave-uniform: the input is held as a window of 64 aligned
// words, one per lane, and an element's bytes are read out of it with v_readlane; the window is
// refilled when an element starts in its last two words.  Only aligned words holding a byte of
// in[0..n) are loaded.  Returns whether the block decoded to exactly `want` bytes.
__device__ bool decode_block(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t want, uint32_t lane) {
    const uint32_t al = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(in) & 3u);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(in - al);
    const uint32_t nw = (al + n + 3u) >> 2;  // aligned words holding the block
    uint32_t w0 = 0, win = lane < nw ? words[lane] : 0u;
    auto bytes_at = [&](uint32_t i) -> uint64_t {  // the 5 bytes at in[i..], little-endian
        const uint32_t p = al + i;
        uint32_t wi = p >> 2;
        if (wi - w0 > 62u) {
            w0 = wi;
            win = w0 + lane < nw ? words[w0 + lane] : 0u;
        }
        wi -= w0;
        const uint32_t l = __builtin_amdgcn_readlane(win, wi), h = __builtin_amdgcn_readlane(win, wi + 1u);
        return ((static_cast<uint64_t>(h) << 32) | l) >> (8u * (p & 3u));
    };
    uint32_t i = 0, o = 0, last_off = 0;
    {  // the block's uvarint: the index pass has checked it; the walk needs its size
        uint32_t dec = 0;
        if (s2f::uvarint(bytes_at(0), n, &dec, &i) != 0 || dec != want) return false;
    }
    while (i < n) {
        s2f::Elem e;
        if (s2f::element(bytes_at(i), n - i, o, want, last_off, &e) != 0) return false;
        const uint32_t len = uni(e.len), hdr = uni(e.hdr);
        if (!e.copy) {
            compdev::wave_copy(out + o, in + i + hdr, len, lane);
            i += hdr + len;
        } else {
            const uint32_t off = uni(e.off);
            // The source may be what the previous element's lanes stored: order this wave's stores
            // before its loads at workgroup scope (one CU, one vector L1).
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            const uint8_t* src = out + o - off;
            uint8_t* dst = out + o;
            if (off >= len) {
                for (uint32_t k = lane; k < len; k += 64u) dst[k] = src[k];
            } else {  // periodic extension: only bytes written before this element are read
                for (uint32_t k = lane; k < len; k += 64u) dst[k] = src[k % off];
            }
            last_off = off;
            i += hdr;
        }
        o += len;
    }
    return o == want;
}

__global__ __launch_bounds__(64) void decode_blocks_kernel(DecArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.gbase[a.n];
    for (;;) {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(a.ticket, 1u);
        b = uni(b);
        if (b >= total) return;
        const Desc d = *block_desc(a, b);
        const uint32_t c = d.content & ~s2f::kDescRaw;
        bool ok = true;
        if (d.content & s2f::kDescRaw)
            compdev::wave_copy(a.out + d.out_off, a.in + d.in_off, d.out_len, lane);
        else
            ok = decode_block(a.in + d.in_off, d.in_len, a.out + d.out_off, d.out_len, lane);
        if (!ok && lane == 0) atomicCAS(&a.status[c], 0, s2f::kBadMsg);
    }
}

__global__ __launch_bounds__(64 * kCrcWaves) void decode_crc_kernel(DecArgs a) {
    __shared__ uint32_t tab[256 * 32];
    compdev::crc_table_fill(tab, kCrc32cPoly, 64u * kCrcWaves);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t total = a.gbase[a.n];
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * kCrcWaves;
    for (uint64_t b = blockIdx.x * kCrcWaves + uni(threadIdx.x >> 6); b < total; b += step) {
        const Desc d = *block_desc(a, b);
        const uint8_t* p = a.out + d.out_off;
        // pieces counted back from the block's end: the first is the short one, every later one
        // shifts the running value by x^(8 * 32768) = x^(2^18)
        const uint32_t pieces = (d.out_len + kPiece - 1u) / kPiece;
        uint32_t at = 0, raw = 0;
        for (uint32_t j = 0; j < pieces; j++) {
            const uint32_t plen = j == 0 ? d.out_len - (pieces - 1u) * kPiece : kPiece;
            raw = multmodp(raw, a.x2nc[18], kCrc32cPoly) ^ piece_crc(p + at, plen, tab, a.x2nc, kCrc32cPoly, lane);
            at += plen;
        }
        const uint32_t crc = compdev::crc_finish(raw, d.out_len, a.x2nc, kCrc32cPoly);
        if (lane == 0 && s2f::mask_crc(crc) != d.crc) atomicCAS(&a.status[d.content & ~s2f::kDescRaw], 0, s2f::kBadMsg);
    }
}

__global__ __launch_bounds__(256) void decode_final_kernel(DecArgs a) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < a.n) a.out_lens[c] = a.status[c] == 0 ? a.total[c] : 0u;
}

}  // namespace decdev

namespace {
uint64_t align256d(uint64_t x) { return (x + 255u) & ~uint64_t(255); }
struct DecWs {
    uint64_t qbase, gbase, total, ticket, desc;
};
DecWs dec_ws(uint32_t n) {
    DecWs l{};
    l.qbase = 0;
    l.gbase = align256d(l.qbase + (uint64_t(n) + 2u) * 8u);
    l.total = align256d(l.gbase + (uint64_t(n) + 1u) * 8u);
    l.ticket = align256d(l.total + uint64_t(n) * 8u);
    l.desc = align256d(l.ticket + 4u);
    return l;
}
}  // namespace

uint64_t decompress_workspace_size(uint64_t total_out_cap_bytes, uint32_t nchunks) {
    return dec_ws(nchunks).desc + (uint64_t(nchunks) + (total_out_cap_bytes >> s2f::kQuotaShift)) * sizeof(s2f::Desc);
}

int launch_decompress(uint32_t header_id, const uint8_t* d_comp, const uint64_t* d_offsets, const uint64_t* d_comp_lens,
                      uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets, const uint64_t* d_out_caps,
                      uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes, void* stream) {
    const DecWs l = dec_ws(nchunks);
    if (work_bytes < l.desc || (reinterpret_cast<uintptr_t>(d_work) & 7u))
        return set_error(-22, "workspace too small or not 8-byte aligned (kcdc_decompress_workspace_size)");
    decdev::DecArgs a{};
    a.in = d_comp;
    a.in_offs = d_offsets;
    a.in_lens = d_comp_lens;
    a.out = d_out;
    a.out_offs = d_out_offsets;
    a.out_caps = d_out_caps;
    a.out_lens = d_out_lens;
    a.status = d_status;
    uint8_t* w = static_cast<uint8_t*>(d_work);
    a.qbase = reinterpret_cast<uint64_t*>(w + l.qbase);
    a.gbase = reinterpret_cast<uint64_t*>(w + l.gbase);
    a.total = reinterpret_cast<uint64_t*>(w + l.total);
    a.ticket = reinterpret_cast<uint32_t*>(w + l.ticket);
    a.desc = reinterpret_cast<s2f::Desc*>(w + l.desc);
    a.max_desc = (work_bytes - l.desc) / sizeof(s2f::Desc);
    if (a.max_desc > 0x7fffffffull) a.max_desc = 0x7fffffffull;  // the decode ticket is 32 bits
    a.n = nchunks;
    a.header_id = header_id;
    compdev::crc_x2n_table(compdev::kCrc32cPoly, a.x2nc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(decdev::decode_scan_kernel<decdev::kScanQuota>, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(decdev::decode_index_kernel, dim3((nchunks + 63u) / 64u), dim3(64), 0, st, a);
    hipLaunchKernelGGL(decdev::decode_scan_kernel<decdev::kScanBlocks>, dim3(1), dim3(1024), 0, st, a);
    if (a.max_desc > 0) {
        const uint32_t waves = cap_chunk_grid(  // KCDC_TEST_CHUNK_GRID
            static_cast<uint32_t>(a.max_desc < decdev::kDecodeWaves ? a.max_desc : decdev::kDecodeWaves));
        hipLaunchKernelGGL(decdev::decode_blocks_kernel, dim3(waves), dim3(64), 0, st, a);
        hipLaunchKernelGGL(decdev::decode_crc_kernel, dim3((waves + decdev::kCrcWaves - 1u) / decdev::kCrcWaves),
                           dim3(64 * decdev::kCrcWaves), 0, st, a);
    }
    hipLaunchKernelGGL(decdev::decode_final_kernel, dim3((nchunks + 255u) / 256u), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error(-5, std::string("decompression kernel launch: ") + hipGetErrorString(e));
}

}  // namespace kcdc
