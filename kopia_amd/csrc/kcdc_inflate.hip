// Inflate on the device: the read path's Decompress for the deflate-*, gzip* and pgzip*
// compressors (compressor_deflate.go:64-78, compressor_gzip.go:68-85, compressor_pgzip.go;
// called per content by committed_read_manager.go:336).
//
// A deflate stream cannot be indexed (blocks start at any bit), so the unit of parallelism is the
// content: persistent single-wave workgroups take contents by ticket.
//   init     the ticket's zero and the CRC shift table (inflate_init_kernel)
//   inflate  one wave per content, wave-uniform: the decoder of kcdc_inflate_format.h over a wave
//            Io -- the input as a register window of 64 aligned words feeding a 64-bit bit buffer
//            through v_readlane, decode tables in LDS (filled by the lanes side by side), literals
//            gathered one to a lane and stored 64 at a time (in a run of them, looked up at 64 bit
//            positions at once and walked with v_readlane), matches copied output -> output a byte
//            per lane, stored blocks by wave_copy (inflate_kernel)
//   crc      gzip* / pgzip* only: the CRC-32 of every content's first member against its trailer,
//            in 32 KiB pieces combined by shifts, a wave per content (inflate_crc_kernel); a later
//            member of a content (no registered writer emits one) is checked by its inflate wave
//   final    d_out_lens (inflate_final_kernel)
// LDS: 9208 bytes per wave (two dynamic tables, the fixed code's tables, the lengths, the build
// scratch and the kernel's arguments), 16 waves per CU.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kcdc_inflate_format.h"
#include "kcdc_internal.h"
#include "kcdc_wave.h"

namespace kcdc {
namespace infdev {

using compdev::kCrcPoly;
using compdev::kPiece;
using compdev::multmodp;

constexpr uint32_t kCrcWaves = 4;
constexpr uint32_t kInflateWaves = 256u * 16u;  // the persistent grid: 16 waves for each of 256 CUs

struct Rec {              // per content, between the passes
    uint64_t total;       // decoded bytes
    uint64_t first_len;   // gzip: bytes of the first member ...
    uint32_t first_crc;   // ... and the CRC-32 its trailer stores
    uint32_t pad[3];
};
static_assert(sizeof(Rec) == 32, "Rec is 32 bytes");

struct InfArgs {
    const uint8_t* in;
    const uint64_t* in_offs;
    const uint64_t* in_lens;
    uint8_t* out;
    const uint64_t* out_offs;
    const uint64_t* out_caps;
    uint64_t* out_lens;
    int32_t* status;
    uint32_t* ticket;  // [1]: next content
    Rec* rec;          // [n]
    uint32_t n;
    uint32_t header_id;
    uint32_t gz;
    uint32_t* x2n;     // [32]: x^(2^k) mod the CRC-32 polynomial
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// v in a VGPR: keeps the CRC shift arithmetic on uniform values out of the SGPRs, where the
// 32-step chains of multmodp's multiples are hoisted out of loops and spill.
__device__ __forceinline__ uint32_t vec(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
// compdev::crc_finish on the vector unit.
__device__ __forceinline__ uint32_t crc_finish_v(uint32_t raw, uint64_t n, const uint32_t* x2n) {
    uint32_t z = vec(0x80000000u);  // x^0
    for (int bit = 0; n; bit++, n >>= 1)
        if (n & 1u) z = multmodp(z, vec(x2n[(3 + bit) & 31]), kCrcPoly);
    return raw ^ multmodp(z, vec(0xFFFFFFFFu), kCrcPoly) ^ 0xFFFFFFFFu;
}
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return (static_cast<uint64_t>(uni(static_cast<uint32_t>(v >> 32))) << 32) | uni(static_cast<uint32_t>(v));
}

// tab[start], tab[start + step], ... below tab[end] = val, the lanes side by side; the stores are
// ordered before this wave's later reads of the table.
__device__ __forceinline__ void wave_fill(uint32_t* tab, uint32_t start, uint32_t step, uint32_t end, uint32_t val,
                                          uint32_t lane) {
    for (uint32_t i = start + lane * step; i < end; i += 64u * step) tab[i] = val;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct Lds {
    uint32_t lt[inff::kLitCap];
    uint32_t dt[inff::kDistCap];
    uint32_t flt[inff::kFixLitCap];
    uint32_t fdt[inff::kFixDistCap];
    inff::Build build;
    uint8_t lens[inff::kMaxLens];
    InfArgs args;  // the kernel's arguments: read from here, they occupy no SGPRs between uses
};

// Raw CRC-32 (register 0) of p[0..len) by one wave without a table: lane l takes the 2^j bytes
// that end (63 - l) * 2^j bytes before the end, a bit at a time, and the lanes combine in a tree.
// Slow, and only for a second or later gzip member.
__device__ uint32_t wave_crc_bitwise(const uint8_t* p, uint64_t len, const uint32_t* x2n, uint32_t lane) {
    uint32_t j = 0;
    while ((uint64_t(64) << j) < len) j++;
    const uint64_t cs = uint64_t(1) << j, back = (64u - lane) * cs;  // the lane's bytes start `back` before the end
    uint64_t pos = back > len ? 0u : len - back;
    const uint64_t end = back - cs > len ? 0u : len - (back - cs);
    uint32_t r = 0;
    for (; pos < end; pos++) r = inff::crc32_byte(r, p[pos]);
#pragma unroll
    for (uint32_t t = 0; t < 6u; t++) {
        const uint32_t right = __shfl_down(r, 1u << t, 64);
        if (((lane >> t) & 1u) == 0u) r = multmodp(r, vec(x2n[(3u + j + t) & 31u]), kCrcPoly) ^ right;
    }
    return __shfl(r, 0, 64);
}

// The wave Io of inff::inflate_content.  Every member is called by all 64 lanes with equal
// arguments; `lane` alone differs.
struct WaveIo {
    typedef uint32_t pos_t;  // contents of 4 GiB or more never get here
    const uint8_t* in;
    pos_t n;
    uint8_t* out;
    Lds* lds;
    uint32_t content;
    uint32_t lane;
    // the input window: aligned words [w0, w0 + 64) of the content, one per lane
    const uint32_t* words;
    uint32_t al;
    pos_t nw, w0;
    uint32_t win;
    // literals not yet stored: lane k holds output byte lit_at + k
    uint32_t lit_reg, lit_n;
    pos_t lit_at;

    __device__ WaveIo(const uint8_t* in_, pos_t n_, uint8_t* out_, Lds* lds_, uint32_t content_, uint32_t lane_)
        : in(in_), n(n_), out(out_), lds(lds_), content(content_), lane(lane_) {
        al = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(in) & 3u);
        words = reinterpret_cast<const uint32_t*>(in - al);
        nw = n ? static_cast<pos_t>((uint64_t(al) + n + 3u) >> 2) : 0u;  // aligned words holding a byte of the content
        w0 = 0;
        win = lane < nw ? words[lane] : 0u;
        lit_reg = 0;
        lit_n = 0;
        lit_at = 0;
    }
    __device__ pos_t size() const { return n; }
    __device__ uint32_t u(uint32_t v) const { return uni(v); }
    // the 4 bytes at content byte i, little-endian; bytes of words past the content are zeros
    __device__ uint32_t fetch32(pos_t i) {
        const uint64_t p = uint64_t(al) + i;
        pos_t wi = static_cast<pos_t>(p >> 2);
        if (wi - w0 > 62u) {
            w0 = wi;
            win = w0 + lane < nw ? words[w0 + lane] : 0u;
        }
        const uint32_t k = static_cast<uint32_t>(wi - w0);
        const uint32_t l = __builtin_amdgcn_readlane(win, k), h = __builtin_amdgcn_readlane(win, k + 1u);
        return __builtin_amdgcn_alignbit(h, l, 8u * (static_cast<uint32_t>(p) & 3u));
    }
    __device__ uint32_t byte(pos_t i) { return fetch32(i) & 255u; }  // i < n
    __device__ void refill(inff::Bits<pos_t>& bb) {
        while (bb.cnt <= 32u && bb.pos < n) {
            const pos_t left = n - bb.pos;
            const uint32_t take = left < 4u ? static_cast<uint32_t>(left) : 4u;
            uint32_t w = fetch32(bb.pos);
            if (take < 4u) w &= (1u << (8u * take)) - 1u;
            bb.buf |= static_cast<uint64_t>(w) << bb.cnt;
            bb.cnt += 8u * take;
            bb.pos += take;
        }
    }
    __device__ void fill(uint32_t* tab, uint32_t start, uint32_t step, uint32_t end, uint32_t val) {
        wave_fill(tab, start, step, end, val, lane);
    }
    __device__ uint8_t* lens() { return lds->lens; }
    __device__ inff::Build* build() { return &lds->build; }
    __device__ uint32_t* lit_table() { return lds->lt; }
    __device__ uint32_t* dist_table() { return lds->dt; }
    __device__ const uint32_t* fixed_lit_table() const { return lds->flt; }
    __device__ const uint32_t* fixed_dist_table() const { return lds->fdt; }

    __device__ void flush() {
        if (lane < lit_n) out[lit_at + lane] = static_cast<uint8_t>(lit_reg);
        lit_n = 0;
    }
    __device__ void literal(pos_t o, uint32_t v) {  // o < cap
        if (lit_n == 0) lit_at = o;
        if (lane == lit_n) lit_reg = v;
        if (++lit_n == 64u) flush();
    }
    // inff::literal_run's parts: the buffer filled to 57 bits or more, lane k's look at the code
    // that starts at bit k, and a lane's result read back with v_readlane.
    __device__ void top_up(inff::Bits<pos_t>& bb) {
#pragma nounroll
        while (bb.cnt <= 56u && bb.pos < n) {
            const pos_t left = n - bb.pos;
            uint32_t take = (64u - bb.cnt) >> 3;
            take = take > 4u ? 4u : take;
            take = left < take ? static_cast<uint32_t>(left) : take;
            uint32_t w = fetch32(bb.pos);
            if (take < 4u) w &= (1u << (8u * take)) - 1u;
            bb.buf |= static_cast<uint64_t>(w) << bb.cnt;
            bb.cnt += 8u * take;
            bb.pos += take;
        }
    }
    __device__ uint32_t look_ahead(const inff::Bits<pos_t>& bb, const uint32_t* tab, uint32_t held) const {
        return lane < held ? inff::literal_at(tab, static_cast<uint32_t>(bb.buf >> lane) & 0x7fffu) : 0u;
    }
    __device__ uint32_t looked(uint32_t mine, uint32_t at) const { return __builtin_amdgcn_readlane(mine, at); }
    __device__ void stored(pos_t at, pos_t o, uint32_t len) {  // [at, +len) in the content, [o, +len) in the slot
        flush();
        compdev::wave_copy(out + o, in + at, len, lane);
    }
    __device__ void match(pos_t o, uint32_t len, uint32_t dist) {  // dist <= o, o + len <= cap
        flush();
        // The source may be what earlier lanes' stores of this wave wrote: order them before the
        // loads at workgroup scope (one CU, one vector L1).
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint8_t* src = out + o - dist;
        uint8_t* dst = out + o;
        if (dist >= len) {
            for (uint32_t k = lane; k < len; k += 64u) dst[k] = src[k];
        } else {  // periodic extension: only bytes written before this match are read
            for (uint32_t k = lane; k < len; k += 64u) dst[k] = src[k % dist];
        }
    }
    // The rare paths below take the lane and the kernel's arguments afresh (vec, the LDS copy), so
    // that nothing of theirs is kept in SGPRs across the symbol loop.
    __device__ void first_member(pos_t len, uint32_t crc) {
        if (vec(lane) == 0) {
            Rec* rec = lds->args.rec + content;
            rec->first_len = len;
            rec->first_crc = crc;
        }
    }
    __device__ bool member_crc(pos_t from, pos_t len, uint32_t crc) {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint32_t* x2n = lds->args.x2n;
        const uint32_t raw = wave_crc_bitwise(out + from, len, x2n, vec(lane));
        return uni(crc_finish_v(raw, len, x2n)) == crc;
    }
};

// The ticket's zero and the CRC shift table, before the other passes.
__global__ __launch_bounds__(64) void inflate_init_kernel(InfArgs a) {
    if (threadIdx.x != 0) return;
    *a.ticket = 0;
    uint32_t p = 1u << 30;  // x^1 (crc_x2n_table, stored as it goes)
    for (int k = 0; k < 32; k++) {
        a.x2n[k] = p;
        p = multmodp(p, p, kCrcPoly);
    }
}

// The fixed code's tables need the fill alone.
struct FillIo {
    uint32_t lane;
    __device__ void fill(uint32_t* tab, uint32_t start, uint32_t step, uint32_t end, uint32_t val) {
        wave_fill(tab, start, step, end, val, lane);
    }
};

__global__ __launch_bounds__(64) void inflate_kernel(InfArgs a) {
    __shared__ Lds lds;
    const uint32_t lane = threadIdx.x;
    FillIo fio{lane};
    inff::build_fixed(fio, lds.lens, lds.flt, lds.fdt, &lds.build);
    if (lane == 0) lds.args = a;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const InfArgs& sa = lds.args;
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(sa.ticket, 1u);
        c = uni(c);
        if (c >= uni(sa.n)) return;
        const uint64_t in_off = uni64(sa.in_offs[c]), n = uni64(sa.in_lens[c]);
        const uint64_t out_off = uni64(sa.out_offs[c]), cap = uni64(sa.out_caps[c]);
        if (lane == 0) {
            Rec* rec = sa.rec + c;
            rec->first_len = 0;
            rec->first_crc = 0;
        }
        // positions are 32 bits here: a content of 4 GiB or more is refused, and no content decodes
        // to more than 4 GiB - 1
        int32_t st = inff::kBadMsg;
        uint32_t total = 0;
        if (n <= 0xffffffffull) {
            WaveIo io(sa.in + in_off, static_cast<uint32_t>(n), sa.out + out_off, &lds, c, lane);
            st = inff::inflate_content(io, uni(sa.header_id), uni(sa.gz) != 0,
                                       cap < 0xffffffffull ? static_cast<uint32_t>(cap) : 0xffffffffu, &total);
            io.flush();
        }
        if (vec(lane) == 0) {
            sa.status[c] = st;
            sa.rec[c].total = st == 0 ? total : 0u;
        }
    }
}

// gzip* / pgzip*: the first member's CRC-32, as decode_crc_kernel checks a block's CRC-32C.
__global__ __launch_bounds__(64 * kCrcWaves) void inflate_crc_kernel(InfArgs a) {
    __shared__ uint32_t tab[256 * 32];
    __shared__ uint32_t x2n[32];
    compdev::crc_table_fill(tab, kCrcPoly, 64u * kCrcWaves);
    if (threadIdx.x < 32u) x2n[threadIdx.x] = a.x2n[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t step = gridDim.x * kCrcWaves;
    for (uint32_t c = blockIdx.x * kCrcWaves + uni(threadIdx.x >> 6); c < a.n; c += step) {
        if (a.status[c] != 0) continue;
        const uint64_t len = uni64(a.rec[c].first_len);
        const uint8_t* p = a.out + a.out_offs[c];
        // pieces counted back from the member's end: the first is the short one, every later one
        // shifts the running value by x^(8 * 32768) = x^(2^18)
        const uint64_t pieces = (len + kPiece - 1u) / kPiece;
        uint64_t at = 0;
        uint32_t raw = 0;
        for (uint64_t j = 0; j < pieces; j++) {
            const uint32_t plen = j == 0 ? static_cast<uint32_t>(len - (pieces - 1u) * kPiece) : kPiece;
            raw = multmodp(raw, vec(x2n[18]), kCrcPoly) ^ compdev::piece_crc(p + at, plen, tab, x2n, kCrcPoly, lane);
            at += plen;
        }
        const uint32_t crc = crc_finish_v(raw, len, x2n);
        if (lane == 0 && crc != a.rec[c].first_crc) a.status[c] = inff::kBadMsg;
    }
}

__global__ __launch_bounds__(256) void inflate_final_kernel(InfArgs a) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < a.n) a.out_lens[c] = a.status[c] == 0 ? a.rec[c].total : 0u;
}

}  // namespace infdev

namespace {
constexpr uint64_t kInfX2nOff = 64, kInfRecOff = 256;  // the ticket, the CRC shift table, then the records
}

uint64_t inflate_workspace_size(uint32_t nchunks) { return kInfRecOff + uint64_t(nchunks) * sizeof(infdev::Rec); }

int launch_inflate(uint32_t header_id, bool gz, const uint8_t* d_comp, const uint64_t* d_offsets,
                   const uint64_t* d_comp_lens, uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets,
                   const uint64_t* d_out_caps, uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes,
                   void* stream) {
    if (work_bytes < inflate_workspace_size(nchunks) || (reinterpret_cast<uintptr_t>(d_work) & 7u))
        return set_error(-22, "workspace too small or not 8-byte aligned (kcdc_inflate_workspace_size)");
    infdev::InfArgs a{};
    a.in = d_comp;
    a.in_offs = d_offsets;
    a.in_lens = d_comp_lens;
    a.out = d_out;
    a.out_offs = d_out_offsets;
    a.out_caps = d_out_caps;
    a.out_lens = d_out_lens;
    a.status = d_status;
    uint8_t* w = static_cast<uint8_t*>(d_work);
    a.ticket = reinterpret_cast<uint32_t*>(w);
    a.x2n = reinterpret_cast<uint32_t*>(w + kInfX2nOff);
    a.rec = reinterpret_cast<infdev::Rec*>(w + kInfRecOff);
    a.n = nchunks;
    a.header_id = header_id;
    a.gz = gz ? 1u : 0u;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(infdev::inflate_init_kernel, dim3(1), dim3(64), 0, st, a);
    const uint32_t waves = cap_chunk_grid(nchunks < infdev::kInflateWaves ? nchunks : infdev::kInflateWaves);  // KCDC_TEST_CHUNK_GRID
    hipLaunchKernelGGL(infdev::inflate_kernel, dim3(waves), dim3(64), 0, st, a);
    if (gz)
        hipLaunchKernelGGL(infdev::inflate_crc_kernel, dim3((waves + infdev::kCrcWaves - 1u) / infdev::kCrcWaves),
                           dim3(64 * infdev::kCrcWaves), 0, st, a);
    hipLaunchKernelGGL(infdev::inflate_final_kernel, dim3((nchunks + 255u) / 256u), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error(-5, std::string("inflate kernel launch: ") + hipGetErrorString(e));
}

}  // namespace kcdc
