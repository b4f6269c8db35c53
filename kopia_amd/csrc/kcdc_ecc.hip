// Error correction of chunks on the device: Kopia's repo/ecc, REED-SOLOMON-CRC32
// (ecc_rs_crc.go).  Stored layout of one chunk (Encrypt, ecc_rs_crc.go:157-250):
//   ([CRC32][parity shard])+ ([CRC32][data shard])+
// over the logical input BE32(len) || bytes || zero padding, cut into blocks of
// DataShards x ShardSize bytes.  Nothing of the logical input is staged: the kernels read the
// chunk's bytes where they lie, at any alignment, and make up the 4 length bytes and the zeros.
//
// Encode is two kernels on the caller's stream:
//   ecc_parity_kernel   one lane per 4 byte columns of a block (blocks of one chunk side by side
//                       in a workgroup, so small shards fill the lanes too).  For each data word
//                       the packed doublings d, 2d .. 128d are formed once (gf_dbl) and every
//                       parity row of a tile of 8 XORs the ones its coefficient's bits select.
//                       Four coefficients of a row come in one word, pinned to a scalar register:
//                       the bit masks are SALU work, the vector side keeps an AND and an XOR.
//   ecc_records_kernel  the CRC-32 of every record and the copy of the data records.  A group of
//                       G = 1..64 lanes takes one shard, 16 bytes per lane and more for shards over
//                       1 KiB, segments counted back from the shard's END: the raw CRC (register
//                       0, no final XOR) ignores leading zeros, so the partials combine as
//                       sum raw(seg_j) * x^(8 * seg * (G-1-j)) (zlib's crc32_combine, as the gzip
//                       trailer in kcdc_compress.hip) with one multiply per lane and an XOR over
//                       the group; crc32 of S zero bytes supplies the init / final-XOR terms.
//                       The byte steps are sliced by 4: four tables in LDS, four independent
//                       lookups per 32-bit word.
// Decode phase 1 (Decrypt, ecc_rs_crc.go:254-323) is the same records kernel reading the stored
// bytes: it checks the CRCs, copies the data payload to the output slot and records the failed
// shards of each block (256 bits per block) in the workspace.  Phase 2 (ReconstructData, :325)
// runs on the host for the erasure patterns found and reuses the parity kernel's row loop for
// the missing data shards (ecc_repair_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kcdc.h"
#include "kcdc_hip.h"
#include "kcdc_internal.h"

namespace kcdc {
namespace {
namespace eccdev {

constexpr uint64_t kMaxLen = 0xFFFFFFFFull - 3;  // len + 4 must fit the BE32 prefix's range
constexpr uint64_t kNoRoom = ~0ull;              // blk_off of a chunk the decode skips
constexpr uint32_t kRowTile = 8;                 // parity rows accumulated per pass over the data
constexpr uint32_t kThreads = 256;
constexpr uint32_t kGridY = 32;                  // workgroups that share one chunk
constexpr uint32_t kSegBytes = 16;               // bytes of a shard one lane CRCs before its multiply (32: 0.73x the rate)

// ------------------------------------------------------------------ CRC-32 (IEEE, reflected)
constexpr uint32_t kCrcPoly = 0xEDB88320u;
__host__ __device__ constexpr uint32_t multmodp(uint32_t a, uint32_t b) {  // a * b mod P
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= ((a >> i) & 1u) ? b : 0u;
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}
struct X2n {
    uint32_t v[32];  // x^(2^k) mod P (zlib's x2n_table)
};
constexpr X2n make_x2n() {
    X2n t{};
    uint32_t p = 1u << 30;  // x^1
    t.v[0] = p;
    for (int n = 1; n < 32; n++) t.v[n] = p = multmodp(p, p);
    return t;
}
__constant__ X2n kX2n = make_x2n();
__device__ uint32_t xpow8(uint64_t n) {  // x^(8n) mod P (zlib's x2nmodp(n, 3))
    uint32_t p = 1u << 31, k = 3;
    while (n) {
        if (n & 1u) p = multmodp(kX2n.v[k & 31u], p);
        n >>= 1;
        k++;
    }
    return p;
}

// ------------------------------------------------------------------ bytes in place
// `len` bytes at src, after `pre` made-up bytes (the big-endian length) and before endless zeros.
struct Bytes {
    const uint8_t* src;
    uint64_t len;
    uint32_t pre;  // 0: stored bytes; 4: the logical input of Encrypt
    __device__ __forceinline__ uint32_t byte(uint64_t q) const {
        if (q < pre) return (static_cast<uint32_t>(len) >> (8u * (3u - static_cast<uint32_t>(q)))) & 0xffu;
        q -= pre;
        return q < len ? src[q] : 0u;
    }
    // bytes q .. q+nb-1 (nb <= 4), little-endian packed, the rest zero
    __device__ __forceinline__ uint32_t word(uint64_t q, uint32_t nb) const {
        if (nb == 4u && q >= pre && q - pre + 4u <= len) {
            uint32_t w;
            __builtin_memcpy(&w, src + (q - pre), 4);
            return w;
        }
        uint32_t w = 0;
        for (uint32_t k = 0; k < nb; k++) w |= byte(q + k) << (8u * k);
        return w;
    }
};
__device__ __forceinline__ void put_word(uint8_t* dst, uint32_t v, uint32_t nb) {
    if (nb == 4u) {
        __builtin_memcpy(dst, &v, 4);
        return;
    }
    for (uint32_t k = 0; k < nb; k++) dst[k] = static_cast<uint8_t>(v >> (8u * k));
}

// ------------------------------------------------------------------ GF(2^8) rows on packed words
__device__ __forceinline__ uint32_t gf_dbl(uint32_t x) {  // 4 bytes times 2, mod 0x11d
    return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du);
}
// out(r, XOR_k coef[r][k] * in(k)) for r < rows, kRowTile rows per pass over the inputs.  A row of
// coef is nin bytes padded with zeros to whole 32-bit words (coef_stride), 4-byte aligned, so four
// coefficients of a row arrive in one word; coef, rows and nin are uniform across the workgroup
// and the word is pinned to a scalar register, where the bit masks are formed (SALU), leaving an
// AND and an XOR per selected product on the vector side.  Lanes with !active read and write nothing.
__host__ __device__ constexpr uint32_t coef_stride(uint32_t nin) { return (nin + 3u) & ~3u; }
template <class In, class Out>
__device__ __forceinline__ void rs_rows(const uint8_t* __restrict__ coef, uint32_t rows, uint32_t nin, bool active, In in,
                                        Out out) {
    const uint32_t* __restrict__ coef32 = reinterpret_cast<const uint32_t*>(coef);
    const uint32_t words = coef_stride(nin) / 4u;
    for (uint32_t r0 = 0; r0 < rows; r0 += kRowTile) {
        const uint32_t nr = rows - r0 < kRowTile ? rows - r0 : kRowTile;
        uint32_t acc[kRowTile] = {};
        for (uint32_t k0 = 0; k0 < nin; k0 += 4u) {
            uint32_t cw[kRowTile];
#pragma unroll
            for (uint32_t j = 0; j < kRowTile; j++)
                cw[j] = j < nr ? __builtin_amdgcn_readfirstlane(coef32[size_t(r0 + j) * words + (k0 >> 2)]) : 0u;
#pragma unroll
            for (uint32_t kk = 0; kk < 4u; kk++) {
                if (k0 + kk >= nin) break;
                uint32_t x[8];
                x[0] = active ? in(k0 + kk) : 0u;
#pragma unroll
                for (int i = 1; i < 8; i++) x[i] = gf_dbl(x[i - 1]);
#pragma unroll
                for (uint32_t j = 0; j < kRowTile; j++) {
                    if (j < nr) {
                        const uint32_t c = cw[j] >> (8u * kk);
#pragma unroll
                        for (int i = 0; i < 8; i++) acc[j] ^= x[i] & (0u - ((c >> i) & 1u));
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (uint32_t j = 0; j < kRowTile; j++)
                if (j < nr) out(r0 + j, acc[j]);
        }
    }
}

struct EncArgs {
    const uint8_t* data;
    const uint64_t* offs;
    const uint64_t* lens;
    uint8_t* out;
    const uint64_t* out_offs;
    int32_t* status;
    EccParams prm;
    const uint8_t* mat;  // parity rows of the repository's code (coef_stride(data) bytes each), then the small code's 2
};

__global__ __launch_bounds__(kThreads) void ecc_parity_kernel(EncArgs a) {
    const uint32_t c = blockIdx.x;
    const uint64_t len = a.lens[c];
    if (len >= kMaxLen) return;
    const EccGeo g = ecc_geo_original(a.prm, len);
    const uint32_t S = g.shard, W = (S + 3u) / 4u;
    const uint64_t items = g.blocks * W;
    if (uint64_t(blockIdx.y) * kThreads >= items) return;
    const uint8_t* mat = g.small ? a.mat + size_t(a.prm.parity) * coef_stride(a.prm.data) : a.mat;
    const Bytes in{a.data + a.offs[c], len, kEccLengthSize};
    uint8_t* out = a.out + a.out_offs[c];
    for (uint64_t base = uint64_t(blockIdx.y) * kThreads; base < items; base += uint64_t(gridDim.y) * kThreads) {
        const uint64_t it = base + threadIdx.x;
        const bool active = it < items;
        const uint64_t b = it / W;
        const uint32_t col = static_cast<uint32_t>(it % W) * 4u;
        const uint32_t nb = S - col < 4u ? S - col : 4u;
        rs_rows(
            mat, g.parity, g.data, active,
            [&](uint32_t d) { return in.word((b * g.data + d) * S + col, nb); },
            [&](uint32_t p, uint32_t v) { put_word(out + (b * g.parity + p) * g.rec() + kEccCrcSize + col, v, nb); });
    }
}

struct DecArgs {
    const uint8_t* in;
    const uint64_t* offs;
    const uint64_t* lens;  // stored lengths
    uint32_t n;
    uint8_t* out;
    const uint64_t* out_offs;
    uint64_t* out_lens;
    int32_t* status;
    EccParams prm;
    uint64_t* blk_off;    // first mask slot of chunk i, or kNoRoom
    uint32_t* len_stage;  // rebuilt length bytes of chunk i (repair)
    uint32_t* masks;      // 8 words per block: bit s set = shard s of the block failed its CRC
    uint64_t mask_blocks;
};

// One thread block; chunk i's mask slots start at the running sum of the blocks before it.
__global__ __launch_bounds__(1024) void ecc_decode_init_kernel(DecArgs a) {
    __shared__ uint64_t part[1024];
    __shared__ uint64_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < a.n; base += 1024u) {
        const uint32_t i = base + t;
        uint64_t nb = 0;
        int32_t st = 0;
        if (i < a.n) {
            const uint64_t slen = a.lens[i];
            if (slen < kEccMinStored) st = KCDC_EINVAL;
            else nb = ecc_geo_stored(a.prm, slen).blocks;
        }
        part[t] = nb;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {
            const uint64_t v = t >= d ? part[t - d] : 0ull;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        const uint64_t off = carry + part[t] - nb;
        if (i < a.n) {
            if (st == 0 && off + nb > a.mask_blocks) st = KCDC_ENOMEM;
            a.blk_off[i] = st == 0 ? off : kNoRoom;
            a.status[i] = st;
            a.out_lens[i] = 0;
            a.len_stage[i] = 0;
        }
        __syncthreads();
        if (t == 1023u) carry += part[1023];
        __syncthreads();
    }
}

// kDecode = false: CRC and store every record of Encrypt's output (parity payloads are there
// already).  kDecode = true: check every stored record and copy the data payload out.
template <bool kDecode>
__global__ __launch_bounds__(kThreads) void ecc_records_kernel(EncArgs e, DecArgs d) {
    __shared__ uint32_t tab[4][256];  // slicing by 4: tab[k][b] = the register after byte b and k zero bytes
    __shared__ uint32_t pw[64];
    __shared__ uint32_t zcrc_s;
    const uint32_t c = blockIdx.x;
    const uint64_t len = kDecode ? d.lens[c] : e.lens[c];  // stored length when decoding
    EccGeo g;
    if (kDecode) {
        if (d.blk_off[c] == kNoRoom) return;  // status set by the init kernel
        g = ecc_geo_stored(d.prm, len);
    } else {
        if (blockIdx.y == 0 && threadIdx.x == 0) e.status[c] = len >= kMaxLen ? KCDC_EFBIG : 0;
        if (len >= kMaxLen) return;
        g = ecc_geo_original(e.prm, len);
    }
    const uint32_t S = g.shard;
    uint32_t G = 1;
    while (G < 64u && G * kSegBytes < S) G <<= 1;
    const uint32_t seg = ((S + G - 1u) / G + 3u) & ~3u;  // G * seg >= S
    const uint64_t npar = g.blocks * g.parity, par_bytes = g.parity_bytes();
    // data records: those Encrypt stores; when decoding, every data shard of every block
    const uint64_t store = g.pad ? uint64_t(g.data) * S * g.blocks : len + kEccLengthSize;
    const uint64_t ndata = kDecode ? g.blocks * g.data : ecc_ceil(store, S);
    const uint64_t data_region = kDecode ? (len > par_bytes ? len - par_bytes : 0) : 0;
    const uint64_t cap = kDecode ? [&] {
        const uint64_t pay = ecc_stored_payload(g, len);
        return pay > kEccLengthSize ? pay - kEccLengthSize : 0;
    }() : 0;
    const uint64_t items = (npar + ndata) * G;
    if (uint64_t(blockIdx.y) * kThreads >= items) return;

    {
        uint32_t r = threadIdx.x;
        for (int k = 0; k < 8; k++) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
        tab[0][threadIdx.x] = r;
        for (int s = 1; s < 4; s++) {  // one more zero byte: 8 more register steps
            for (int k = 0; k < 8; k++) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
            tab[s][threadIdx.x] = r;
        }
        if (threadIdx.x < 64u) pw[threadIdx.x] = xpow8(uint64_t(seg) * threadIdx.x);
        if (threadIdx.x == 64u) zcrc_s = multmodp(0xFFFFFFFFu, xpow8(S)) ^ 0xFFFFFFFFu;  // crc32 of S zero bytes
    }
    __syncthreads();
    const uint32_t zcrc = zcrc_s;

    const Bytes logical{kDecode ? nullptr : e.data + e.offs[c], len, kEccLengthSize};
    uint8_t* const enc_out = kDecode ? nullptr : e.out + e.out_offs[c];
    const Bytes stored{kDecode ? d.in + d.offs[c] : enc_out, kDecode ? len : ~0ull, 0};
    uint8_t* const slot = kDecode ? d.out + d.out_offs[c] : nullptr;

    for (uint64_t base = uint64_t(blockIdx.y) * kThreads; base < items; base += uint64_t(gridDim.y) * kThreads) {
        const uint64_t it = base + threadIdx.x;
        const bool active = it < items;
        const uint64_t r = it / G;
        const uint32_t j = static_cast<uint32_t>(it & (G - 1u));
        const bool par = r < npar;
        const uint64_t q = par ? 0 : r - npar;                                 // data record index
        const uint64_t rs = par ? r * g.rec() : par_bytes + q * g.rec();       // record start in the stored bytes
        // where the shard's bytes come from: the stored bytes, or (encoding a data record) the logical input
        const bool from_logical = !kDecode && !par;
        const uint64_t src0 = from_logical ? q * S : rs + kEccCrcSize;
        const uint64_t left = from_logical ? (store - q * S < S ? store - q * S : S) : 0;  // payload bytes to store
        const int64_t start = int64_t(S) - int64_t(G - j) * int64_t(seg);
        uint32_t reg = 0;
        if (active) {
            for (uint32_t i = 0; i < seg; i += 4u) {
                const int64_t pos = start + int64_t(i);
                if (pos <= -4) continue;
                uint32_t w;
                if (pos >= 0) {
                    w = from_logical ? logical.word(src0 + pos, 4u) : stored.word(src0 + pos, 4u);
                } else {
                    w = 0;
                    for (int64_t k = -pos; k < 4; k++)
                        w |= (from_logical ? logical.byte(src0 + pos + k) : stored.byte(src0 + pos + k)) << (8 * k);
                }
                reg ^= w;  // four independent lookups instead of a chain of four
                reg = tab[3][reg & 0xffu] ^ tab[2][(reg >> 8) & 0xffu] ^ tab[1][(reg >> 16) & 0xffu] ^ tab[0][reg >> 24];
                if (from_logical) {  // Encrypt's output.Append(shard[:left])
                    uint8_t* dst = enc_out + rs + kEccCrcSize;
                    if (pos >= 0 && uint64_t(pos) + 4u <= left) {
                        put_word(dst + pos, w, 4u);
                    } else {
                        for (int k = 0; k < 4; k++)
                            if (pos + k >= 0 && uint64_t(pos + k) < left) dst[pos + k] = static_cast<uint8_t>(w >> (8 * k));
                    }
                } else if (kDecode && !par) {  // logical byte q*S + pos goes to slot byte q*S + pos - 4
                    const int64_t o = int64_t(q * S) + pos - int64_t(kEccLengthSize);
                    if (pos >= 0 && o >= 0 && uint64_t(o) + 4u <= cap) {
                        put_word(slot + o, w, 4u);
                    } else {
                        for (int k = 0; k < 4; k++)
                            if (pos + k >= 0 && o + k >= 0 && uint64_t(o + k) < cap) slot[o + k] = static_cast<uint8_t>(w >> (8 * k));
                    }
                }
            }
        }
        uint32_t v = active ? multmodp(reg, pw[G - 1u - j]) : 0u;
        for (uint32_t off = 1; off < G; off <<= 1) v ^= __shfl_xor(v, static_cast<int>(off), 64);
        if (active && j == 0) {
            const uint32_t crc = v ^ zcrc;
            if (!kDecode) {
                uint8_t* dst = enc_out + rs;
                for (int k = 0; k < 4; k++) dst[k] = static_cast<uint8_t>(crc >> (8 * (3 - k)));
            } else {
                // data shards that start in the padding are not checked (ecc_rs_crc.go:297-303)
                const bool checked = par || q * g.rec() < data_region;
                uint32_t have = 0;
                for (int k = 0; k < 4; k++) have = (have << 8) | stored.byte(rs + k);
                if (checked && have != crc) {
                    const uint64_t b = par ? r / g.parity : q / g.data;
                    const uint32_t bit = par ? g.data + static_cast<uint32_t>(r % g.parity) : static_cast<uint32_t>(q % g.data);
                    atomicOr(&d.masks[(d.blk_off[c] + b) * 8u + (bit >> 5)], 1u << (bit & 31u));
                    atomicMax(&d.status[c], KCDC_ECC_DAMAGED);
                }
            }
        }
    }
}

// The in-band length of chunk c from the stored bytes (readLength, ecc_rs_crc.go:352-394), a byte
// from len_stage instead where stage_mask says the repair rebuilt it.
__device__ uint64_t inband_length(const DecArgs& a, uint32_t c, const EccGeo& g, uint64_t slen, uint32_t stage_mask) {
    const Bytes stored{a.in + a.offs[c], slen, 0};
    uint64_t L = 0;
    for (uint32_t k = 0; k < kEccLengthSize; k++) {
        uint32_t b;
        if ((stage_mask >> k) & 1u) b = (a.len_stage[c] >> (8u * k)) & 0xffu;
        else b = stored.byte(g.parity_bytes() + uint64_t(k / g.shard) * g.rec() + kEccCrcSize + k % g.shard);
        L = (L << 8) | b;
    }
    return L;
}

// One workgroup per chunk: settle status, length and (for a chunk that hands back nothing) the slot.
// flags: 0x100 = lost (more shards failed in a block than it has parity); low 4 bits = stage_mask.
__device__ void settle_chunk(const DecArgs& a, uint32_t c, uint32_t flags) {
    const uint64_t slen = a.lens[c];
    const EccGeo g = ecc_geo_stored(a.prm, slen);
    const uint64_t pay = ecc_stored_payload(g, slen);
    const uint64_t cap = pay > kEccLengthSize ? pay - kEccLengthSize : 0;
    const uint64_t L = inband_length(a, c, g, slen, flags & 0xfu);
    const bool bad = (flags & 0x100u) || L > cap;
    if (bad) {
        uint8_t* slot = a.out + a.out_offs[c];
        for (uint64_t i = threadIdx.x; i < cap; i += blockDim.x) slot[i] = 0;
    }
    if (threadIdx.x == 0) {
        a.status[c] = bad ? KCDC_EBADMSG : 0;
        a.out_lens[c] = bad ? 0 : L;
    }
}

__global__ __launch_bounds__(kThreads) void ecc_decode_finish_kernel(DecArgs a) {
    const uint32_t c = blockIdx.x;
    if (a.blk_off[c] == kNoRoom || a.status[c] != 0) return;  // refused, or damaged: the repair settles it
    settle_chunk(a, c, 0);
}

struct RepJob {  // one damaged block with missing data shards
    uint64_t block;
    uint32_t chunk;
    uint32_t rows, nsrc;  // missing data shards; stored shards they are rebuilt from
    uint32_t coef_off;    // rows of coef_stride(nsrc) decode coefficients (a multiple of 4)
    uint32_t idx_off;     // nsrc source shard indices, then rows target shard indices
    uint32_t pad;
};
struct RepFin {
    uint32_t chunk, flags;
};

__global__ __launch_bounds__(kThreads) void ecc_repair_kernel(DecArgs a, const RepJob* jobs, const uint8_t* coef,
                                                               const uint16_t* idx) {
    const RepJob job = jobs[blockIdx.x];
    const uint32_t c = job.chunk;
    const uint64_t slen = a.lens[c];
    const EccGeo g = ecc_geo_stored(a.prm, slen);
    const uint32_t S = g.shard, W = (S + 3u) / 4u;
    const uint64_t pay = ecc_stored_payload(g, slen);
    const uint64_t cap = pay > kEccLengthSize ? pay - kEccLengthSize : 0;
    const Bytes stored{a.in + a.offs[c], slen, 0};
    uint8_t* slot = a.out + a.out_offs[c];
    uint8_t* stage = reinterpret_cast<uint8_t*>(a.len_stage + c);
    const uint16_t* srcs = idx + job.idx_off;
    const uint16_t* tgts = srcs + job.nsrc;
    const uint64_t b = job.block;
    for (uint32_t base = blockIdx.y * kThreads; base < W; base += gridDim.y * kThreads) {
        const uint32_t w = base + threadIdx.x;
        const bool active = w < W;
        const uint32_t col = w * 4u;
        const uint32_t nb = active ? (S - col < 4u ? S - col : 4u) : 0u;
        rs_rows(
            coef + job.coef_off, job.rows, job.nsrc, active,
            [&](uint32_t k) {
                const uint32_t s = srcs[k];
                const uint64_t rs = s < g.data ? g.parity_bytes() + (b * g.data + s) * g.rec()
                                               : (b * g.parity + (s - g.data)) * g.rec();
                return stored.word(rs + kEccCrcSize + col, nb);
            },
            [&](uint32_t row, uint32_t v) {
                const uint64_t q0 = (b * g.data + tgts[row]) * S + col;  // logical position
                for (uint32_t k = 0; k < nb; k++) {
                    const uint64_t q = q0 + k;
                    const uint8_t byte = static_cast<uint8_t>(v >> (8u * k));
                    if (q < kEccLengthSize) stage[q] = byte;
                    else if (q - kEccLengthSize < cap) slot[q - kEccLengthSize] = byte;
                }
            });
    }
}

__global__ __launch_bounds__(kThreads) void ecc_repair_finish_kernel(DecArgs a, const RepFin* fin) {
    const RepFin f = fin[blockIdx.x];
    settle_chunk(a, f.chunk, f.flags);
}

}  // namespace eccdev

using eccdev::DecArgs;
using eccdev::EncArgs;

// ------------------------------------------------------------------ host side
// Rows of nin coefficients, each padded with zeros to coef_stride(nin) bytes (rs_rows).
std::vector<uint8_t> pad_rows(const std::vector<uint8_t>& m, uint32_t rows, uint32_t nin) {
    const uint32_t st = eccdev::coef_stride(nin);
    std::vector<uint8_t> out(size_t(rows) * st, 0);
    for (uint32_t r = 0; r < rows; r++) std::copy(m.begin() + size_t(r) * nin, m.begin() + size_t(r + 1) * nin, out.begin() + size_t(r) * st);
    return out;
}

// The coding matrices of one parameter set on one device, uploaded once and kept for the process.
const uint8_t* device_matrix(const EccParams& p, int* err) {
    static std::mutex mu;
    static std::map<uint64_t, uint8_t*> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return *err = set_error(-5, "hipGetDevice failed"), nullptr;
    const uint64_t key = (uint64_t(dev) << 32) | (uint64_t(p.data) << 16) | p.parity;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    std::vector<uint8_t> big(size_t(p.data) * p.parity), small(size_t(kEccSmallData) * kEccSmallParity);
    if ((*err = ecc_matrix(p.data, p.parity, big.data())) != 0) return nullptr;
    if ((*err = ecc_matrix(kEccSmallData, kEccSmallParity, small.data())) != 0) return nullptr;
    std::vector<uint8_t> m = pad_rows(big, p.parity, p.data);
    const std::vector<uint8_t> ms = pad_rows(small, kEccSmallParity, kEccSmallData);
    m.insert(m.end(), ms.begin(), ms.end());
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), m.size());
    if (e == hipSuccess) e = hipMemcpy(d, m.data(), m.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return *err = hip_error(e, "ECC coding matrix upload"), nullptr;
    }
    cache[key] = d;
    return d;
}

struct EccWs {
    uint64_t blk_off, len_stage, masks, total;
};
uint64_t align256(uint64_t x) { return (x + 255u) & ~uint64_t(255); }
// A block of a multi-block chunk is at least (128 + 2) * (4 + 1) stored bytes.
constexpr uint64_t kMinBlockBytes = 650;
EccWs ecc_ws(uint64_t total_stored, uint32_t n) {
    EccWs l{};
    l.blk_off = 0;
    l.len_stage = align256(uint64_t(n) * 8u);
    l.masks = align256(l.len_stage + uint64_t(n) * 4u);
    l.total = align256(l.masks + 32u * (total_stored / kMinBlockBytes + n));
    return l;
}

int ecc_args(const char* alg, int32_t overhead, int32_t max_shard, EccParams* p) {
    if (!ecc_known(alg)) return set_error(-2, std::string("unknown ECC algorithm: ") + (alg ? alg : "(null)"));
    return ecc_params(overhead, max_shard, p);
}

int dec_args(const char* alg, int32_t overhead, int32_t max_shard, const uint8_t* d_stored, const uint64_t* d_offsets,
             const uint64_t* d_stored_lens, uint32_t n, uint8_t* d_out, const uint64_t* d_out_offsets,
             uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes, DecArgs* a) {
    EccParams p{};
    const int rc = ecc_args(alg, overhead, max_shard, &p);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!d_stored || !d_offsets || !d_stored_lens || !d_out || !d_out_offsets || !d_out_lens || !d_status || !d_work)
        return set_error(-22, "null argument");
    const EccWs l = ecc_ws(0, n);
    if (work_bytes < l.total) return set_error(-22, "workspace too small (kcdc_ecc_workspace_size)");
    uint8_t* w = static_cast<uint8_t*>(d_work);
    *a = DecArgs{d_stored, d_offsets, d_stored_lens, n, d_out, d_out_offsets, d_out_lens, d_status, p,
                 reinterpret_cast<uint64_t*>(w + l.blk_off), reinterpret_cast<uint32_t*>(w + l.len_stage),
                 reinterpret_cast<uint32_t*>(w + l.masks), (work_bytes - l.masks) / 32u};
    return 0;
}

// ReconstructData for one erasure pattern: the decode rows of the missing data shards over the
// good data shards and the first |missing| good parity shards.  x = A^-1 (parity_R + M[R][good] d)
// with A = M[R][missing]; the code is MDS, so any surviving set gives the same bytes.
struct Pattern {
    std::vector<uint16_t> srcs, tgts;
    std::vector<uint8_t> coef;  // tgts rows of coef_stride(srcs) bytes
};
bool solve_pattern(const uint8_t* mat, uint32_t D, uint32_t P, const uint32_t mask[8], Pattern* out) {
    auto bad = [&](uint32_t s) { return (mask[s >> 5] >> (s & 31u)) & 1u; };
    std::vector<uint16_t> miss, good, rows;
    for (uint32_t s = 0; s < D; s++) (bad(s) ? miss : good).push_back(static_cast<uint16_t>(s));
    const uint32_t e = static_cast<uint32_t>(miss.size());
    for (uint32_t r = 0; r < P && rows.size() < e; r++)
        if (!bad(D + r)) rows.push_back(static_cast<uint16_t>(r));
    if (rows.size() < e) return false;
    // [A | I] -> [I | A^-1]
    std::vector<uint8_t> A(size_t(e) * e), inv(size_t(e) * e, 0);
    for (uint32_t i = 0; i < e; i++) {
        inv[size_t(i) * e + i] = 1;
        for (uint32_t j = 0; j < e; j++) A[size_t(i) * e + j] = mat[size_t(rows[i]) * D + miss[j]];
    }
    for (uint32_t c = 0; c < e; c++) {
        uint32_t piv = c;
        while (piv < e && A[size_t(piv) * e + c] == 0) piv++;
        if (piv == e) return false;  // cannot happen for an MDS code
        if (piv != c)
            for (uint32_t k = 0; k < e; k++) {
                std::swap(A[size_t(piv) * e + k], A[size_t(c) * e + k]);
                std::swap(inv[size_t(piv) * e + k], inv[size_t(c) * e + k]);
            }
        const uint8_t s = gf_inv(A[size_t(c) * e + c]);
        for (uint32_t k = 0; k < e; k++) {
            A[size_t(c) * e + k] = gf_mul(A[size_t(c) * e + k], s);
            inv[size_t(c) * e + k] = gf_mul(inv[size_t(c) * e + k], s);
        }
        for (uint32_t r = 0; r < e; r++) {
            const uint8_t f = A[size_t(r) * e + c];
            if (r == c || f == 0) continue;
            for (uint32_t k = 0; k < e; k++) {
                A[size_t(r) * e + k] ^= gf_mul(f, A[size_t(c) * e + k]);
                inv[size_t(r) * e + k] ^= gf_mul(f, inv[size_t(c) * e + k]);
            }
        }
    }
    out->tgts = miss;
    out->srcs = good;
    for (uint16_t r : rows) out->srcs.push_back(static_cast<uint16_t>(D + r));
    const uint32_t ns = static_cast<uint32_t>(out->srcs.size()), ng = static_cast<uint32_t>(good.size());
    const uint32_t cs = eccdev::coef_stride(ns);
    out->coef.assign(size_t(e) * cs, 0);
    for (uint32_t m = 0; m < e; m++) {
        for (uint32_t gi = 0; gi < ng; gi++) {
            uint8_t acc = 0;
            for (uint32_t i = 0; i < e; i++) acc ^= gf_mul(inv[size_t(m) * e + i], mat[size_t(rows[i]) * D + good[gi]]);
            out->coef[size_t(m) * cs + gi] = acc;
        }
        for (uint32_t i = 0; i < e; i++) out->coef[size_t(m) * cs + ng + i] = inv[size_t(m) * e + i];
    }
    return true;
}

template <class T>
int upload(const std::vector<T>& v, T** d) {
    *d = nullptr;
    if (v.empty()) return 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), v.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : hip_error(e, "ECC repair tables upload");
}

}  // namespace
}  // namespace kcdc

using namespace kcdc;

extern "C" uint64_t kcdc_ecc_workspace_size(uint64_t total_stored_bytes, uint32_t nchunks) {
    return ecc_ws(total_stored_bytes, nchunks).total;
}

extern "C" int kcdc_ecc_encode_chunks_device(const char* alg, int32_t overhead_percent, int32_t max_shard_size,
                                             const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_lens,
                                             uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets,
                                             int32_t* d_status, void* stream) {
    EccParams p{};
    int rc = ecc_args(alg, overhead_percent, max_shard_size, &p);
    if (rc) return rc;
    if (nchunks == 0) return 0;
    if (!d_data || !d_offsets || !d_lens || !d_out || !d_out_offsets || !d_status) return set_error(-22, "null argument");
    const uint8_t* mat = device_matrix(p, &rc);
    if (!mat) return rc;
    const EncArgs a{d_data, d_offsets, d_lens, d_out, d_out_offsets, d_status, p, mat};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(nchunks, eccdev::kGridY);
    hipLaunchKernelGGL(eccdev::ecc_parity_kernel, grid, dim3(eccdev::kThreads), 0, st, a);
    hipLaunchKernelGGL(eccdev::ecc_records_kernel<false>, grid, dim3(eccdev::kThreads), 0, st, a, DecArgs{});
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_error(e, "ECC encode kernel launch");
}

extern "C" int kcdc_ecc_decode_chunks_device(const char* alg, int32_t overhead_percent, int32_t max_shard_size,
                                             const uint8_t* d_stored, const uint64_t* d_offsets,
                                             const uint64_t* d_stored_lens, uint32_t nchunks, uint8_t* d_out,
                                             const uint64_t* d_out_offsets, uint64_t* d_out_lens, int32_t* d_status,
                                             void* d_work, uint64_t work_bytes, void* stream) {
    DecArgs a{};
    const int rc = dec_args(alg, overhead_percent, max_shard_size, d_stored, d_offsets, d_stored_lens, nchunks, d_out,
                            d_out_offsets, d_out_lens, d_status, d_work, work_bytes, &a);
    if (rc || nchunks == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = a.mask_blocks ? hipMemsetAsync(a.masks, 0, a.mask_blocks * 32u, st) : hipSuccess;
    if (e != hipSuccess) return hip_error(e, "ECC mask clear");
    const dim3 grid(nchunks, eccdev::kGridY);
    hipLaunchKernelGGL(eccdev::ecc_decode_init_kernel, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(eccdev::ecc_records_kernel<true>, grid, dim3(eccdev::kThreads), 0, st, EncArgs{}, a);
    hipLaunchKernelGGL(eccdev::ecc_decode_finish_kernel, dim3(nchunks), dim3(eccdev::kThreads), 0, st, a);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_error(e, "ECC decode kernel launch");
}

extern "C" int kcdc_ecc_repair_chunks_device(const char* alg, int32_t overhead_percent, int32_t max_shard_size,
                                             const uint8_t* d_stored, const uint64_t* d_offsets,
                                             const uint64_t* d_stored_lens, uint32_t nchunks, uint8_t* d_out,
                                             const uint64_t* d_out_offsets, uint64_t* d_out_lens, int32_t* d_status,
                                             void* d_work, uint64_t work_bytes, void* stream) {
    DecArgs a{};
    int rc = dec_args(alg, overhead_percent, max_shard_size, d_stored, d_offsets, d_stored_lens, nchunks, d_out,
                      d_out_offsets, d_out_lens, d_status, d_work, work_bytes, &a);
    if (rc || nchunks == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_error(e, "ECC repair: stream sync");
    std::vector<int32_t> status(nchunks);
    if ((e = hipMemcpy(status.data(), d_status, size_t(nchunks) * 4u, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_error(e, "ECC repair: status readback");
    std::vector<uint32_t> damaged;
    for (uint32_t i = 0; i < nchunks; i++)
        if (status[i] == KCDC_ECC_DAMAGED) damaged.push_back(i);
    if (damaged.empty()) return 0;
    std::vector<uint64_t> lens(nchunks), blk_off(nchunks);
    if ((e = hipMemcpy(lens.data(), d_stored_lens, size_t(nchunks) * 8u, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(blk_off.data(), a.blk_off, size_t(nchunks) * 8u, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_error(e, "ECC repair: length readback");

    const EccParams& p = a.prm;
    std::vector<uint8_t> big(size_t(p.data) * p.parity), small(size_t(kEccSmallData) * kEccSmallParity);
    if ((rc = ecc_matrix(p.data, p.parity, big.data())) != 0) return rc;
    if ((rc = ecc_matrix(kEccSmallData, kEccSmallParity, small.data())) != 0) return rc;

    // pattern -> its tables' place in the uploads (per code: the small code's patterns are keyed apart)
    struct Placed {
        uint32_t coef_off, idx_off, rows, nsrc;
    };
    std::map<std::vector<uint32_t>, Placed> placed;
    std::vector<uint8_t> coef;
    std::vector<uint16_t> idx;
    std::vector<eccdev::RepJob> jobs;
    std::vector<eccdev::RepFin> fin;
    std::vector<uint32_t> masks;
    for (uint32_t c : damaged) {
        const EccGeo g = ecc_geo_stored(p, lens[c]);
        if (blk_off[c] == eccdev::kNoRoom || blk_off[c] + g.blocks > a.mask_blocks)
            return set_error(-22, "ECC repair: not the workspace of this launch's decode call");
        masks.resize(size_t(g.blocks) * 8u);
        if ((e = hipMemcpy(masks.data(), a.masks + blk_off[c] * 8u, masks.size() * 4u, hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_error(e, "ECC repair: mask readback");
        uint32_t flags = 0;
        const size_t first_job = jobs.size();
        for (uint64_t b = 0; b < g.blocks && !(flags & 0x100u); b++) {
            const uint32_t* m = &masks[size_t(b) * 8u];
            uint32_t nbad = 0, nbad_data = 0;
            for (uint32_t s = 0; s < g.shards(); s++)
                if ((m[s >> 5] >> (s & 31u)) & 1u) {
                    nbad++;
                    if (s < g.data) nbad_data++;
                }
            if (nbad > g.parity) {  // reedsolomon.ErrTooFewShards
                flags = 0x100u;
                break;
            }
            if (nbad_data == 0) continue;  // lost parity needs no rebuilding
            std::vector<uint32_t> key(m, m + 8);
            key.push_back(g.small ? 1u : 0u);
            auto it = placed.find(key);
            if (it == placed.end()) {
                Pattern pat;
                if (!solve_pattern(g.small ? small.data() : big.data(), g.data, g.parity, m, &pat))
                    return set_error(-5, "ECC repair: singular decode matrix");
                const Placed pl{static_cast<uint32_t>(coef.size()), static_cast<uint32_t>(idx.size()),
                                static_cast<uint32_t>(pat.tgts.size()), static_cast<uint32_t>(pat.srcs.size())};
                coef.insert(coef.end(), pat.coef.begin(), pat.coef.end());
                idx.insert(idx.end(), pat.srcs.begin(), pat.srcs.end());
                idx.insert(idx.end(), pat.tgts.begin(), pat.tgts.end());
                it = placed.emplace(key, pl).first;
            }
            const Placed& pl = it->second;
            jobs.push_back(eccdev::RepJob{b, c, pl.rows, pl.nsrc, pl.coef_off, pl.idx_off, 0});
            if (b == 0)  // the shards that hold the 4 length bytes (readLength, ecc_rs_crc.go:352-394)
                for (uint32_t k = 0; k < kEccLengthSize; k++) {
                    const uint32_t s = k / g.shard;
                    if ((m[s >> 5] >> (s & 31u)) & 1u) flags |= 1u << k;
                }
        }
        if (flags & 0x100u) jobs.resize(first_job);
        fin.push_back(eccdev::RepFin{c, flags});
    }

    uint8_t* d_coef = nullptr;
    uint16_t* d_idx = nullptr;
    eccdev::RepJob* d_jobs = nullptr;
    eccdev::RepFin* d_fin = nullptr;
    rc = upload(coef, &d_coef);
    if (!rc) rc = upload(idx, &d_idx);
    if (!rc) rc = upload(jobs, &d_jobs);
    if (!rc) rc = upload(fin, &d_fin);
    if (!rc) {
        if (!jobs.empty())
            hipLaunchKernelGGL(eccdev::ecc_repair_kernel, dim3(static_cast<uint32_t>(jobs.size()), 4), dim3(eccdev::kThreads),
                               0, st, a, d_jobs, d_coef, d_idx);
        hipLaunchKernelGGL(eccdev::ecc_repair_finish_kernel, dim3(static_cast<uint32_t>(fin.size())),
                           dim3(eccdev::kThreads), 0, st, a, d_fin);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = hip_error(e, "ECC repair kernels");
    }
    if (d_coef) (void)hipFree(d_coef);
    if (d_idx) (void)hipFree(d_idx);
    if (d_jobs) (void)hipFree(d_jobs);
    if (d_fin) (void)hipFree(d_fin);
    return rc;
}
