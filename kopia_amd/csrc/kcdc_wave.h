// Wave-level helpers shared by the compression, decompression and inflate kernels
// (kcdc_compress.hip, kcdc_decompress.hip, kcdc_inflate.hip): the CRC shift machinery of zlib's crc32_combine (multmodp, the x^(2^k)
// tables, the LDS byte table, the CRC of a 32 KiB piece by one wave) and a copy of bytes at any
// alignment by one wave.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KCDC_WAVE_HD __host__ __device__ __forceinline__
#else
#define KCDC_WAVE_HD inline
#endif

namespace kcdc {
namespace compdev {

// crc32(A || B) = crc32(A) * x^(8|B|) ^ crc32(B) in GF(2)[x] / P (zlib's crc32_combine), and the
// raw CRC (register 0, no final XOR) ignores leading zero bytes.
constexpr uint32_t kCrcPoly = 0xEDB88320u;   // CRC-32 (gzip), reflected
constexpr uint32_t kCrc32cPoly = 0x82F63B78u; // CRC-32C (Castagnoli: the S2 / Snappy framing), reflected
KCDC_WAVE_HD uint32_t multmodp(uint32_t a, uint32_t b, uint32_t poly = kCrcPoly) {
    uint32_t p = 0;  // a * b mod P (reflected)
    for (int i = 31; i >= 0; i--) {
        p ^= ((a >> i) & 1u) ? b : 0u;
        b = (b >> 1) ^ (poly & (0u - (b & 1u)));
    }
    return p;
}

// out[k] = x^(2^k) mod P (zlib's x2n_table)
KCDC_WAVE_HD void crc_x2n_table(uint32_t poly, uint32_t out[32]) {
    uint32_t p = 1u << 30;  // x^1
    for (int k = 0; k < 32; k++) {
        out[k] = p;
        p = multmodp(p, p, poly);
    }
}

// The standard CRC (register ~0, final XOR) of an n-byte message from its raw CRC (register 0, no
// final XOR): raw ^ (~0 * x^(8 n) mod P) ^ ~0.  x2n: crc_x2n_table of the same polynomial.
KCDC_WAVE_HD uint32_t crc_finish(uint32_t raw, uint64_t n, const uint32_t* x2n, uint32_t poly) {
    uint32_t z = 0x80000000u;  // x^0
    for (int bit = 0; n; bit++, n >>= 1)
        if (n & 1u) z = multmodp(z, x2n[(3 + bit) & 31], poly);
    return raw ^ multmodp(z, 0xFFFFFFFFu, poly) ^ 0xFFFFFFFFu;
}

#if defined(__HIPCC__)
// The byte table of `poly` in LDS, 32 copies: lane l reads copy l & 31 (conflict free), entry x of
// copy c at tab[32 x + ((c + x) & 31)].  Every thread of the workgroup calls it; a barrier follows.
__device__ __forceinline__ void crc_table_fill(uint32_t* tab, uint32_t poly, uint32_t nthreads) {
    for (uint32_t x = threadIdx.x; x < 256u; x += nthreads) {
        uint32_t r = x;
        for (int k = 0; k < 8; k++) r = (r >> 1) ^ (poly & (0u - (r & 1u)));
        for (uint32_t c = 0; c < 32u; c++) tab[32u * x + ((c + x) & 31u)] = r;
    }
}

// n bytes from src to dst, both at any alignment, by one wave: byte stores for dst's partial
// head and tail words, aligned dword stores (from two aligned loads + alignbit) in between.
// Only aligned source words holding a byte of [src, src + n) are read.
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
    const uint32_t head = min(n, static_cast<uint32_t>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    if (lane < head) dst[lane] = src[lane];
    const uint32_t m = (n - head) >> 2;
    uint32_t* __restrict__ dw = reinterpret_cast<uint32_t*>(dst + head);
    const uint8_t* s0 = src + head;
    const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(s0) & 3u);
    const uint32_t* __restrict__ sw = reinterpret_cast<const uint32_t*>(s0 - sh);
    // 8 words per lane in flight per round (loads first, then stores): one dependent load per
    // 256 bytes left a copy latency-bound at the emit kernel's two waves per CU
    constexpr uint32_t kU = 8;
    uint32_t i = lane;
    for (; i + 64u * (kU - 1u) < m; i += 64u * kU) {
        uint32_t w0[kU], w1[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) {
            w0[u] = sw[i + 64u * u];
            w1[u] = sh ? sw[i + 64u * u + 1u] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) dw[i + 64u * u] = __builtin_amdgcn_alignbit(w1[u], w0[u], 8u * sh);
    }
    for (; i < m; i += 64u) {
        const uint32_t w0 = sw[i];
        const uint32_t w1 = sh ? sw[i + 1] : 0u;
        dw[i] = __builtin_amdgcn_alignbit(w1, w0, 8u * sh);
    }
    const uint32_t done = head + 4u * m;
    if (lane < n - done) dst[done + lane] = src[done + lane];
}

constexpr uint32_t kPiece = 32768;  // CRC piece: 64 lanes of 512 bytes
// Raw CRC of `poly` (register 0) of the `len` <= kPiece bytes at p by one wave: lanes take 512 bytes each,
// counted back from the piece's end (bytes before it count as zeros, which a raw CRC ignores), and
// combine in a 6-level tree with x^(2^(12+j)).  All lanes return the value of lane 0's tree.
__device__ __forceinline__ uint32_t piece_crc(const uint8_t* p, uint32_t len, const uint32_t* tab,
                                              const uint32_t* x2nc, uint32_t poly, uint32_t lane) {
    const uint32_t sel = lane & 31u;
    int32_t pos = static_cast<int32_t>(len) - static_cast<int32_t>(kPiece) + 512 * static_cast<int32_t>(lane);
    const int32_t end = pos + 512;  // <= len
    if (pos < 0) pos = 0;
    uint32_t r = 0;
    auto byte = [&](uint32_t v) { r = (r >> 8) ^ tab[32u * ((r ^ v) & 255u) + sel]; };
    while (pos < end && (reinterpret_cast<uintptr_t>(p + pos) & 3u)) byte(p[pos++]);
    for (; pos + 4 <= end; pos += 4) {
        r ^= *reinterpret_cast<const uint32_t*>(p + pos);
#pragma unroll
        for (int t = 0; t < 4; t++) r = (r >> 8) ^ tab[32u * (r & 255u) + sel];
    }
    while (pos < end) byte(p[pos++]);
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const uint32_t right = __shfl_down(r, 1u << j, 64);
        // the shift constant pinned in a VGPR: as a uniform value its 32-step chain of multiples is
        // hoisted out of the caller's loop into SGPRs, six chains of them, and those spill
        uint32_t shift = x2nc[12 + j];
        asm volatile("" : "+v"(shift));
        if (((lane >> j) & 1u) == 0u) r = multmodp(r, shift, poly) ^ right;
    }
    return __shfl(r, 0, 64);
}
#endif

}  // namespace compdev
}  // namespace kcdc
