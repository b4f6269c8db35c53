// Splitter kernels, part 1 of 9: what every other part builds on.  The vector and wave
// constants, the tile limits, the one-instruction roll (roll3), wave-uniform values (uni64),
// byte extraction (byte_at) and the Loader: a stream addressed in coordinates through a buffer
// descriptor whose range check turns the bytes before and after the stream into zeros.
//
// Key identity: the rolling hash is never reset inside a stream and always
// equals the hash of the 64 bytes ending at the current position (zero bytes before the stream
// start).  So cand(p) := hash(p) & mask == 0 is a pure function of bytes p-63..p; every kernel
// of kcdc_split_*.h rests on that.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_split_config.h"

namespace kcdc {
namespace dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr int kBlk = 128;               // bytes per lane per step (one cache line)
constexpr int kNdw = kBlk / 4;          // dwords per lane per step
constexpr int64_t kLaneMax = 2048;      // max bytes per lane segment (tile = 64 x kLaneMax)
constexpr uint64_t kTileDiv = 256;  // batch lane segments <= avg / kTileDiv (tiles ~ avg / 4), >= 256 B
constexpr uint64_t kBuzLaneMax = 2048;  // the buzhash batch kernel's lane segment cap
constexpr int kSchedWindow = 16;        // bytes per scheduling window in the warm-up / exact loops
constexpr int kLookahead = 16;          // 128-byte steps: table reads issued this many bytes ahead (VGPR bound)

enum Mode { kWarm = 0, kFast = 1 };

__device__ __forceinline__ uint32_t rotl1(uint32_t h) { return __builtin_amdgcn_alignbit(h, h, 31); }
__device__ __forceinline__ uint32_t rotl_n(uint32_t v, uint32_t r) { return r ? (v << r) | (v >> (32 - r)) : v; }

// h' = rotl(h,1) ^ a ^ b as ONE v_bitop3 (truth table 0x96 = 3-input XOR; gfx950 has no
// v_xor3).  hipcc otherwise emits xor + bitop3 per byte.  The builtin, not inline asm:
// the hazard recognizer pads inline-asm VALU with s_nops (76 per 128 bytes).
__device__ __forceinline__ uint32_t roll3(uint32_t h, uint32_t a, uint32_t b) {
    return __builtin_amdgcn_bitop3_b32(rotl1(h), a, b, 0x96);
}

__device__ __forceinline__ uint64_t uni64(uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// Byte i of a block held as dwords.
template <int N>
__device__ __forceinline__ uint32_t byte_at(const uint32_t (&dw)[N], int i) {
    return __builtin_amdgcn_perm(0u, dw[i >> 2], 0x0c0c0c00u | static_cast<uint32_t>(i & 3));
}

// ---------------------------------------------------------------- loaders
// A stream is addressed in "coordinates" c = position + off0 relative to the
// 16-byte-aligned base `abase`; coordinates < off0 are the virtual zero bytes
// before the stream start.  Loads go through a buffer descriptor whose range
// check returns zeros for out-of-range (including negative) offsets.
struct Loader {
    __amdgpu_buffer_rsrc_t rsrc;
    u32x4 d;       // the same descriptor as four dwords (operand of the inline-asm LDS-DMA)
    int64_t tb;    // coordinate of descriptor offset 0
    int64_t off0;  // stream misalignment (0..15)

    template <int N>
    __device__ __forceinline__ void load(int64_t c, uint32_t (&dw)[N]) const {
        const int32_t vo = static_cast<int32_t>(c - tb);
#pragma unroll
        for (int j = 0; j < N / 4; j++) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo + 16 * j, 0, 0);
            dw[4 * j + 0] = v.x;
            dw[4 * j + 1] = v.y;
            dw[4 * j + 2] = v.z;
            dw[4 * j + 3] = v.w;
        }
        if (c == 0 && off0) {  // zero the bytes that precede the stream in its first granule
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const int64_t keep_from = off0 - 4 * d;  // first byte of dword d to keep
                const uint32_t m = keep_from <= 0 ? 0xFFFFFFFFu
                                                  : (keep_from >= 4 ? 0u : (0xFFFFFFFFu << (8 * keep_from)));
                dw[d] &= m;
            }
        }
    }
};

__device__ __forceinline__ Loader make_loader(const uint8_t* abase, int64_t off0, int64_t nbytes_coord, int64_t tb) {
    // tb >= 0 and a multiple of 16; the descriptor covers [tb, round_up16(nbytes_coord)).
    int64_t nrec = ((nbytes_coord + 15) & ~int64_t(15)) - tb;
    if (nrec > 0x7FFFFF00ll) nrec = 0x7FFFFF00ll;
    if (nrec < 0) nrec = 0;
    Loader L;
    L.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(abase + tb), static_cast<short>(0),
                                               static_cast<int>(nrec), 0x00020000);
    const uint64_t base = reinterpret_cast<uint64_t>(abase + tb);
    L.d.x = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
    L.d.y = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32) & 0xFFFFu);  // stride 0
    L.d.z = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(nrec));
    L.d.w = 0x00020000u;
    L.tb = tb;
    L.off0 = off0;
    return L;
}

}  // namespace dev
}  // namespace kcdc
