// Splitter kernels, part 3 of 9: the batch kernels' arguments and the LDS-DMA feed.
// BatchArgs (one launch: streams, cut ranges, queue workspace, hash parameters), HashSmem /
// fill_tables / make_hash (the per-workgroup tables of the scan_region() kernels), then the feed
// of the batch and long-path kernels: bytes arrive by LDS-DMA in 128-byte steps, one coalesced
// request per line, into per-wave step slots with a swizzle that keeps the ds_read_b128 lane
// groups conflict-free (dma_step128 / read_step128).  TileGeom: the lane segments of a tile.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_internal.h"
#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_hash.h"

namespace kcdc {
namespace dev {

// ------------------------------------------------------------ batch kernel
struct BatchArgs {
    const uint8_t* const* ptrs;
    const uint64_t* lens;
    uint64_t* cuts;
    const uint64_t* cut_base;
    uint64_t* counts;
    uint32_t* queue;  // persistent-wave work counter (zeroed before each launch)
    // Time-sliced stream queue (LDS-DMA kernel): header words kQHead (tickets taken),
    // kQTail (streams yielded), kQDone (streams finished), kQErr (spin give-ups); ring[P]
    // holds {push number + 1, sid} of yielded streams (0 = empty; zeroed per launch, reset
    // on take).
    uint32_t* ring;
    uint64_t* help;       // help slots of the pipelined buzhash kernel (split_batch_pipe_kernel), else null
    uint32_t help_waves;  // launch waves = help slots
    uint32_t ring_mask;
    uint64_t* trace;  // KCDC_TRACE builds: 8 words per wave (split_batch_pipe_kernel) (else null)
    uint64_t cuts_cap;
    const uint64_t* cut_end;  // optional: stream i's cut range ends at cut_end[i] (else cut_base[i+1] / cuts_cap)
    const uint64_t* starts;   // optional: stream i's first chunk starts at starts[i] (else 0); the bytes before
                              // it are the window history of a continued stream (kcdc_bw_*)
    const uint64_t* resume;   // optional (with starts): the first chunk's test range resumes at resume[i]
    uint64_t min_size, max_size;
    const uint32_t* buz;
    const uint64_t* rk_out;
    const uint64_t* rk_mod;
    uint32_t nstreams;
    uint32_t mask;     // buzhash: the candidate mask in the rotated frame (below); rabin: as is
    uint32_t rk_shift;
    // buzhash rotated frame: the tables hold rotl(T, buz_rot), so every hash value is
    // rotl(H, buz_rot) and the test is (h & mask) == 0 with mask = rotl(avg - 1, buz_rot).
    // For avg a power of two buz_rot = 32 - log2(avg) moves the mask to the top bits and
    // "candidate" becomes h <= buz_lim (= ~mask): the hot loop's test is a bare v_min3.
    uint32_t buz_rot;
    uint32_t buz_lim;  // ~mask when mask is a top-bits mask (else unused)
    // Batch tiles: bytes per lane segment at most (a tile is 64 of them, ~avg/4): the scan of
    // a chunk's region stops at the tile holding its first candidate, and a tile of avg bytes
    // overshoots by ~58 % on average (exponential candidate gaps), one of avg/4 by ~13 %.
    uint32_t lane_cap;
    // Batch kernels: a region is published to helpers in windows of this many tiles (0:
    // the whole region).  Helpers claim a published window's tiles from its top down, so over a
    // whole region they scan its far end, which the owner's first candidate usually makes moot;
    // a window keeps them just ahead of the owner (re-published as the owner passes it).
    uint32_t help_window;
};

// End of stream sid's cut range (exclusive).
__device__ __forceinline__ uint64_t cut_end_of(const BatchArgs& a, uint32_t sid) {
    return a.cut_end ? a.cut_end[sid] : sid + 1 < a.nstreams ? a.cut_base[sid + 1] : a.cuts_cap;
}

template <int KIND>
struct HashSmem;
template <>
struct HashSmem<kBuzhash> {
    BuzShared s;
};
template <>
struct HashSmem<kRabinKarp> {
    RabinShared s;
};

template <int KIND>
__device__ __forceinline__ void fill_tables(HashSmem<KIND>& sm, const BatchArgs& a) {
    if constexpr (KIND == kBuzhash) {
        for (uint32_t i = threadIdx.x; i < 256u * 64u; i += blockDim.x) sm.s.tab[i] = rotl_n(a.buz[i >> 6], a.buz_rot);
    } else {
        for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) {
            sm.s.out[i] = a.rk_out[i];
            sm.s.mod[i] = a.rk_mod[i];
        }
    }
    __syncthreads();
}

template <int KIND>
__device__ __forceinline__ auto make_hash(HashSmem<KIND>& sm, const BatchArgs& a, int lane) {
    if constexpr (KIND == kBuzhash) {
        BuzRing h;
        h.tab = reinterpret_cast<const char*>(sm.s.tab);
        h.lane4 = static_cast<uint32_t>(lane) * 4u;
        h.mask = a.mask;
        h.h = 0;
        return h;
    } else {
        Rabin h;
        h.tab = &sm.s;
        h.mask = a.mask;
        h.shift = a.rk_shift;
        h.v = 0;
        return h;
    }
}

// ------------------------------------------------ LDS-DMA fed batch path
// The per-lane 16-byte loads of scan_region() touch 64 different cache lines per instruction
// and are bound by the L1/L2 request rate, not HBM.  The batch and long-path kernels instead
// fetch every step by LDS-DMA (buffer_load_dwordx4 ... nt lds): each 128-byte line of a lane
// segment is one coalesced request (dma_step128), written to the wave's slot with a swizzle
// that keeps the ds_read_b128 lane groups conflict-free (read_step128).
// 8 waves x one 8 KiB step slot + 4 KiB warm slot (64 KiB table; 2 waves/SIMD, no VGPR spills):
// 4096 x 4 MiB 1.62 ms vs 12 waves 1.68, 7 waves 1.68 (round 1); deeper pipelines were slower
// (8 x 3 slots 1.68, 6 x 4 1.81, 4 x 6 2.00).
constexpr int kDmaWaves = 8;  // waves per workgroup (one workgroup per CU)
// Each step fetches 128 bytes (one whole cache line) of every lane segment, staged through
// ONE 8 KiB slot per wave: the step's bytes move to VGPRs at its start, which frees the
// slot for the next step's DMA while the step is hashed.
constexpr int kSlot = 64 * kWave;          // 4 KiB: one 64-byte piece of every lane (warm slot)
constexpr int kSlotBytes = 128 * kWave;    // 8 KiB: one 128-byte step of every lane
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// The table and the DMA slots are SEPARATE __shared__ objects: LDS lowering then gives
// them distinct alias scopes, so the waitcnt pass knows a table read cannot alias an
// in-flight LDS-DMA into a slot.  In one struct every table read waited vmcnt(0) for the
// DMA just issued, which serialised the prefetch with the hashing.
struct DmaSlots {
    __attribute__((aligned(16))) uint8_t b[kDmaWaves][1][kSlotBytes];
};
constexpr int kRkWaves = kDmaWaves;  // waves per workgroup of the Rabin-Karp DMA kernels
struct RkSlots {
    __attribute__((aligned(16))) uint8_t b[kRkWaves][1][kSlotBytes];
};

// One LDS-DMA wave instruction (64 lanes x 16 B -> 1 KiB at LDS address m0), written as
// inline asm so the waitcnt pass does not see an LDS-DMA: with several DMA sites and slots
// it ran out of alias-tracking slots and made table reads wait vmcnt for in-flight slot
// fills.  Every slot read here is preceded by an explicit s_waitcnt; M0 is used by no other
// code in these kernels.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {  // LDS byte address of a __shared__ pointer
    return __builtin_amdgcn_readfirstlane(
        static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_ptr_t)(const_cast<void*>(p)))));
}
__device__ __forceinline__ void dma_lds16(const u32x4& d, uint32_t m0, int32_t voff) {
    // nt: the stream bytes are read once (membench: 128-B runs 6.65 vs 6.38 TB/s without it)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen nt lds"
                 :: "s"(m0), "v"(voff), "s"(d) : "memory");
}

__device__ __forceinline__ void dma_piece(const Loader& ld, int64_t tb, uint32_t slot, int64_t ct,
                                          int64_t L, int64_t piece, int lane) {
    // descriptor offsets in 32 bits (ct - tb <= 64, a tile < 2^31 bytes): no per-lane 64-bit values
    const int32_t base = static_cast<int32_t>(ct - tb) + 64 * static_cast<int32_t>(piece), Li = static_cast<int32_t>(L);
    uint32_t sl = slot;  // opaque per call (as dma_step128): the m0 values are scalar adds, not spills
    asm volatile("" : "+s"(sl));
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int l = 16 * i + (lane >> 2);
        const int jj = (lane & 3) ^ ((l >> 2) & 3);
        dma_lds16(ld.d, sl + 1024u * i, base + l * Li + 16 * jj);
    }
}

__device__ __forceinline__ void read_piece(const uint8_t* slot, int lane, int64_t c, int64_t off0,
                                           uint32_t (&dw)[16]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int q = 4 * lane + (j ^ ((lane >> 2) & 3));
        const u32x4 v = *reinterpret_cast<const u32x4*>(slot + 16 * q);
        dw[4 * j + 0] = v.x;
        dw[4 * j + 1] = v.y;
        dw[4 * j + 2] = v.z;
        dw[4 * j + 3] = v.w;
    }
    if (c == 0 && off0) {  // bytes before the stream start are virtual zeros
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int64_t keep_from = off0 - 4 * d;
            const uint32_t m = keep_from <= 0 ? 0xFFFFFFFFu
                                              : (keep_from >= 4 ? 0u : (0xFFFFFFFFu << (8 * keep_from)));
            dw[d] &= m;
        }
    }
}

// 128-byte runs: DMA lane d of instruction i (0..7) fetches chunk (d&7) ^ sw(l) of lane
// l = 8i + d/8, so lane l's line lands at slot + 128 l with chunk j at granule j ^ sw(l);
// sw(l) = (l >> 1) & 7 gives every ds_read_b128 lane group 16 distinct 16-byte bank slots.
__device__ __forceinline__ void dma_step128(const Loader& ld, int64_t tb, uint32_t slot, int64_t ct,
                                            int64_t L, int64_t n, int lane) {
    const int32_t base = static_cast<int32_t>(ct - tb) + 128 * static_cast<int32_t>(n), Li = static_cast<int32_t>(L);
    // the slot address made opaque per call: its eight m0 values are then one scalar add each,
    // not eight values kept across the hash loop (they were SGPR spills, a v_readlane per DMA)
    uint32_t sl = slot;
    asm volatile("" : "+s"(sl));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int l = 8 * i + (lane >> 3);
        const int jj = (lane & 7) ^ ((l >> 1) & 7);
        dma_lds16(ld.d, sl + 1024u * i, base + l * Li + 16 * jj);
    }
}

__device__ __forceinline__ void read_step128(const uint8_t* slot, int lane, int64_t c, int64_t off0,
                                             uint32_t (&dw)[32]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(slot + 128 * lane + 16 * (j ^ ((lane >> 1) & 7)));
        dw[4 * j + 0] = v.x;
        dw[4 * j + 1] = v.y;
        dw[4 * j + 2] = v.z;
        dw[4 * j + 3] = v.w;
    }
    if (c == 0 && off0) {  // bytes before the stream start are virtual zeros
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int64_t keep_from = off0 - 4 * d;
            const uint32_t m = keep_from <= 0 ? 0xFFFFFFFFu
                                              : (keep_from >= 4 ? 0u : (0xFFFFFFFFu << (8 * keep_from)));
            dw[d] &= m;
        }
    }
}

// The same with the head test precomputed (head: this lane's step starts at coordinate 0).
__device__ __forceinline__ void read_step128h(const uint8_t* slot, int lane, bool head, int64_t off0,
                                              uint32_t (&dw)[32]) {
    read_step128(slot, lane, head ? 0 : 1, off0, dw);
}

// Geometry of the tile starting at ct (lane segments of L bytes, nb 128-byte steps).
struct TileGeom {
    int64_t L;
    int nb;
    Loader ld;
};
__device__ __forceinline__ TileGeom tile_geom(int64_t ct, int64_t hi, const uint8_t* abase, int64_t off0,
                                              int64_t nbytes_coord, int64_t lane_cap = kLaneMax) {
    const int64_t rem = hi - ct + 1;
    int64_t per = (rem + kWave - 1) / kWave;
    per = (per + 127) & ~int64_t(127);
    TileGeom g;
    g.L = per < lane_cap ? per : lane_cap;
    g.nb = static_cast<int>(g.L / 128);
    g.ld = make_loader(abase, off0, nbytes_coord, ct >= 64 ? ct - 64 : 0);
    return g;
}

// Scan budget meaning "never yield" (a visit's quantum when no stream waits).
constexpr int64_t kNoYield = int64_t(1) << 62;

}  // namespace dev
}  // namespace kcdc
