// Splitter kernels, part 4 of 9: the ticketed ring queue and the help slots.
// Agent-scope atomics, the queue header's word layout, PStream (a wave's current stream or help
// task), pcheck (KCDC_DEBUG_CHECKS builds), ring entries and tickets, the blocking take and the
// steal scan, and the help slots through which a region's owner publishes its tiles to waiting
// waves.  Both batch kernels run over this queue; tests/queue_model.py is its Python model.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_hash.h"
#include "kcdc_split_feed.h"

namespace kcdc {
namespace dev {

// ------------------------------------------- agent-scope atomics, queue header
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(1))) uint64_t gu64;
__device__ __forceinline__ uint32_t ld_agent(uint32_t* p) {
    return __hip_atomic_load((gu32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_agent64(uint64_t* p) {
    return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent64(uint64_t* p, uint64_t v) {
    __hip_atomic_store((gu64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t add_agent(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_add((gu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t bcast(uint32_t v) { return __builtin_amdgcn_readfirstlane(__shfl(v, 0)); }
__device__ __forceinline__ uint64_t bcast64(uint64_t v) {
    return (static_cast<uint64_t>(bcast(static_cast<uint32_t>(v >> 32))) << 32) | bcast(static_cast<uint32_t>(v));
}
// Header words (uint32 offsets) 2 KiB apart: hammered counters do not share DRAM pages.
// Word 0 holds the 64-bit {head, tail} ticket counter (kQHT, below).
constexpr int kQDone = 512, kQErr = 1536, kQSteal = 1024, kQHelp = 1600;
// Rarely read words (kept out of the kernel arguments, whose SGPRs the hot loop needs):
// kQCfg+0 spin cap, kQCfg+1 steal period; kQFlags.. one flag per workgroup (grid <= 256):
// 0 until workgroup b starts (1) or a waiting wave requeues its preassigned streams (2).
constexpr int kQCfg = 1040, kQFlags = 1088;
constexpr uint32_t kMaxPipeGrid = 256;
constexpr size_t kQHeaderBytes = 8192;
// Header words 1792.. : debug-build failure record (pcheck, KCDC_DEBUG_CHECKS).
[[maybe_unused]] constexpr int kQStat = 1792;
// Header words 1664.. : held-ticket audit (help tasks) -- [0] help tasks whose ticket register
// disagreed with the ticket's memory copy, [1] [2] the first such pair (register, memory);
// diagnostic builds (KCDC_HELP_DIAG) also [3] a bitmask of wave-uniform control values seen
// lane-divergent at the loop top and [4] the count of such observations.
constexpr int kQDiag = 1664;
// A waiting wave gives up (error word; a stream it held a ticket for is then reported failed)
// only after this many polls with no stream finishing: a bug guard that keeps the kernel
// bounded, >= 60 s; no correct launch waits that long (one wave scans >= 6 GB/s).
constexpr uint32_t kSpinCap = 1u << 26;
constexpr uint32_t kStealSpins = 256;                            // ~0.5 ms of polling between steal scans

// ======================================================= pipelined persistent kernel
// One per-wave state machine over tiles.  Every tile warms its 64 lanes on the 64 bytes
// before their segments (a 4 KiB piece in the wave's warm slot) and hashes 16 steps of
// 128-byte runs (8 KiB step slot).  The warm piece and first step of the NEXT tile are
// DMA'd during the current tile's last step, so a tile boundary exposes no latency:
//  * next tile of the same region: known in advance (the owner's claim on it, below);
//  * next stream (quantum spent, or the region's last tile with no further region): the
//    next ticket is taken by an atomic at the START of that tile and its ring entry
//    (progress + stream parameters, 7 tagged 16-byte sc1 granules) loaded mid-tile.
// What a stream switch hides and what it does not (buzhash kernel):
//  * hidden under the hashing: the entry DMA, in a tile of three or more steps;
//  * exposed: the ticket add, waited for at the top of the switching tile together with
//    the tile's fills (~0.7 us there, traced: DESIGN.md §2.1); the adopted stream's first fill, issued after the
//    tile (visit_adopt's prefetch) behind the requeue write and the help close; in a one-
//    or two-step tile the entry DMA too; and a candidate that ends the stream: the next
//    ticket is then taken by the blocking take (atomic, entry load, fill: three round
//    trips in a row).
// A candidate that ends a region early (the next region is not known before the tile ends)
// and the first tile of the launch expose a DMA latency too.
// A region whose lo is the last byte of a 128-byte line starts its grid at lo + 1
// (region_ct0): regions of whole tiles end without a one-step tile.
//
// Intra-region help (round 4).  At the end of a batch -- and in any launch with fewer streams
// than waves (a writer round, a handful of files) -- waves wait with nothing to scan while each
// remaining region is walked tile by tile by the one wave that owns its stream: launch time vs
// stream count (profiles/r04/tail) put that tail at ~0.2 ms of a 1.4 ms config-2 launch.
// cand(p) is a pure function of the 64 bytes ending at p, so any wave can scan
// any tile of a region; only the FIRST candidate decides the cut.  So every owner publishes its
// region in its help slot: the tile grid (tile 0 at ct0, T bytes per tile, K tiles, region end
// hi) and a claim word {epoch | top | bottom}.  The owner claims its tiles from the bottom (one
// atomic add per tile, issued a step ahead of need); a waiting wave claims the top tile by
// compare-and-swap, scans it as a one-tile task and posts the tile's first candidate, tagged with
// the slot's epoch, in the slot's result row.  An owner whose claim fails resolves the region
// from the row: the first candidate in tile order, else the forced cut; a row entry still pending
// after kHelpWaitTicks is scanned by the owner itself, so no owner depends on another wave.
constexpr int64_t kPipeYield = 768 << 10;  // visit quantum while streams wait (384 K-1.5 M: within noise)
constexpr int kPEntryLanes = 8;
constexpr int kPEntryStride = 128;

struct WarmSlots {
    __attribute__((aligned(16))) uint8_t b[kDmaWaves][kSlot];  // 4 KiB: the 64 bytes before each lane segment
};
static_assert(sizeof(DmaSlots) + sizeof(WarmSlots) + sizeof(BuzShared) <= 160 * 1024,
              "step slots + warm slots + table exceed the CU's 160 KiB of LDS");

struct PStream {
    uint32_t sid;    // | kHelpBit for a help task
    int64_t n, off0;
    const uint8_t* abase;
    uint64_t cb, cap, cnt;  // help task: cb = owner slot, cnt = tile index
    int64_t s, ct;          // chunk start (help task: the owner's tile 0); next tile coordinate (< 0: not set up)
    uint32_t epoch;         // help task: the owner slot's epoch
    int64_t aux;            // help task: the region end (coordinate)
};
constexpr uint32_t kHelpBit = 0x80000000u;

__device__ __forceinline__ void pstream_fresh(PStream& st, uint32_t sid, uint64_t p, uint64_t n, uint64_t cb,
                                              uint64_t cend) {
    st.sid = sid;
    st.n = static_cast<int64_t>(n);
    st.off0 = static_cast<int64_t>(p & 15u);
    st.abase = reinterpret_cast<const uint8_t*>(p - static_cast<uint64_t>(st.off0));
    st.cb = cb;
    st.cap = cend > cb ? cend - cb : 0;
    st.cnt = 0;
    st.s = 0;
    st.ct = -1;
    st.epoch = 0;
    st.aux = 0;
}

// Pin every field to a scalar register: the uniformity analysis otherwise loses track of
// values carried through the switch paths, and each LDS-DMA (its buffer descriptor must be
// scalar) then sits in a readfirstlane waterfall loop.
__device__ __forceinline__ void uniformize(PStream& st) {
    st.sid = __builtin_amdgcn_readfirstlane(st.sid);
    st.n = static_cast<int64_t>(uni64(static_cast<uint64_t>(st.n)));
    st.off0 = static_cast<int64_t>(uni64(static_cast<uint64_t>(st.off0)));
    st.abase = reinterpret_cast<const uint8_t*>(uni64(reinterpret_cast<uint64_t>(st.abase)));
    st.cb = uni64(st.cb);
    st.cap = uni64(st.cap);
    st.cnt = uni64(st.cnt);
    st.s = static_cast<int64_t>(uni64(static_cast<uint64_t>(st.s)));
    st.ct = static_cast<int64_t>(uni64(static_cast<uint64_t>(st.ct)));
    st.epoch = __builtin_amdgcn_readfirstlane(st.epoch);
    st.aux = static_cast<int64_t>(uni64(static_cast<uint64_t>(st.aux)));
}

__device__ __forceinline__ void emit_cut(const BatchArgs& a, PStream& st, int lane, int64_t v) {
    if (lane == 0 && st.cnt < st.cap) a.cuts[st.cb + st.cnt] = static_cast<uint64_t>(v);
    st.cnt++;
}

// Tile 0 of the region [lo, hi] of the chunk starting at s (lo = s + min - 1 + off0, coordinates).
// Tiles start on 128-byte lines, so tile 0 is the line holding lo.  line_start (the buzhash batch
// kernel): when lo is the LAST byte of its line, tile 0 starts at lo + 1 instead -- lane 0's state
// after the warm-up of that tile is the hash at lo, which the kernel tests there.  The old grid
// spent a whole tile position on that one byte: with min and max - min multiples of the tile, a
// region without a candidate took a one-step tile more: a stream switch with nothing to hide its
// round trips under (7.8 us a tile in the trace of DESIGN.md §2.1; next to no fetch, its other
// lanes lie past the stream's end and are clipped).  A one-byte region (lo == hi) keeps the line rule.
// Only an owner's tile 0 can start at lo + 1: helpers claim tiles >= 1 (help_publish sets bottom
// = 1, help_find claims top - 1 >= bottom), windows and pending tiles re-start at tile >= 1, and
// resume_ct's tiles hold a position > lo.
__device__ __forceinline__ int64_t region_ct0(const BatchArgs& a, int64_t s, int64_t n, int64_t off0, bool line_start) {
    const int64_t lo = s + static_cast<int64_t>(a.min_size) - 1 + off0;
    if (line_start && (lo & 127) == 127) {
        const int64_t mx = s + static_cast<int64_t>(a.max_size) - 1;
        if (lo < (mx < n - 1 ? mx : n - 1) + off0) return lo + 1;
    }
    return lo & ~int64_t(127);
}

// Set up the next region to scan (chunks whose test range starts past the end are cut
// at once); returns false when the stream is finished (all cuts emitted).
__device__ __forceinline__ bool pstream_region(const BatchArgs& a, PStream& st, int lane, bool line_start = false) {
    while (st.ct < 0) {
        if (st.s >= st.n) return false;
        const int64_t pf = st.s + static_cast<int64_t>(a.min_size) - 1;
        if (pf >= st.n) {  // last chunk [s, n): nothing to test (splitter_buzhash32.go:29-40, 60-67)
            emit_cut(a, st, lane, st.n);
            st.s = st.n;
            return false;
        }
        st.ct = region_ct0(a, st.s, st.n, st.off0, line_start);
    }
    return true;
}

// First tile coordinate of stream e's first region when a previous round already tested the
// positions below resume[e] (kcdc_bw_*): the scan starts at the tile holding min(resume, region
// end) instead of at s + min - 1; -1 (set up as usual) otherwise.
__device__ __forceinline__ int64_t resume_ct(const BatchArgs& a, uint32_t e, int64_t s, int64_t n, int64_t off0) {
    if (!a.resume) return -1;
    const int64_t r = static_cast<int64_t>(a.resume[e]);
    const int64_t lo = s + static_cast<int64_t>(a.min_size) - 1;
    const int64_t mx = s + static_cast<int64_t>(a.max_size) - 1;
    const int64_t hi = mx < n - 1 ? mx : n - 1;
    if (lo > n - 1 || r <= lo) return -1;
    return ((r > hi ? hi : r) + off0) & ~int64_t(127);
}

// Ring entry of a yielded stream: granule l (< 7) = {tag, lo, hi, l == 0 ? sid : 0} of
// word l in {cnt, s, ct, ptr, n, cb, cap}.  Written by lane 0 alone (7 uniform 16-byte
// stores): a per-lane select chain over the words miscompiled (a word's high half read
// an undefined register).
__device__ __forceinline__ u32x4 pgranule(uint32_t tag, uint64_t w, uint32_t x) {
    u32x4 v;
    v.x = tag;
    v.y = static_cast<uint32_t>(w);
    v.z = static_cast<uint32_t>(w >> 32);
    v.w = x;
    return v;
}
// readlane returns int: widen through uint32_t, or a low word with bit 31 set sign-extends
// into the high word (it did: pointers came back as 0xFFFFFFFF'xxxxxxxx).
__device__ __forceinline__ uint64_t rl64(const u32x4& v, int l) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(v.y, l));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(v.z, l));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ void pentry_decode(PStream& st, const u32x4& v) {
    st.sid = __builtin_amdgcn_readlane(v.w, 0);
    st.cnt = rl64(v, 0);
    st.s = static_cast<int64_t>(rl64(v, 1));
    st.ct = static_cast<int64_t>(rl64(v, 2));
    const uint64_t p = rl64(v, 3);
    st.off0 = static_cast<int64_t>(p & 15u);
    st.abase = reinterpret_cast<const uint8_t*>(p - static_cast<uint64_t>(st.off0));
    st.n = static_cast<int64_t>(rl64(v, 4));
    st.cb = rl64(v, 5);
    st.cap = rl64(v, 6);
    st.aux = 0;
    st.epoch = 0;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pring_rsrc(const BatchArgs& a) {
    return __builtin_amdgcn_make_buffer_rsrc(a.ring, static_cast<short>(0),
                                             static_cast<int>((a.ring_mask + 1u) * kPEntryStride), 0x00020000);
}
// Every lane loads (lane & 7): no divergent load, so no copy of the result that would
// make the compiler wait for it early.
__device__ __forceinline__ u32x4 pentry_load(const BatchArgs& a, int lane, uint32_t e) {
    return __builtin_amdgcn_raw_buffer_load_b128(pring_rsrc(a),
                                                 static_cast<int>((e & a.ring_mask) * kPEntryStride) + 16 * (lane & 7), 0,
                                                 16 /* sc1 */);
}
__device__ __forceinline__ bool pentry_ok(const u32x4& v, int lane, uint32_t e) {
    return __ballot(lane < kPEntryLanes - 1 && v.x != e + 1u) == 0;
}

// Debug builds: validate a resolved stream against the batch arrays; on a mismatch record
// {code, sid, ticket, detail} in header words kQStat+16.. and return false (wave exits).
__device__ __forceinline__ bool pcheck(const BatchArgs& a, int lane, const PStream& st, uint32_t tk, uint32_t where) {
#if KCDC_DEBUG_CHECKS
    if (st.sid & kHelpBit) return true;
    uint32_t code = 0;
    uint64_t detail = 0;
    const uint32_t sid = st.sid;
    if (sid >= a.nstreams) {
        code = 1;
        detail = st.sid;
    } else {
        const uint64_t p = uni64(reinterpret_cast<uint64_t>(a.ptrs[sid]));
        const uint64_t cb = uni64(a.cut_base[sid]);
        if (reinterpret_cast<uint64_t>(st.abase) + static_cast<uint64_t>(st.off0) != p) {
            code = 2;
            detail = reinterpret_cast<uint64_t>(st.abase);
        } else if (static_cast<uint64_t>(st.n) != uni64(a.lens[sid])) {
            code = 3;
            detail = static_cast<uint64_t>(st.n);
        } else if (st.cb != cb) {
            code = 4;
            detail = st.cb;
        } else if (st.cnt > st.cap) {
            code = 5;
            detail = st.cnt;
        } else if (st.cap != uni64(cut_end_of(a, sid)) - cb) {
            code = 7;
            detail = st.cap;
        } else if (st.s < 0 || st.s > st.n) {
            code = 6;
            detail = static_cast<uint64_t>(st.s);
        }
    }
    if (code) {
        if (lane == 0) {
            if (atomicAdd(a.queue + kQErr, 1u) == 0) {
                a.queue[kQStat + 16] = code | (where << 8);
                a.queue[kQStat + 17] = st.sid;
                a.queue[kQStat + 18] = tk;
                a.queue[kQStat + 19] = static_cast<uint32_t>(detail);
                a.queue[kQStat + 20] = static_cast<uint32_t>(detail >> 32);
                a.queue[kQStat + 21] = static_cast<uint32_t>(st.s);
                a.queue[kQStat + 22] = static_cast<uint32_t>(st.ct);
                a.queue[kQStat + 23] = static_cast<uint32_t>(st.cnt);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return false;
    }
#endif
    return true;
}

// Queue counter: ONE 64-bit word {head = tickets taken (low), tail = entries reserved
// (high)} at header words 0..1, so a wave that yields one stream and takes the next does
// both with one atomic.  Entries 0..n-1 are the streams' initial states (init_ring_kernel
// writes them and sets tail = n); a reserved entry that ends up unused (its stream
// finished in the tile) is written as a tombstone (sid 0xFFFFFFFF), which a taker skips.
constexpr int kQHT = 0;
constexpr uint32_t kTombstone = 0xFFFFFFFFu;
__device__ __forceinline__ uint64_t qht_add(const BatchArgs& a, int lane, uint64_t inc) {
    uint64_t v = 0;
    if (lane == 0)
        v = __hip_atomic_fetch_add((gu64*)(reinterpret_cast<uint64_t*>(a.queue + kQHT)), inc, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
#if KCDC_DEBUG_CHECKS  // entries reserved (kQStat+32)
    if (lane == 0 && (inc >> 32)) add_agent(a.queue + kQStat + 32, static_cast<uint32_t>(inc >> 32));
#endif
    return v;  // lane 0's register
}
__device__ __forceinline__ uint64_t qht_value(uint32_t lo_raw, uint32_t hi_raw) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(lo_raw, 0));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(hi_raw, 0));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ uint64_t qht_take(const BatchArgs& a, int lane, uint64_t inc) {  // blocking
    const uint64_t raw = qht_add(a, lane, inc);
    return qht_value(static_cast<uint32_t>(raw), static_cast<uint32_t>(raw >> 32));
}

// Preassigned first tickets are spread over the grid: wave w of workgroup b holds ticket
// w * grid + b, so a launch with fewer streams than waves puts at most one owner on a CU (the
// others' SIMDs and DMA queues stay free for helpers).
__device__ __forceinline__ uint32_t first_ticket(uint32_t block, uint32_t wave) { return wave * gridDim.x + block; }

__device__ __forceinline__ void pwrite(const BatchArgs& a, int lane, uint32_t e, const PStream& st, bool tomb);

// Forward progress without co-residency.  Each wave's first ticket is preassigned
// (first_ticket, init_ring_kernel), so a workgroup that is not resident -- another kernel holds
// its CU -- would keep its streams while the resident waves wait for them.  A wave that has
// waited kStealSpins polls scans the workgroup flags; for a workgroup that has not started it
// swaps the flag 0 -> 2 and requeues that workgroup's preassigned streams as fresh ring
// entries (their initial states, rebuilt from the batch arrays).  A workgroup that starts
// later finds its flag at 2 and takes its tickets from the counter.  A waiting wave then
// waits only on entries reserved by running waves (written without blocking) or on streams
// held by running waves, so every wait ends.
__device__ bool try_steal(const BatchArgs& a, int lane, uint32_t wg_waves) {
    uint32_t found = 0xFFFFFFFFu;
    uint32_t* const flags = a.queue + kQFlags;
    const uint32_t nwg = gridDim.x;
    for (uint32_t b0 = 0; b0 < nwg; b0 += kWave) {
        const uint32_t b = b0 + static_cast<uint32_t>(lane);
        const uint32_t f = b < nwg ? ld_agent(flags + b) : 1u;
        const uint64_t m = __ballot(f == 0u);
        if (m) {
            found = b0 + static_cast<uint32_t>(__builtin_ctzll(m));
            break;
        }
    }
    found = __builtin_amdgcn_readfirstlane(found);
    if (found == 0xFFFFFFFFu) return false;
    uint32_t old = 1u;
    if (lane == 0) {
        old = 0u;
        __hip_atomic_compare_exchange_strong((gu32*)(flags + found), &old, 2u, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (bcast(old) != 0u) return false;  // it started (or another wave stole it) meanwhile
    uint32_t k = 0;
    for (uint32_t w = 0; w < wg_waves; w++) k += first_ticket(found, w) < a.nstreams ? 1u : 0u;
    if (k == 0) return true;
    const uint64_t ht = qht_take(a, lane, static_cast<uint64_t>(k) << 32);  // reserve k entries
    const uint32_t e0 = static_cast<uint32_t>(ht >> 32);
    for (uint32_t w = 0; w < k; w++) {  // first_ticket grows with w: the first k waves held streams
        const uint32_t sid = first_ticket(found, w);
        PStream st;
        const uint64_t cb = uni64(a.cut_base[sid]);
        pstream_fresh(st, sid, uni64(reinterpret_cast<uint64_t>(a.ptrs[sid])), uni64(a.lens[sid]), cb,
                      uni64(cut_end_of(a, sid)));
        if (a.starts) st.s = static_cast<int64_t>(uni64(a.starts[sid]));
        st.ct = resume_ct(a, sid, st.s, st.n, st.off0);
        uniformize(st);
        pwrite(a, lane, e0 + w, st, false);
    }
    if (lane == 0) add_agent(a.queue + kQSteal, 1u);
    return true;
}

// ------------------------------------------------------------------ help slots
// Slot g (one per launch wave) in the help area: claim word at 128 * g (own line), the region
// granules at kHelpParams + 64 * g, the result row at kHelpRows + 8 * kHelpTiles * g, and bit g
// of the published-slots bitmap at kHelpBits (set while the region is open: waiting waves read
// the bitmap, then the claim words of set slots, instead of probing slots blindly).
//   claim  {epoch:24 | top:20 | bottom:20}: tiles [0, bottom) are the owner's, [top, K) the
//          helpers'; epoch 0 = nothing published (init_ring_kernel zeroes every claim word).
//   params 4 granules {epoch, lo, hi, x}: {ptr, sid}, {n, K}, {ct0, T}, {hi, 0}.
//   row[k] {epoch:24 | state:8 | rel:32}: state 1 no candidate in tile k, 2 first candidate at
//          ct0 + rel; anything else (or another epoch) pending.  Posted by atomic max, so a
//          stale helper's older epoch never overwrites a newer result.
// a region is open to helpers while top >= bottom + kHelpGap (1 vs 2: 1.295 vs 1.332 ms on
// config 2, same-process A/B, profiles/r04/third/)
constexpr uint32_t kHelpGap = 1u;
constexpr uint64_t kHelpMinAvg = 1ull << 20;  // the launch's help policy (batch_plan): averages from here up (1 MiB)
// Every region is published (a tail-only policy -- publish only in visits that began with no
// stream waiting -- lost 2-10 % at 1M-4M; DESIGN.md §2.1, profiles/r05/help_tail_only/).
constexpr int64_t kHelpSplit = 2;     // sub-tiles per help task (lane segments lane_cap / 2, >= 256 B)
constexpr int kHelpTiles = 128;          // regions of up to 128 tiles take help (every registered name)
constexpr uint32_t kHelpMinTiles = 3u;  // the owner's tile, its next one, and at least one more
constexpr uint64_t kHelpWaitTicks = 20000;  // 200 us of s_memrealtime (a tile takes 15-40 us)
__device__ __forceinline__ size_t help_params_off(uint32_t nw) { return 128ull * nw; }
__device__ __forceinline__ size_t help_rows_off(uint32_t nw) { return 128ull * nw + 64ull * nw; }
__device__ __forceinline__ size_t help_bits_off(uint32_t nw) { return help_rows_off(nw) + 8ull * kHelpTiles * nw; }
__device__ __forceinline__ uint32_t* help_bits(const BatchArgs& a) {
    return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.help) + help_bits_off(a.help_waves));
}
__device__ __forceinline__ uint64_t* help_claim(const BatchArgs& a, uint32_t g) {
    return reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(a.help) + 128ull * g);
}
__device__ __forceinline__ uint64_t* help_row(const BatchArgs& a, uint32_t g) {
    return reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(a.help) + help_rows_off(a.help_waves)) +
           static_cast<uint64_t>(kHelpTiles) * g;
}
__device__ __forceinline__ uint64_t hclaim(uint32_t ep, uint32_t top, uint32_t bot) {
    return (static_cast<uint64_t>(ep) << 40) | (static_cast<uint64_t>(top) << 20) | bot;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t help_params_rsrc(const BatchArgs& a) {
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.help) + help_params_off(a.help_waves),
                                             static_cast<short>(0), static_cast<int>(64u * a.help_waves), 0x00020000);
}

// Owner: publish region [ct0, hi] (K tiles of T bytes, tile 0 already the owner's) in slot g
// under epoch ep.  Order: the row zeroed and the granules stored write-through (sc1), drained,
// then the claim word -- a helper that sees epoch ep in the claim word reads granules and a row
// of that epoch (or of a later one, when the owner has moved on and waits for nothing).
__device__ void help_publish(const BatchArgs& a, int lane, uint32_t g, uint32_t ep, const PStream& st, int64_t ct0,
                             int64_t hi, uint32_t K, int64_t T) {
    uint64_t* row = help_row(a, g);
    for (uint32_t k = static_cast<uint32_t>(lane); k < K; k += kWave)
        __hip_atomic_store((gu64*)(row + k), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) {
        const __amdgpu_buffer_rsrc_t r = help_params_rsrc(a);
        const int base = static_cast<int>(64u * g);
        const uint64_t p = reinterpret_cast<uint64_t>(st.abase) + static_cast<uint64_t>(st.off0);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(ep, p, st.sid), r, base + 0, 0, 16 /* sc1 */);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(ep, static_cast<uint64_t>(st.n), K), r, base + 16, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(ep, static_cast<uint64_t>(ct0), static_cast<uint32_t>(T)), r,
                                               base + 32, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(ep, static_cast<uint64_t>(hi), 0), r, base + 48, 0, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        __hip_atomic_store((gu64*)help_claim(a, g), hclaim(ep, K, 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or((gu32*)(help_bits(a) + (g >> 5)), 1u << (g & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Owner: no more tiles of this slot's region for helpers (the region or the visit ended).  The
// closed word carries the epoch with bit 23 set: claims of the open epoch fail, and a helper
// still scanning one of its tiles sees the change (every 4th step) and stops.
constexpr uint32_t kHelpClosed = 1u << 23;
__device__ __forceinline__ void help_close(const BatchArgs& a, int lane, uint32_t g, uint32_t ep) {
    if (lane == 0) {
        __hip_atomic_store((gu64*)help_claim(a, g), hclaim(ep | kHelpClosed, 0, 0), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_and((gu32*)(help_bits(a) + (g >> 5)), ~(1u << (g & 31u)), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Owner: read its claim word back by LDS-DMA (sc1, past L1) into LDS at m0 (16 bytes per lane,
// every lane the same granule: the word lands at m0).  The waitcnt pass does not see it (as the
// slot fills), so nothing waits for it inside the hash loop; the reader's own vmcnt wait does.
__device__ __forceinline__ void help_claim_dma(const BatchArgs& a, int lane, uint32_t g, uint32_t m0) {
    (void)lane;
    u32x4 d;
    const uint64_t base = reinterpret_cast<uint64_t>(a.help);
    d.x = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
    d.y = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32) & 0xFFFFu);
    d.z = __builtin_amdgcn_readfirstlane(128u * a.help_waves);
    d.w = 0x00020000u;
    const int32_t off = static_cast<int32_t>(128u * g);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen sc1 lds"
                 :: "s"(m0), "v"(off), "s"(d) : "memory");
}
// Helper: post tile k's first candidate (coordinate f, or -1) to slot g's row under epoch ep.
__device__ __forceinline__ void help_post(const BatchArgs& a, int lane, uint32_t g, uint32_t ep, uint32_t k,
                                          int64_t ct0, int64_t f) {
    const uint64_t v = (static_cast<uint64_t>(ep) << 40) |
                       (f >= 0 ? (2ull << 32) | static_cast<uint64_t>(static_cast<uint32_t>(f - ct0)) : (1ull << 32));
    if (lane == 0) {
        __hip_atomic_fetch_max((gu64*)(help_row(a, g) + k), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        add_agent(a.queue + kQHelp, 1u);
    }
}
// The ticket a wave holds while it runs help tasks: kept in memory (word 2 of its help slot's
// claim line) from the moment the help task is taken, and taken back from there when the task
// ends, besides the copy in the task's cap field.  held_get audits the two (header words kQDiag..).
__device__ __forceinline__ void held_put(const BatchArgs& a, int lane, uint32_t me, uint32_t t) {
    if (lane == 0)
        __hip_atomic_store((gu64*)(help_claim(a, me) + 2), 0x100000000ull | t, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t held_get(const BatchArgs& a, int lane, uint32_t me, uint32_t reg) {
    const uint64_t raw = ld_agent64(help_claim(a, me) + 2);
    const uint32_t t = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(raw), 0));
    if (t != reg && lane == 0) {
        if (atomicAdd(a.queue + kQDiag, 1u) == 0) {
            a.queue[kQDiag + 1] = reg;
            a.queue[kQDiag + 2] = t;
        }
    }
    return t;  // always memory's copy: the register copy is only audited
}
// Diagnostic builds: bit `bit` when v is not the same in every lane (a wave-uniform control value
// held lane-divergent).
__device__ __forceinline__ uint32_t divergent_bit(uint32_t v, int bit) {
    return __ballot(v != static_cast<uint32_t>(__shfl(static_cast<int>(v), 0))) != 0 ? 1u << bit : 0u;
}
__device__ __forceinline__ void diag_record(const BatchArgs& a, int lane, uint32_t bits) {
    if (bits && lane == 0) {
        atomicOr(a.queue + kQDiag + 3, bits);
        atomicAdd(a.queue + kQDiag + 4, 1u);
    }
}
// Owner whose claim failed: the helpers hold tiles [k0, K).  Returns the region's first
// candidate (coordinate) among them, -1 if they have none, or -2 - k when tile k is still
// pending after kHelpWaitTicks (the owner then scans from tile k itself).
__device__ int64_t help_wait(const BatchArgs& a, int lane, uint32_t g, uint32_t ep, uint32_t k0, uint32_t K,
                             int64_t ct0) {
    const uint64_t* row = help_row(a, g);
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        int64_t res = -1;
        uint32_t pend_at = 0xFFFFFFFFu;
        for (uint32_t b = k0; b < K; b += kWave) {
            const uint32_t k = b + static_cast<uint32_t>(lane);
            const uint64_t v = k < K ? ld_agent64(const_cast<uint64_t*>(row + k)) : 0ull;
            const bool mine = k < K && static_cast<uint32_t>(v >> 40) == ep;
            const uint32_t stt = mine ? static_cast<uint32_t>(v >> 32) & 0xFFu : 0u;
            const uint64_t pend = __ballot(k < K && stt != 1u && stt != 2u);
            const uint64_t cand = __ballot(stt == 2u);
            const uint64_t ev = pend | cand;
            if (ev) {
                const int f = __builtin_ctzll(ev);
                if ((cand >> f) & 1ull) {
                    const uint32_t rel = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(v), f));
                    res = ct0 + static_cast<int64_t>(rel);
                } else {
                    pend_at = b + static_cast<uint32_t>(f);
                }
                break;
            }
        }
        if (pend_at == 0xFFFFFFFFu) return res;
        if (__builtin_amdgcn_s_memrealtime() - t0 > kHelpWaitTicks) return -2 - static_cast<int64_t>(pend_at);
        __builtin_amdgcn_s_sleep(8);
    }
}
// Waiting wave: claim the top tile of an open region with many unclaimed tiles.  The bitmap
// names the open slots; each lane takes one set bit of one bitmap word (words and bits start at
// positions that rotate with the wave and the attempt, so waiting waves spread over the owners),
// reads that slot's claim word, and the lane with the most unclaimed tiles (ties: rotated) tries
// the compare-and-swap.  On success `task` is a one-tile help task: sid | kHelpBit, the stream's
// pointer and length, s = the owner's tile 0, ct = the tile, aux = the tile's end, cb = slot,
// cnt = tile index, epoch.
__device__ bool help_find(const BatchArgs& a, int lane, uint32_t me, uint32_t attempt, PStream& task) {
    const uint32_t nw = a.help_waves, nwords = (nw + 31u) >> 5;
    const uint32_t rot = me * 7u + attempt * 13u;
    const uint32_t wi = (static_cast<uint32_t>(lane) + rot) % nwords;
    uint32_t bits = static_cast<uint32_t>(lane) < nwords ? ld_agent(help_bits(a) + wi) : 0u;
    if (wi == (me >> 5)) bits &= ~(1u << (me & 31u));  // not our own slot
    uint32_t g = 0xFFFFFFFFu;
    if (bits) {
        const uint32_t r = (rot >> 3) & 31u;
        const uint32_t rb = (bits >> r) | (r ? bits << (32u - r) : 0u);  // rotate right by r
        g = (wi << 5) + ((static_cast<uint32_t>(__builtin_ctz(rb)) + r) & 31u);
    }
    const uint64_t c = g < nw ? ld_agent64(help_claim(a, g)) : 0ull;
    const uint32_t ep = static_cast<uint32_t>(c >> 40), top = static_cast<uint32_t>(c >> 20) & 0xFFFFFu,
                   bot = static_cast<uint32_t>(c) & 0xFFFFFu;
    // claim only tiles >= bottom + kHelpGap - 1 (gap 1: up to the owner's next tile, which the
    // owner then takes from the row instead of scanning it)
    const bool open = ep != 0u && !(ep & kHelpClosed) && top >= bot + kHelpGap;
    const uint32_t key = open ? ((top - bot) << 6) | ((static_cast<uint32_t>(lane) + rot) & 63u) : 0u;
    uint32_t best = key;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = max(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d)));
    best = __builtin_amdgcn_readfirstlane(best);
    if (best == 0u) return false;
    const int f = __builtin_ctzll(__ballot(key == best));
    const uint32_t gs = static_cast<uint32_t>(__builtin_amdgcn_readlane(g, f));
    const uint64_t cw = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(c >> 32), f)))
                         << 32) |
                        static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(c), f));
    uint64_t old = cw;
    if (lane == 0)
        __hip_atomic_compare_exchange_strong((gu64*)help_claim(a, gs), &old, cw - (1ull << 20), __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (qht_value(static_cast<uint32_t>(old), static_cast<uint32_t>(old >> 32)) != cw) return false;  // lost the race
    const uint32_t eps = static_cast<uint32_t>(cw >> 40);
    const uint32_t k = (static_cast<uint32_t>(cw >> 20) & 0xFFFFFu) - 1u;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(help_params_rsrc(a), static_cast<int>(64u * gs) + 16 * (lane & 3),
                                                          0, 16 /* sc1 */);
    if (__ballot(lane < 4 && v.x != eps) != 0) return false;  // the owner has moved on: nobody waits for this tile
    const uint64_t p = rl64(v, 0);
    task.sid = static_cast<uint32_t>(__builtin_amdgcn_readlane(v.w, 0)) | kHelpBit;
    task.off0 = static_cast<int64_t>(p & 15u);
    task.abase = reinterpret_cast<const uint8_t*>(p - static_cast<uint64_t>(task.off0));
    task.n = static_cast<int64_t>(rl64(v, 1));
    task.s = static_cast<int64_t>(rl64(v, 2));  // tile 0
    const int64_t T = static_cast<int64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(v.w, 2)));
    task.ct = task.s + static_cast<int64_t>(k) * T;
    const int64_t rhi = static_cast<int64_t>(rl64(v, 3));
    task.aux = task.ct + T - 1 < rhi ? task.ct + T - 1 : rhi;  // the tile's end
    task.cb = gs;
    task.cnt = k;
    task.cap = 0;
    task.epoch = eps;
    return true;
}

// Blocking resolution of ticket t (its ring entry, polled): 1 resolved, 2 tombstone (take
// another ticket), 3 a help task in st (the ticket is still held), 0 every stream is done, or
// the wave gave up (error word) -- it exits.
//   Polling backoff: in the tail ~1,000 waves poll their entry and the done counter; once 8 polls
//   in a row saw no stream finish they sleep s_sleep 32 (1.339-1.344 vs 1.363 ms on config 2,
//   profiles/r03/buz/kbench_poll_*.log) and read the done counter every 4th poll.
//   Help: a waiting wave looks for a tile to help with every kHelpEvery polls (help_find).
constexpr uint32_t kPollAfter = 8, kDoneEvery = 4, kHelpEvery = 2;
__device__ int presolve(const BatchArgs& a, int lane, uint32_t t, PStream& st, uint32_t wg_waves, uint32_t me,
                        bool can_help) {
    const uint32_t n = a.nstreams;
    const uint32_t spin_cap = ld_agent(a.queue + kQCfg), steal_spins = ld_agent(a.queue + kQCfg + 1);
    uint32_t idle = 0;            // polls since a stream last finished
    uint32_t seen = ~0u;          // lane 0: streams done at the last poll
    for (uint32_t spin = 0;; spin++) {
        const u32x4 v = pentry_load(a, lane, t);
        if (pentry_ok(v, lane, t)) {
            if (static_cast<uint32_t>(__builtin_amdgcn_readlane(v.w, 0)) == kTombstone) return 2;
            pentry_decode(st, v);
            return 1;
        }
        uint32_t stop = 0;
        if (lane == 0 && spin % kDoneEvery == 0) {
            // Progress = streams finishing.  Not the {head, tail} word: every ticket take and
            // yield is an atomic on it, and waiting waves polling it slowed those by ~7%.
            const uint32_t done = ld_agent(a.queue + kQDone);
            idle = done == seen ? idle + 1 : 0;
            seen = done;
            if (done >= n) {
                stop = 1;
            } else if (idle + 1u >= spin_cap) {  // this poll included: a cap of 1 gives up at once (test knob)
                add_agent(a.queue + kQErr, 1u);
                // post-mortem (tools/batch_probe.py): the ticket this wave gave up on, in the spare
                // words of its help slot's claim line
                if (a.help && me < a.help_waves) help_claim(a, me)[1] = 0x100000000ull | t;
                stop = 1;
            }
        }
        if (bcast(stop)) return 0;
        if (steal_spins && spin % steal_spins == steal_spins - 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA is in flight here either
            try_steal(a, lane, wg_waves);
            continue;  // poll the entry again at once
        }
        if (can_help && spin % kHelpEvery == kHelpEvery - 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (help_find(a, lane, me, spin / kHelpEvery, st)) return 3;
        }
        // back off while nothing finishes: ~1,000 waiting waves polling two words every 0.5 us
        // load the L2 channel of the done counter in the batch's tail
        if (bcast(idle) >= kPollAfter)
            __builtin_amdgcn_s_sleep(32);
        else
            __builtin_amdgcn_s_sleep(16);
    }
}

// Write entry e (tag e + 1): the stream's state, or a tombstone.
__device__ __forceinline__ void pwrite(const BatchArgs& a, int lane, uint32_t e, const PStream& st, bool tomb) {
    const uint32_t tag = e + 1u;
    const uint64_t p = reinterpret_cast<uint64_t>(st.abase) + static_cast<uint64_t>(st.off0);
    const __amdgpu_buffer_rsrc_t r = pring_rsrc(a);
    const int base = static_cast<int>((e & a.ring_mask) * kPEntryStride);
#if KCDC_DEBUG_CHECKS  // entry writes (kQStat+33), and a slot written twice under one tag (code 9)
    if (lane == 0) {
        add_agent(a.queue + kQStat + 33, 1u);
        const u32x4 old = __builtin_amdgcn_raw_buffer_load_b128(r, base, 0, 16);
        const uint32_t ht_tail = ld_agent(a.queue + kQHT + 1);
        if ((old.x == tag || e >= ht_tail) && atomicAdd(a.queue + kQErr, 1u) == 0) {
            a.queue[kQStat + 16] = old.x == tag ? 9u : 10u;
            a.queue[kQStat + 17] = st.sid;
            a.queue[kQStat + 18] = e;
            a.queue[kQStat + 19] = ht_tail;
        }
    }
#endif
    if (lane == 0) {
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, st.cnt, tomb ? kTombstone : st.sid), r, base + 0, 0,
                                               16 /* sc1 */);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, static_cast<uint64_t>(st.s), 0), r, base + 16, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, static_cast<uint64_t>(st.ct), 0), r, base + 32, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, p, 0), r, base + 48, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, static_cast<uint64_t>(st.n), 0), r, base + 64, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, st.cb, 0), r, base + 80, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(pgranule(tag, st.cap, 0), r, base + 96, 0, 16);
    }
}

// Mid-tile fetch of ring entry e by LDS-DMA (sc1) into the wave's warm slot, which is idle
// between the tile's warm-up and its last step; read back after the last step's explicit
// vmcnt wait.  A compiler-visible load instead would be in flight when the step's
// (inline-asm, invisible) LDS-DMAs issue, and the waitcnt pass would then put a vmcnt
// wait into the hash loop that also drains those DMAs.
__device__ __forceinline__ void pentry_dma(const BatchArgs& a, int lane, uint32_t e, uint32_t m0) {
    u32x4 d;
    const uint64_t base = reinterpret_cast<uint64_t>(a.ring);
    d.x = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
    d.y = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32) & 0xFFFFu);
    d.z = __builtin_amdgcn_readfirstlane((a.ring_mask + 1u) * kPEntryStride);
    d.w = 0x00020000u;
    const int32_t off = static_cast<int32_t>((e & a.ring_mask) * kPEntryStride) + 16 * (lane & 7);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen sc1 lds"
                 :: "s"(m0), "v"(off), "s"(d) : "memory");
}

// Region bounds (coordinates) of the stream's current chunk; a help task's is its tile
// [ct, region end].
__device__ __forceinline__ void pregion(const BatchArgs& a, const PStream& st, int64_t& lo, int64_t& hi) {
    if (st.sid & kHelpBit) {
        lo = st.ct;
        hi = st.aux;
        return;
    }
    const int64_t mn = static_cast<int64_t>(a.min_size), mx = static_cast<int64_t>(a.max_size);
    lo = st.s + mn - 1 + st.off0;
    hi = (st.s + mx - 1 < st.n - 1 ? st.s + mx - 1 : st.n - 1) + st.off0;
}

__device__ __forceinline__ void ptile_issue(const PStream& st, int64_t hi, uint32_t wl, uint32_t sl, int lane,
                                            int64_t lane_cap) {
    const TileGeom g = tile_geom(st.ct, hi, st.abase, st.off0, st.off0 + st.n, lane_cap);
    dma_piece(g.ld, g.ld.tb, wl, st.ct, g.L, -1, lane);
    dma_step128(g.ld, g.ld.tb, sl, st.ct, g.L, 0, lane);
}

// Visit quantum from the number of streams queued behind the taken ticket: none waiting ->
// run to completion; otherwise 768 KiB (short tail quanta measured no gain, and helpers now
// split the tail's regions).
__device__ __forceinline__ int64_t pipe_quantum(int64_t backlog, int64_t q = kPipeYield) { return backlog <= 0 ? kNoYield : q; }
// The buzhash kernel's quantum in tiles, at least 512 KiB: the K tiles of a whole region
// (region_bytes = max - min) in equal visits of at most 8 tiles, so no region ends in a short
// visit that pays a hand-off for a few tiles.  512K and 1M (K = 6, 12) keep round 4's 6 tiles =
// 768 KiB; 2M and larger averages (K = 24, 48, ..) get 8 x 128 KiB = 1 MiB; 128K and 256K get
// 512 KiB.  Round 4 chose 6 tiles against the constant 768 KiB in one process
// (profiles/r04/third/ab_quantum_tiles_*.log): 128K 3.415 vs 3.639 ms, 256K 2.697 vs 2.843, 4M
// 1.296 vs 1.309 (512 KiB at 4M: 1.334 vs 1.286 ms); all bit-exact.  Round 7, 8 tiles against 6
// (profiles/r07/handoff/): config 2 -1.1..-2.3 %, where region_ct0's line start makes a region
// without a candidate 16 whole tiles (two visits instead of 6 + 6 + 4); 2M within the noise; 1M
// (8 + 4) +5.5 %, hence the equal visits.
__device__ __forceinline__ int64_t pipe_quantum_tiles(int64_t backlog, uint32_t lane_cap, uint64_t region_bytes) {
    constexpr uint32_t kMostTiles = 8;
    const uint32_t T = static_cast<uint32_t>(kWave) * lane_cap;
    const uint32_t K = static_cast<uint32_t>((region_bytes + T - 1) / T);
    const uint32_t visits = (K + kMostTiles - 1) / kMostTiles;
    const int64_t kTiles = visits ? (K + visits - 1) / visits : kMostTiles;
    const int64_t kMax = kTiles * kWave * 2048;  // (lanes above 2 KiB: as with 2 KiB lanes)
    const int64_t q = kTiles * kWave * static_cast<int64_t>(lane_cap);
    return pipe_quantum(backlog, q < (512 << 10) ? (512 << 10) : q > kMax ? kMax : q);
}

}  // namespace dev
}  // namespace kcdc
