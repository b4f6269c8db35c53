// Splitter kernels, part 5 of 9: the visit protocol (Visit, Tile, visit_*).
// What a wave does between two tile scans, as split_batch_pipe_kernel (kcdc_split_buz.h) uses it;
// split_batch_rk_kernel spells the same statements out itself (kcdc_split_rk.h says why) and takes
// only the kHs* flags from here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_feed.h"
#include "kcdc_split_queue.h"

namespace kcdc {
namespace dev {

// ------------------------------------------------------------ the visit protocol
// What split_batch_pipe_kernel and split_batch_rk_kernel share: taking streams from the ticketed
// ring, publishing regions to helpers, the plan of a tile (claim, yield, next ticket), and what
// follows a tile's scan (help post, cut, requeue, the next stream).  The kernels keep the feed,
// the hash, the candidate checks and the steps at which the atomics and DMAs are issued.  All of
// it is wave-uniform and inlined at one site per kernel (presolve and try_steal are large).
// Regions are set up by region_ct0's line-start rule: the one user of these functions, the buzhash
// kernel, tests lo on the warm state of a tile that starts at lo + 1.
constexpr uint32_t kHsPub = 1u << 16;     // the current region is published (claims are on)
constexpr uint32_t kHsNeedPub = 1u << 17; // the region at cur.ct is new to this wave
constexpr uint32_t kHsHelped = 1u << 18;  // the last claim saw helpers on the region: no yield
struct Visit {
    PStream cur;
    int64_t budget = kNoYield;
    // Help state of this wave's own slot (wave-uniform, packed: SGPRs are what these kernels run
    // short of): hep = the epoch of the last publish; hs = the published region's tile count
    // (bits 0-7), the index of the tile being scanned (8-15) and the kHs* flags.
    uint32_t hep = 0, hs = kHsNeedPub;
    // Pending blocking take (set right before jumping to the loop top, so none of it is live
    // across the hash loop).
    bool need_take = true;
    uint32_t take_t = 0xFFFFFFFFu, take_claim = 0xFFFFFFFFu;
    int64_t take_backlog = 0;
    bool issued = false;  // this tile's first fill (buzhash: warm piece + step 0) is in flight
    __device__ __forceinline__ uint32_t hK() const { return hs & 0xFFu; }
    __device__ __forceinline__ uint32_t htile() const { return (hs >> 8) & 0xFFu; }
    // Take at the loop top: ticket t (held), or ~0u for a fresh one.
    __device__ __forceinline__ void take(uint32_t t, int64_t backlog) {
        need_take = true;
        take_t = t;
        take_backlog = backlog;
        take_claim = 0xFFFFFFFFu;
    }
};
// The wave-uniform facts of the tile being scanned: visit_tile's plan, the kernel's claim and
// prefetch results, and the atomics' raw values.
struct Tile {
    bool is_help, last_of_region;
    int64_t ct, ct_next, hi;  // the tile [ct, ct_next) of the region ending at hi
    bool switching, reserve, claim_next;
    uint64_t ht_raw = 0;      // the next stream's ticket add, as returned to lane 0
    uint32_t tk = 0;          // that ticket (set_ticket)
    int64_t nbacklog = 0;
    uint64_t pe_raw = 0;      // this stream's reserved entry, as returned to lane 0
    bool res_issued = false;
    bool claim_ok = false, claim_known;
    bool next_issued = false;  // the region's next tile is prefetched
    __device__ __forceinline__ void set_ticket(uint32_t ht_lo, uint32_t ht_hi) {
        if (!switching) return;
        const uint64_t ht = qht_value(ht_lo, ht_hi);
        tk = static_cast<uint32_t>(ht);
        nbacklog = static_cast<int64_t>(ht >> 32) + (reserve ? 1 : 0) - static_cast<int64_t>(tk) - 1;
    }
    // cw: the owner's claim word after this tile's add
    __device__ __forceinline__ void claim_decode(Visit& v, uint64_t cw) {
        const uint32_t top = static_cast<uint32_t>(cw >> 20) & 0xFFFFFu, bot = static_cast<uint32_t>(cw) & 0xFFFFFu;
        claim_ok = static_cast<uint32_t>(cw >> 40) == v.hep && bot <= top;
        if (top < v.hK()) v.hs |= kHsHelped;
        claim_known = true;
    }
    // This stream's ring entry, reserved late (in the tile's last step or fill, else at its end).
    __device__ __forceinline__ void reserve_entry(const BatchArgs& a, int lane) {
        pe_raw = qht_add(a, lane, 1ull << 32);
        res_issued = true;
    }
};

// First ticket: preassigned (see init_ring_kernel), unless a waiting wave has requeued
// this workgroup's streams before it started (try_steal): then take one from the counter.
template <uint32_t WG_WAVES>
__device__ __forceinline__ void visit_first_ticket(const BatchArgs& a, int lane, uint32_t wave, Visit& v) {
    uint32_t claim = 1u;
    if (lane == 0) {
        claim = 0u;
        __hip_atomic_compare_exchange_strong((gu32*)(a.queue + kQFlags + blockIdx.x), &claim, 1u,
                                             __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t t0 = first_ticket(blockIdx.x, wave);
    const int64_t nw = static_cast<int64_t>(gridDim.x) * WG_WAVES;
    v.take_t = t0 < a.nstreams ? t0 : 0xFFFFFFFFu;
    v.take_backlog = static_cast<int64_t>(a.nstreams) - nw;
    v.take_claim = t0 < a.nstreams ? (claim & 3u) : 0xFFFFFFFFu;
}

// The pending blocking take (v.take_t: a ticket already held, or ~0u to take one): the next
// stream with a region to scan, or a help task; false when every stream is done.  No LDS-DMA
// may be in flight.
// v.take_claim: the first take's claim of this workgroup's preassigned tickets (lane 0's CAS
// result: 0 or 1 ours, 2 the streams were requeued by try_steal), issued before the first
// resolve and checked after it so its round trip overlaps the entry load; ~0u elsewhere
// (a constant at those sites: no claim state stays live across the main loop).
// quantum(backlog): the visit's byte budget.
template <uint32_t WG_WAVES, class Quantum>
__device__ __forceinline__ bool visit_take(const BatchArgs& a, int lane, uint32_t me, Visit& v, Quantum quantum) {
    PStream& cur = v.cur;
    uint32_t t = v.take_t, claim = v.take_claim;
    v.need_take = false;
    v.issued = false;
    v.hs |= kHsNeedPub;
    for (;;) {
        int64_t backlog = v.take_backlog;  // queue depth behind a ticket already held (caller's estimate)
        if (t == 0xFFFFFFFFu) {
            const uint64_t ht = qht_take(a, lane, 1);
            t = static_cast<uint32_t>(ht);
            backlog = static_cast<int64_t>(ht >> 32) - static_cast<int64_t>(t) - 1;
        }
        const uint32_t held = t;
        const int r = presolve(a, lane, held, cur, WG_WAVES, me, a.help != nullptr && claim == 0xFFFFFFFFu);
        if (r == 0) return false;
        if (r == 3) {  // a help task; the ticket stays held (in cap, unused by help tasks, and in memory)
            held_put(a, lane, me, held);
            cur.cap = held;
            uniformize(cur);
            return true;
        }
        t = 0xFFFFFFFFu;
        if (claim != 0xFFFFFFFFu) {
            const bool requeued = bcast(claim) == 2u;
            claim = 0xFFFFFFFFu;
            if (requeued) continue;  // requeued by another wave: take a fresh ticket
        }
        if (r == 2) continue;  // tombstone
        uniformize(cur);
        if (!pcheck(a, lane, cur, held, 1)) return false;
        v.budget = quantum(backlog);
        if (pstream_region(a, cur, lane, /*line_start=*/true)) return true;
        if (lane == 0) {  // nothing left to scan
            a.counts[cur.sid] = cur.cnt;
            add_agent(a.queue + kQDone, 1u);
        }
    }
}

// Loop top, diagnostic builds: wave-uniform control values held lane-divergent, before the
// blocking take and before the tile.
__device__ __forceinline__ void visit_diag_take(const BatchArgs& a, int lane, const Visit& v) {
#if KCDC_HELP_DIAG
    diag_record(a, lane, divergent_bit(v.need_take, 0) | divergent_bit(v.take_t, 1) | divergent_bit(v.issued, 2));
#endif
}
__device__ __forceinline__ void visit_diag_tile(const BatchArgs& a, int lane, const Visit& v) {
#if KCDC_HELP_DIAG
    diag_record(a, lane, divergent_bit(v.hs, 3) | divergent_bit(v.hep, 4) | divergent_bit(v.cur.sid, 5) |
                             divergent_bit(static_cast<uint32_t>(v.cur.cap), 6) |
                             divergent_bit(static_cast<uint32_t>(v.cur.ct), 7) |
                             divergent_bit(static_cast<uint32_t>(v.budget), 8));
#endif
}

// The plan of the tile [v.cur.ct, + tile_bytes) of the region ending at hi (T: bytes per full
// own tile): publishes a region new to this wave, and issues the next stream's ticket add when
// this is the visit's last tile.
__device__ __forceinline__ Tile visit_tile(const BatchArgs& a, int lane, uint32_t me, Visit& v, bool is_help, int64_t hi,
                                           int64_t tile_bytes, int64_t T) {
    const PStream& cur = v.cur;
    Tile t;
    t.is_help = is_help;
    t.ct = cur.ct;
    t.ct_next = t.ct + tile_bytes;
    t.hi = hi;
    t.last_of_region = t.ct_next > hi;
    // A region new to this wave: publish it when it is long enough to share.
    if ((v.hs & kHsNeedPub) && !is_help) {
        const uint32_t K = static_cast<uint32_t>((hi - t.ct + T) / T);
        v.hs = 0;
        if (a.help && K >= kHelpMinTiles && K <= static_cast<uint32_t>(kHelpTiles)) {
            // a window of the region (help_window tiles from here), re-published as the owner
            // passes its end
            const uint32_t Kw = a.help_window && K > a.help_window ? a.help_window : K;
            v.hep++;
            v.hs = kHsPub | Kw;
            help_publish(a, lane, me, v.hep, cur, t.ct, Kw < K ? t.ct + static_cast<int64_t>(Kw) * T - 1 : hi, Kw, T);
        }
    }
    // The owner's claim on its next tile: an atomic add on its slot's bottom, issued and read
    // back by the kernel inside the tile.
    const bool claim_next_r = (v.hs & kHsPub) && !is_help && !t.last_of_region && v.htile() + 1u < v.hK();
    // (a help task never yields: its wave's budget is the last own visit's leftover, and a
    // reservation made here would never be written -- its ticket's taker would wait to the end)
    const bool budget_out = !is_help && !(v.hs & kHsHelped) && v.budget - tile_bytes <= 0;  // (with helpers: no yield)
    bool ends_nocand = false;  // no candidate in this tile => the stream is finished
    if (!is_help && t.last_of_region) {
        const int64_t mx = static_cast<int64_t>(a.max_size);
        const int64_t s2 = cur.s + mx - 1 <= cur.n - 1 ? cur.s + mx : cur.n;
        ends_nocand = s2 >= cur.n || s2 + static_cast<int64_t>(a.min_size) - 1 >= cur.n;
    }
    // The visit's last tile (absent a candidate): take the next ticket now, and reserve
    // this stream's entry too when it will be yielded -- one atomic, hidden by the DMAs.
    t.switching = !is_help && (budget_out || ends_nocand);
    t.reserve = budget_out && !ends_nocand;
    t.claim_next = claim_next_r && !t.switching;  // a yielding owner claims nothing more
    t.claim_known = !t.claim_next;
    if (t.switching) t.ht_raw = qht_add(a, lane, 1);  // the next stream's ticket
    return t;
}

// After a tile's scan (f: the coordinate of its first candidate, or -1): a help task posts and
// goes on or ends; an owner resolves the region's cut (a hit, the forced cut, the helpers'
// posts, or the next tile), then goes on with its stream or requeues it.  T: bytes per full own
// tile (a parameter again: kept in the Tile it would live across the hash loop).  True: back to
// the loop top (same stream, or v.need_take); false: the wave switches streams (visit_adopt follows).
__device__ __forceinline__ bool visit_resolve(const BatchArgs& a, int lane, uint32_t me, Visit& v, Tile& t, int64_t f,
                                              int64_t T) {
    PStream& cur = v.cur;
    if (t.reserve && !t.res_issued) t.reserve_entry(a, lane);
    if (t.is_help) {
        bool done = true;
        if (f >= 0 || t.last_of_region) {  // post the tile's first candidate to its owner's row
            help_post(a, lane, static_cast<uint32_t>(cur.cb), cur.epoch, static_cast<uint32_t>(cur.cnt), cur.s, f);
        } else {  // the next sub-tile (prefetched), unless the owner has closed the region
            const uint64_t w = ld_agent64(help_claim(a, static_cast<uint32_t>(cur.cb)));
            done = static_cast<uint32_t>(qht_value(static_cast<uint32_t>(w), static_cast<uint32_t>(w >> 32)) >> 40) !=
                   cur.epoch;
        }
        if (!done) {
            cur.ct = t.ct_next;
            v.issued = t.next_issued;
            return true;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the post, or a dropped prefetch
        // (the held ticket is taken back from memory, here where both ending paths have joined:
        // DESIGN.md §2.1c)
        v.take(held_get(a, lane, me, static_cast<uint32_t>(cur.cap)), 0);
        return true;
    }
    bool region_changed = true;
    const int64_t mx = static_cast<int64_t>(a.max_size);
    const int64_t forced = cur.s + mx - 1 <= cur.n - 1 ? cur.s + mx : cur.n;  // max-size cut / the end
    int64_t cut = -1;  // this region's cut, once known
    if (f >= 0) {
        cut = f - cur.off0 + 1;
    } else if (t.last_of_region) {  // forced cut at max size (splitter_buzhash32.go:60-64,
        cut = forced;               // splitter_rabinkarp64.go:60-64) or the end
    } else if (t.claim_next && !t.claim_ok) {  // the helpers hold the rest of the region
        const int64_t ct0 = t.ct - static_cast<int64_t>(v.htile()) * T;  // the published tile 0
        const int64_t r = help_wait(a, lane, me, v.hep, v.htile() + 1u, v.hK(), ct0);
        const int64_t wend = ct0 + static_cast<int64_t>(v.hK()) * T;  // past the published window
        if (r >= 0) {
            cut = r - cur.off0 + 1;
        } else if (r == -1 && wend <= t.hi) {  // no candidate in the window: publish the next one
            cur.ct = wend;
            help_close(a, lane, me, v.hep);
            v.hs = kHsNeedPub;
            region_changed = false;
        } else if (r == -1) {
            cut = forced;
        } else {  // a tile still pending: scan on from it, unshared
            cur.ct = ct0 + (-2 - r) * T;
            help_close(a, lane, me, v.hep);
            v.hs = 0;
            region_changed = false;
        }
    } else {
        cur.ct = t.ct_next;
        v.hs += 1u << 8;  // htile++
        v.budget -= t.ct_next - t.ct;
        region_changed = false;
        if ((v.hs & kHsPub) && v.htile() >= v.hK()) {  // past its published window: the next one
            help_close(a, lane, me, v.hep);
            v.hs = kHsNeedPub;
        }
    }
    if (cut >= 0) {
        emit_cut(a, cur, lane, cut);
        cur.s = cut;
        cur.ct = -1;
    }
    if (region_changed) {
        if (v.hs & kHsPub) help_close(a, lane, me, v.hep);
        v.hs = kHsNeedPub;
    }
    const bool live = pstream_region(a, cur, lane, /*line_start=*/true);
    if (!live && lane == 0) {
        a.counts[cur.sid] = cur.cnt;
        add_agent(a.queue + kQDone, 1u);
    }
    if (!t.switching && live) {  // same stream, next tile
        v.issued = t.next_issued && !region_changed;
        if (t.next_issued && region_changed) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stale prefetch
        return true;
    }
    // ---- switch streams: requeue this one first (its reserve atomic was issued in the
    // last step, so no prefetch DMA is in flight behind it)
    if (v.hs & kHsPub) help_close(a, lane, me, v.hep);  // a yielded region is not ours to share any more
    v.hs = kHsNeedPub;
    if (t.reserve) {
        const uint32_t pe = static_cast<uint32_t>(
            qht_value(static_cast<uint32_t>(t.pe_raw), static_cast<uint32_t>(t.pe_raw >> 32)) >> 32);
        pwrite(a, lane, pe, cur, !live);
    } else if (live) {  // a candidate kept the stream alive past its predicted last tile
        const uint64_t ht = qht_take(a, lane, 1ull << 32);
        pwrite(a, lane, static_cast<uint32_t>(ht >> 32), cur, false);
    }
    return false;
}

// The wave switches streams (visit_resolve returned false): adopt the next stream from its ring
// entry, which the kernel's DMA of ticket tk has landed at `entry` (entry_landed; the DMA is
// drained), or leave the ticket to a blocking take at the loop top.  tk is ~0u when the tile took
// no ticket (the stream ended on a candidate: a fresh one is taken); nbacklog: the queue depth
// behind tk.  prefetch(nx): the kernel may issue the adopted
// stream's first tile and return true.  False when the wave must exit (a failed check).
template <class Quantum, class Prefetch>
__device__ __forceinline__ bool visit_adopt(const BatchArgs& a, int lane, Visit& v, const uint8_t* entry, bool entry_landed,
                                            uint32_t tk, int64_t nbacklog, Quantum quantum, Prefetch prefetch) {
    if (entry_landed) {
        const u32x4 ev = *reinterpret_cast<const u32x4*>(entry + 16 * (lane & 7));
        if (pentry_ok(ev, lane, tk) && static_cast<uint32_t>(__builtin_amdgcn_readlane(ev.w, 0)) != kTombstone) {
            PStream nx;
            pentry_decode(nx, ev);
            uniformize(nx);
            if (!pcheck(a, lane, nx, tk, 2)) return false;
            v.issued = prefetch(nx);
            v.cur = nx;
            v.budget = quantum(nbacklog);
            if (pstream_region(a, v.cur, lane, /*line_start=*/true)) return true;
            if (lane == 0) {  // nothing left to scan in it
                a.counts[v.cur.sid] = v.cur.cnt;
                add_agent(a.queue + kQDone, 1u);
            }
            v.take(0xFFFFFFFFu, 0);
            return true;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no prefetch may remain in flight
    v.take(tk, nbacklog);
    return true;
}

}  // namespace dev
}  // namespace kcdc
