// Splitter kernels, part 6 of 9: split_batch_pipe_kernel, the batch hot path (buzhash).
// Persistent waves, one stream per wave at a time through the ticketed ring queue; a stream is
// walked in TILES of 64 lanes x L bytes of its test region [s+min-1, s+max-1], lane l hashing
// segment l after warming up on the 64 bytes before it.  Bytes arrive by LDS-DMA in 128-byte
// steps; per byte one v_perm (table address), one ds_read of the 64x replicated table (lane l
// hits bank l%32), a T-ring register for the leaving byte, v_alignbit and v_bitop3, and a
// running v_min3 candidate test in the rotated frame.  A step whose min passes is re-run
// exactly; the earliest lane's candidate is the cut.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_hash.h"
#include "kcdc_split_feed.h"
#include "kcdc_split_queue.h"
#include "kcdc_split_visit.h"

namespace kcdc {
namespace dev {

template <bool TOP>
__global__ __launch_bounds__(kDmaWaves * kWave, kDmaWaves / 4) void split_batch_pipe_kernel(BatchArgs a) {
    __shared__ BuzShared smtab;
    __shared__ DmaSlots smslots;
    __shared__ WarmSlots smwarm;
    fill_buz_table(smtab, a.buz, a.buz_rot);
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t me = blockIdx.x * kDmaWaves + wave;  // this wave's help slot
    BuzRing hash;
    hash.tab = reinterpret_cast<const char*>(smtab.tab);
    hash.lane4 = static_cast<uint32_t>(lane) * 4u;
    hash.mask = a.mask;
    hash.h = 0;
    uint8_t* sl = smslots.b[wave][0];
    uint8_t* wl = smwarm.b[wave];
    const uint32_t sl32 = lds_addr(sl), wl32 = lds_addr(wl);
#if KCDC_TRACE  // per wave at trace[8 * global wave]: start, end, ticks in blocking takes, the last take's
                // start, help tiles, their ticks, the end of the wave's last own tile, own tiles; and the
                // hand-off sums at trace[8 * waves + 5 * global wave], each {count << 32 | ticks}: tile
                // start to the end of the tile-top wait in switching own tiles (it covers the ticket add)
                // and in the other own tiles (prefetched tiles that publish nothing only; a wait timed
                // by itself misses the add, whose result the compiler waits for a few instructions
                // earlier), adopt prefetch to the end of the adopted tile's top wait, one-step own tiles (whole tile), blocking takes of a
                // fresh ticket after the wave's first stream that returned work (those after a cut)
    const uint32_t gw = blockIdx.x * kDmaWaves + wave;
    uint64_t tr_block = 0, tr_last = 0, tr_help = 0, tr_help_t = 0, tr_own_end = 0, tr_own = 0;
    uint64_t tr_wsw = 0, tr_wns = 0, tr_adopt = 0, tr_one = 0, tr_cut = 0, tr_pf = 0;
    if (lane == 0) a.trace[8 * gw] = __builtin_amdgcn_s_memrealtime();
#define KCDC_PRET                                                                 \
    do {                                                                          \
        if (lane == 0) {                                                          \
            a.trace[8 * gw + 1] = __builtin_amdgcn_s_memrealtime();                \
            a.trace[8 * gw + 2] = tr_block;                                       \
            a.trace[8 * gw + 3] = tr_last;                                        \
            a.trace[8 * gw + 4] = tr_help;                                        \
            a.trace[8 * gw + 5] = tr_help_t;                                      \
            a.trace[8 * gw + 6] = tr_own_end;                                     \
            a.trace[8 * gw + 7] = tr_own;                                         \
            uint64_t* const tr_x = a.trace + 8ull * gridDim.x * kDmaWaves + 5ull * gw;  \
            tr_x[0] = tr_wsw;                                                     \
            tr_x[1] = tr_wns;                                                     \
            tr_x[2] = tr_adopt;                                                   \
            tr_x[3] = tr_one;                                                     \
            tr_x[4] = tr_cut;                                                     \
        }                                                                         \
        return;                                                                   \
    } while (0)
#else
#define KCDC_PRET return
#endif
    const uint32_t lim = TOP ? a.buz_lim : 0u;
    // help sub-tiles halve the lane segments (>= 256 B): shift = sid's help bit & this (integer
    // arithmetic: a select on a bool here became a VALU-materialised shift next to the DMAs)
    const uint32_t help_shift = __builtin_amdgcn_readfirstlane(a.lane_cap >= 512u ? 1u : 0u);
    static_assert(kHelpSplit == 2, "help sub-tiles: one halving");

    Visit v;
    PStream& cur = v.cur;
    // The buzhash visit quantum (pipe_quantum_tiles) for visit_take and visit_adopt.
    const auto quantum = [&](int64_t backlog) { return pipe_quantum_tiles(backlog, a.lane_cap, a.max_size - a.min_size); };
    visit_first_ticket<kDmaWaves>(a, lane, wave, v);
    for (;;) {
        visit_diag_take(a, lane, v);
        // The one blocking take site (inlined once: presolve and try_steal are large).
        if (v.need_take) {
#if KCDC_TRACE
            const uint64_t tb0 = __builtin_amdgcn_s_memrealtime();
            tr_last = tb0;
            const bool tr_fresh = v.take_t == 0xFFFFFFFFu && tr_own != 0;
#endif
            const bool taken = visit_take<kDmaWaves>(a, lane, me, v, quantum);
#if KCDC_TRACE
            const uint64_t tr_dt = __builtin_amdgcn_s_memrealtime() - tb0;
            tr_block += tr_dt;
            if (taken && tr_fresh) tr_cut += (1ull << 32) + tr_dt;
#endif
            if (!taken) KCDC_PRET;
        }
        visit_diag_tile(a, lane, v);
        uniformize(cur);
        if (!pcheck(a, lane, cur, 0xFFFFFFFFu, 5)) KCDC_PRET;
        const bool is_help = (cur.sid & kHelpBit) != 0;
#if KCDC_TRACE
        const uint64_t tr_t0 = __builtin_amdgcn_s_memrealtime();
        if (is_help) tr_help++;
        else tr_own++;
        const bool tr_pre = v.issued && !(v.hs & kHsNeedPub);  // prefetched, and publishes nothing
#endif
        int64_t lo, hi;
        pregion(a, cur, lo, hi);
        // A help task's tile (one owner tile, up to hi) goes in kHelpSplit sub-tiles: it stops at
        // the first one with a candidate, or when its owner has closed the region meanwhile.
        const int64_t lcap = static_cast<int64_t>(a.lane_cap >> ((cur.sid >> 31) & help_shift));
        const TileGeom g = tile_geom(cur.ct, hi, cur.abase, cur.off0, cur.off0 + cur.n, lcap);
        if (!v.issued) ptile_issue(cur, hi, wl32, sl32, lane, lcap);
        // The owner's claim on its next tile (atomic add on its slot's bottom) is issued in step 0
        // behind the refill DMA and read in step 2 (or at the tile end for one- and two-step tiles).
        Tile tile = visit_tile(a, lane, me, v, is_help, hi, kWave * g.L, kWave * static_cast<int64_t>(a.lane_cap));
        const int64_t ct = tile.ct, ct_next = tile.ct_next;
        const bool last_of_region = tile.last_of_region, switching = tile.switching, claim_next = tile.claim_next;
        // Lane positions as 32-bit offsets from the tile start (a tile < 2^31 bytes): 64-bit
        // per-lane values live across the hash loop cost VGPRs this kernel does not have.
        const int32_t cl0 = lane * static_cast<int32_t>(g.L);
        const int32_t hi_rel = static_cast<int32_t>(hi - ct < 0x7FFFFFFF ? hi - ct : 0x7FFFFFFF);
        uint32_t ht_lo = static_cast<uint32_t>(tile.ht_raw), ht_hi = static_cast<uint32_t>(tile.ht_raw >> 32);
        {
            uint32_t w16[16];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(ht_lo), "+v"(ht_hi)::"memory");
#if KCDC_TRACE
            const uint64_t tr_w1 = __builtin_amdgcn_s_memrealtime();
            if (!is_help) {
                if (tr_pre && switching) tr_wsw += (1ull << 32) + (tr_w1 - tr_t0);
                else if (tr_pre) tr_wns += (1ull << 32) + (tr_w1 - tr_t0);
                if (tr_pf) tr_adopt += (1ull << 32) + (tr_w1 - tr_pf);
            }
            tr_pf = 0;
#endif
            read_piece(wl, lane, 1, cur.off0, w16);  // (the piece before coordinate 0 reads as zeros)
            hash.clear();
            hash.template block<kWarm>(w16);
        }
        tile.set_ticket(ht_lo, ht_hi);
        // Offset from ct of this lane's first candidate.  A region's tile 0 that starts at lo + 1
        // (region_ct0) tests lo here: lane 0's state after the warm-up is the hash at ct - 1, and
        // lo precedes every position of the tile.  (A help task's lo is its ct.)
        constexpr int32_t kNoCand = INT32_MIN;
        int32_t found = kNoCand;
        if (ct == lo + 1 && lane == 0 && (hash.h & hash.mask) == 0) found = -1;
        const int poll_step = g.nb > 1 ? g.nb / 2 : 0;
        // The owner's claim on tile htile + 1: an atomic add on its slot's bottom in step 0 (no
        // return value: nothing stays live across the hashing), the word read back by an sc1
        // LDS-DMA into the idle warm slot in step 1 (behind step 1's wait, which the add has
        // passed) and looked at in the last step, before the next tile's prefetch.  One- and
        // two-step tiles read it at the tile end (and prefetch nothing).
        for (int n = 0; n < g.nb; n++) {
            const int32_t cl = cl0 + 128 * n;
            const uint32_t st0 = hash.save();
            uint32_t dw[32];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            read_step128h(sl, lane, ct == 0 && cl == 0, cur.off0, dw);
            if (claim_next && n >= 2 && n == g.nb - 1) tile.claim_decode(v, *reinterpret_cast<const uint64_t*>(wl));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot free: refill it
            __builtin_amdgcn_sched_barrier(0);

            if (tile.reserve && n == g.nb - 1) tile.reserve_entry(a, lane);  // this stream's entry, reserved late
            if (switching && n == poll_step) {
                pentry_dma(a, lane, tile.tk, wl32);
                if (n == g.nb - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing to hide it under
            }
            if (claim_next && n == 1) help_claim_dma(a, lane, me, wl32);
            if (n + 1 < g.nb) {
                dma_step128(g.ld, g.ld.tb, sl32, ct, g.L, n + 1, lane);
            } else if (!switching && !last_of_region && tile.claim_known && (!claim_next || tile.claim_ok) &&
                       __ballot(found != kNoCand) == 0) {
                // (a candidate in an earlier step means the region's cut is in this tile: the
                // next tile would be a stale prefetch, 12 KiB of HBM traffic per chunk wasted --
                // 9 % of R at 128K, where chunks span ~4 tiles)
                PStream t2 = cur;  // next tile of this region (ours)
                t2.ct = ct_next;
                ptile_issue(t2, hi, wl32, sl32, lane, lcap);
                tile.next_issued = true;
            }
            if (claim_next && n == 0 && lane == 0)
                __hip_atomic_fetch_add((gu64*)help_claim(a, me), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t m = hash.template step128<TOP>(dw, 0u);
            __builtin_amdgcn_sched_barrier(0);
            if (m <= lim && found == kNoCand && cl <= hi_rel) {  // rare: exact re-run from global memory
                const int64_t c = ct + cl;
                uint32_t prv[16], cur32[32];
                g.ld.load(c - 64, prv);
                g.ld.load(c, cur32);
                const int64_t blo = lo - c, bhi = hi - c;
                const uint32_t idx = hash.exact(st0, prv, cur32, blo < 0 ? 0 : static_cast<int>(blo),
                                                bhi > 127 ? 127 : static_cast<int>(bhi));
                if (idx < 128u) found = cl + static_cast<int32_t>(idx);
                // a wait the waitcnt pass sees: its scoreboard otherwise keeps these loads
                // pending around the loop and waits for them in the hash loop (draining DMAs)
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            }
        }
        // ---- end of tile
        if (!tile.claim_known) {  // a one- or two-step tile: its claim is read here
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (g.nb == 2) {
                tile.claim_decode(v, *reinterpret_cast<const uint64_t*>(wl));
            } else {
                const uint64_t raw = ld_agent64(help_claim(a, me));
                tile.claim_decode(v, qht_value(static_cast<uint32_t>(raw), static_cast<uint32_t>(raw >> 32)));
            }
        }
        const uint64_t hit = __ballot(found != kNoCand);
#if KCDC_TRACE
        if (is_help) tr_help_t += __builtin_amdgcn_s_memrealtime() - tr_t0;
        else {
            tr_own_end = __builtin_amdgcn_s_memrealtime();
            if (g.nb == 1) tr_one += (1ull << 32) + (tr_own_end - tr_t0);
        }
#endif
        // the tile's first candidate (coordinate), or -1
        const int64_t f = hit ? ct + __builtin_amdgcn_readfirstlane(__shfl(found, __builtin_ctzll(hit))) : -1;
        if (visit_resolve(a, lane, me, v, tile, f, kWave * static_cast<int64_t>(a.lane_cap))) continue;
        // ---- switch streams: the next one's entry landed in the warm slot (the last step's wait
        // drained it); prefetch its first tile now, under this tile's bookkeeping
        const auto prefetch = [&](PStream& nx) {
            if (nx.ct < 0 && nx.s < nx.n && nx.s + static_cast<int64_t>(a.min_size) - 1 < nx.n)
                nx.ct = region_ct0(a, nx.s, nx.n, nx.off0, /*line_start=*/true);
            if (nx.ct < 0) return false;
            int64_t nlo, nhi;
            pregion(a, nx, nlo, nhi);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // entry read before the slot refill
            ptile_issue(nx, nhi, wl32, sl32, lane, a.lane_cap);
#if KCDC_TRACE
            tr_pf = __builtin_amdgcn_s_memrealtime();
#endif
            return true;
        };
        if (!visit_adopt(a, lane, v, wl, switching, switching ? tile.tk : 0xFFFFFFFFu, tile.nbacklog, quantum, prefetch)) KCDC_PRET;
    }
}
#undef KCDC_PRET

}  // namespace dev
}  // namespace kcdc
