"""GPU: where the buzhash batch kernel starts a region's tile grid, bit-exact against the C oracle.

A region [lo, hi] is scanned in tiles that start on 128-byte lines.  When lo is the last byte of
its line, split_batch_pipe_kernel starts tile 0 at lo + 1 and tests lo on lane 0's state after the
tile's warm-up (region_ct0, kopia_amd/csrc/kcdc_split_queue.h); everywhere else tile 0 is the line
holding lo, its head below lo clipped.  lo = s + min - 1 + off0 in coordinates (off0 = the stream
pointer's low four bits), and min is a multiple of 128, so a first region takes the new rule
exactly at 16-byte aligned pointers and a later region where the cut before it put it.

Planted natural candidates (tests/batch_model.py) at lo - 1 (must not cut), lo, lo + 1 and the
last byte of the first tile; pointers misaligned by 0, 1, 15 and 16 bytes; streams of min,
min + 1, min + 127, min + 128 and min + 129 bytes (no region, a one-byte region -- which keeps
the line rule --, regions that end in tile 0's first step) and long ones; second regions that
start on the last byte of a line (new rule, with a candidate planted on that very lo) and in the
middle of one (old rule).  Each layout runs with help off, help forced on and help in windows of
3 tiles, then with 2,304 aliased pointers for the launch's 2,048 waves, so that visits yield and
regions are first set up by the wave that adopts a stream from the ring.

The second half walks the stream hand-offs at the 8-tile visit quantum of the averages from 2M
up (DYNAMIC-2M-BUZHASH, more streams than waves): plants around the tile boundaries where a visit
yields and the next wave resumes, streams that end on a candidate in the first, second, a middle,
the second-to-last and the last step of a visit's first and last tile, region tails of one and
two steps in the switching position, and the 1-poll cap of tests/test_gpu_queue.py over streams
of which a third leave tombstones.  All of it is placed on the kernel's own grid (grid()).

Every launch is bounded by a small KCDC_TEST_SPIN_CAP: a protocol slip ends as an error within
seconds."""
from functools import lru_cache

import numpy as np
import pytest

import batch_model as bm
from kopia_amd import _lib
from oracle import coracle
from test_gpu_batch_edges import REGIMES, _compare, _knobs_of, _launch, knobs, plan

KIND = "buzhash"
# (name, average, lane cap): 32 KiB tiles at 128K; 16 KiB and 128 KiB tiles at 1M
GEOMS = {"128K-512": ("DYNAMIC-128K-BUZHASH", 128 << 10, 512),
         "1M-256": ("DYNAMIC-1M-BUZHASH", 1 << 20, 256),
         "1M-2048": ("DYNAMIC-1M-BUZHASH", 1 << 20, 2048)}
MISALIGN = (0, 1, 15, 16)


def tile0(avg, lane_cap, s, n, off0):
    """(ct, L) of tile 0 of the region of the chunk starting at s: region_ct0 and tile_geom."""
    lo, hi = bm.region(avg, s, n, off0)
    ct = lo + 1 if lo % 128 == 127 and lo < hi else lo & ~127
    return bm.tiles_between(KIND, lane_cap, ct, hi)[0]


def test_tile0_model():
    """The restated rule on the flagship shape: 4 MiB streams at DYNAMIC-4M, aligned pointers."""
    avg, n = 4 << 20, 4 << 20
    assert tile0(avg, 2048, 0, n, 0) == (2 << 20, 2048)            # lo = 2 MiB - 1: the grid starts at lo + 1,
    lo, hi = bm.region(avg, 0, n, 0)
    assert len(bm.tiles_between(KIND, 2048, lo + 1, hi)) == 16      # 16 full tiles instead of
    assert len(bm.tiles(KIND, 2048, avg, 0, n, 0)) == 17            # 16 and a one-step tile
    assert tile0(avg, 2048, 0, n, 1)[0] == 2 << 20                 # off0 = 1: lo is a line's first byte
    assert tile0(avg, 2048, 0, (2 << 20), 0)[0] == (2 << 20) - 128  # a one-byte region keeps the line rule


def cases(avg, lane_cap):
    """[(label, n, misalignment, items)]"""
    mn = avg // 2
    T = bm.WAVE * lane_cap
    out = []
    for mis in MISALIGN:
        off0 = mis % 16
        lo = mn - 1
        # short streams: every plant that fits
        for extra in (0, 1, 127, 128, 129):
            n = mn + extra
            out.append((f"n min+{extra} mis {mis} bare", n, mis, ()))
            for dl in (-1, 0, 1):
                if lo + dl <= n - 1:
                    out.append((f"n min+{extra} mis {mis} lo{dl:+d}", n, mis, (("w", lo + dl),)))
        # long streams: the first region's edge, a further plant behind lo - 1
        n = mn + 9 * T + 13  # (10 tiles: more than a visit's quantum, 6 tiles at 1M: a stream without a cut yields)
        ct, L = tile0(avg, lane_cap, 0, n, off0)
        last = ct + bm.WAVE * L - 1 - off0
        assert L == lane_cap and lo < last < n
        out.append((f"long mis {mis} lo-1", n, mis, (("w", lo - 1), ("w", lo + 2 * T + 77))))
        out.append((f"long mis {mis} lo-1 alone", n, mis, (("w", lo - 1),)))
        out.append((f"long mis {mis} lo", n, mis, (("w", lo),)))
        out.append((f"long mis {mis} lo+1", n, mis, (("w", lo + 1),)))
        out.append((f"long mis {mis} tile 0's last byte", n, mis, (("w", last),)))
        out.append((f"long mis {mis} tile 1's first byte", n, mis, (("w", last + 1),)))
        # second regions: the first cut at c, so lo2 = c + min - 1; (lo2 + off0) % 128 == 127 takes
        # the new rule (a candidate on lo2 itself, next to it, or none), == 63 the old one
        for r, what in ((127, "line end"), (63, "mid-line")):
            p = lo + T + 300
            p += (r - (p + 1 + mn - 1 + off0)) % 128
            c = p + 1
            lo2 = c + mn - 1
            assert (lo2 + off0) % 128 == r
            n2 = c + mn + 3 * T + 5
            assert n2 <= bm.BG_LEN
            for dl in (-1, 0, 1):
                out.append((f"second region {what} mis {mis} lo2{dl:+d}", n2, mis, (("w", p), ("w", lo2 + dl))))
            out.append((f"second region {what} mis {mis} bare", n2, mis, (("w", p),)))
            out.append((f"second region {what} mis {mis} one byte", c + mn, mis, (("w", p),)))
            out.append((f"second region {what} mis {mis} two bytes", c + mn + 1, mis, (("w", p), ("w", lo2 + 1))))
    return [bm.Case(label, n, mis, items) for label, n, mis, items in out]


class Layout:
    """The streams of the cases in one device buffer, each `misalignment` bytes (Case.off0 here:
    0, 1, 15 or 16) past a 256-byte boundary, with the oracle's cuts."""

    def __init__(self, name, avg, cs, built):
        import torch
        self.cases = cs
        offs, o = [], 0
        for c in cs:
            offs.append(o + c.off0)
            o += (c.off0 + c.n + 256 + 255) & ~255
        host = np.zeros(o, dtype=np.uint8)
        views = []
        for (d, _), at in zip(built, offs):
            host[at:at + d.size] = d
            views.append(host[at:at + d.size])
        self.want = [w.tolist() for w in coracle.split_batch(name, views, nthreads=16)]
        for c, (d, planted), w in zip(cs, built, self.want):  # the model's word on its own input
            assert bm.expected(planted, c.n, avg).tolist() == w, c.label
        self.buf = torch.from_numpy(host).to("cuda:0")
        assert self.buf.data_ptr() % 256 == 0
        self.ptrs = [self.buf.data_ptr() + at for at in offs]
        self.lens = [c.n for c in cs]
        assert {p % 256 for p in self.ptrs} <= set(MISALIGN)


@lru_cache(maxsize=None)
def built(geom):
    """(cases, [(bytes, planted candidates)]) of a geometry."""
    _, avg, cap = GEOMS[geom]
    cs = cases(avg, cap)
    return cs, [bm.plant(KIND, avg, c.n, c.items) for c in cs]


@lru_cache(maxsize=None)
def layout(geom):
    name, avg, _ = GEOMS[geom]
    return Layout(name, avg, *built(geom))


@pytest.fixture(scope="module", autouse=True)
def _release_layouts():
    yield
    import torch
    layout.cache_clear()
    built.cache_clear()
    torch.cuda.empty_cache()


def test_cases_reach_both_rules():
    """The layouts hold regions under each rule, decided at lo, next to it and not at all."""
    for geom, (name, avg, cap) in GEOMS.items():
        new = old = 0
        for c, (_, planted) in zip(*built(geom)):
            off0 = c.off0 % 16
            s = 0
            for cut in bm.expected(planted, c.n, avg).tolist():
                if bm.region(avg, s, c.n, off0) is not None:
                    lo, hi = bm.region(avg, s, c.n, off0)
                    if tile0(avg, cap, s, c.n, off0)[0] == lo + 1:
                        new += 1
                    else:
                        old += 1
                s = cut
        assert new >= 40 and old >= 40, (name, cap, new, old)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_region_start(gpu, geom, regime):
    name, avg, cap = GEOMS[geom]
    g = layout(geom)
    kv = REGIMES[regime]
    tag = f"{name} lanes {cap} {regime}"
    with knobs(_knobs_of(KIND, cap, kv)):
        p = plan(name, len(g.ptrs))
        assert p[0] == cap and p[1] == (kv[_lib.TEST_NO_HELP] == 2), (tag, p)
        got, helps, _ = _launch(gpu, name, g.ptrs, g.lens)
    _compare(tag, g.cases, got, g.want)
    if kv[_lib.TEST_NO_HELP] == 1:
        assert helps == 0, tag
    else:
        assert helps > 0, f"{tag}: no tile was helped"


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["1M-2048"])
def test_region_start_with_backlog(gpu, geom):
    """2,304 stream pointers (aliases of the layout's streams) for 2,048 launch waves: first visits
    run with a backlog and yield after their quantum, and the streams queued behind them are set up
    by the waves that adopt them from the ring (the switching tile's prefetch, or a blocking take).
    With help off the yields are certain: the ring must have grown past its one entry per stream."""
    name, avg, cap = GEOMS[geom]
    g = layout(geom)
    reps = -(-2304 // len(g.cases))
    ptrs, lens, want, rcases = g.ptrs * reps, g.lens * reps, g.want * reps, g.cases * reps
    ns = len(ptrs)
    for regime, kv in [("backlog, help off", {_lib.TEST_NO_HELP: 1}), ("backlog, help by policy", {})]:
        tag = f"{name} lanes {cap} {regime}"
        with knobs(_knobs_of(KIND, cap, kv)):
            p = plan(name, ns)
            assert p[0] == cap and ns > p[3], (tag, p)
            got, _, entries = _launch(gpu, name, ptrs, lens)
        _compare(tag, rcases, got, want)
        assert entries > ns if kv else entries >= ns, (tag, entries, ns)


# ------------------------------------------------------------------ hand-offs at the 8-tile quantum
# DYNAMIC-2M-BUZHASH, 128 KiB tiles (16 steps of 128 bytes per lane): a whole region is 24 tiles and
# pipe_quantum_tiles gives visits of 8 (at 1M and below: 6, which tests/test_gpu_batch_edges.py
# walks).  With a backlog a first visit scans tiles 0..7, takes its next ticket at the top of tile 7
# (the switching tile) and yields; the wave that adopts the stream starts at tile 8.  Every plant
# below is placed on the grid the kernel uses (grid(): region_ct0's start, then tile_geom), at
# 16-byte aligned pointers (the line start) and at misaligned ones (the line rule).
H_NAME, H_AVG, H_CAP, H_Q = "DYNAMIC-2M-BUZHASH", 2 << 20, 2048, 8
H_T = bm.WAVE * H_CAP


def grid(avg, lane_cap, s, n, off0):
    """[(ct, L)] of the own tiles of the region of the chunk starting at s, by the kernel's rule."""
    _, hi = bm.region(avg, s, n, off0)
    return bm.tiles_between(KIND, lane_cap, tile0(avg, lane_cap, s, n, off0)[0], hi)


def test_quantum_model():
    """pipe_quantum_tiles restated: the region's K tiles in equal visits of at most 8."""
    def q(avg, cap):
        K = -(-(2 * avg - avg // 2) // (bm.WAVE * cap))
        return -(-K // -(-K // 8))
    assert [q(a << 20, 2048) for a in (1, 2, 4, 8)] == [6, 8, 8, 8] and q(512 << 10, 2048) == 6
    assert q(H_AVG, H_CAP) == H_Q


def boundary_cases():
    """One plant per stream around the start of tiles 7, 8 and 9 (8 is where a resumed wave starts);
    every stream goes on for min + a tile after its plant, so none ends as a tombstone."""
    mn = H_AVG // 2
    out = []
    for k in (H_Q - 2, H_Q - 1, H_Q):
        for dl in (-64, -1, 0, 1, 63, 64, 127, 128):
            for mis in (0, 1, 16):
                n = mn + (k + 2) * H_T + mn + H_T
                ts = grid(H_AVG, H_CAP, 0, n, mis % 16)
                assert ts[k + 1][1] == H_CAP and ts[k + 1][0] == ts[0][0] + (k + 1) * H_T
                out.append(bm.Case(f"tile {k}|{k + 1} delta {dl:+d} mis {mis}", n, mis,
                                   (("w", ts[k + 1][0] - mis % 16 + dl),)))
    return out


STEPS = (0, 1, 8, 14, 15)  # of the 16 steps of a full tile: first, second, middle, second-to-last, last


def ending_cases():
    """Streams that END on a candidate (the cut leaves min - 1 bytes: no further region) in step
    0, 1, 8, 14 or 15 of lane 5 of tile 0 (a visit's first tile), tile 7 (its last: the switching
    tile, whose reserved entry then becomes a tombstone) and tile 8 (the resumed visit's first).
    Streams ending in tile 0 or 8 take their next stream by the blocking take."""
    mn = H_AVG // 2
    out = []
    for tile in (0, H_Q - 1, H_Q):
        for step in STEPS:
            for mis in (0, 1):
                off0 = mis % 16
                ct = grid(H_AVG, H_CAP, 0, mn + 20 * H_T, off0)[0][0] + tile * H_T
                p = ct + 5 * H_CAP + 128 * step + 17 - off0
                n = p + mn
                ts = grid(H_AVG, H_CAP, 0, n, off0)
                assert ts[tile] == (ct, H_CAP) and bm.expected([p], n, H_AVG).tolist() == [p + 1, n]
                out.append(bm.Case(f"ends in tile {tile} step {step} mis {mis}", n, mis, (("w", p),)))
    return out


def tail_cases():
    """Streams without a candidate whose one region ends R bytes into tile 3 or tile 8: that tile
    is the stream's last (the switching position) and has one step (R <= 64 x 128) or two."""
    mn = H_AVG // 2
    out = []
    for k in (3, H_Q):
        for R in (1, 128, 64 * 128, 64 * 128 + 1, 64 * 256):
            for mis in (0, 1, 16):
                off0 = mis % 16
                ct0 = grid(H_AVG, H_CAP, 0, mn + 20 * H_T, off0)[0][0]
                n = ct0 + k * H_T + R - off0
                ts = grid(H_AVG, H_CAP, 0, n, off0)
                assert len(ts) == k + 1 and ts[k - 1][1] == H_CAP and ts[k][1] == (128 if R <= 64 * 128 else 256)
                assert n < 2 * H_AVG
                out.append(bm.Case(f"tail of {ts[k][1] // 128} step(s) in tile {k}, R {R} mis {mis}", n, mis, ()))
    return out


H_SETS = {"boundaries": boundary_cases, "endings": ending_cases, "tails": tail_cases}


@lru_cache(maxsize=None)
def hlayout(which):
    cs = H_SETS[which]()
    return Layout(H_NAME, H_AVG, cs, [bm.plant(KIND, H_AVG, c.n, c.items) for c in cs])


@pytest.fixture(scope="module", autouse=True)
def _release_hlayouts():
    yield
    hlayout.cache_clear()


def _aliased(g, ns=2304):
    reps = -(-ns // len(g.cases))
    return g.ptrs * reps, g.lens * reps, g.want * reps, g.cases * reps


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(H_SETS))
def test_handoffs_with_backlog(gpu, which):
    """2,304 aliased pointers for 2,048 launch waves: visits yield after 8 tiles and streams are
    adopted from the ring.  Help off (the yields are certain: the ring grows), then the launch's
    own help policy; every cut list against the oracle."""
    g = hlayout(which)
    ptrs, lens, want, rcases = _aliased(g)
    ns = len(ptrs)
    for regime, kv in [("help off", {_lib.TEST_NO_HELP: 1}), ("help by policy", {})]:
        tag = f"{H_NAME} {which}, backlog, {regime}"
        with knobs(_knobs_of(KIND, H_CAP, kv)):
            p = plan(H_NAME, ns)
            assert p[0] == H_CAP and ns > p[3], (tag, p)
            got, _, entries = _launch(gpu, H_NAME, ptrs, lens)
        _compare(tag, rcases, got, want)
        if kv and which != "tails":  # (the tails' streams of 4 tiles end within their first visit)
            assert entries > ns, (tag, entries, ns)


@pytest.mark.gpu
def test_unwritten_and_tombstone_entries(gpu):
    """The 1-poll cap of tests/test_gpu_queue.py on the ending streams: a third of them (tile 7)
    end in their switching tile, so their reserved entries are tombstones, and a wave that finds
    the entry behind its ticket not yet written gives up at once.  Every launch is exact, or
    raises KCDC_EIO with exactly the unfinished streams marked failed; the streams that did finish
    are exact either way."""
    import torch
    from kopia_amd import batch
    g = hlayout("endings")
    ptrs, lens, want, _ = _aliased(g)
    ns = len(ptrs)
    lib = _lib.lib()
    b = batch.make_device_batch(H_NAME, ptrs, lens, gpu)
    for _ in range(3):
        with knobs({_lib.TEST_SPIN_CAP: 1, _lib.TEST_NO_STEAL: 1, _lib.TEST_LANE_CAP: H_CAP, _lib.TEST_NO_HELP: 1}):
            batch.split_batch_device(H_NAME, b)
            torch.cuda.synchronize()
            giveups = _lib.check(lib.kcdc_test_queue_stat(_lib.STAT_GIVEUPS))
            done = _lib.check(lib.kcdc_test_queue_stat(_lib.STAT_DONE))
            entries = _lib.check(lib.kcdc_test_queue_stat(_lib.STAT_ENTRIES))
        # the ring starts with one entry per stream; every further one was reserved by a yielding
        # wave, and the streams that end in tile 7 leave theirs as tombstones
        assert entries > ns, (entries, ns)
        counts = b.counts.cpu().numpy()[:ns].view(np.uint64)
        lost = int((counts == np.uint64(_lib.COUNT_FAILED)).sum())
        assert lost == ns - done, (lost, done)
        if lost:
            assert giveups > 0
            with pytest.raises(_lib.KcdcError) as e:
                batch.read_cuts(b)
            assert e.value.code == _lib.KCDC_EIO
        else:
            got = batch.read_cuts(b)
            assert all(got[i].tolist() == want[i] for i in range(ns))
        cuts = b.cuts.cpu().numpy().view(np.uint64)
        base = b.cut_base.cpu().numpy().view(np.uint64)
        for i in np.nonzero(counts != np.uint64(_lib.COUNT_FAILED))[0]:
            c = int(counts[i])
            assert cuts[int(base[i]):int(base[i]) + c].tolist() == want[i], i
