"""The CPU model of the batch kernels' tile geometry and its planted inputs (tests/batch_model.py)
against the hashes' definitions and the C oracle.  What tests/test_gpu_batch_edges.py asserts about
its inputs -- where a planted candidate lies, and that it is the stream's only one -- rests on this."""
import numpy as np
import pytest

import batch_model as bm
import long_model as lm
from oracle import coracle

AVERAGES = [64 << 10, 128 << 10, 512 << 10, 1 << 20, 4 << 20]  # every average the GPU tests plant at
# (kind, lane cap, average) of the GPU tests' geometries G1-G4 and the backlog launches
GEOMS = [("buzhash", 512, 128 << 10), ("rabinkarp", 512, 128 << 10), ("buzhash", 2048, 512 << 10),
         ("rabinkarp", 2048, 512 << 10), ("buzhash", 4096, 512 << 10), ("buzhash", 4096, 4 << 20),
         ("buzhash", 2048, 1 << 20), ("rabinkarp", 2048, 1 << 20)]


def _name(kind, avg):
    return f"DYNAMIC-{avg >> 20}M-{kind.upper()}" if avg >= 1 << 20 else f"DYNAMIC-{avg >> 10}K-{kind.upper()}"


@pytest.mark.parametrize("kind", bm.KINDS)
def test_seed_windows_are_natural_candidates(kind):
    ws = bm.seeds(kind)
    assert len(ws) >= 16 and len({w.tobytes() for w in ws}) == len(ws)
    for w in ws:
        assert w.size == 64 and w.all()
        h = bm.window_hash(kind, w)
        assert h != 0
        for avg in AVERAGES:
            assert h & (avg - 1) == 0
    # made for a smaller average they need not hold at a larger one: the construction obeys `avg`
    small = bm.seed_windows(kind, 4096, 8, np.random.default_rng(1))
    hs = [bm.window_hash(kind, w) for w in small]
    assert all(h and h & 4095 == 0 for h in hs) and any(h & ((4 << 20) - 1) for h in hs)


@pytest.mark.parametrize("kind", bm.KINDS)
def test_seed_window_needs_every_byte(kind):
    """No byte of a seed window may be missing (read as zero) or changed: the hash then leaves the
    candidate set at the largest average -- what a zero-run plant cannot show.  The one exception
    is the hash's own: a Rabin-Karp byte in slot k contributes b * x^(8k) mod P, which for
    22 <= 8k and 8k + 7 < 53 + 3 touches none of the 22 masked bits before the reduction does
    (slots 3..6, window bytes 57..60): those four bytes cannot matter to any implementation."""
    w = bm.seeds(kind)[0]
    mask = bm.SEED_AVG - 1
    for i in range(64):
        if kind == "rabinkarp" and 3 <= 63 - i <= 6:
            continue
        for v in (0, int(w[i]) ^ 1):
            x = w.copy()
            x[i] = v
            assert bm.window_hash(kind, x) & mask, (i, v)


def test_background_is_candidate_free():
    bg = bm.background()
    assert bg.size == bm.BG_LEN and bg.all()
    for kind in bm.KINDS:
        for a, b in [(0, 1 << 20), (bm.BG_LEN - (1 << 20), bm.BG_LEN)]:
            assert lm.candidates_in(kind, bm.BG_AVG, bg, a, b).size == 0


def test_plant_finds_what_it_planted_and_refuses_overlaps():
    avg, n = 128 << 10, 300000
    for kind in bm.KINDS:
        d, planted = bm.plant(kind, avg, n, [("w", 100000), ("w", 100064), ("z", 200000, 3), ("w", n - 1)])
        assert planted.tolist() == [100000, 100064, 200000, 200001, 200002, n - 1]
        np.testing.assert_array_equal(lm.candidates(kind, avg, d), planted)  # the whole stream
        assert d[100000 - 63:100065].all() and not d[200000 - 63:200003].any()
        with pytest.raises(AssertionError):
            bm.plant(kind, avg, n, [("w", 100000), ("w", 100063)])


@pytest.mark.parametrize("kind,lane_cap,avg", GEOMS)
def test_planted_layouts_match_the_oracle(kind, lane_cap, avg):
    """rule(planted candidates) is what the C oracle cuts, for a sample of every sweep (its ends and
    every 16th delta), every named corner, and the few-stream and backlog sets."""
    name = _name(kind, avg)
    cases = bm.few_stream_cases(kind, lane_cap, avg)
    if avg < 4 << 20:  # (at 4M the GPU tests use the few-stream set only; the rest outgrows the background)
        cases += bm.corners(kind, lane_cap, avg) + bm.backlog_cases(kind, lane_cap, avg, 6 if kind == "buzhash" else 3)
    if avg < 1 << 20:
        for anchor in bm.anchors(kind, lane_cap, avg):
            sw = bm.sweep(kind, lane_cap, avg, anchor, bm.THIN)
            assert {c.off0 for c in sw} == set(range(16)), anchor  # every misalignment in every sweep
            cases += sw[::16] + [sw[-1]]
    built = bm.build(kind, avg, cases)
    want = coracle.split_batch(name, [np.asarray(d) for d, _ in built], nthreads=8)
    for c, (d, planted), w in zip(cases, built, want):
        assert bm.expected(planted, c.n, avg).tolist() == w.tolist(), c.label


def test_kept_alive_geometry():
    """DYNAMIC-128K-BUZHASH with 4 KiB lanes: one tile holds the whole region."""
    c = bm.kept_alive("buzhash", 4096, 128 << 10)
    k, lane, off, L, last = bm.locate("buzhash", 4096, 128 << 10, 0, c.n, c.off0, c.items[0][1])
    assert (k, last) == (0, True) and L == 3200 and lane > 0
    d, planted = bm.plant("buzhash", 128 << 10, c.n, c.items)
    assert coracle.split_stream("DYNAMIC-128K-BUZHASH", d).tolist() == [int(planted[0]) + 1, c.n]


GRID = [(kind, cap, avg, s, n, off0)
        for kind, cap, avg in [("buzhash", 256, 64 << 10), ("buzhash", 512, 128 << 10), ("buzhash", 4096, 128 << 10),
                               ("rabinkarp", 512, 128 << 10), ("rabinkarp", 2048, 512 << 10), ("buzhash", 2048, 512 << 10)]
        for s in (0, 77777)
        for n in (s + avg // 2, s + avg // 2 + 1, s + avg // 2 + 127, s + avg // 2 + 128 * 64, s + avg // 2 + 128 * 64 + 1,
                  s + avg, s + avg + 12345, s + 2 * avg - 1, s + 2 * avg, s + 2 * avg + 1, s + 3 * avg)
        for off0 in (0, 1, 9, 15)]


def test_tiles_cover_the_region_exactly_once():
    """The own tiles of a region are contiguous from lo & ~127, every tile but the last is full, the
    last one starts at or before hi and ends past it; a tile's lanes partition it; the sub-tiles of
    a help task cover their owner tile up to hi in the same way."""
    for kind, cap, avg, s, n, off0 in GRID:
        lo, hi = bm.region(avg, s, n, off0)
        ts = bm.tiles(kind, cap, avg, s, n, off0)
        full, u = bm.own_lane(kind, cap), bm.unit(kind)
        assert ts[0][0] == lo & ~127 and lo - ts[0][0] < 128
        at = ts[0][0]
        for i, (ct, L) in enumerate(ts):
            assert ct == at and L % u == 0 and 0 < L <= full and ct <= hi
            assert L == full or i == len(ts) - 1
            at = ct + bm.WAVE * L
        assert at > hi and at - hi - 1 < bm.WAVE * u + bm.WAVE  # the overshoot: under one rounding unit per lane
        T = bm.WAVE * full
        for k in range(1, len(ts)):
            sub = bm.help_subtiles(kind, cap, avg, s, n, off0, k)
            end = min(ts[k][0] + T - 1, hi)
            assert sub[0][0] == ts[k][0] and all(a + bm.WAVE * L == b for (a, L), (b, _) in zip(sub, sub[1:]))
            assert sub[-1][0] <= end < sub[-1][0] + bm.WAVE * sub[-1][1]
            assert len(sub) <= 2 and all(L <= bm.help_lane(kind, cap) for _, L in sub)
    assert bm.region(128 << 10, 5, 5 + (64 << 10) - 1, 3) is None  # shorter than min: no test region


def test_locate_and_position_are_inverse():
    rng = np.random.default_rng(7)
    for kind, cap, avg, s, n, off0 in GRID:
        lo, hi = bm.region(avg, s, n, off0)
        ts = bm.tiles(kind, cap, avg, s, n, off0)
        g = (kind, cap, avg, s, n, off0)
        ps = {lo - off0, hi - off0, ts[0][0] - off0, ts[-1][0] - off0, ts[-1][0] + bm.WAVE * ts[-1][1] - 1 - off0}
        ps |= {int(p) for p in rng.integers(ts[0][0] - off0, hi - off0 + 1, 16)}
        for p in ps:
            k, lane, off, L, last = bm.locate(*g, p)
            assert 0 <= lane < bm.WAVE and 0 <= off < L == ts[k][1] and last == (k == len(ts) - 1)
            assert bm.position(*g, k, lane, off) == p
        assert bm.locate(*g, lo - off0)[:2] == (0, (lo - ts[0][0]) // ts[0][1])
        assert bm.locate(*g, hi - off0)[4]
        for k, (ct, L) in enumerate(ts):
            for lane, off in [(0, 0), (63, L - 1), (31, L // 2)]:
                assert bm.locate(*g, bm.position(*g, k, lane, off))[:4] == (k, lane, off, L)


def test_step_of():
    assert bm.step_of("buzhash", 127, 512) == (0, 127) and bm.step_of("buzhash", 128, 512) == (1, 0)
    assert bm.step_of("rabinkarp", 511, 1024) == (0, 7, 63)      # chain A's last byte
    assert bm.step_of("rabinkarp", 512, 1024) == (1, 0, 0)       # chain B's first
    assert bm.step_of("rabinkarp", 1023, 1024) == (1, 7, 63)     # the drain step's last byte
