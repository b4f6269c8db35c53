"""GPU: the batch kernels (split_batch_pipe_kernel for buzhash, split_batch_rk_kernel for
Rabin-Karp) on the seams of their tile geometry, through kcdc_split_batch_device, bit-exact
against the C oracle.

The random-data suites (test_gpu_parity.py, test_gpu_help.py) pin the queue and help protocol, but
a cut lands on a seam there only by chance: on DYNAMIC-4M-BUZHASH about one candidate in 2,000 is
the first byte of a lane and one in 130,000 the first byte of a tile.  Here every seam gets a
candidate planted on it and around it (tests/batch_model.py, pinned to the oracle and to the
hashes' definitions by tests/test_batch_model.py): the 64 bytes a lane warms from its neighbour's
tail, tile 0's head below lo, the overshoot past hi, the ragged last tile, the half-lane sub-tiles
of a help task, the two chains of a Rabin-Karp lane, and the tile a yielded stream resumes on.
The planted windows are natural -- no zero byte, a non-zero hash -- so each of their 64 bytes has
to reach the hash from the right place; a window of zeros would hash to 0 with bytes missing.

One planted candidate decides one chunk; the cases are short streams (one min size plus a few
tiles), many per launch, every one at its own misalignment (all of 0..15 in every sweep).

  geometries  G1 DYNAMIC-128K-*: buzhash lanes 512 (32 KiB tiles), Rabin-Karp 1024 (64 KiB);
              G2 DYNAMIC-512K-*: the default lanes, 2048 and 4096 (128 and 256 KiB tiles);
              G3 G2's buzhash with 4 KiB lanes (KCDC_TEST_LANE_CAP = 4096);
              G4 DYNAMIC-4M-BUZHASH with few streams, where the plan itself takes 4 KiB lanes.
  sweeps      one candidate per stream at anchor + delta (batch_model.sweep): lo, hi with the
              stream going on, hi = n - 1 with 1 .. 64 * 128 + 1 bytes left in the ragged last tile,
              the tile boundaries 0|1, 1|2 and a far one, the lane boundaries 0|1, 31|32, 62|63,
              the middle of a Rabin-Karp lane, the middle of a tile; delta over every value in
              -129..129 on G1, over -65..65 and +-127..129 on G2 and G3.
  corners     batch_model.corners: which of two candidates in a tile, a lane, a step, a chain
              wins; lo - 1 | lo; hi | hi + 1; a stream a candidate keeps alive; zero runs.
  regimes     R1 help off; R2 help forced on, whole regions published; R3 help forced on, windows of
              3 tiles; every layout under all three, each compared with the oracle (so identical
              across them).  R4: 2,304 aliased stream pointers, so visits run with a backlog and
              yield after their quantum, with plants around the tile a resumed wave starts on.

Which wave scans a far tile under help -- its owner or a helper, and then in which sub-tile -- is
a matter of timing; nothing here asserts it.  What is asserted is that help happened at all
(STAT_HELPS) where regions are long enough to publish, and that no wave gave up.

Every test first checks the lane cap its layout assumes against the library's own plan
(kcdc_test_batch_plan), and bounds its launches with a small KCDC_TEST_SPIN_CAP so a regression
fails fast."""
import ctypes as C
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

import batch_model as bm
from kopia_amd import _lib, batch
from oracle import coracle

pytestmark = pytest.mark.gpu
SPIN_CAP = 200000
# geometry: (average, {kind: BatchArgs::lane_cap}, deltas)
GEOMS = {"G1": (128 << 10, {"buzhash": 512, "rabinkarp": 512}, bm.FULL),
         "G2": (512 << 10, {"buzhash": 2048, "rabinkarp": 2048}, bm.THIN),
         "G3": (512 << 10, {"buzhash": 4096}, bm.THIN)}
REGIMES = {"R1 help off": {_lib.TEST_NO_HELP: 1},
           "R2 help on, whole regions": {_lib.TEST_NO_HELP: 2, _lib.TEST_HELP_WINDOW: 255},
           "R3 help on, windows of 3": {_lib.TEST_NO_HELP: 2, _lib.TEST_HELP_WINDOW: 3}}


def _name(kind, avg):
    return f"DYNAMIC-{avg >> 20}M-{kind.upper()}" if avg >= 1 << 20 else f"DYNAMIC-{avg >> 10}K-{kind.upper()}"


@contextmanager
def knobs(kv):
    """Test knobs set for the block and back at 0 after it, whatever happens inside."""
    lib = _lib.lib()
    try:
        for k, v in kv.items():
            assert lib.kcdc_test_set(k, v) == 0, _lib.last_error()
        yield
    finally:
        for k in kv:
            lib.kcdc_test_set(k, 0)


def _knobs_of(kind, lane_cap, regime=None):
    kv = {_lib.TEST_SPIN_CAP: SPIN_CAP}
    if kind == "buzhash" and lane_cap:  # (the knob is the buzhash kernel's; Rabin-Karp keeps its rule)
        kv[_lib.TEST_LANE_CAP] = lane_cap
    kv.update(regime or {})
    return kv


def plan(name, ns):
    """(lane_cap, helpers, help_window, waves) of a launch of ns streams under the current knobs."""
    out = (C.c_uint32 * 4)()
    _lib.check(_lib.lib().kcdc_test_batch_plan(name.encode(), ns, out))
    return tuple(int(x) for x in out)


def _stat(key):
    return _lib.check(_lib.lib().kcdc_test_queue_stat(key))


class Group:
    """The streams of some cases in one device buffer, each off0 bytes past a 256-byte boundary,
    with the oracle's cuts."""

    def __init__(self, name, kind, avg, cases):
        import torch
        self.cases = cases
        built = bm.build(kind, avg, cases)
        offs, o = [], 0
        for c in cases:
            offs.append(o + c.off0)
            o += (c.off0 + c.n + 256 + 255) & ~255
        host = np.zeros(o, dtype=np.uint8)
        views = []
        for (d, _), at in zip(built, offs):
            host[at:at + d.size] = d
            views.append(host[at:at + d.size])
        self.want = [w.tolist() for w in coracle.split_batch(name, views, nthreads=16)]
        for c, (d, planted), w in zip(cases, built, self.want):  # the model's word on its own input
            assert bm.expected(planted, c.n, avg).tolist() == w, c.label
        self.buf = torch.from_numpy(host).to("cuda:0")
        assert self.buf.data_ptr() % 256 == 0
        self.ptrs = [self.buf.data_ptr() + at for at in offs]
        self.lens = [c.n for c in cases]
        assert sorted({p % 16 for p in self.ptrs}) == sorted({c.off0 for c in cases})


@lru_cache(maxsize=None)
def group(geom, kind, anchor):
    avg, caps, deltas = GEOMS[geom]
    cases = bm.corners(kind, caps[kind], avg) if anchor == "corners" else bm.sweep(kind, caps[kind], avg, anchor, deltas)
    return Group(_name(kind, avg), kind, avg, cases)


@pytest.fixture(scope="module", autouse=True)
def _release_layouts():
    yield
    import torch
    group.cache_clear()
    torch.cuda.empty_cache()


def _launch(gpu, name, ptrs, lens):
    """One launch; (cuts per stream, helps, ring entries)."""
    import torch
    b = batch.make_device_batch(name, ptrs, lens, gpu)
    batch.split_batch_device(name, b)
    torch.cuda.synchronize()
    assert _stat(_lib.STAT_GIVEUPS) == 0, "a wave gave up waiting"
    assert _stat(_lib.STAT_DONE) == len(ptrs)
    assert _stat(_lib.STAT_TICKET_AUDIT) == 0
    return batch.read_cuts(b), _stat(_lib.STAT_HELPS), _stat(_lib.STAT_ENTRIES)


def _compare(tag, cases, got, want):
    bad = [f"{c.label}: got {g.tolist()[:4]} want {w[:4]}" for c, g, w in zip(cases, got, want) if g.tolist() != w]
    assert not bad, f"{tag}: {len(bad)} of {len(cases)} streams differ: " + "; ".join(bad[:6])


def _cases():
    for geom, (avg, caps, _) in GEOMS.items():
        for kind, cap in caps.items():
            for anchor in bm.anchors(kind, cap, avg) + ["corners"]:
                yield pytest.param(geom, kind, anchor, id=f"{geom}-{kind}-{anchor}")


@pytest.mark.parametrize("geom,kind,anchor", list(_cases()))
def test_planted_seam(gpu, geom, kind, anchor):
    """One anchor's sweep (or the named corners) of one geometry, under R1, R2 and R3."""
    avg, caps, _ = GEOMS[geom]
    name, cap = _name(kind, avg), caps[kind]
    g = group(geom, kind, anchor)
    # long enough to publish (>= kHelpMinTiles tiles) in every stream: all but the ragged-end sweeps
    shareable = not anchor.startswith("end")
    for regime, kv in REGIMES.items():
        tag = f"{geom} {name} lanes {bm.own_lane(kind, cap)} {regime} anchor {anchor}"
        with knobs(_knobs_of(kind, cap, kv)):
            p = plan(name, len(g.ptrs))
            assert p[0] == cap and p[1] == (kv[_lib.TEST_NO_HELP] == 2), (tag, p)
            assert p[2] == (3 if kv.get(_lib.TEST_HELP_WINDOW) == 3 else 0), (tag, p)
            got, helps, _ = _launch(gpu, name, g.ptrs, g.lens)
        _compare(tag, g.cases, got, g.want)
        if kv[_lib.TEST_NO_HELP] == 1:
            assert helps == 0, tag
        elif shareable:
            assert helps > 0, f"{tag}: no tile was helped"


def test_few_streams_take_4k_lanes_by_plan(gpu):
    """G4: DYNAMIC-4M-BUZHASH with a dozen streams: help is on by the policy and the plan doubles
    the lanes to 4 KiB without the knob."""
    kind, avg, name = "buzhash", 4 << 20, "DYNAMIC-4M-BUZHASH"
    cases = bm.few_stream_cases(kind, 4096, avg)
    assert 12 <= len(cases) <= 16
    g = Group(name, kind, avg, cases)
    with knobs({_lib.TEST_SPIN_CAP: SPIN_CAP}):
        p = plan(name, len(cases))
        assert p[:2] == (4096, 1) and p[3] >= 1024, p
        assert plan(name, 4096)[0] == 2048  # (with more streams than waves the lanes stay at 2 KiB)
        got, helps, _ = _launch(gpu, name, g.ptrs, g.lens)
    _compare(f"G4 {name} lanes 4096 by plan", cases, got, g.want)
    assert helps > 0


@pytest.mark.parametrize("regime", list(REGIMES))
def test_candidate_keeps_a_finished_stream_alive(gpu, regime):
    """visit_resolve's `else if (live)`: the wave took its next ticket expecting the stream to end
    with this tile (the forced cut would leave less than min), a candidate cuts earlier, and the
    stream goes back into the ring on a fresh entry.  DYNAMIC-128K-BUZHASH with 4 KiB lanes: one
    tile holds the whole region, the candidate lies well inside it."""
    kind, avg, cap, name = "buzhash", 128 << 10, 4096, "DYNAMIC-128K-BUZHASH"
    cases = [bm.kept_alive(kind, cap, avg, off0) for off0 in range(16)]
    g = Group(name, kind, avg, cases)
    assert all(len(w) == 2 and w[1] - w[0] >= avg // 2 for w in g.want)
    with knobs(_knobs_of(kind, cap, REGIMES[regime])):
        assert plan(name, len(cases))[0] == cap
        got, _, entries = _launch(gpu, name, g.ptrs, g.lens)
    _compare(f"kept alive, {name} lanes {cap} {regime}", cases, got, g.want)
    # the ring starts with one entry per stream (init_ring_kernel: tail = n); each requeue adds one
    assert entries >= 2 * len(cases), entries


@pytest.mark.parametrize("kind", bm.KINDS)
@pytest.mark.parametrize("avg", [512 << 10, 1 << 20])
def test_resumed_visits(gpu, kind, avg):
    """R4: 2,304 stream pointers (144 aliases of each planted stream) for 2,048 launch waves, so
    every first visit runs with a backlog and yields after its quantum (6 buzhash tiles, 3
    Rabin-Karp tiles); the plants sit around the tile boundaries next to the quantum's end, so a
    resumed wave's first tile starts on or next to a candidate whose window the wave before it
    scanned up to.  With help off the yields are certain: the ring (one entry per stream at the
    start, init_ring_kernel) must have grown, and no yielded stream of this layout can end as a
    tombstone (every stream stays alive after its plant), so every further entry is a requeue.
    Then the same launch under the launch's own help policy."""
    name, cap = _name(kind, avg), 2048
    q = 6 if kind == "buzhash" else 3
    cases = bm.backlog_cases(kind, cap, avg, q)
    assert len(cases) >= 16
    g = Group(name, kind, avg, cases)
    reps = -(-2304 // len(cases))
    ptrs, lens, want, rcases = g.ptrs * reps, g.lens * reps, g.want * reps, cases * reps
    ns = len(ptrs)
    assert ns >= 2304
    for regime, kv in [("R4 backlog, help off", {_lib.TEST_NO_HELP: 1}), ("R4 backlog, help by policy", {})]:
        tag = f"{name} lanes {bm.own_lane(kind, cap)} {regime}"
        with knobs(_knobs_of(kind, cap, kv)):
            p = plan(name, ns)
            assert p[0] == cap and ns > p[3], (tag, p)
            got, _, entries = _launch(gpu, name, ptrs, lens)
        _compare(tag, rcases, got, want)
        assert entries > ns if kv else entries >= ns, (tag, entries, ns)
