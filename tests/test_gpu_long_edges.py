"""GPU: the long-stream path (kcdc_split_long_device, and the long streams of
kcdc_split_files_device) at the edges of its resolvers.

The scan keeps the first kSegK = 8 candidates of every 128 KiB coordinate segment; a stream
whose segments all fit resolves in parallel (resolve_par_kernel), one with a truncated segment
serially (resolve_kernel), which rescans where a truncated segment may hide the candidate it
needs.  tests/test_gpu_long.py feeds inputs where no segment is truncated or every one is.
Here the inputs sit between and on the corners:

  B1  the KAT input at averages 8192 / 16384: truncated segments scattered among complete ones;
  B2  planted streams: a scrubbed (candidate-free) background with runs of 63 + k zero bytes,
      each of which is exactly k consecutive candidates for both hashes, placed so that cuts fall
      on the last and first byte of a segment, on the 8th listed and the first unlisted candidate,
      with exactly 8, 9 and 12 candidates in a segment, two forced cuts in a row and a short tail;
      candidate-free streams around the lo >= n tail;
  B3  several long streams in one launch (kcdc_split_files_device), serial and parallel mixed;
  B4  the cuts_cap overflow contract of both resolvers;
  B5  the parallel resolver's node-table fallback (KCDC_TEST_PAR_NODE_CAP);
  B6  the scan kernels' own seams (cand_scan_dma_kernel, cand_scan_rk_kernel: the batch kernels'
      feed, their own segment loop): natural planted windows -- no zero byte, a non-zero hash, so
      every one of their 64 bytes has to be fetched from the right place, which a zero run cannot
      show -- swept over a 128 KiB segment boundary, the 2 KiB lane boundaries 0|1 and 31|32 and
      the middle of a lane, where Rabin-Karp's chain A meets chain B.

Every comparison is bit-exact against the C oracle.  Every test first asserts, from the CPU model
(tests/long_model.py, pinned to the oracle by tests/test_long_model.py), that its input is in the
regime it is meant to reach, and afterwards, through kcdc_test_long_stat, that the resolver it
expects took the stream: a test that lands in another regime fails."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import batch_model as bm
import long_model as lm
from kopia_amd import _lib, batch
from kopia_amd import splitter as ks
from oracle import coracle

pytestmark = pytest.mark.gpu
SEED = 0x6B6F706961
SEG = lm.SEG
KINDS = ["buzhash", "rabinkarp"]
NAME = {"buzhash": "DYNAMIC-1M-BUZHASH", "rabinkarp": "DYNAMIC-1M-RABINKARP"}
AVG = 1 << 20
MN, MX = AVG // 2, 2 * AVG
SENTINEL = -7


class knob:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        assert _lib.lib().kcdc_test_set(self.key, self.value) == 0

    def __exit__(self, *exc):
        _lib.lib().kcdc_test_set(self.key, 0)


def _long_stat():
    """(streams, serially resolved streams) of the last long-path launch; synchronise first."""
    lib = _lib.lib()
    return _lib.check(lib.kcdc_test_long_stat(_lib.LONG_STREAMS)), _lib.check(lib.kcdc_test_long_stat(_lib.LONG_SERIAL))


# ------------------------------------------------------------------ inputs (host, built once)
# A chain of links (delta, j, k): cut candidate i lies at p_i = p_{i-1} + MN + delta, i.e. delta
# bytes past the first position (lo) at which the chunk after cut i-1 may end, and is member j of
# a run of k consecutive candidates -- so the j members before it are below lo and must be skipped.
FAR = 2 * MX + 4 * SEG + 77  # two forced cuts, then a candidate 4 segments and 77 bytes past lo
LINKS_TRUNC = [(None, 0, 1), (0, 8, 9), (1, 0, 1), (2047, 0, 8), (0, 7, 8), (0, 8, 12), (FAR, 0, 1), (0, 0, 1)]
LINKS_COMPLETE = [(None, 0, 1), (0, 7, 8), (1, 0, 1), (2047, 0, 8), (0, 7, 8), (0, 5, 6), (FAR, 0, 1), (0, 0, 1)]
PHASES = [SEG - 1, SEG - 1, 0, 2047, 2047, 2047, 2124, 2124]  # (p_i + off0) % SEG
TAIL = 12345


def _chain(links, off0):
    """(cut candidates p_i, all planted candidates, stream length)."""
    ps, planted = [], []
    for delta, j, k in links:
        p = 5 * SEG - 1 - off0 if delta is None else ps[-1] + MN + delta
        ps.append(p)
        planted += list(range(p - j, p - j + k))
    return ps, np.asarray(planted, dtype=np.int64), ps[-1] + MN + TAIL


def _expected_cuts(ps, n):
    """What the chunk rule gives when the planted candidates are the only ones."""
    cuts = [p + 1 for p in ps[:6]] + [ps[5] + 1 + MX, ps[5] + 1 + 2 * MX] + [p + 1 for p in ps[6:]] + [n]
    return np.asarray(cuts, dtype=np.int64)


BG_LEN = _chain(LINKS_TRUNC, 0)[2] + 64


@lru_cache(maxsize=1)
def background() -> np.ndarray:
    """Counter-PRNG bytes without zero bytes and without one candidate of either hash at the
    1 MiB average (batch_model.scrubbed, the scrub the batch kernels' planted tests share)."""
    return bm.scrubbed(4242, BG_LEN, AVG)


def _plant(n, planted) -> np.ndarray:
    """The first n background bytes with each maximal run of planted candidates c .. c + k - 1
    made by zeroing bytes c - 63 .. c + k - 1.  Asserts from the model, for both hashes, that
    the stream's candidate set is exactly `planted`: the background has none, and the zeroing
    changes only the windows ending within 63 bytes past a run, which are hashed here."""
    d = background()[:n].copy()
    planted = np.asarray(planted, dtype=np.int64)
    starts = planted[np.concatenate([[True], np.diff(planted) != 1])] if planted.size else planted
    ends = planted[np.concatenate([np.diff(planted) != 1, [True]])] if planted.size else planted
    for a, b in zip(starts, ends):
        assert a - (lm.WINDOW - 1) >= 0 and b < n
        d[a - (lm.WINDOW - 1):b + 1] = 0
    for kind in KINDS:
        found = [lm.candidates_in(kind, AVG, d, int(a) - (lm.WINDOW - 1), int(b) + lm.WINDOW) for a, b in zip(starts, ends)]
        found = np.concatenate(found) if found else np.zeros(0, dtype=np.int64)
        np.testing.assert_array_equal(found, planted, kind)
    d.setflags(write=False)
    return d


@lru_cache(maxsize=None)
def chain_stream(which: str, off0: int):
    """(host bytes, expected cuts, planted candidates) of a planted chain at alignment off0,
    with its preconditions asserted: segment populations, cut phases, and the oracle's cuts."""
    links = LINKS_TRUNC if which == "trunc" else LINKS_COMPLETE
    ps, planted, n = _chain(links, off0)
    host = _plant(n, planted)
    assert [(p + off0) % SEG for p in ps] == PHASES
    counts, unlisted = lm.segment_stats(planted, off0, n)
    if which == "trunc":
        assert sorted(set(counts.tolist()) - {0}) == [1, 8, 9, 12]
        # the 9th candidate of the 9-segment, on the segment's last byte, and the 9th of the 12
        assert ps[1] in unlisted and ps[5] in unlisted and unlisted.size == 1 + 4
    else:
        assert sorted(set(counts.tolist()) - {0}) == [1, 6, 8] and unlisted.size == 0
    want = _expected_cuts(ps, n)
    for kind in KINDS:
        np.testing.assert_array_equal(coracle.split_stream(NAME[kind], host), want, kind)
        np.testing.assert_array_equal(lm.rule(planted, n, MN, MX), want)
    return host, want, planted


FREE_LENGTHS = [2 * MX, 2 * MX + 1, 2 * MX + MN - 1, 2 * MX + MN, 2 * MX + MN + 1]


@lru_cache(maxsize=None)
def free_stream(n: int, last_byte_candidate: bool = False):
    """A candidate-free stream of n bytes (optionally with one candidate planted on byte n - 1),
    its expected cuts and its candidates."""
    planted = np.asarray([n - 1] if last_byte_candidate else [], dtype=np.int64)
    host = _plant(n, planted)
    want = lm.rule(planted, n, MN, MX)
    assert want.tolist() == [MX, 2 * MX] + ([n] if n > 2 * MX else [])
    for kind in KINDS:
        np.testing.assert_array_equal(coracle.split_stream(NAME[kind], host), want, kind)
    return host, want, planted


@lru_cache(maxsize=None)
def random_stream(sid: int, n: int):
    """Unscrubbed counter-PRNG bytes; no segment is truncated at the 1 MiB average."""
    host = coracle.gen_stream(SEED, sid, n)
    for kind in KINDS:
        for off0 in (0, 15):
            counts, _ = lm.segment_stats(lm.candidates(kind, AVG, host), off0, n)
            assert counts.max(initial=0) <= lm.SEG_K
    host.setflags(write=False)
    return host


# ------------------------------------------------------------------ device helpers
def _arena(gpu, items):
    """One device buffer holding every (host bytes, off0) of `items`, each starting off0 bytes
    past a 256-byte boundary, with slack between them; returns (buffer, device pointers)."""
    import torch
    offs, o = [], 0
    for host, off0 in items:
        offs.append(o + off0)
        o += (off0 + host.size + 256 + 255) & ~255
    buf = torch.zeros(o, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 256 == 0
    for (host, _), at in zip(items, offs):
        buf[at:at + host.size] = torch.from_numpy(np.array(host)).to(gpu)
    return buf, [buf.data_ptr() + at for at in offs]


def _long_alone(gpu, name, ptr, n, serial=None):
    """kcdc_split_long_device on one resident stream; asserts the resolver when `serial` is given."""
    import torch
    with knob(_lib.TEST_LONG_STAT, 1):
        cuts, count, _ws = batch.split_long_device(name, ptr, n, gpu)
        torch.cuda.synchronize()
        got = batch.read_long(cuts, count)
        if serial is not None:
            assert _long_stat() == (1, int(serial))
    return got


def _long_host(gpu, name, host, off0, serial):
    buf, (ptr,) = _arena(gpu, [(host, off0)])
    return _long_alone(gpu, name, ptr, host.size, serial)


def _files(gpu, name, ptrs, lens, caps=None, slack=0):
    """kcdc_split_files_device with the caller's cut ranges (default: kcdc_cut_capacity each);
    returns (cuts incl. `slack` sentinel slots past cuts_cap, counts, bases, cuts_cap, stats)."""
    import torch
    n = len(ptrs)
    caps = [ks.cut_capacity(name, int(L)) for L in lens] if caps is None else caps
    base = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    cap = int(sum(caps))
    cuts = torch.full((cap + slack,), SENTINEL, dtype=torch.int64, device=gpu)
    counts = torch.zeros(n, dtype=torch.int64, device=gpu)
    p = np.asarray(ptrs, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    with knob(_lib.TEST_LONG_STAT, 1):
        _lib.check(_lib.lib().kcdc_split_files_device(name.encode(), p.ctypes.data, ln.ctypes.data, n, cuts.data_ptr(),
                                                      cap, base.ctypes.data, counts.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
        torch.cuda.synchronize()
        stat = _long_stat()
    return cuts.cpu().numpy(), counts.cpu().numpy(), base.astype(np.int64), cap, stat


# ------------------------------------------------------------------ B1: sporadic truncation
@lru_cache(maxsize=None)
def _kat_hashes(kind: str):
    host = coracle.gorand_read(5, 5_000_000)
    host.setflags(write=False)
    return host, lm.hashes(kind, host)


@pytest.mark.parametrize("misalign", [0, 5])
@pytest.mark.parametrize("avg", [8192, 16384])
@pytest.mark.parametrize("kind", KINDS)
def test_sporadic_truncation(gpu, kind, avg, misalign):
    """Truncated segments among complete ones; many cuts land on candidates the scan did not
    list, which only the serial resolver's rescan finds."""
    host, h = _kat_hashes(kind)
    want = coracle.split_stream_kind(kind, avg, host)
    counts, unlisted = lm.segment_stats(lm.candidates_of(h, avg), misalign, host.size)
    truncated = int((counts > lm.SEG_K).sum())
    on_unlisted = int(np.isin(want - 1, unlisted).sum())
    print(f"{kind}-{avg} off0 {misalign}: {truncated} truncated of {counts.size} segments, "
          f"{int((counts == 8).sum())} with 8, {int((counts == 9).sum())} with 9, {on_unlisted} cuts on unlisted")
    assert truncated >= 10 and int((counts <= lm.SEG_K).sum()) >= 1 and on_unlisted >= 20
    if avg == 16384:
        assert (counts == 8).any() and (counts == 9).any()
    got = _long_host(gpu, ks.custom_algorithm(kind, avg), host, misalign, serial=True)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------ B2: planted candidates
@pytest.mark.parametrize("off0", [0, 5, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_planted_truncated_chain(gpu, kind, off0):
    """Segments of exactly 9 and 12 candidates: the serial resolver, with its rescan starting on
    a segment's last byte (seg_end == lo + 1) and on the first unlisted candidate of 12."""
    host, want, _ = chain_stream("trunc", off0)
    np.testing.assert_array_equal(_long_host(gpu, NAME[kind], host, off0, serial=True), want)


@pytest.mark.parametrize("off0", [0, 5, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_planted_complete_chain(gpu, kind, off0):
    """No segment above 8 candidates (two with exactly 8, one run across a lane boundary, one
    ending on a segment's last byte): the parallel resolver, with two forced cuts in step A."""
    host, want, _ = chain_stream("complete", off0)
    np.testing.assert_array_equal(_long_host(gpu, NAME[kind], host, off0, serial=False), want)


@pytest.mark.parametrize("kind", KINDS)
def test_candidate_free_tails(gpu, kind):
    """Forced cuts only, with the tail after them one byte either side of min (lo >= n, and a
    rescan range of one byte); then one candidate on the stream's last byte."""
    cases = [free_stream(n) for n in FREE_LENGTHS] + [free_stream(2 * MX + MN, True)]
    assert cases[-1][2].tolist() == [2 * MX + MN - 1]
    buf, ptrs = _arena(gpu, [(host, i % 16) for i, (host, _, _) in enumerate(cases)])
    for (host, want, _), ptr in zip(cases, ptrs):
        np.testing.assert_array_equal(_long_alone(gpu, NAME[kind], ptr, host.size, serial=False), want, str(host.size))


# ------------------------------------------------------------------ B3: several long streams
def _mixed_items():
    """[(host, off0, expected cuts or None, serial)]: every stream >= 1 MiB and the total far below
    2000 x the smallest, so kcdc_split_files_device routes all of them to the long path."""
    t, tw, _ = chain_stream("trunc", 5)
    c, cw, _ = chain_stream("complete", 15)
    f, fw, _ = free_stream(2 * MX + MN + 1)
    m0, m1, r = random_stream(70, 1 << 20), random_stream(71, 1 << 20), random_stream(72, 3 << 20)
    items = [(t, 5, tw, 1), (c, 15, cw, 0), (f, 0, fw, 0), (m0, 0, None, 0), (m1, 15, None, 0), (r, 3, None, 0)]
    sizes = [h.size for h, _, _, _ in items]
    assert min(sizes) >= 1 << 20 and sum(sizes) < 2000 * min(sizes) // 4
    assert (m0.size + SEG - 1) // SEG == 8 and (m1.size + 15 + SEG - 1) // SEG == 9
    return items


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_long_streams_in_one_launch(gpu, kind, reverse):
    """Six long streams in one launch_split_long_multi: a serial one among parallel ones, streams
    with and without candidates, 8 against 9 segments for the same bytes.  Reversed, every
    stream's segment base, list slice and node base (lbeg + 2j) differ."""
    name = NAME[kind]
    items = _mixed_items()[::-1] if reverse else _mixed_items()
    buf, ptrs = _arena(gpu, [(h, o) for h, o, _, _ in items])
    lens = [h.size for h, _, _, _ in items]
    cuts, counts, base, cap, stat = _files(gpu, name, ptrs, lens, slack=8)
    assert stat == (len(items), sum(s for _, _, _, s in items))
    assert (cuts[cap:] == SENTINEL).all()
    for i, (host, _off0, want, serial) in enumerate(items):
        want = coracle.split_stream(name, host) if want is None else want
        np.testing.assert_array_equal(cuts[base[i]:base[i] + counts[i]], want, f"stream {i}")
        np.testing.assert_array_equal(_long_alone(gpu, name, ptrs[i], host.size, serial=bool(serial)), want, f"alone {i}")


# ------------------------------------------------------------------ B4: capacity
@pytest.mark.parametrize("which", ["trunc", "complete"])
@pytest.mark.parametrize("kind", KINDS)
def test_long_cut_capacity(gpu, kind, which):
    """cuts_cap below the true count, for the serial and for the parallel resolver: d_count is the
    true count, cuts[:cuts_cap] the oracle's prefix, and nothing is written past cuts_cap."""
    import torch
    name, off0 = NAME[kind], 5
    host, want, _ = chain_stream(which, off0)
    buf, (ptr,) = _arena(gpu, [(host, off0)])
    lib = _lib.lib()
    ws = torch.empty(int(lib.kcdc_long_workspace_bytes(name.encode(), host.size)), dtype=torch.uint8, device=gpu)
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for cap in (want.size - 1, 1, 0):
        cuts = torch.full((want.size + 8,), SENTINEL, dtype=torch.int64, device=gpu)
        count = torch.zeros(1, dtype=torch.int64, device=gpu)
        with knob(_lib.TEST_LONG_STAT, 1):
            _lib.check(lib.kcdc_split_long_device(name.encode(), ptr, host.size, cuts.data_ptr(), cap, count.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), st))
            torch.cuda.synchronize()
            assert _long_stat() == (1, int(which == "trunc"))
        c = cuts.cpu().numpy()
        assert int(count.item()) == want.size, cap
        np.testing.assert_array_equal(c[:cap], want[:cap], str(cap))
        assert (c[cap:] == SENTINEL).all(), cap


@pytest.mark.parametrize("which", ["trunc", "complete"])
@pytest.mark.parametrize("kind", KINDS)
def test_files_overflowing_long_stream_stays_in_its_range(gpu, kind, which):
    """Three long streams, the middle one's cut range a single slot: its true count is reported,
    its first cut written, and its neighbours' ranges and the slots past cuts_cap stay exact."""
    name = NAME[kind]
    mid, mid_want, _ = chain_stream(which, 5)
    a, b = random_stream(72, 3 << 20), random_stream(70, 1 << 20)
    wa, wb = coracle.split_stream(name, a), coracle.split_stream(name, b)
    buf, ptrs = _arena(gpu, [(a, 0), (mid, 5), (b, 15)])
    caps = [ks.cut_capacity(name, a.size), 1, wb.size]  # (the last range exactly full)
    cuts, counts, base, cap, stat = _files(gpu, name, ptrs, [a.size, mid.size, b.size], caps=caps, slack=8)
    assert stat == (3, int(which == "trunc"))
    assert counts.tolist() == [wa.size, mid_want.size, wb.size] and mid_want.size > 1
    assert cuts[base[1]] == mid_want[0]
    np.testing.assert_array_equal(cuts[:wa.size], wa)
    assert (cuts[wa.size:base[1]] == SENTINEL).all()
    np.testing.assert_array_equal(cuts[base[2]:cap], wb)
    assert (cuts[cap:] == SENTINEL).all()


# ------------------------------------------------------------------ B5: node-table fallback
@pytest.mark.parametrize("kind", KINDS)
def test_par_node_cap_fallback(gpu, kind):
    """Streams whose nodes (candidates + START + END, based at lbeg + 2j) do not fit the parallel
    resolver's tables resolve serially, with the same cuts.  Three complete streams of M_0, M_1,
    M_2 candidates: tables of (M_0 + 2) + (M_1 + 2) nodes hold the first two, one node less only
    the first."""
    name = NAME[kind]
    items = [chain_stream("complete", 0), free_stream(2 * MX + MN, True), chain_stream("complete", 15)]
    offs = [0, 7, 15]
    m = [int(p.size) for _, _, p in items]
    assert m[0] == m[2] == sum(k for _, _, k in LINKS_COMPLETE) and m[1] == 1
    buf, ptrs = _arena(gpu, [(h, o) for (h, _, _), o in zip(items, offs)])
    lens = [h.size for h, _, _ in items]
    fit2 = (m[0] + 2) + (m[1] + 2)
    for node_cap, serial in [(0, 0), (fit2, 1), (fit2 - 1, 2), (m[0] + 2, 2), (m[0] + 1, 3)]:
        try:
            assert _lib.lib().kcdc_test_set(_lib.TEST_PAR_NODE_CAP, node_cap) == 0
            cuts, counts, base, cap, stat = _files(gpu, name, ptrs, lens, slack=8)
        finally:
            _lib.lib().kcdc_test_set(_lib.TEST_PAR_NODE_CAP, 0)
        assert stat == (3, serial), node_cap
        for i, (_, want, _) in enumerate(items):
            np.testing.assert_array_equal(cuts[base[i]:base[i] + counts[i]], want, f"cap {node_cap} stream {i}")
        assert (cuts[cap:] == SENTINEL).all()


# ------------------------------------------------------------------ B6: the scan kernels' seams
SWEEP_AVG = 64 << 10  # a custom average: min 32 KiB, max 128 KiB, so streams stay at 5 segments
SWEEP_N = 5 * SEG
# anchor -> coordinate (stream position + off0) of the seam
SWEEP_ANCHORS = {"segment 2|3": 3 * SEG, "lane 0|1": 2 * SEG + lm.LANE, "lane 31|32": 2 * SEG + 32 * lm.LANE,
                 "mid lane 5": 2 * SEG + 5 * lm.LANE + lm.LANE // 2}


@lru_cache(maxsize=None)
def sweep_streams(kind: str, anchor: str):
    """[(delta, off0, host bytes, expected cuts)]: one natural candidate at the seam + delta, and
    before it a second one that makes the chunk rule ask for it (every plant decides a cut)."""
    out = []
    mn, mx = SWEEP_AVG // 2, 2 * SWEEP_AVG
    for i, delta in enumerate(range(-65, 66)):
        off0 = (7 * i + len(anchor)) % 16
        p = SWEEP_ANCHORS[anchor] - off0 + delta
        for items in ([("w", p - 40000), ("w", p)], [("w", p)]):
            host, planted = bm.plant(kind, SWEEP_AVG, SWEEP_N, items)
            want = lm.rule(planted, SWEEP_N, mn, mx)
            if p + 1 in want.tolist():
                break
        else:
            raise AssertionError(f"{anchor} delta {delta}: the plant decides no cut")
        counts, unlisted = lm.segment_stats(planted, off0, SWEEP_N)
        assert counts.max() <= 2 and unlisted.size == 0
        np.testing.assert_array_equal(coracle.split_stream_kind(kind, SWEEP_AVG, host), want)
        out.append((delta, off0, host, want))
    assert {o for _, o, _, _ in out} == set(range(16))
    return out


@pytest.mark.parametrize("anchor", list(SWEEP_ANCHORS))
@pytest.mark.parametrize("kind", KINDS)
def test_scan_seams(gpu, kind, anchor):
    """Natural candidates within 65 bytes either side of a segment boundary, two lane boundaries
    and a lane's middle (where Rabin-Karp's chain A meets chain B; a plain step boundary for buzhash):
    the scan must list each one, whichever lane, chain and
    segment its window straddles.  No segment is truncated: the parallel resolver takes them."""
    name = ks.custom_algorithm(kind, SWEEP_AVG)
    cases = sweep_streams(kind, anchor)
    buf, ptrs = _arena(gpu, [(host, off0) for _, off0, host, _ in cases])
    for (delta, off0, host, want), ptr in zip(cases, ptrs):
        got = _long_alone(gpu, name, ptr, host.size, serial=False)
        np.testing.assert_array_equal(got, want, f"{kind} {anchor} delta {delta} off0 {off0}")
