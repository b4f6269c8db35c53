"""GPU: the resident scan server behind private streaming handles (kcdc_splitter_next ->
server_scan_first in kcdc_kernels.hip, scan_server_kernel in kcdc_split_scan.h).  Cuts must be identical with the
server on and off and equal the oracle's, across the server's idle exit and relaunch, scratch
growth to whole-chunk slices, and concurrent handles (the busy server falls back to a launch).
test_wave_seams plants candidates on the seams between the eight waves' sub-ranges of a
copy-then-scan request (scan_request_cp), which serves the server, a private handle's own launch
and a group's launch alike."""
import threading
import time

import numpy as np
import pytest

import batch_model as bm
from kopia_amd import _lib
from kopia_amd import splitter as ks
from oracle import coracle

pytestmark = pytest.mark.gpu
SEED = 0x6B6F706961


def _feed(name, data, slices, s=None):
    s = s or ks.GetFactory(name)()
    cuts, i, k = [], 0, 0
    n = len(data)
    mv = memoryview(data)
    while i < n:
        num = min(slices[k % len(slices)], n - i)
        k += 1
        r = s.NextSplitPoint(mv[i:i + num])
        if r == -1:
            i += num
            continue
        i += r
        cuts.append(i)
    if not cuts or cuts[-1] != n:
        cuts.append(n)
    s.Close()
    return cuts


@pytest.fixture
def server(request):
    L = _lib.lib()
    yield L
    L.kcdc_test_set(_lib.TEST_NO_SERVER, 0)


@pytest.mark.parametrize("name", ["DYNAMIC-4M-BUZHASH", "DYNAMIC-1M-RABINKARP", "DYNAMIC-128K-BUZHASH"])
def test_server_on_off_oracle(gpu, server, name):
    data = coracle.gen_stream(SEED, 11, 24 << 20).tobytes()
    want = coracle.split_stream(name, np.frombuffer(data, np.uint8)).tolist()
    for off in (0, 1):
        server.kcdc_test_set(_lib.TEST_NO_SERVER, off)
        before = server.kcdc_test_server_requests()
        assert _feed(name, data, [64 << 10, 1000, 300000, 7]) == want, ("no_server", off)
        served = server.kcdc_test_server_requests() - before
        assert (served > 0) if off == 0 else (served == 0), (off, served)  # the path under test ran


def test_server_idle_relaunch(gpu, server):
    """The server exits after ~2 ms without requests; later calls relaunch it transparently."""
    name = "DYNAMIC-128K-BUZHASH"
    data = coracle.gen_stream(SEED, 12, 4 << 20).tobytes()
    want = coracle.split_stream(name, np.frombuffer(data, np.uint8)).tolist()
    s = ks.GetFactory(name)()
    cuts, i = [], 0
    mv = memoryview(data)
    while i < len(data):
        num = min(96 << 10, len(data) - i)
        r = s.NextSplitPoint(mv[i:i + num])
        time.sleep(0.004)  # past the idle limit: every call finds the server gone
        if r == -1:
            i += num
            continue
        i += r
        cuts.append(i)
    s.Close()
    if not cuts or cuts[-1] != len(data):
        cuts.append(len(data))
    assert cuts == want
    assert server.kcdc_test_server_requests() > 0


def test_server_scratch_growth(gpu, server):
    """Slices from 1 KiB up to whole 16 MiB (more than max_size): the server's scratch grows
    (the running server is drained first)."""
    name = "DYNAMIC-8M-BUZHASH"
    data = coracle.gen_stream(SEED, 13, 64 << 20).tobytes()
    want = coracle.split_stream(name, np.frombuffer(data, np.uint8)).tolist()
    assert _feed(name, data, [1 << 10, 64 << 10, 5 << 20, 16 << 20]) == want


def test_server_concurrent_handles(gpu, server):
    """Eight writers with private handles at once: with more than one private handle open the
    scans are launched side by side instead of queueing on the one-workgroup server; every
    writer's cuts equal the oracle's."""
    name = "DYNAMIC-1M-BUZHASH"
    streams = [coracle.gen_stream(SEED, 20 + w, 12 << 20).tobytes() for w in range(8)]
    wants = [coracle.split_stream(name, np.frombuffer(d, np.uint8)).tolist() for d in streams]
    got = [None] * 8

    def run(w):
        got[w] = _feed(name, streams[w], [64 << 10, 33333])

    th = [threading.Thread(target=run, args=(w,)) for w in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == wants


# ------------------------------------------------------------------ wave seams of a request
SLICE = 64 << 10
SCAN_WAVES = 8  # dev::kScanWaves: a request's span is scanned in this many sub-ranges


def _per(span):
    """Bytes per sub-range of a request of `span` positions: roundup64(ceil(span / 8))."""
    return (-(-span // SCAN_WAVES) + 63) & ~63


def _requests(avg, n, cands, slice_len=SLICE):
    """What _feed's calls ask of the GPU, from kcdc_splitter_next's arithmetic (kcdc_api.cpp): each
    request as (first position, span), in stream positions, and the cuts that follow when the
    stream's candidates are `cands`.  Below the minimum size nothing is tested; from there to the
    maximum size the rest of the slice is one request."""
    mn, mx = avg // 2, avg * 2
    reqs, cuts, i, count = [], [], 0, 0
    while i < n:
        num = min(slice_len, n - i)
        p, rest, r = i, num, -1
        fast = max(0, min(mn - count - 1, rest))
        count, p, rest = count + fast, p + fast, rest - fast
        fp = max(0, min(mx - count, rest))
        if fp > 0:
            reqs.append((p, fp))
            hit = [c for c in cands if p <= c < p + fp]
            if hit:
                r, count = fast + hit[0] - p + 1, 0
            else:
                count, fast = count + fp, fast + fp
        if r < 0 and count >= mx:
            r, count = fast, 0
        if r < 0:
            i += num
        else:
            i += r
            cuts.append(i)
    if not cuts or cuts[-1] != n:
        cuts.append(n)
    return reqs, cuts


def _seam_streams(kind, avg, n):
    """(label, bytes, planted candidates, [(candidate, sub-range, offset in it)]) per stream: one
    candidate on the last byte of sub-range w - 1, one on the first byte of sub-range w, for w in
    {1, 7}, each in a full 64 KiB request of an otherwise candidate-free stream; and one stream
    with candidates in sub-ranges 5 and 2 of one request."""
    blank, _ = _requests(avg, n, [])
    full = [r for r in blank if r[1] == SLICE]
    out = []
    for w, (p0, span) in ((1, full[0]), (7, full[1])):
        per = _per(span)
        out.append((f"last byte of sub-range {w - 1}", [p0 + w * per - 1], [(w - 1, per - 1)]))
        out.append((f"first byte of sub-range {w}", [p0 + w * per], [(w, 0)]))
    p0, span = full[2]
    per = _per(span)
    out.append(("sub-ranges 5 and 2", [p0 + 5 * per + 100, p0 + 2 * per + 17], [(5, 100), (2, 17)]))
    streams = []
    for label, pos, where in out:
        data, planted = bm.plant(kind, avg, n, [("w", c) for c in pos])
        streams.append((label, data, planted.tolist(), list(zip(pos, where))))
    return streams


@pytest.mark.parametrize("name,kind", [("DYNAMIC-128K-BUZHASH", "buzhash"), ("DYNAMIC-128K-RABINKARP", "rabinkarp")])
def test_wave_seams(gpu, server, name, kind):
    """A candidate on the last byte of one wave's sub-range, on the first byte of the next, and
    two candidates in sub-ranges 5 and 2 of one request (the earlier wins): cuts equal the oracle's
    through the server, a private handle's own launch and a grouped handle."""
    avg, n = 128 << 10, (512 << 10) + 4321
    for label, data, planted, where in _seam_streams(kind, avg, n):
        reqs, model_cuts = _requests(avg, n, planted)
        for c, (w, off) in where:  # the planted positions do fall on the seams
            p0, span = next(r for r in reqs if r[0] <= c < r[0] + r[1])
            assert span == SLICE and divmod(c - p0, _per(span)) == (w, off), (label, c, p0, span)
        if len(where) == 2:  # both in the same request, the later sub-range planted first
            assert len({next(r for r in reqs if r[0] <= c < r[0] + r[1]) for c, _ in where}) == 1
            assert min(planted) + 1 in model_cuts and max(planted) + 1 not in model_cuts
        want = coracle.split_stream(name, data).tolist()
        assert model_cuts == want, label  # the request model above follows the same rule
        raw = data.tobytes()
        for off in (0, 1):
            server.kcdc_test_set(_lib.TEST_NO_SERVER, off)
            before = server.kcdc_test_server_requests()
            assert _feed(name, raw, [SLICE]) == want, (label, "no_server", off)
            served = server.kcdc_test_server_requests() - before
            assert (served > 0) if off == 0 else (served == 0), (label, off, served)
        g = ks.SplitterGroup(name, 0)
        try:
            assert _feed(name, raw, [SLICE], g.splitter()) == want, (label, "group")
        finally:
            g.close()
