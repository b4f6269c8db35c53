"""GPU: the content-ID set (kcdc_dedup_*, kopia_amd/dedup.py) against the literal loop of
tests/dedup_model.py: every case of tests/dedup_cases.py with canaries in and guards around the
outputs, determinism across grids, a million IDs against a loaded set, two sets on two streams, and
the write path hash -> claim -> pack on one stream with no synchronisation between the calls."""
import numpy as np
import pytest

import dedup_cases as dc
import dedup_model as dm
from kopia_amd import _lib
from kopia_amd import dedup as kd
from kopia_amd import hashing as kh
from kopia_amd import packing as kp

pytestmark = pytest.mark.gpu
GUARD = 64
KEEP_CANARY, FIRST_CANARY, TOTALS_CANARY = 0xA5, 0x5A5A5A5A, -7777


def lib_home(id_len, max_keys, prefix, one):
    return _lib.lib().kcdc_test_dedup_home(id_len, max_keys, prefix, one)


class Pending:
    """One call's guarded device outputs; read() checks the guards and brings them to
    dedup_model.run's form."""

    def __init__(self, op, n, dev, stream):
        import torch
        self.op, self.n = op, n
        with torch.cuda.stream(stream):
            self.bytes = torch.full((n + 2 * GUARD,), KEEP_CANARY, dtype=torch.uint8, device=dev)
            self.first = torch.full((n + 2 * GUARD,), FIRST_CANARY, dtype=torch.int32, device=dev)
            self.totals = torch.full((3 + 2,), TOTALS_CANARY, dtype=torch.int64, device=dev)

    def read(self):
        n = self.n
        b = self.bytes.cpu().numpy()
        f = self.first.cpu().numpy().view(np.uint32)
        t = self.totals.cpu().numpy()
        assert (b[:GUARD] == KEEP_CANARY).all() and (b[GUARD + n:] == KEEP_CANARY).all(), "byte guards"
        assert (f[:GUARD] == FIRST_CANARY).all() and (f[GUARD + n:] == FIRST_CANARY).all(), "first guards"
        assert t[0] == TOTALS_CANARY and t[4] == TOTALS_CANARY, "totals guards"
        b, f = b[GUARD:GUARD + n], f[GUARD:GUARD + n]
        if self.op == "lookup":
            assert (f == FIRST_CANARY).all() and (t == TOTALS_CANARY).all()
            return ("l", b.tolist())
        if self.op == "claim":
            return ("t", int(t[1]), int(t[2]), int(t[3]), b.tolist(), f.tolist())
        assert (b == KEEP_CANARY).all() and (f == FIRST_CANARY).all()
        return ("t", int(t[1]), int(t[2]), int(t[3]))


def launch(cs, c, dev, stream, keepalive):
    """Start call `c` (a dedup_cases.Call, not a grow) on the set; returns its Pending."""
    import torch
    P = lambda t, off: t.data_ptr() + off
    if c.op == "clear":
        cs.clear(stream)
        return None
    n = len(c.ids)
    stride = c.stride or cs.id_len
    with torch.cuda.stream(stream):
        buf = torch.from_numpy(dc.buffer_of(c, cs.id_len)).to(dev)
    keepalive.append(buf)
    ids = P(buf, c.offset) if n else 0
    p = Pending(c.op, n, dev, stream)
    L, st = _lib.lib(), stream.cuda_stream
    if c.op == "claim":
        rc = cs.claim_raw(ids, stride, n, P(p.bytes, GUARD), P(p.first, 4 * GUARD), P(p.totals, 8), stream, c.prefix)
    elif c.op == "insert":
        rc = L.kcdc_dedup_insert_device(cs._h, c.prefix, ids, stride, n, P(p.totals, 8), st)
    else:
        rc = L.kcdc_dedup_lookup_device(cs._h, c.prefix, ids, stride, n, P(p.bytes, GUARD), st)
    assert rc == 0, _lib.last_error()
    return p


def run_gpu(vec, dev, stream=None):
    """Every call of the vector on a fresh set, no synchronisation between them; the results in
    dedup_model.run's form."""
    import torch
    stream = stream or torch.cuda.current_stream(dev)
    cs = kd.ContentSet(dev, vec.id_len, vec.max_keys)
    sets, pending, keepalive = [cs], [], []
    for c in vec.calls:
        if c.op == "grow":
            to = kd.ContentSet(dev, vec.id_len, c.max_keys)
            p = Pending("grow", 0, dev, stream)
            rc = _lib.lib().kcdc_dedup_grow_device(cs._h, to._h, p.totals.data_ptr() + 8, stream.cuda_stream)
            assert rc == 0, _lib.last_error()
            pending.append(p)
            sets.append(to)
            cs = to
        else:
            pending.append(launch(cs, c, dev, stream, keepalive))
    stream.synchronize()
    out = [("c",) if p is None else p.read() for p in pending]
    stored = 0
    for r in out:
        stored = r[3] if r[0] == "t" else 0 if r[0] == "c" else stored
    assert cs.count(stream) == stored
    for s in sets:
        s.close()
    return out


@pytest.fixture(scope="module")
def vectors():
    return {v.tag: v for v in dc.small_vectors(lib_home)}


SMALL_TAGS = ([v.tag for v in dc.size_vectors()] + ["copies64", "copies200", "shuffled", "repeat", "twins-len32",
                                                     "twins-len28", "one-home", "full", "lookup", "clear"])


@pytest.mark.parametrize("tag", SMALL_TAGS)
def test_cases_match_the_model(gpu, vectors, tag):
    """Cases 1-9: sizes around the wave, strides and odd alignments; copies of one ID; shuffled
    repeats; old and new IDs; near twins and prefixes; one probe chain that wraps; the refusal at
    max_keys and the grow; lookup, clear."""
    v = vectors[tag]
    assert run_gpu(v, gpu) == dm.run(v)


def test_count_and_refusal_leave_the_set(gpu):
    """Case 7 step by step: count at max_keys, the refused claim's outputs, count and lookup after."""
    import torch
    ids = dc.rand_ids(np.random.default_rng(7), 1001, 16)
    cs = kd.ContentSet.new(gpu, 16, 1000)
    d = torch.from_numpy(ids).to(gpu)
    t = cs.insert(d[:1000])
    assert cs.count() == 1000 and t.cpu().tolist() == [0, 1000, 1000]
    keep, first, t = cs.claim(d[1000:])
    assert t.cpu().tolist() == [kd.ENOSPC, 0, 1000]
    assert keep.cpu().tolist() == [0] and kd.first_numpy(first).tolist() == [kd.KNOWN]
    assert cs.count() == 1000 and cs.lookup(d).cpu().tolist() == [1] * 1000 + [0]
    big = kd.ContentSet.new(gpu, 16, 4000)
    assert cs.grow(big).cpu().tolist() == [0, 1000, 1000]
    keep, first, t = big.claim(d[1000:])
    assert (keep.cpu().tolist(), kd.first_numpy(first).tolist(), t.cpu().tolist()) == ([1], [0], [0, 1, 1001])
    assert big.lookup(d).cpu().tolist() == [1] * 1001 and big.count() == 1001 and cs.count() == 1000
    # the Python surface: prefixes as letters, empty calls, a strided view of wider rows
    wide = torch.zeros((5, 40), dtype=torch.uint8, device=gpu)
    wide[:, 3:19] = d[:5]
    assert big.lookup(wide[:, 3:19]).cpu().tolist() == [1] * 5
    assert big.lookup(wide[:, 3:19], prefix="k").cpu().tolist() == [0] * 5
    keep, _, t = big.claim(d[:0], want_first=False)
    assert keep.numel() == 0 and t.cpu().tolist() == [0, 0, 1001]
    cs.close()
    big.close()


def test_same_answer_from_any_grid(gpu):
    """Case 10: case 3's input plus 2^16 IDs with 30 % duplicates on fresh sets, one workgroup
    against the default grid: byte-identical outputs, equal to the model's."""
    ids = np.concatenate([dc.shuffled_ids(), dc.mixed_ids(10, 1 << 16, 30)])
    v = dc.Vec("grids", 16, 2 * len(ids), [dc.Call("claim", ids), dc.Call("claim", ids[::3].copy())])
    L = _lib.lib()
    try:
        assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, 1) == 0
        one = run_gpu(v, gpu)
    finally:
        assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, 0) == 0
    many = run_gpu(v, gpu)
    assert one == many
    assert many == dm.run(v)
    assert 0 < sum(many[0][4]) < len(ids)


def test_a_million_ids_against_a_loaded_set(gpu):
    """Case 11: 2^20 IDs with 30 % duplicates against a set preloaded with 2^20 others."""
    n = 1 << 20
    v = dc.Vec("million", 16, 2 * n, [dc.Call("insert", dc.rand_ids(np.random.default_rng(110), n, 16)),
                                       dc.Call("claim", dc.mixed_ids(111, n, 30))])
    got, want = run_gpu(v, gpu), dm.run(v)
    assert got[0] == want[0] == ("t", 0, n, n)
    assert got[1][:4] == want[1][:4]
    assert np.array_equal(np.array(got[1][4], np.uint8), np.array(want[1][4], np.uint8))
    assert np.array_equal(np.array(got[1][5], np.uint32), np.array(want[1][5], np.uint32))


def test_two_sets_on_two_streams(gpu):
    """Case 12: claims on two sets interleaved on two streams; each equals its own model."""
    import torch
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    vecs = []
    for k in range(2):
        pool = dc.rand_ids(np.random.default_rng(120 + k), 3000, 28)
        rng = np.random.default_rng(130 + k)
        vecs.append(dc.Vec(f"stream{k}", 28, 20000, [dc.Call("claim", pool[rng.integers(0, 3000, 2500)], stride=28 + k)
                                                    for _ in range(4)]))
    sets = [kd.ContentSet(gpu, 28, 20000) for _ in vecs]
    torch.cuda.synchronize(gpu)
    keepalive, pending = [], [[], []]
    for step in range(4):
        for k in range(2):
            pending[k].append(launch(sets[k], vecs[k].calls[step], gpu, streams[k], keepalive))
    for k in range(2):
        streams[k].synchronize()
        assert [p.read() for p in pending[k]] == dm.run(vecs[k]), k
    for s in sets:
        s.close()


def test_hash_claim_pack_on_one_stream(gpu):
    """Case 13: hash_chunks_device -> claim (IDs read where the hash left them) -> pack_chunks_device
    with the claim's device mask, one stream, no synchronisation between the calls: 200 chunks of
    1-64 KiB, 60 of them repeats, 40 known from an earlier batch.  Entries, packs and pack bytes
    equal those of the same pack call given the model's mask as a host array."""
    import torch
    rng = np.random.default_rng(13)
    name, key = "BLAKE3-256-128", bytes(range(32))
    # every other chunk is low-entropy, so the compressor's keep-or-drop rule goes both ways
    unique = [rng.integers(0, 256 if k % 2 else 4, int(rng.integers(1 << 10, (64 << 10) + 1)), dtype=np.uint8)
              for k in range(140)]
    order = np.concatenate([np.arange(140), rng.integers(0, 140, 60)])
    rng.shuffle(order)
    known = rng.permutation(140)[:40]
    chunks = [unique[i] for i in order]
    earlier = [unique[i] for i in known] + [rng.integers(0, 256, 5000, dtype=np.uint8) for _ in range(10)]

    def table(cs):
        lens = np.array([len(c) for c in cs], np.int64)
        return np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64), lens

    (offs0, lens0), (offs, lens) = table(earlier), table(chunks)
    n = len(chunks)
    nonces = torch.from_numpy(rng.integers(0, 256, (n, 12), dtype=np.uint8)).to(gpu)
    packer = kp.Packer("CHACHA20-POLY1305-HMAC-SHA256", bytes(range(100, 132)), 1 << 20, compression="zstd-fastest")
    st = torch.cuda.Stream(gpu)
    with torch.cuda.stream(st):
        d0 = torch.from_numpy(np.concatenate(earlier)).to(gpu)
        d1 = torch.from_numpy(np.concatenate(chunks)).to(gpu)
        cs = kd.ContentSet(gpu, kh.hash_size(name), 1000)
        ids0 = kh.hash_chunks_device(name, d0.data_ptr(), offs0, lens0, key, gpu, stream=st)
        t0 = cs.insert(ids0, stream=st)
        ids = kh.hash_chunks_device(name, d1.data_ptr(), offs, lens, key, gpu, stream=st)
        keep, first, t1 = cs.claim(ids, stream=st)
        got = packer.pack_chunks_device(d1.data_ptr(), offs, lens, ids, nonces, gpu, keep=keep, stream=st,
                                        id_len=ids.shape[1], id_stride=ids.stride(0))
        st.synchronize()
        # the model's mask from the digests, and the same pack call with it as a host array
        m = dm.Model(1000)
        assert tuple(t0.cpu().tolist()) == m.insert(ids0.cpu().numpy())
        want_keep, want_first, want_t = m.claim(ids.cpu().numpy())
        assert keep.cpu().tolist() == want_keep and kd.first_numpy(first).tolist() == want_first
        assert tuple(t1.cpu().tolist()) == want_t
        assert sum(want_keep) == 100 and want_first.count(dm.KNOWN) == sum(1 for i in order if i in set(known))
        ref = packer.pack_chunks_device(d1.data_ptr(), offs, lens, ids, nonces, gpu, keep=want_keep, stream=st,
                                        id_len=ids.shape[1], id_stride=ids.stride(0))
        st.synchronize()
    (pack_a, ent_a, rows_a, tot_a), (pack_b, ent_b, rows_b, tot_b) = got, ref
    totals = tot_a.cpu().tolist()
    assert totals == tot_b.cpu().tolist() and totals[0] >= 2
    ea, eb = kp.entries_numpy(ent_a), kp.entries_numpy(ent_b)
    assert ea.tolist() == eb.tolist()
    assert [int(s) for s in ea["status"]] == [0 if k else kp.PACK_SKIPPED for k in want_keep]
    ra, rb = kp.packs_numpy(rows_a, totals[0]), kp.packs_numpy(rows_b, totals[0])
    assert ra.tolist() == rb.tolist()
    ha, hb = pack_a.cpu().numpy(), pack_b.cpu().numpy()
    for start, length, _, _ in ra.tolist():
        assert np.array_equal(ha[start:start + length], hb[start:start + length])
    cs.close()
