"""GPU: kcdc_pack_chunks_device (compress, seal, ECC and place in one call) against the literal
loop of addToPackUnlocked (tests/pack_model.py), the AEAD oracles (oracle/aead.py, oracle/aesgcm.py),
tests/ecc_model.py and the library's own stage entry points.

Every call runs with d_pack pre-filled with a canary, a guard after pack_cap, and guard bytes on
both sides of d_work; after it everything outside the contents' bytes must still hold the canary:
leads, gaps between packs, the tail, and the whole buffer on a refusal."""
from functools import lru_cache

import numpy as np
import pytest

import ecc_model as em
import far_layout as fl
import many_chunks as mc
import pack_cases as pc
import pack_model as pm
from kopia_amd import _lib
from kopia_amd import compression as kc
from kopia_amd import ecc as kecc
from kopia_amd import encryption as ke
from kopia_amd import packing as kp
from oracle import aead, aesgcm

pytestmark = pytest.mark.gpu
GCM, CHACHA = "AES256-GCM-HMAC-SHA256", "CHACHA20-POLY1305-HMAC-SHA256"
ORACLE = {GCM: aesgcm, CHACHA: aead}
MASTER = bytes(range(100, 132))
SECRET = aead.derive_key(MASTER)
ECC_NAME = "REED-SOLOMON-CRC32"
CANARY, GUARD = 0xC7, 512


@lru_cache(maxsize=None)
def ids_and_nonces(n):
    rng = np.random.default_rng(4242 + n)
    return rng.integers(0, 256, (n, 16), dtype=np.uint8), rng.integers(0, 256, (n, 12), dtype=np.uint8)


def upload(a, dev):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


class Run:
    """One call's outputs on the host."""


def run_pack(dev, d_data, offs, lens, alg, vec, comp=None, stream=None, sync=True, data_ptr=None, pack_tensor=None):
    """The call described by `vec` (a pack_cases.Vec: parameters, mask, caps) over chunks
    [offs[i], +lens[i]) of d_data.  Caps the Vec leaves open come from kcdc_pack_bounds with the true
    total."""
    import torch
    n = len(lens)
    ids, nonces = ids_and_nonces(n)
    total = vec.true_total() if vec.max_total is None else vec.max_total
    packer = kp.Packer(alg, SECRET, vec.max_pack_size, compression=comp, ecc=ECC_NAME if vec.ecc else None,
                       ecc_overhead_percent=vec.ecc[0] if vec.ecc else 0, ecc_max_shard_size=vec.ecc[1] if vec.ecc else 0,
                       pack_lead=vec.lead, open_fill=vec.open_fill, max_total_bytes=total)
    pb, mp, wb = packer.bounds(n)
    r = Run()
    r.pack_cap = pb if vec.pack_cap is None else vec.pack_cap
    r.packs_cap = mp if vec.packs_cap is None else vec.packs_cap
    stream = stream or torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        r.d_pack = pack_tensor if pack_tensor is not None else torch.full((r.pack_cap + GUARD,), CANARY,
                                                                          dtype=torch.uint8, device=dev)
        r.d_entries = torch.full((max(n, 1), 6), -1, dtype=torch.int32, device=dev)
        r.d_packs = torch.full((r.packs_cap + 1, 24), CANARY, dtype=torch.uint8, device=dev)
        r.d_totals = torch.full((2,), -1, dtype=torch.int64, device=dev)
        r.d_work = torch.full((wb + 256 + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
        r.keep = (upload(np.asarray(offs, np.int64), dev), upload(np.asarray(lens, np.int64), dev),
                  None if vec.keep is None else upload(np.asarray(vec.keep, np.uint8), dev), upload(ids, dev),
                  upload(nonces, dev), d_data, packer)
    r.work_at = (r.d_work.data_ptr() + GUARD + 255) // 256 * 256 - r.d_work.data_ptr()
    r.wb = wb
    r.rc = packer.pack_chunks_raw(d_data.data_ptr() if data_ptr is None else data_ptr, r.keep[0], r.keep[1], r.keep[2],
                                  n, r.keep[3], 16, 16, r.keep[4], r.d_pack, r.pack_cap, r.d_entries, r.d_packs,
                                  r.packs_cap, r.d_totals, r.d_work.data_ptr() + r.work_at, wb, stream)
    r.n, r.stream = n, stream
    if sync:
        collect(r)
    return r


def collect(r):
    assert r.rc == 0, _lib.last_error()
    r.stream.synchronize()
    r.totals = tuple(int(x) for x in r.d_totals.cpu().numpy())
    r.entries = [tuple(int(x) for x in e) for e in kp.entries_numpy(r.d_entries)[:r.n]]
    r.packs = [tuple(int(x) for x in p) for p in kp.packs_numpy(r.d_packs, min(r.totals[0], r.packs_cap))]
    r.places = [(r.packs[e[0]][0] + e[1], e[2]) for e in r.entries if e[5] == 0]
    work = r.d_work.cpu().numpy()
    assert (work[:r.work_at] == CANARY).all() and (work[r.work_at + r.wb:] == CANARY).all(), "workspace guards"
    # rows past the packs are untouched (a refused call may leave rows it wrote before it refused), and
    # the row after packs_cap always is
    refused = r.n > 0 and all(e[5] in (pm.ENOMEM, pm.EOVERFLOW) for e in r.entries)
    rows = r.d_packs.cpu().numpy()
    assert (rows[r.packs_cap if refused else r.totals[0]:] == CANARY).all(), "rows past the packs"


def pack_host(r):
    return r.d_pack.cpu().numpy()


def check_model(r, want: pm.Result, buf=None):
    """Entries, rows and totals equal the model's; nothing outside the contents was written."""
    assert r.entries == want.entries
    assert r.packs == want.packs
    assert r.totals == want.totals
    buf = pack_host(r) if buf is None else buf
    assert mc.outside_intact(buf, [p[0] for p in r.places], [p[1] for p in r.places], CANARY)
    return buf


def seal(alg, i, n, plain: bytes) -> bytes:
    ids, nonces = ids_and_nonces(n)
    return ORACLE[alg].kopia_encrypt(SECRET, ids[i].tobytes(), nonces[i].tobytes(), plain)


def check_bytes(r, buf, want_contents):
    """want_contents[i]: the stored bytes of packed chunk i (None for one that took no room)."""
    at = iter(r.places)
    wrong = []
    for i, w in enumerate(want_contents):
        if r.entries[i][5] != 0:
            continue
        o, ln = next(at)
        if ln != len(w) or buf[o:o + ln].tobytes() != w:
            wrong.append(i)
    assert not wrong, wrong[:8]


def read_back(dev, r, alg, ecc=None, comp=None, sel=None):
    """The read path over the pack, addressed by the entries alone: ECC decode, open, decompress
    by header ID.  Returns the plaintexts of the packed chunks (in chunk order) as bytes."""
    import torch
    idx = [i for i, e in enumerate(r.entries) if e[5] == 0 and (sel is None or i in sel)]
    if not idx:
        return idx, []
    ent = [r.entries[i] for i in idx]
    offs = np.array([r.packs[e[0]][0] + e[1] for e in ent], np.int64)
    lens = np.array([e[2] for e in ent], np.int64)
    ptr = r.d_pack.data_ptr()
    if ecc:
        a = kecc.CreateAlgorithm(kecc.Options(OverheadPercent=ecc[0], MaxShardSize=ecc[1]))
        so, total = a.plain_layout(lens)
        d_sealed = torch.zeros(total, dtype=torch.uint8, device=dev)
        dec = a.decrypt_chunks_device(ptr, offs, lens, d_sealed, so, dev)
        assert (dec.status.cpu().numpy() == 0).all()
        offs, lens, ptr = so, dec.out_lens.cpu().numpy().astype(np.int64), d_sealed.data_ptr()
    enc = ke.Encryptor(alg, MASTER)
    po, total = ke.plain_layout(lens, alg)
    d_plain = torch.zeros(total + 4, dtype=torch.uint8, device=dev)
    ids, _ = ids_and_nonces(r.n)
    st = enc.decrypt_chunks_device(ptr, offs, lens, upload(ids[idx], dev), 16, d_plain, po, dev)
    assert (st.cpu().numpy() == 0).all()
    plens = lens - 28
    out = [None] * len(idx)
    comp_at = [k for k, e in enumerate(ent) if e[4] != 0]
    if comp_at:
        c = kc.Compressor(comp)
        assert all(ent[k][4] == c.header_id for k in comp_at)
        caps = np.array([ent[k][3] for k in comp_at], np.int64)
        oo = np.concatenate(([0], np.cumsum((caps + 16 + 3) & ~3)[:-1])).astype(np.int64)
        d_out = torch.zeros(int(((caps + 16 + 3) & ~3).sum()) + 16, dtype=torch.uint8, device=dev)
        decode = (c.decompress_chunks_device if comp in kc.DecompressibleAlgorithms() else
                  c.inflate_chunks_device if comp in kc.InflatableAlgorithms() else c.zstd_decode_chunks_device)
        ol, st = decode(d_plain.data_ptr(), po[comp_at], plens[comp_at], d_out, oo, caps, dev)
        assert (st.cpu().numpy() == 0).all()
        ol, host = ol.cpu().numpy(), d_out.cpu().numpy()
        for j, k in enumerate(comp_at):
            out[k] = host[oo[j]:oo[j] + ol[j]].tobytes()
    host = d_plain.cpu().numpy()
    for k in range(len(idx)):
        if out[k] is None:
            out[k] = host[po[k]:po[k] + plens[k]].tobytes()
    return idx, out


def originals(host, offs, lens, idx):
    return [host[offs[i]:offs[i] + lens[i]].tobytes() for i in idx]


# ------------------------------------------------------------------ 1. byte-exact, no compressor, no ECC
@lru_cache(maxsize=None)
def exact_case():
    host, offs = pc.sources(pc.EXACT_LENS)
    return host, offs, np.array(pc.EXACT_LENS, np.int64)


@lru_cache(maxsize=None)
def exact_seals(alg):
    host, offs, lens = exact_case()
    return [seal(alg, i, len(lens), host[offs[i]:offs[i] + lens[i]].tobytes()) for i in range(len(lens))]


@pytest.mark.parametrize("mps", pc.EXACT_PACK_SIZES)
@pytest.mark.parametrize("alg", [GCM, CHACHA])
def test_byte_exact(gpu, alg, mps):
    host, offs, lens = exact_case()
    vec = pc.Vec(lens.tolist(), mps, lead=37)
    r = run_pack(gpu, upload(host, gpu), offs, lens, alg, vec)
    buf = check_model(r, vec.model())
    check_bytes(r, buf, exact_seals(alg))


# ------------------------------------------------------------------ 2. keep-or-drop
def comp_case():
    lens = [0, 1, 3, 7, 40, 41, 100, 101, 700, 701, 5000, 5001, 33000, 33001, 70001, 70002]
    host, offs = pc.sources(lens, seed=11)  # even chunks text-like, odd ones random
    return host, offs, np.array(lens, np.int64)


@pytest.mark.parametrize("comp", ["deflate-default", "gzip", "s2-default", "zstd"])
def test_keep_or_drop(gpu, comp):
    import torch
    host, offs, lens = comp_case()
    n = len(lens)
    d = upload(host, gpu)
    c = kc.Compressor(comp)
    co, total = kc.compressed_layout(lens)
    d_comp = torch.zeros(total, dtype=torch.uint8, device=gpu)
    out_lens, hids = c.compress_chunks_device(d.data_ptr(), offs, lens, d_comp, co, gpu)
    out_lens, hids, comp_host = out_lens.cpu().numpy(), hids.cpu().numpy(), d_comp.cpu().numpy()
    kept = [bool(out_lens[i] < lens[i]) for i in range(n)]
    assert [int(h) for h in hids] == [c.header_id if k else 0 for k in kept]
    assert any(kept) and not all(kept), "the input must give a content of each kind"

    vec = pc.Vec(lens.tolist(), 1 << 16, lead=37, comp_lens=[int(x) for x in out_lens], header_id=c.header_id)
    r = run_pack(gpu, d, offs, lens, CHACHA, vec, comp=comp)
    buf = check_model(r, vec.model())
    for i, e in enumerate(r.entries):
        assert e[4] == int(hids[i]) and e[2] - 28 == (int(out_lens[i]) if kept[i] else int(lens[i])), i
    plains = [comp_host[co[i]:co[i] + out_lens[i]].tobytes() if kept[i] else host[offs[i]:offs[i] + lens[i]].tobytes()
              for i in range(n)]
    check_bytes(r, buf, [seal(CHACHA, i, n, p) for i, p in enumerate(plains)])
    idx, got = read_back(gpu, r, CHACHA, comp=comp)
    assert got == originals(host, offs, lens, idx)


# ------------------------------------------------------------------ 3. ECC
@pytest.mark.parametrize("alg", [GCM, CHACHA])
@pytest.mark.parametrize("opt", pc.ECC_OPTS)
def test_ecc(gpu, opt, alg):
    lens = pc.ecc_lengths(opt)
    m = em.ReedSolomonCrcECC(*opt)
    sealed = [n + 28 + 4 for n in lens]
    assert min(sealed) <= m.threshold_parity_input < m.threshold_blocks_input < max(sealed)
    assert m.sizes_from_original(lens[-1] + 28).blocks > 1
    host, offs = pc.sources(lens, seed=opt[0])
    lens = np.array(lens, np.int64)
    vec = pc.Vec(lens.tolist(), 1 << 16, lead=37, ecc=opt)
    r = run_pack(gpu, upload(host, gpu), offs, lens, alg, vec)
    buf = check_model(r, vec.model())
    n = len(lens)
    check_bytes(r, buf, [m.encrypt(seal(alg, i, n, host[offs[i]:offs[i] + lens[i]].tobytes())) for i in range(n)])
    idx, got = read_back(gpu, r, alg, ecc=opt)
    assert got == originals(host, offs, lens, idx)


# ------------------------------------------------------------------ 4. placement seams, 5. masks
SEAMS = {v.tag: v for v in pc.seam_vectors() + pc.mask_vectors()}


@pytest.mark.parametrize("tag", sorted(SEAMS))
def test_placement(gpu, tag):
    vec = SEAMS[tag]
    lens = np.array(vec.lengths, np.int64)
    host, offs = pc.sources(vec.lengths, seed=3)
    r = run_pack(gpu, upload(host, gpu), offs, lens, CHACHA, vec)
    want = vec.model()
    check_model(r, want)
    if tag in ("empty", "all-skipped"):
        assert r.totals == (0, 0)
    idx, got = read_back(gpu, r, CHACHA)
    assert got == originals(host, offs, lens, idx)
    # a few contents against the oracle, first and last of every pack among them
    ends = {p[2] for p in want.packs} | {i for i in idx if i + 1 == len(lens) or want.entries[i + 1][0] != want.entries[i][0]}
    buf = pack_host(r)
    for i in sorted(ends & set(idx))[:12]:
        o = r.packs[r.entries[i][0]][0] + r.entries[i][1]
        w = seal(CHACHA, i, len(lens), host[offs[i]:offs[i] + lens[i]].tobytes())
        assert buf[o:o + len(w)].tobytes() == w, i


@lru_cache(maxsize=None)
def many_case():
    n = 66000
    rng = np.random.default_rng(66)
    lens = rng.integers(1, 41, n).astype(np.int64)
    gaps = rng.integers(0, 3, n)
    offs = np.cumsum(gaps + np.concatenate(([0], lens[:-1]))) + 1
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 16, dtype=np.uint8)
    keep = (rng.random(n) < 0.9).astype(np.uint8)
    vec = pc.Vec(lens.tolist(), 4096, lead=37, open_fill=1000, keep=keep.tolist())
    return host, offs, lens, vec, vec.model()


@pytest.mark.parametrize("cap", [0, 3])
def test_many_chunks(gpu, cap):
    """66,000 chunks of 1..40 bytes: past 2^16, several entries per scan thread, hundreds of packs;
    again with the gather's persistent grid capped."""
    host, offs, lens, vec, want = many_case()
    assert want.totals[0] > 64
    L = _lib.lib()
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, cap) == 0
    try:
        r = run_pack(gpu, upload(host, gpu), offs, lens, CHACHA, vec)
    finally:
        assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, 0) == 0
    check_model(r, want)
    idx, got = read_back(gpu, r, CHACHA)
    assert got == originals(host, offs, lens, idx)
    buf = pack_host(r)
    for i in idx[:3] + idx[-3:] + [j for j in idx if 65530 <= j <= 65540]:
        o = r.packs[r.entries[i][0]][0] + r.entries[i][1]
        w = seal(CHACHA, i, len(lens), host[offs[i]:offs[i] + lens[i]].tobytes())
        assert buf[o:o + len(w)].tobytes() == w, i


def test_no_chunks(gpu):
    import torch
    packer = kp.Packer(CHACHA, SECRET, 4096)
    totals = torch.full((2,), -1, dtype=torch.int64, device=gpu)
    rc = packer.pack_chunks_raw(None, None, None, None, 0, None, 16, 16, None, None, 0, None, None, 0, totals, None, 0,
                                torch.cuda.current_stream(gpu))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("tag", ["enomem", "total-exact", "pack-cap-short", "pack-cap-exact", "packs-cap-short",
                                 "packs-cap-exact"])
def test_refusals(gpu, tag):
    vec = {v.tag: v for v in pc.refusal_vectors()}[tag]
    lens = np.array(vec.lengths, np.int64)
    host, offs = pc.sources(vec.lengths, seed=5)
    r = run_pack(gpu, upload(host, gpu), offs, lens, GCM, vec)
    want = vec.model()
    buf = check_model(r, want)
    if "short" in tag or tag == "enomem":
        code = pm.ENOMEM if tag == "enomem" else pm.EOVERFLOW
        assert r.totals == (0, 0) and {e[5] for e in r.entries} == {code}
        assert (buf == CANARY).all()
    else:
        idx, got = read_back(gpu, r, GCM)
        assert len(idx) == len(lens) and got == originals(host, offs, lens, idx)


def test_chunk_at_the_seal_limit(gpu):
    """A chunk one byte past the seal's limit among good ones: it alone gets KCDC_EFBIG (its bytes
    are never read: the table names a length, the buffer is small) and the others are packed as if
    it were skipped."""
    lens = np.array([50, pm.SEAL_MAX_LEN + 1, 60, 70], np.int64)
    host, offs = pc.sources([50, 0, 60, 70], seed=9)
    vec = pc.Vec(lens.tolist(), 128)
    r = run_pack(gpu, upload(host, gpu), offs, lens, CHACHA, vec)
    check_model(r, vec.model())
    assert [e[5] for e in r.entries] == [0, _lib.KCDC_EFBIG, 0, 0]
    skipped = pc.Vec(lens.tolist(), 128, keep=[1, 0, 1, 1]).model()
    assert [e[:3] for e in r.entries if e[5] == 0] == [e[:3] for e in skipped.entries if e[5] == 0]
    idx, got = read_back(gpu, r, CHACHA)
    assert got == originals(host, offs, lens, idx)


# ------------------------------------------------------------------ 8. two calls on two streams
def test_two_streams(gpu):
    import torch
    host, offs, lens = exact_case()
    d = upload(host, gpu)
    torch.cuda.synchronize()
    vecs = [pc.Vec(lens.tolist(), 4096, lead=37), pc.Vec(lens.tolist(), 1 << 20, lead=0, open_fill=5)]
    algs = [CHACHA, GCM]
    runs = [run_pack(gpu, d, offs, lens, a, v, stream=torch.cuda.Stream(gpu), sync=False) for a, v in zip(algs, vecs)]
    for r, a, v in zip(runs, algs, vecs):
        collect(r)
        check_bytes(r, check_model(r, v.model()), exact_seals(a))


# ------------------------------------------------------------------ 9. far lines
MIN_FREE = 14 << 30


def need_memory(dev):
    import torch
    free, _ = torch.cuda.mem_get_info(dev)
    if free < MIN_FREE:
        pytest.skip(f"{free >> 20} MiB of device memory free, the far-line buffers need {MIN_FREE >> 20}")


@pytest.mark.parametrize("alg,comp", [(CHACHA, None), (GCM, "deflate-default")])
def test_far_sources(gpu, alg, comp):
    """Source chunks on the 2^31, 2^32 and address-carry lines of a 4 GiB buffer (tests/far_layout.py):
    the pack equals the pack of the near twin (every offset moved below 32 MiB) byte for byte, and
    reads back to the chunks."""
    import torch
    need_memory(gpu)
    src = torch.empty(fl.SIZE, dtype=torch.uint8, device=gpu)
    lay = fl.layout(src.data_ptr())
    rng = np.random.default_rng(31)
    words = np.frombuffer(b"content-defined chunks of a tree of small files, packed ", np.uint8)
    host = []
    for k in range(len(lay.xs)):  # half of every window compressible
        h = rng.integers(0, 256, fl.WINDOW, dtype=np.uint8)
        h[:fl.HALF] = np.resize(words, fl.HALF)
        host.append(h)
    vec = pc.Vec(lay.lens.tolist(), 1 << 20, lead=37)
    runs = []
    for near in (True, False):  # the twin first: its windows may overlap a far window
        for (ws, wl), h in zip(lay.windows(near), host):
            src[ws:ws + wl] = upload(h, gpu)
        offs = lay.near(lay.offs) if near else lay.offs
        r = run_pack(gpu, src, offs, lay.lens, alg, vec, comp=comp)
        r.buf = pack_host(r)
        runs.append(r)
    twin, far = runs
    assert far.entries == twin.entries and far.packs == twin.packs and far.totals == twin.totals
    assert np.array_equal(far.buf, twin.buf)
    assert all(e[5] == 0 for e in far.entries) and far.totals[0] >= 2
    assert mc.outside_intact(far.buf, [p[0] for p in far.places], [p[1] for p in far.places], CANARY)
    if comp is None:
        check_model(far, vec.model(), far.buf)
    else:
        assert any(e[4] for e in far.entries) and not all(e[4] for e in far.entries)
    idx, got = read_back(gpu, far, alg, comp=comp)
    wins = lay.windows()
    assert got == [fl.take(host, wins, int(lay.offs[i]), int(lay.lens[i])) for i in idx]


def test_pack_past_4g(gpu):
    """Packs that pass 4 GiB inside d_pack: four contents just under the seal's limit read from one
    shared source region, small ones between and after them.  The small contents beyond the line
    against the oracle, the large ones by a device decrypt."""
    import torch
    need_memory(gpu)
    big = pm.SEAL_MAX_LEN
    small = [0, 1, 36, 100, 4097]
    lens = np.array(([big] + small[:2]) * 4 + small, np.int64)
    n = len(lens)
    rng = np.random.default_rng(77)
    src = torch.from_numpy(rng.integers(0, 256, 1 << 20, dtype=np.uint8)).to(gpu).repeat(1 << 10)
    offs = np.array([(3 * i) % 50 if lens[i] < big else 0 for i in range(n)], np.int64)
    src[:64] = upload(rng.integers(0, 256, 64, dtype=np.uint8), gpu)
    head = src[:8192].cpu().numpy()
    vec = pc.Vec(lens.tolist(), 1 << 30, lead=37)
    want = vec.model()
    assert want.totals[1] > (1 << 32) + 4000
    r = run_pack(gpu, src, offs, lens, CHACHA, vec)
    assert r.entries == want.entries and r.packs == want.packs and r.totals == want.totals
    # everything outside the contents, on the device
    pos, clean = 0, True
    for o, ln in sorted(r.places) + [(r.d_pack.numel(), 0)]:
        clean = clean and bool((r.d_pack[pos:o] == CANARY).all())
        pos = o + ln
    assert clean
    beyond = [i for i in range(n) if lens[i] < big and r.packs[r.entries[i][0]][0] + r.entries[i][1] >= 1 << 32]
    assert len(beyond) >= 3
    for i in range(n):
        if lens[i] < big:
            o = r.packs[r.entries[i][0]][0] + r.entries[i][1]
            w = seal(CHACHA, i, n, head[offs[i]:offs[i] + lens[i]].tobytes())
            assert r.d_pack[o:o + len(w)].cpu().numpy().tobytes() == w, i
    enc = ke.Encryptor(CHACHA, MASTER)
    ids, _ = ids_and_nonces(n)
    tmp = torch.empty(big + 64, dtype=torch.uint8, device=gpu)
    for i in range(n):
        if lens[i] == big:
            o = r.packs[r.entries[i][0]][0] + r.entries[i][1]
            st = enc.decrypt_chunks_device(r.d_pack.data_ptr(), [o], [big + 28], upload(ids[i:i + 1], gpu), 16, tmp, [0], gpu)
            assert st.cpu().tolist() == [0], i
            assert torch.equal(tmp[:big], src[:big]), i


def test_pack_pointer_below_4g_line(gpu):
    """d_pack itself sits just below a multiple of 2^32 in absolute address: the packs cross the line
    where the address carries into the high word."""
    import torch
    need_memory(gpu)
    area = torch.empty((1 << 32) + (8 << 20), dtype=torch.uint8, device=gpu)
    line = -area.data_ptr() % (1 << 32)  # the first byte of the area at a multiple of 2^32
    if line < 1000:
        line += 1 << 32
    host, offs, lens = exact_case()
    vec = pc.Vec(lens.tolist(), 4096, lead=37)
    want = vec.model()
    at = line - 1000
    assert (area.data_ptr() + at) >> 32 != (area.data_ptr() + at + want.totals[1]) >> 32
    view = area[at:at + (8 << 20) - 4096]
    view.fill_(CANARY)
    r = run_pack(gpu, upload(host, gpu), offs, lens, CHACHA, vec, pack_tensor=view)
    check_bytes(r, check_model(r, want), exact_seals(CHACHA))
