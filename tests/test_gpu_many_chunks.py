"""GPU: every per-chunk entry point over calls of thousands of tiny and empty chunks (the population
of tests/many_chunks.py, pinned by tests/test_many_chunks.py), and the same calls with the
persistent grids capped to a few workgroups (KCDC_TEST_CHUNK_GRID).

What only such calls reach: the one-workgroup prefix scans with several entries per thread (crypt
units, compress spans, S2 quota and blocks, the 1024-chunk rounds of the ECC scan); the bisection of
a prefix with runs of duplicates (empty and refused chunks, at the start, across the scan seam and
as the call's last entries); a wave's walk across dozens of chunks in the crypt unit kernels; more
blocks than waves in the S2 decode; the ECC decode's KCDC_ENOMEM and the repair call's refusal of
another launch's workspace; kcdc_hash_chunks_device without an order, with unsorted orders and with
a stride above the hash size.

Every chunk of every call is compared with its oracle (OpenSSL's AEADs, oracle/hashes.py,
tests/ecc_model.py, zlib / libzstd / the S2 oracle and Snappy, the S2 model); statuses are compared
as whole vectors; every output buffer is checked outside its slots."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import ecc_model as em
import many_chunks as mc
import test_gpu_compress as tgc
import test_gpu_decompress as tgd
import test_s2_vectors as sv
from kopia_amd import _lib
from kopia_amd import compression as kc
from kopia_amd import ecc as kecc
from kopia_amd import encryption as ke
from oracle import aead, openssl_aead
from oracle.hashes import kopia_hash

pytestmark = pytest.mark.gpu
FILL = 0xAB
MASTER = bytes(range(100, 132))
EBADMSG, EINVAL, ENOMEM, DAMAGED = _lib.KCDC_EBADMSG, _lib.KCDC_EINVAL, _lib.KCDC_ENOMEM, _lib.KCDC_ECC_DAMAGED


@pytest.fixture
def grid(request):
    """At most this many workgroups in the persistent per-chunk kernels (0: the default grid)."""
    L = _lib.lib()
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, request.param) == 0
    yield request.param
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, 0) == 0


def _pop(n):
    """(host bytes, offsets, lengths); the shared host bytes stay read-only, the tables are copies."""
    host, offs, lens = mc.population(n, mc.SEED)
    return host, offs.copy(), lens.copy()


def _upload(a, dev):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _first_wrong(got, want):
    """Indices (a few) of the chunks whose bytes differ: got and want are lists of bytes."""
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


# ------------------------------------------------------------------ seal / open
@lru_cache(maxsize=None)
def _ids_and_nonces(n):
    rng = np.random.default_rng(1000 + n)
    return rng.integers(0, 256, (n, 16), dtype=np.uint8), bytes(rng.integers(0, 256, 12 * n, dtype=np.uint8))


@lru_cache(maxsize=None)
def _sealed_oracle(alg, n):
    """Every chunk of the population sealed by OpenSSL with the call's content IDs and nonces."""
    assert openssl_aead.available()
    ivs, nonces = _ids_and_nonces(n)
    pop = _pop(n)
    s, secret = openssl_aead.Sealer(alg), aead.derive_key(MASTER)
    return [s.kopia_encrypt(secret, ivs[i].tobytes(), nonces[12 * i:12 * i + 12], mc.chunk(pop, i)) for i in range(n)]


@pytest.mark.parametrize("grid", (0, 1, 3), indirect=True)
@pytest.mark.parametrize("n", mc.COUNTS)
@pytest.mark.parametrize("alg", [ke.ChaCha20Poly1305, ke.Aes256Gcm])
def test_seal_and_open(alg, n, grid, gpu):
    """Seal: every chunk equals OpenSSL's, an empty one is its nonce and tag, nothing outside the
    slots (sealed length rounded up to 4) changes.  Open, with four forged tags and one sealed length
    of 27 at sealed offsets of every alignment: the exact status vector, every good plaintext, zeroed
    forged slots, guards intact."""
    import torch
    pop = _pop(n)
    host, offs, lens = pop
    ivs, nonces = _ids_and_nonces(n)
    want = _sealed_oracle(alg, n)
    enc = ke.Encryptor(alg, MASTER)
    d, d_ivs = _upload(host, gpu), _upload(ivs, gpu)
    slot = (lens + 28 + 3) & ~3
    oo, total = mc.slots(slot, align=4)
    out = torch.full((total,), FILL, dtype=torch.uint8, device=gpu)
    st = enc.encrypt_chunks_device(d.data_ptr(), offs, lens, d_ivs, 16, out, oo, gpu, nonces=nonces)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    sealed = out.cpu().numpy()
    got = [sealed[oo[i]:oo[i] + lens[i] + 28].tobytes() for i in range(n)]
    assert not _first_wrong(got, want), [(i, int(lens[i])) for i in _first_wrong(got, want)]
    for i in np.flatnonzero(lens == 0):
        assert len(got[i]) == 28 and got[i][:12] == nonces[12 * i:12 * i + 12], i
    assert mc.outside_intact(sealed, oo, slot, FILL), "seal wrote outside its slots"

    # open: forged tags at the first and the last chunk with bytes, a large one, the one after the seam run
    filled = np.flatnonzero(lens)
    forged = {int(filled[0]), mc.large_indices(lens)[1], int(filled[-1])}
    if n > mc.after_seam():
        forged.add(mc.after_seam())
    short = next(int(i) for i in filled if i >= 10 and int(i) not in forged)
    slens = lens + 28
    soffs, stotal = mc.slots(slens)
    assert len({int(o) % 16 for o in soffs}) == 16
    src = np.zeros(stotal + 32, np.uint8)
    for i in range(n):
        src[soffs[i]:soffs[i] + slens[i]] = np.frombuffer(want[i], np.uint8)
    for i in forged:
        src[soffs[i] + 12 + lens[i]] ^= 0x40  # the first tag byte
    slens = slens.copy()
    slens[short] = 27
    pslot = (np.maximum(slens - 28, 0) + 3) & ~3
    po, ptotal = mc.slots(pslot, align=4)
    d_src = _upload(src, gpu)
    pout = torch.full((ptotal,), FILL, dtype=torch.uint8, device=gpu)
    st2 = enc.decrypt_chunks_device(d_src.data_ptr(), soffs, slens, d_ivs, 16, pout, po, gpu)
    torch.cuda.synchronize()
    want_st = [EBADMSG if i in forged else EINVAL if i == short else 0 for i in range(n)]
    assert st2.cpu().tolist() == want_st
    plain = pout.cpu().numpy()
    for i in range(n):
        got_i = plain[po[i]:po[i] + lens[i]]
        if i in forged:
            assert not got_i.any(), f"forged chunk {i}: unauthenticated bytes left"
        elif i != short:
            assert got_i.tobytes() == mc.chunk(pop, i), (i, int(lens[i]))
    assert mc.outside_intact(plain, po, pslot, FILL), "open wrote outside its slots"


@pytest.mark.parametrize("grid", (1, 2), indirect=True)
@pytest.mark.parametrize("alg", [ke.ChaCha20Poly1305, ke.Aes256Gcm])
def test_seal_full_units_across_chunks(alg, grid, gpu):
    """Chunks whose last 4 KiB unit is full, followed by tiny and empty ones, under one or two
    workgroups: a ChaCha wave leaves such a chunk with its Poly1305 run of full units still unfolded
    (a chunk with a partial last unit folds it there), so the fold at the chunk change is what puts
    the run into the tag.  No chunk of the population is a multiple of 4 KiB long.  Every sealed chunk
    equals OpenSSL's; the device opens them all."""
    import torch
    lens = []
    for k in range(12):
        lens += [4096 * (1 + k % 3), k % 5, 0, 4096, 8192, 17 + k]
    lens = np.array(lens + [4096], np.int64)
    n = len(lens)
    rng = np.random.default_rng(77)
    offs = np.cumsum(rng.integers(1, 4, n) + np.concatenate(([0], lens[:-1])))
    host = np.frombuffer(sv.mixed(int(offs[-1] + lens[-1]) + 16, 78), np.uint8)
    ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    nonces = bytes(rng.integers(0, 256, 12 * n, dtype=np.uint8))
    s, secret = openssl_aead.Sealer(alg), aead.derive_key(MASTER)
    chunks = [host[offs[i]:offs[i] + lens[i]].tobytes() for i in range(n)]
    want = [s.kopia_encrypt(secret, ivs[i].tobytes(), nonces[12 * i:12 * i + 12], chunks[i]) for i in range(n)]
    enc = ke.Encryptor(alg, MASTER)
    d, d_ivs = _upload(host, gpu), _upload(ivs, gpu)
    slot = (lens + 28 + 3) & ~3
    oo, total = mc.slots(slot, align=4)
    out = torch.full((total,), FILL, dtype=torch.uint8, device=gpu)
    st = enc.encrypt_chunks_device(d.data_ptr(), offs, lens, d_ivs, 16, out, oo, gpu, nonces=nonces)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    sealed = out.cpu().numpy()
    got = [sealed[oo[i]:oo[i] + lens[i] + 28].tobytes() for i in range(n)]
    assert not _first_wrong(got, want), [(i, int(lens[i])) for i in _first_wrong(got, want)]
    assert mc.outside_intact(sealed, oo, slot, FILL)
    pslot = (lens + 3) & ~3
    po, ptotal = mc.slots(pslot, align=4)
    pout = torch.full((ptotal,), FILL, dtype=torch.uint8, device=gpu)
    st2 = enc.decrypt_chunks_device(out.data_ptr(), oo, lens + 28, d_ivs, 16, pout, po, gpu)
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == [0] * n
    plain = pout.cpu().numpy()
    assert not _first_wrong([plain[po[i]:po[i] + lens[i]].tobytes() for i in range(n)], chunks)
    assert mc.outside_intact(plain, po, pslot, FILL)


# ------------------------------------------------------------------ compress
def _compress(name, n, dev):
    """The population through one compress call into guarded slots: (out bytes, slot offsets, bounds,
    lengths, header IDs)."""
    import torch
    host, offs, lens = _pop(n)
    bounds = np.array([kc.compress_bound(int(x)) for x in lens], np.int64)
    oo, total = mc.slots(bounds)
    d = _upload(host, dev)
    out = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
    ol, ids = kc.Compressor(name).compress_chunks_device(d.data_ptr(), offs, lens, out, oo, dev)
    torch.cuda.synchronize()
    return out.cpu().numpy(), oo, bounds, ol.cpu().numpy(), ids.cpu().numpy()


@pytest.mark.parametrize("n", mc.COUNTS)
@pytest.mark.parametrize("name", ["deflate-default", "gzip", "s2-default", "zstd"])
def test_compress(name, n, gpu):
    """Every chunk round-trips through its independent decoder within its bound and carries the
    keep-or-drop ID (test_gpu_compress._check); no byte outside the compress_bound-wide slots at odd
    offsets changes; a chunk of 6 bytes or fewer cannot shrink (a stream is at least 6 bytes), so
    its ID is 0."""
    host, offs, lens = _pop(n)
    out, oo, bounds, ol, ids = _compress(name, n, gpu)
    tgc._check(name, host, offs, lens, out, oo, ol, ids)
    assert mc.outside_intact(out, oo, bounds, FILL), "compress wrote outside its slots"
    tiny = np.flatnonzero(lens <= 6)
    assert len(tiny) > 0.05 * n and not ids[tiny].any()
    assert ids[mc.large_indices(lens)].all()  # 70000 mixed bytes shrink


# ------------------------------------------------------------------ S2 decompress
_OWN = {}


def _own_streams(n, dev):
    """The device's own s2-default stream of every chunk, from one compress call (checked against
    the oracle by test_compress)."""
    if n not in _OWN:
        out, oo, _, ol, _ = _compress(sv.NAME, n, dev)
        _OWN[n] = [out[oo[i]:oo[i] + ol[i]].tobytes() for i in range(n)]
    return _OWN[n]


FOREIGN_BLOCK = 64
EXTRA_DESC = 1100  # descriptors per content beyond the minimum: a large chunk in 64-byte blocks has 1094


def _corrupt(blob, truncate):
    """A content the decoder must refuse: cut short (the framing walk fails: no block of it is listed)
    or, where it has a data chunk, with a bit of that chunk's stored CRC flipped (the block is listed
    and decoded, the CRC pass refuses it)."""
    at = 4 + len(sv.IDENT_S2) + 4  # header ID, stream identifier, chunk header: the first data chunk's CRC
    if truncate or len(blob) < at + 4:
        return blob[:-3]
    return blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:]


@pytest.mark.parametrize("grid", (0, 1, 5), indirect=True)
@pytest.mark.parametrize("n", mc.COUNTS)
def test_s2_decompress(n, grid, gpu):
    """Even contents are the device's own streams, odd ones Snappy blocks of 64 bytes in Snappy framing
    (many blocks per content, more blocks than waves under a capped grid); corrupt contents in runs
    (5..9, 1023..1025, the last one) own no block or a refused one.  Good contents decode to their
    chunks, corrupt ones get the model's status and length 0, guards intact (_decompress)."""
    pop = _pop(n)
    lens = pop[2]
    own = _own_streams(n, gpu)
    chunks = [mc.chunk(pop, i) for i in range(n)]
    blobs = [own[i] if i % 2 == 0 else sv.content(sv.snappy_framed(chunks[i], block_size=FOREIGN_BLOCK)) for i in range(n)]
    bad = sorted({5, 6, 7, 8, 9, n - 1} | {i for i in (1023, 1024, 1025) if i < n})
    for k, i in enumerate(bad):
        blobs[i] = _corrupt(blobs[i], truncate=k % 2 == 0)
    caps = [int(x) for x in lens]
    # the documented remedy for contents with more data chunks than 1 + cap / 16 KiB: a larger workspace
    L = _lib.lib()
    wb = int(L.kcdc_decompress_workspace_size(sum(len(b) for b in blobs), sum(caps), n)) + 32 * EXTRA_DESC * n
    assert max(-(-c // FOREIGN_BLOCK) for c in caps) <= EXTRA_DESC
    out, out_offs, got_lens, st = tgd._decompress(sv.NAME, blobs, caps, gpu, work_bytes=wb)
    want_st = [0] * n
    for i in bad:
        want_st[i] = sv.model_decode(blobs[i], sv.NAME, caps[i], 1 + (caps[i] >> 14) + EXTRA_DESC)[0]
        assert want_st[i] == EBADMSG, i
    assert st.tolist() == want_st
    assert got_lens.tolist() == [0 if want_st[i] else caps[i] for i in range(n)]
    got = [out[out_offs[i]:out_offs[i] + got_lens[i]].tobytes() for i in range(n)]
    want = [b"" if want_st[i] else chunks[i] for i in range(n)]
    assert not _first_wrong(got, want), [(i, caps[i]) for i in _first_wrong(got, want)]


# ------------------------------------------------------------------ ECC
CANARY = 0xA5
ECC_OPTS = [(2, 1024), (10, 0)]


@lru_cache(maxsize=None)
def _ecc_model(o, ms, n):
    m = em.ReedSolomonCrcECC(o, ms)
    pop = _pop(n)
    return m, [m.encrypt(mc.chunk(pop, i)) for i in range(n)]


def _algo(o, ms):
    return kecc.CreateAlgorithm(kecc.Options(OverheadPercent=o, MaxShardSize=ms))


def _data_shard_at(m, length, shard, block=0):
    """Offset, in a stored chunk of `length` original bytes, of data shard `shard` of block `block`:
    its CRC, then its payload."""
    s = m.sizes_from_original(length)
    rec = 4 + s.shard_size
    return s.parity * rec * s.blocks + (block * s.data + shard) * rec


def _flip(buf, i):
    buf[i] = 0 if buf[i] >= 128 else 255  # flipByte, ecc_utils_test.go:66-72


@pytest.mark.parametrize("n", mc.COUNTS)
@pytest.mark.parametrize("o,ms", ECC_OPTS)
def test_ecc(o, ms, n, gpu):
    """Encode equals the model for every chunk; the clean decode returns every chunk; with three
    chunks damaged in one data shard each and a large one in one shard more than its parity, the
    decode marks exactly those, the repair restores three and refuses the fourth with a zeroed slot;
    so it does for the first chunk of every 1024-chunk round of the scan, damaged in disjoint shards."""
    import torch
    pop = _pop(n)
    host, offs, lens = pop
    m, want = _ecc_model(o, ms, n)
    a = _algo(o, ms)
    sizes = np.array([a.encoded_size(int(x)) for x in lens], np.int64)
    assert sizes.tolist() == [len(w) for w in want]
    oo, total = mc.slots(sizes)
    d = _upload(host, gpu)
    enc_out = torch.full((total,), CANARY, dtype=torch.uint8, device=gpu)
    st = a.encrypt_chunks_device(d.data_ptr(), offs, lens, enc_out, oo, gpu)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    stored = enc_out.cpu().numpy()
    got = [stored[oo[i]:oo[i] + sizes[i]].tobytes() for i in range(n)]
    assert not _first_wrong(got, want), [(i, int(lens[i])) for i in _first_wrong(got, want)]
    assert mc.outside_intact(stored, oo, sizes, CANARY), "encode wrote outside its slots"

    bounds = np.array([a.decoded_bound(int(s)) for s in sizes], np.int64)
    po, ptotal = mc.slots(bounds)
    chunks = [mc.chunk(pop, i) for i in range(n)]

    def decode(stored_host):
        d_st = _upload(stored_host, gpu)
        out = torch.full((ptotal,), CANARY, dtype=torch.uint8, device=gpu)
        dec = a.decrypt_chunks_device(d_st.data_ptr(), oo, sizes, out, po, gpu)
        torch.cuda.synchronize()
        return out, dec

    def check(out, dec, want_st, zeroed=()):
        assert dec.status.cpu().tolist() == want_st
        plain, out_lens = out.cpu().numpy(), dec.out_lens.cpu().tolist()
        assert out_lens == [0 if want_st[i] else int(lens[i]) for i in range(n)]
        got = [plain[po[i]:po[i] + out_lens[i]].tobytes() for i in range(n)]
        ref = [b"" if want_st[i] else chunks[i] for i in range(n)]
        assert not _first_wrong(got, ref), _first_wrong(got, ref)
        for i in zeroed:
            assert not plain[po[i]:po[i] + bounds[i]].any(), i
        assert mc.outside_intact(plain, po, bounds, CANARY), "decode wrote outside its slots"

    out, dec = decode(stored)
    check(out, dec, [0] * n)
    assert dec.repair().cpu().tolist() == [0] * n  # nothing to repair: a no-op

    damaged = stored.copy()
    last = int(np.flatnonzero(lens)[-1])
    one = [i for i in (3, 1030) if i < n] + [last]
    for k, i in enumerate(one):  # shard 0's payload (the length bytes), shard 1's payload, shard 2's CRC
        _flip(damaged, int(oo[i]) + _data_shard_at(m, int(lens[i]), k % 3) + (0 if k % 3 == 2 else 4))
    # The first chunk of every 1024-chunk round of the decode's scan, each in other data shards (two,
    # one, one: each within the small code's two parity shards).  Their mask blocks are distinct only
    # by the blocks of the rounds before them; were they shared, the shards would add up past repair.
    rounds = [j for j in range(0, n, 1024)]
    assert all(m.sizes_from_original(int(lens[j])).data == em.SMALL_DATA for j in rounds)
    for k, j in enumerate(rounds):
        for shard in ((0, 1), (2,), (3,))[k]:
            _flip(damaged, int(oo[j]) + _data_shard_at(m, int(lens[j]), shard) + 4)
    one += rounds
    lost = mc.large_indices(lens)[1]
    s = m.sizes_from_original(int(lens[lost]))
    for k in range(s.parity + 1):
        _flip(damaged, int(oo[lost]) + _data_shard_at(m, int(lens[lost]), 5 + k, block=s.blocks // 2) + 4 + k)
    with pytest.raises(ValueError):
        m.decrypt(damaged[oo[lost]:oo[lost] + sizes[lost]].tobytes())
    for i in one:
        assert m.decrypt(damaged[oo[i]:oo[i] + sizes[i]].tobytes()) == chunks[i]
    out, dec = decode(damaged)
    check(out, dec, [DAMAGED if i in one or i == lost else 0 for i in range(n)])
    dec.repair()
    check(out, dec, [EBADMSG if i == lost else 0 for i in range(n)], zeroed=[lost])


def _a256(x):
    return (x + 255) & ~255


def test_ecc_workspace_runs_out(gpu):
    """A workspace of the smallest accepted size at options (10, 0): a large chunk takes 9 mask
    blocks, so the blocks run out partway through the call.  Chunks before the cut decode (and
    repair) exactly, chunks past it get KCDC_ENOMEM, length 0 and an untouched slot whether damaged
    or not, and no workspace byte beyond work_bytes is written.  A repair call whose workspace does
    not hold a damaged chunk's blocks is refused and changes nothing.

    The workspace layout (kcdc_ecc.hip, ecc_ws): 8 bytes per chunk, 4 bytes per chunk, then the
    masks, each part 256-byte aligned; 32 bytes per mask block."""
    import torch
    o, ms, n = 10, 0, mc.COUNTS[0]
    pop = _pop(n)
    lens = pop[2]
    m, want = _ecc_model(o, ms, n)
    a = _algo(o, ms)
    L = _lib.lib()
    sizes = np.array([len(w) for w in want], np.int64)
    oo, total = mc.slots(sizes)
    bounds = np.array([a.decoded_bound(int(s)) for s in sizes], np.int64)
    po, ptotal = mc.slots(bounds)
    chunks = [mc.chunk(pop, i) for i in range(n)]
    clean = np.full(total, CANARY, np.uint8)
    for i in range(n):
        clean[oo[i]:oo[i] + sizes[i]] = np.frombuffer(want[i], np.uint8)

    masks_off = _a256(_a256(8 * n) + 4 * n)
    full = int(L.kcdc_ecc_workspace_size(int(sizes.sum()), n))
    small = int(L.kcdc_ecc_workspace_size(0, n))
    assert full == _a256(masks_off + 32 * (int(sizes.sum()) // 650 + n)) and small == _a256(masks_off + 32 * n)
    mask_blocks = (small - masks_off) // 32
    blocks = np.array([m.sizes_from_stored(int(s)).blocks for s in sizes], np.int64)
    first = np.cumsum(blocks) - blocks
    refused = first + blocks > mask_blocks
    cut = int(np.flatnonzero(refused)[0])
    assert refused[cut:].all() and mc.large_indices(lens)[-1] < cut < n - 8 and blocks.sum() <= (full - masks_off) // 32

    d_meta = [_upload(x, gpu) for x in (oo, sizes, po)]
    d_lens = torch.zeros(n, dtype=torch.int64, device=gpu)
    d_status = torch.zeros(n, dtype=torch.int32, device=gpu)

    def call(fn, d_stored, out, work, wb):
        torch.cuda.synchronize()
        rc = fn(*a._p(), C.c_void_p(d_stored.data_ptr()), d_meta[0].data_ptr(), d_meta[1].data_ptr(), n,
                out.data_ptr(), d_meta[2].data_ptr(), d_lens.data_ptr(), d_status.data_ptr(), work.data_ptr(), wb, None)
        torch.cuda.synchronize()
        return rc

    def check(out, want_st, untouched=()):
        assert d_status.cpu().tolist() == want_st
        plain, out_lens = out.cpu().numpy(), d_lens.cpu().tolist()
        assert out_lens == [0 if want_st[i] else int(lens[i]) for i in range(n)]
        got = [plain[po[i]:po[i] + out_lens[i]].tobytes() for i in range(n)]
        ref = [b"" if want_st[i] else chunks[i] for i in range(n)]
        assert not _first_wrong(got, ref), _first_wrong(got, ref)
        for i in untouched:
            assert (plain[po[i]:po[i] + bounds[i]] == CANARY).all(), i
        assert mc.outside_intact(plain, po, bounds, CANARY)

    def run_small(stored_host, want_st, after_repair):
        work = torch.full((full,), 0xC3, dtype=torch.uint8, device=gpu)
        out = torch.full((ptotal,), CANARY, dtype=torch.uint8, device=gpu)
        d_stored = _upload(stored_host, gpu)
        assert call(L.kcdc_ecc_decode_chunks_device, d_stored, out, work, small) == 0
        check(out, want_st, untouched=range(cut, n))
        assert call(L.kcdc_ecc_repair_chunks_device, d_stored, out, work, small) == 0
        check(out, after_repair, untouched=range(cut, n))
        assert (work.cpu().numpy()[small:] == 0xC3).all(), "the workspace was written beyond work_bytes"

    no_room = [ENOMEM if i >= cut else 0 for i in range(n)]
    run_small(clean, no_room, no_room)
    damaged = clean.copy()
    hit = [5, cut + 2]  # one with room, one without: the second keeps KCDC_ENOMEM and the repair leaves it alone
    for i in hit:
        _flip(damaged, int(oo[i]) + _data_shard_at(m, int(lens[i]), 1) + 4)
    run_small(damaged, [DAMAGED if i == 5 else no_room[i] for i in range(n)], no_room)

    # a repair call with a workspace that does not hold the damaged chunk's mask blocks
    far = int(np.flatnonzero(lens)[-1])
    assert far >= cut
    damaged = clean.copy()
    _flip(damaged, int(oo[far]) + _data_shard_at(m, int(lens[far]), 0) + 4)
    work = torch.full((full,), 0xC3, dtype=torch.uint8, device=gpu)
    out = torch.full((ptotal,), CANARY, dtype=torch.uint8, device=gpu)
    d_stored = _upload(damaged, gpu)
    assert call(L.kcdc_ecc_decode_chunks_device, d_stored, out, work, full) == 0
    marked = [DAMAGED if i == far else 0 for i in range(n)]
    check(out, marked)
    assert call(L.kcdc_ecc_repair_chunks_device, d_stored, out, work, small) == EINVAL
    assert "not the workspace" in _lib.last_error()
    check(out, marked)
    assert call(L.kcdc_ecc_repair_chunks_device, d_stored, out, work, full) == 0
    check(out, [0] * n)


# ------------------------------------------------------------------ hash arguments
HASHES = [("BLAKE2B-256-128", 1), ("BLAKE2B-256-128", 4), ("BLAKE2S-128", 0), ("HMAC-SHA256", 0),
          ("HMAC-SHA3-224", 0), ("BLAKE3-256-128", 0)]
HASH_KEY = bytes(range(7, 39))


@lru_cache(maxsize=None)
def _digests(name, n):
    pop = _pop(n)
    return [kopia_hash(name, HASH_KEY, mc.chunk(pop, i)) for i in range(n)]


@pytest.mark.parametrize("name,lanes", HASHES, ids=[f"{h}-lanes{k}" for h, k in HASHES])
def test_hash_order_and_stride(name, lanes, gpu):
    """kcdc_hash_chunks_device through the C ABI: no order, the reversed order and a random
    permutation, each at the smallest stride and at 64: digest i is chunk i's at d_out + i * stride
    whatever the order, and the bytes between digests keep their fill."""
    import torch
    n = mc.COUNTS[0]
    host, offs, lens = _pop(n)
    want = _digests(name, n)
    size = len(want[0])
    L = _lib.lib()
    d, d_offs, d_lens = _upload(host, gpu), _upload(offs, gpu), _upload(lens, gpu)
    orders = {"none": None, "reversed": np.arange(n - 1, -1, -1, dtype=np.int32),
              "random": np.random.default_rng(9).permutation(n).astype(np.int32)}
    assert L.kcdc_test_set(_lib.TEST_HASH_LANES, lanes) == 0
    try:
        for label, order in orders.items():
            d_order = None if order is None else _upload(order, gpu)
            for stride in sorted({(size + 3) & ~3, 64}):
                out = torch.full((n * stride + 16,), FILL, dtype=torch.uint8, device=gpu)
                rc = L.kcdc_hash_chunks_device(name.encode(), C.c_void_p(d.data_ptr()), d_offs.data_ptr(),
                                               d_lens.data_ptr(), None if d_order is None else d_order.data_ptr(), n,
                                               HASH_KEY, len(HASH_KEY), out.data_ptr(), stride, None)
                assert rc == 0, _lib.last_error()
                torch.cuda.synchronize()
                buf = out.cpu().numpy()
                got = [buf[i * stride:i * stride + size].tobytes() for i in range(n)]
                assert not _first_wrong(got, want), (label, stride, _first_wrong(got, want))
                assert mc.outside_intact(buf, np.arange(n) * stride, [size] * n, FILL), (label, stride)
    finally:
        assert L.kcdc_test_set(_lib.TEST_HASH_LANES, 0) == 0
