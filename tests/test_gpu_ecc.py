"""GPU: REED-SOLOMON-CRC32 error correction of many chunks (kcdc_ecc_encode / _decode /
_repair_chunks_device) against the numpy model of repo/ecc (tests/ecc_model.py, pinned by
tests/test_ecc_model.py): byte-exact encodes at every geometry edge, clean decodes in both
directions, the reference's own damage tests (ecc_rs_crc_test.go:48-104) with its flip positions,
further erasure shapes, the in-band length and stored-length contract, and seal-then-ECC composed
as encryptorWrapper does."""
from functools import lru_cache

import numpy as np
import pytest

import ecc_model as em
from conftest import golden
from kopia_amd import _lib
from kopia_amd import ecc as kecc

pytestmark = pytest.mark.gpu
OPTS = [(2, 1024), (10, 1024), (1, 0), (10, 0), (100, 0)]
CANARY = 0xA5
GAP = 13  # odd, so slots and sources land on every alignment


def pattern(n: int) -> np.ndarray:
    return (np.arange(n, dtype=np.int64) % 255 + 1).astype(np.uint8)  # testPutAndGet


def algo(o, ms):
    return kecc.CreateAlgorithm(kecc.Options(OverheadPercent=o, MaxShardSize=ms))


def edge_lengths(m):
    t = m.threshold_parity_input - 4
    block = m.data * m.max_shard_size
    b = block - 4
    return [0, 1, 2, 3, 8, 9, 14, 15, 20, 21, 26, t, t + 1, 10240, b, b + 1, 2 * block - 4, 2 * block - 3, 1 << 20]


@lru_cache(maxsize=None)
def case(o, ms):
    """The chunks of one option set and the model's encoding of each, computed once."""
    m = em.ReedSolomonCrcECC(o, ms)
    chunks = [pattern(n) for n in edge_lengths(m)]
    chunks.append(np.random.default_rng(o * 7 + ms).integers(0, 256, 70001, dtype=np.uint8))
    return m, chunks, [m.encrypt(c.tobytes()) for c in chunks]


def pack(blobs):
    """Blobs into one canary-filled host buffer at odd offsets: (buffer, offsets, lengths)."""
    lens = np.array([len(b) for b in blobs], np.int64)
    offs = np.zeros(len(blobs), np.int64)
    pos = GAP
    for i, n in enumerate(lens):
        offs[i] = pos
        pos += int(n) + GAP + (i & 1)
    buf = np.full(pos + GAP, CANARY, np.uint8)
    for b, o in zip(blobs, offs):
        buf[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return buf, offs, lens


def slots(sizes):
    sizes = np.asarray(sizes, np.int64)
    offs = np.zeros(len(sizes), np.int64)
    pos = GAP
    for i, n in enumerate(sizes):
        offs[i] = pos
        pos += int(n) + GAP + (i & 1)
    return offs, pos + GAP


def canaries_intact(buf, offs, sizes):
    mask = np.ones(len(buf), bool)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = False
    return bool((buf[mask] == CANARY).all())


def encode(a, chunks, dev, stream=None):
    import torch
    host, offs, lens = pack([c.tobytes() for c in chunks])
    sizes = [a.encoded_size(n) for n in lens]
    oo, total = slots(sizes)
    d = torch.from_numpy(host).to(dev)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    st = a.encrypt_chunks_device(d.data_ptr(), offs, lens, out, oo, dev, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), oo, sizes, st.cpu().numpy()


def decode(a, stored, dev, repair=False, stored_lens=None):
    """Decode stored blobs; returns (out buffer, slot offsets, bounds, status, out_lens[, after repair])."""
    import torch
    host, offs, lens = pack(stored)
    if stored_lens is not None:
        lens = np.asarray(stored_lens, np.int64)
    bounds = [a.decoded_bound(n) for n in lens]
    po, total = slots(bounds)
    d = torch.from_numpy(host).to(dev)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    dec = a.decrypt_chunks_device(d.data_ptr(), offs, lens, out, po, dev)
    torch.cuda.synchronize()
    st0 = dec.status.cpu().numpy().copy()
    if repair:
        dec.repair()
    return out.cpu().numpy(), po, bounds, st0, dec.status.cpu().numpy(), dec.out_lens.cpu().numpy()


def flip(buf: bytearray, i: int):
    buf[i] = 0 if buf[i] >= 128 else 255  # flipByte, ecc_utils_test.go:66-72


# ------------------------------------------------------------------ encode
@pytest.mark.parametrize("o,ms", OPTS)
def test_encode_matches_model(o, ms, gpu):
    m, chunks, want = case(o, ms)
    a = algo(o, ms)
    out, oo, sizes, st = encode(a, chunks, gpu)
    assert st.tolist() == [0] * len(chunks)
    for i, w in enumerate(want):
        assert sizes[i] == len(w)
        got = out[oo[i]:oo[i] + sizes[i]].tobytes()
        assert got == w, f"chunk {i} of {len(chunks[i])} bytes at ({o}, {ms})"
    assert canaries_intact(out, oo, sizes)
    for r in golden("ecc_reference.json")["sizes"]:
        if (r["overhead_percent"], r["max_shard_size"]) == (o, ms):
            i = [len(c) for c in chunks].index(r["original_size"])
            assert sizes[i] == r["original_size"] + r["ecc_size"]


# ------------------------------------------------------------------ clean decode, both directions
@pytest.mark.parametrize("o,ms", OPTS)
def test_decode_clean(o, ms, gpu):
    m, chunks, want = case(o, ms)
    a = algo(o, ms)
    enc_out, oo, sizes, _ = encode(a, chunks, gpu)
    device_stored = [enc_out[oo[i]:oo[i] + sizes[i]].tobytes() for i in range(len(chunks))]
    for stored in (want, device_stored):
        out, po, bounds, st0, st1, lens = decode(a, stored, gpu, repair=True)
        assert st0.tolist() == [0] * len(chunks)
        assert st1.tolist() == [0] * len(chunks)  # the repair call is a no-op
        assert lens.tolist() == [len(c) for c in chunks]
        for i, c in enumerate(chunks):
            assert out[po[i]:po[i] + len(c)].tobytes() == c.tobytes(), f"chunk {i} at ({o}, {ms})"
        assert canaries_intact(out, po, bounds)


# ------------------------------------------------------------------ the reference's damage tests
def damage_cases(m, n):
    s = m.sizes_from_original(n)
    rec = 4 + s.shard_size
    parity = s.parity * rec * s.blocks
    return {
        "data": lambda i: parity + i * rec + 4,      # testRsCrc32ChangeInData
        "data_crc": lambda i: parity + i * rec,      # testRsCrc32ChangeInDataCrc
        "parity": lambda i: i * rec + 4,             # testRsCrc32ChangeInParity
        "parity_crc": lambda i: i * rec,             # testRsCrc32ChangeInParityCrc
    }


REFERENCE_DAMAGE = [
    # (options, size, [(where, count, recovers)])
    ((2, 1024), 1, [("data", 1, True), ("data_crc", 1, True), ("parity", 2, True), ("parity_crc", 2, True)]),
    ((2, 1024), 10240, [("data", 2, True), ("data", 3, False), ("data_crc", 2, True), ("data_crc", 3, False),
                        ("parity", 2, True), ("parity_crc", 2, True)]),
    ((10, 1024), 1 << 20, [("data", 12, True), ("data", 13, False), ("data_crc", 12, True), ("data_crc", 13, False),
                           ("parity", 12, True), ("parity_crc", 12, True)]),
]


@pytest.mark.parametrize("opt,n,cases", REFERENCE_DAMAGE)
def test_reference_damage(opt, n, cases, gpu):
    m, chunks, want = case(*opt)
    a = algo(*opt)
    i = [len(c) for c in chunks].index(n)
    pos = damage_cases(m, n)
    stored = []
    for where, count, _ in cases:
        b = bytearray(want[i])
        for k in range(count):
            flip(b, pos[where](k))
        stored.append(bytes(b))
    out, po, bounds, st0, st1, lens = decode(a, stored, gpu, repair=True)
    assert st0.tolist() == [_lib.KCDC_ECC_DAMAGED] * len(cases)
    for k, (where, count, ok) in enumerate(cases):
        slot = out[po[k]:po[k] + bounds[k]]
        if ok:
            assert st1[k] == 0 and lens[k] == n, (where, count)
            assert slot[:n].tobytes() == chunks[i].tobytes(), (where, count)
        else:
            assert st1[k] == _lib.KCDC_EBADMSG and lens[k] == 0, (where, count)
            assert not slot.any(), (where, count)
            with pytest.raises(ValueError):
                m.decrypt(stored[k])
    assert canaries_intact(out, po, bounds)


# ------------------------------------------------------------------ more damage shapes
def test_damage_shapes(gpu):
    """Block 0's first shard (the length is rebuilt), the truncated last record of a multi-block
    chunk, two blocks with different erasure patterns, and a launch that mixes clean, repairable
    and lost chunks; the small 6+2 code with its length spread over four 1-byte shards."""
    opt = (10, 1024)
    m, chunks, want = case(*opt)
    a = algo(*opt)
    sizes = [len(c) for c in chunks]
    big = sizes.index(1 << 20)
    two = sizes.index(2 * m.data * m.max_shard_size - 3)  # 2 blocks + 1 byte: 3 blocks, last record 1 byte
    s = m.sizes_from_original(1 << 20)
    rec = 4 + s.shard_size
    par = s.parity * rec * s.blocks

    first = bytearray(want[big])
    flip(first, par + 4)          # block 0, shard 0: the length bytes
    flip(first, par + 5 * rec + 9)

    last = bytearray(want[two])
    flip(last, len(last) - 1)     # the truncated record's only payload byte
    flip(last, len(last) - 5 - rec + 100)

    pats = bytearray(want[big])
    for k in (0, 3, 77):          # block 0: three data shards
        flip(pats, par + k * rec + 50)
    flip(pats, 2 * rec + 4)       # and one of its parity shards
    for k in (1, 127):            # block 2: two others
        flip(pats, par + (2 * s.data + k) * rec + 1000)
    flip(pats, (2 * s.parity + 0) * rec)  # and block 2's first parity CRC

    lost = bytearray(want[big])
    for k in range(13):           # block 1: 13 > 12 parity shards
        flip(lost, par + (s.data + k) * rec + 4 + k)

    tiny = bytearray(want[sizes.index(1)])  # 6+2, S = 1: length bytes in shards 0..3
    flip(tiny, 2 * 5 + 4)         # data shard 0
    flip(tiny, 2 * 5 + 3 * 5)     # data shard 3's CRC
    idx = [big, two, big, big, big, sizes.index(1), sizes.index(10240)]
    stored = [bytes(first), bytes(last), bytes(pats), bytes(lost), want[big], bytes(tiny), want[sizes.index(10240)]]
    out, po, bounds, st0, st1, lens = decode(a, stored, gpu, repair=True)
    D = _lib.KCDC_ECC_DAMAGED
    assert st0.tolist() == [D, D, D, D, 0, D, 0]
    assert st1.tolist() == [0, 0, 0, _lib.KCDC_EBADMSG, 0, 0, 0]
    for k, i in enumerate(idx):
        slot = out[po[k]:po[k] + bounds[k]]
        if st1[k] == 0:
            assert lens[k] == sizes[i]
            assert slot[:sizes[i]].tobytes() == chunks[i].tobytes(), f"launch chunk {k}"
            assert m.decrypt(stored[k]) == chunks[i].tobytes()
        else:
            assert lens[k] == 0 and not slot.any()
    assert canaries_intact(out, po, bounds)


# ------------------------------------------------------------------ in-band length, stored length
def test_inband_length_and_short_input(gpu):
    import zlib
    opt = (2, 1024)
    m, chunks, want = case(*opt)
    a = algo(*opt)
    sizes = [len(c) for c in chunks]
    i = sizes.index(10240)
    s = m.sizes_from_original(10240)
    rec = 4 + s.shard_size
    par = s.parity * rec * s.blocks
    b = bytearray(want[i])
    cap = a.decoded_bound(len(b))
    b[par + 4:par + 8] = (cap + 1).to_bytes(4, "big")  # shard 0 claims more than the records hold
    b[par:par + 4] = zlib.crc32(bytes(b[par + 4:par + rec])).to_bytes(4, "big")
    ok = bytearray(want[i])
    ok[par + 4:par + 8] = cap.to_bytes(4, "big")  # all the slot: allowed
    ok[par:par + 4] = zlib.crc32(bytes(ok[par + 4:par + rec])).to_bytes(4, "big")
    stored = [bytes(b), want[sizes.index(1)], bytes(ok), want[i]]
    slens = [len(stored[0]), 39, len(stored[2]), len(stored[3])]
    out, po, bounds, st0, st1, lens = decode(a, stored, gpu, repair=True, stored_lens=slens)
    assert st0.tolist() == st1.tolist() == [_lib.KCDC_EBADMSG, _lib.KCDC_EINVAL, 0, 0]
    assert lens.tolist() == [0, 0, cap, 10240]
    assert not out[po[0]:po[0] + bounds[0]].any()
    assert out[po[2]:po[2] + 10240].tobytes() == chunks[i].tobytes()
    assert out[po[3]:po[3] + 10240].tobytes() == chunks[i].tobytes()
    assert (out[po[1]:po[1] + bounds[1]] == CANARY).all()  # a refused chunk writes nothing
    assert canaries_intact(out, po, bounds)


# ------------------------------------------------------------------ seal then ECC
def test_seal_then_ecc(gpu):
    """encryptorWrapper (repo/format/encryptor_wrapper.go:13-37): Encrypt = seal then ECC, Decrypt =
    ECC (with one shard damaged) then open."""
    import torch
    from kopia_amd import batch
    from kopia_amd import encryption as ke
    from kopia_amd import hashing as kh
    from oracle import coracle
    name = "DYNAMIC-128K-BUZHASH"
    host = coracle.gen_stream(0x6B6F706961, 11, 1 << 20)
    d = torch.from_numpy(host).to(gpu)
    cuts = batch.split_batch_host(name, [host])[0]
    offs, lens = kh.chunk_table([0], [cuts])
    ids = kh.hash_chunks_device(kh.DefaultAlgorithm, d.data_ptr(), offs, lens, bytes(range(32)), gpu).contiguous()
    enc = ke.Encryptor(ke.Aes256Gcm, bytes(range(100, 132)))
    so, stotal = ke.sealed_layout(lens, ke.Aes256Gcm)
    sealed = torch.zeros(stotal, dtype=torch.uint8, device=gpu)
    st = enc.encrypt_chunks_device(d.data_ptr(), offs, lens, ids, 16, sealed, so, gpu)
    slens = np.asarray(lens, np.int64) + enc.Overhead()
    a = kecc.CreateEncryptor(kecc.DefaultAlgorithm, 2)
    eo, esizes, etotal = a.stored_layout(slens)
    stored = torch.zeros(etotal, dtype=torch.uint8, device=gpu)
    st2 = a.encrypt_chunks_device(sealed.data_ptr(), so, slens, stored, eo, gpu)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not st2.cpu().numpy().any()
    m = em.ReedSolomonCrcECC(2, 0)
    sealed_h, stored_h = sealed.cpu().numpy(), stored.cpu().numpy()
    for i in (0, len(lens) - 1):
        assert stored_h[eo[i]:eo[i] + esizes[i]].tobytes() == m.encrypt(sealed_h[so[i]:so[i] + slens[i]].tobytes())
    # damage one data shard of chunk 0 and one parity shard of the last chunk
    g = m.sizes_from_original(int(slens[0]))
    stored[int(eo[0]) + g.parity * (4 + g.shard_size) * g.blocks + 4 + 17] ^= 0x40
    stored[int(eo[-1]) + 4] ^= 1
    po, ptotal = a.plain_layout(esizes)
    back = torch.zeros(ptotal, dtype=torch.uint8, device=gpu)
    dec = a.decrypt_chunks_device(stored.data_ptr(), eo, esizes, back, po, gpu)
    torch.cuda.synchronize()
    want0 = [0] * len(lens)
    want0[0] = want0[-1] = _lib.KCDC_ECC_DAMAGED
    assert dec.status.cpu().tolist() == want0
    assert not dec.repair().cpu().numpy().any()
    assert dec.out_lens.cpu().tolist() == slens.tolist()
    oo, ototal = ke.plain_layout(slens, ke.Aes256Gcm)
    plain = torch.zeros(ototal, dtype=torch.uint8, device=gpu)
    st3 = enc.decrypt_chunks_device(back.data_ptr(), po, slens, ids, 16, plain, oo, gpu)
    torch.cuda.synchronize()
    assert not st3.cpu().numpy().any()
    got = plain.cpu().numpy()
    for i in range(len(lens)):
        assert got[oo[i]:oo[i] + lens[i]].tobytes() == host[offs[i]:offs[i] + lens[i]].tobytes()


# ------------------------------------------------------------------ side stream, empty call
def test_side_stream_status_and_empty_call(gpu):
    """A caller's non-current stream: temporaries, statuses and lengths are ordered on it, so a
    damaged chunk's status survives and a good one reads 0; an empty call does nothing."""
    import torch
    opt = (10, 0)
    m, chunks, want = case(*opt)
    a = algo(*opt)
    pick = [len(c) for c in chunks].index(10240)
    side = torch.cuda.Stream(device=gpu)
    host, offs, lens = pack([chunks[pick].tobytes(), chunks[3].tobytes(), chunks[pick].tobytes()])
    d = torch.from_numpy(host).to(gpu)
    eo, esizes, etotal = a.stored_layout(lens)
    stored = torch.zeros(etotal, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    st = a.encrypt_chunks_device(d.data_ptr(), offs, lens, stored, eo, gpu, stream=side)
    side.synchronize()
    assert st.cpu().tolist() == [0, 0, 0]
    assert stored.cpu().numpy()[eo[2]:eo[2] + esizes[2]].tobytes() == want[pick]
    with torch.cuda.stream(side):
        stored[int(eo[2]) + int(esizes[2]) - 100] ^= 1  # a data byte of chunk 2, on the side stream
    po, ptotal = a.plain_layout(esizes)
    out = torch.zeros(ptotal, dtype=torch.uint8, device=gpu)
    dec = a.decrypt_chunks_device(stored.data_ptr(), eo, esizes, out, po, gpu, stream=side)
    side.synchronize()
    assert dec.status.cpu().tolist() == [0, 0, _lib.KCDC_ECC_DAMAGED]
    assert dec.out_lens.cpu().tolist() == [10240, 3, 0]
    assert dec.repair().cpu().tolist() == [0, 0, 0]
    assert dec.out_lens.cpu().tolist() == [10240, 3, 10240]
    got = out.cpu().numpy()
    assert got[po[2]:po[2] + 10240].tobytes() == chunks[pick].tobytes()
    st0 = a.encrypt_chunks_device(d.data_ptr(), [], [], stored, [], gpu)
    assert st0.numel() == 0
    dec0 = a.decrypt_chunks_device(stored.data_ptr(), [], [], out, [], gpu)
    assert dec0.status.numel() == 0 and dec0.repair().numel() == 0
    L = _lib.lib()
    assert L.kcdc_ecc_encode_chunks_device(b"REED-SOLOMON-CRC32", 2, 0, None, None, None, 0, None, None, None, None) == 0
    assert L.kcdc_ecc_encode_chunks_device(b"NOPE", 2, 0, None, None, None, 0, None, None, None, None) == _lib.KCDC_ENOENT
