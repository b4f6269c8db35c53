"""GPU: every per-chunk entry point over chunks that lie on the 2 GiB and 4 GiB offset lines, and on
the line where the absolute device address crosses a multiple of 2^32 (the population of
tests/far_layout.py, pinned by tests/test_far_layout.py), and the size limits include/kcdc.h states
at 2^32.

Two device buffers of 4 GiB + 8 MiB are allocated once; only a window of 4 MiB around every line
is filled or read back.  A call reads its chunks from the source buffer at far offsets and writes
to slots in the output buffer at far offsets; over the three slot variants the long chunk's slot
straddles every line, ends at it and starts at it.  For every family:
  (a) every result equals the host oracle's (oracle/hashes.py, oracle/aead.py and aesgcm.py, zlib /
      libzstd / the S2 oracle, tests/ecc_model.py);
  (b) the same call on the near twin (every offset moved below 32 MiB, low 16 bits kept) gives the
      same bytes and the same status, length and ID vectors;
  (c) every byte of the output buffer outside the call's slots still holds the canary: the windows
      on the host, the other 4 GiB on the device in pieces of at most 256 MiB.  The positions a
      store with a truncated offset would hit (offset - 2^32, offset - 2^31, offset mod 2^32) are
      among them;
  (d) status, length and ID vectors are compared whole.
Either buffer may lie where its address line is dropped (far_layout.lines); then it has two lines,
the source chunks of a third line write to slots folded onto the two (two long slots share a window,
on opposite sides of the anchor), and a variant without a straddling slot strikes the long chunk
that ends at the first line (far_layout.Layout.struck; the tables for every kept / dropped pair are
built on the CPU by tests/test_far_layout.py::test_slot_tables_of_the_gpu_tests).
The source windows of the twin may overlap a far window (where the address line is low), so a call
uploads its source windows just before it runs, the twin first."""
from functools import lru_cache

import numpy as np
import pytest

import ecc_model as em
import far_layout as fl
import inflate_vectors as iv
import test_gpu_compress as tgc
import test_s2_vectors as sv
from kopia_amd import _lib
from kopia_amd import compression as kc
from kopia_amd import ecc as kecc
from kopia_amd import encryption as ke
from kopia_amd import hashing as kh
from oracle import aead, aesgcm, coracle, deflate
from oracle.hashes import kopia_hash

pytestmark = pytest.mark.gpu
FILL = 0xAB
FILL8 = int.from_bytes(bytes([FILL]) * 8, "little", signed=True)
MIN_FREE = 12 << 30
SEED = 0x6B6F706961
MASTER = bytes(range(100, 132))
EBADMSG, EFBIG, DAMAGED = _lib.KCDC_EBADMSG, _lib.KCDC_EFBIG, _lib.KCDC_ECC_DAMAGED
G4 = 1 << 32
VARIANTS = (0, 1, 2)


class Far:
    """The two buffers, their layouts and the window traffic."""

    def __init__(self, dev):
        import torch
        self.dev = dev
        self.src = torch.full((fl.SIZE,), FILL, dtype=torch.uint8, device=dev)
        self.out = torch.full((fl.SIZE,), FILL, dtype=torch.uint8, device=dev)
        self.ls, self.lo = fl.layout(self.src.data_ptr()), fl.layout(self.out.data_ptr())
        self.out_lines = fl.out_lines(self.ls, self.lo)

    def put(self, buf, windows, host):
        import torch
        for (ws, wl), h in zip(windows, host):
            assert len(h) == wl
            buf[ws:ws + wl] = torch.from_numpy(np.array(h, copy=True)).to(self.dev)

    def get(self, buf, windows):
        return [buf[ws:ws + wl].cpu().numpy() for ws, wl in windows]

    def refill(self, buf, windows):
        for ws, wl in windows:
            buf[ws:ws + wl] = FILL

    def rest_intact(self, buf, windows):
        """Whether every byte of buf outside the windows holds the canary (checked on the device)."""
        import torch
        bad = torch.zeros((), dtype=torch.int64, device=self.dev)
        for a, b in fl.complement(windows, buf.numel()):
            bad += (buf[a:b].view(torch.int64) != FILL8).sum()
        return int(bad.item()) == 0

    def compose(self, lay, offs, blobs, fill=0x5C):
        """Host copies of lay's windows with blobs[i] at the far offset offs[i]."""
        wins = lay.windows()
        host = [np.full(wl, fill, np.uint8) for _, wl in wins]
        for o, b in zip(offs, blobs):
            k = next(k for k, (ws, wl) in enumerate(wins) if ws <= o and o + len(b) <= ws + wl)
            host[k][o - wins[k][0]:o - wins[k][0] + len(b)] = np.frombuffer(b, np.uint8)
        return host

    def run(self, near, src_host, in_offs, out_offs, out_sizes, call):
        """One call at the far offsets or at their twins: upload the source windows, run
        call(src address, input offsets, output tensor, output offsets) -> device vectors, read the
        output windows back, check every byte outside the slots, restore the canary.  Returns
        (Slots, the vectors as numpy arrays)."""
        import torch
        ls, lo = self.ls, self.lo
        sw, ow = ls.windows(near), lo.windows(near)
        self.put(self.src, sw, src_host)
        io = ls.near(in_offs) if near else np.asarray(in_offs, np.int64)
        oo = lo.near(out_offs) if near else np.asarray(out_offs, np.int64)
        vecs = call(self.src.data_ptr(), io, self.out, oo)
        torch.cuda.synchronize()
        vecs = [v.cpu().numpy().copy() for v in vecs]
        host = self.get(self.out, ow)
        rest = self.rest_intact(self.out, ow)
        self.refill(self.out, ow)
        if not rest:  # leave the canary whole for the tests that follow
            self.out.fill_(FILL)
        where = "near" if near else "far"
        assert rest, f"{where}: a byte of the output buffer outside the windows was written"
        assert fl.outside_intact(host, ow, oo, out_sizes, FILL), f"{where}: a byte outside the slots was written"
        return Slots(host, ow, oo), vecs


class Slots:
    def __init__(self, host, windows, offs):
        self.host, self.windows, self.offs = host, windows, offs

    def take(self, i, n, skip=0):
        return fl.take(self.host, self.windows, int(self.offs[i]) + skip, int(n))


@pytest.fixture(scope="module")
def far(gpu):
    import torch
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < MIN_FREE:
        pytest.skip(f"{free >> 20} MiB of device memory free, the far-offset buffers need {MIN_FREE >> 20}")
    f = Far(gpu)
    yield f
    f.src = f.out = None
    torch.cuda.empty_cache()


def _first_wrong(got, want):
    return [(i, len(want[i])) for i in range(len(want)) if got[i] != want[i]][:8]


@lru_cache(maxsize=None)
def _source(kind, nlines):
    """Host bytes of the source windows, other bytes at every line: "stream" is the PRNG stream of
    the splitter tests, "mixed" the compression tests' random, zero, periodic and word stretches."""
    if kind == "stream":
        out = [coracle.gen_stream(SEED, 40 + k, fl.WINDOW) for k in range(nlines)]
    else:
        out = [tgc._mixed(fl.WINDOW, 50 + k) for k in range(nlines)]
    for a in out:
        a.setflags(write=False)
    return out


def _chunks(far, kind):
    ls = far.ls
    host = _source(kind, len(ls.xs))
    return host, [fl.take(host, ls.windows(), int(o), int(n)) for o, n in zip(ls.offs, ls.lens)]


def test_the_buffers_hold_every_line(far):
    """The fixture's own premises: both buffers hold the offset lines, the address line of each is
    where its address crosses a multiple of 2^32 (or is dropped with a reason), chunks of a call sit
    2 GiB apart, and the canary check sees a single byte anywhere."""
    for lay, buf in ((far.ls, far.src), (far.lo, far.out)):
        assert lay.xs[:2] == (1 << 31, G4) and buf.numel() == fl.SIZE and lay.base == buf.data_ptr()
        if lay.dropped is None:
            assert (lay.base + lay.xs[2]) % G4 == 0
        else:
            assert lay.dropped.startswith("A = ") and len(lay.xs) == 2
    assert far.ls.offs.max() > G4 and far.ls.offs.max() - far.ls.offs.min() >= 1 << 31
    wins = far.lo.windows()
    assert far.rest_intact(far.out, wins) and far.rest_intact(far.out, [])
    for at in (0, (1 << 31) - (3 << 20), G4 - (1 << 29) + 5, fl.SIZE - 1):
        if any(ws <= at < ws + wl for ws, wl in wins):
            continue
        far.out[at] = 0
        assert not far.rest_intact(far.out, wins), at
        far.out[at] = FILL
    assert far.rest_intact(far.out, [])


# ------------------------------------------------------------------ hash
HASHES = [("BLAKE2B-256-128", 1), ("BLAKE2B-256-128", 4), ("BLAKE2S-256", 0), ("BLAKE3-256-128", 0), ("HMAC-SHA256", 0),
          ("HMAC-SHA3-256", 0)]
HASH_KEY = bytes(range(7, 39))


@pytest.mark.parametrize("name,lanes", HASHES, ids=[f"{h}-lanes{k}" for h, k in HASHES])
def test_hash(name, lanes, far):
    """Digests of the far chunks and of their twins, with and without the descending-length order,
    equal the oracle's (the digests go to a small tensor: this family has no output line)."""
    import torch
    ls = far.ls
    host, chunks = _chunks(far, "stream")
    want = [kopia_hash(name, HASH_KEY, c) for c in chunks]
    L = _lib.lib()
    assert L.kcdc_test_set(_lib.TEST_HASH_LANES, lanes) == 0
    try:
        for near in (True, False):
            far.put(far.src, ls.windows(near), host)
            offs = ls.near(ls.offs) if near else ls.offs
            for order in (True, False):
                d = kh.hash_chunks_device(name, far.src.data_ptr(), offs, ls.lens, HASH_KEY, far.dev, order=order)
                torch.cuda.synchronize()
                got = [bytes(r) for r in d.cpu().numpy()]
                assert not _first_wrong(got, want), (near, order, _first_wrong(got, want))
    finally:
        assert L.kcdc_test_set(_lib.TEST_HASH_LANES, 0) == 0


# ------------------------------------------------------------------ seal / open
ORACLE = {ke.ChaCha20Poly1305: aead, ke.Aes256Gcm: aesgcm}


@lru_cache(maxsize=None)
def _ids_and_nonces(n):
    rng = np.random.default_rng(2000 + n)
    return rng.integers(0, 256, (n, 16), dtype=np.uint8), bytes(rng.integers(0, 256, 12 * n, dtype=np.uint8))


@pytest.mark.parametrize("alg", [ke.ChaCha20Poly1305, ke.Aes256Gcm])
def test_seal_and_open(alg, far):
    """Seal: every far chunk equals the oracle's Encrypt (both algorithms over every chunk, the long
    ones included: the numpy AES takes a fraction of a second for them), in slots at multiples of 4.
    Open: the sealed chunks are read from far offsets of every alignment and opened into far slots;
    the long chunk whose sealed bytes straddle a line has its tag forged: KCDC_EBADMSG there alone
    and a zeroed slot (tests/test_gpu_crypt.py::test_failed_open_leaves_no_plaintext at small
    offsets).  With three lines every line's long chunk is forged once and opened twice over the
    variants; a buffer whose address line is dropped has no straddler in variant 1, and the first
    line's long chunk, which ends at the line, is forged then (far_layout.Layout.struck)."""
    import torch
    ls, lo = far.ls, far.lo
    n, lens = ls.n, ls.lens
    host, chunks = _chunks(far, "stream")
    ivs, nonces = _ids_and_nonces(n)
    secret = aead.derive_key(MASTER)
    want = [ORACLE[alg].kopia_encrypt(secret, ivs[i].tobytes(), nonces[12 * i:12 * i + 12], chunks[i]) for i in range(n)]
    enc = ke.Encryptor(alg, MASTER)
    d_ivs = torch.from_numpy(ivs.copy()).to(far.dev)
    slot = (lens + 28 + 3) & ~3
    pslot = (lens + 3) & ~3
    for v in VARIANTS:
        oo = lo.slots(slot, 4, v, far.out_lines)

        def seal(src, io, out, o):
            return [enc.encrypt_chunks_device(src, io, lens, d_ivs, 16, out, o, far.dev, nonces=nonces)]

        res = {}
        for near in (True, False):
            got, (st,) = far.run(near, host, ls.offs, oo, slot, seal)
            assert st.tolist() == [0] * n, (v, near)
            res[near] = [got.take(i, lens[i] + 28) for i in range(n)]
        assert not _first_wrong(res[False], want), (v, _first_wrong(res[False], want))
        assert res[True] == res[False], v

        # open, from sealed chunks placed at far offsets of the source buffer
        soffs = ls.slots(lens + 28, 1, v)
        k_hit, hit, straddles = ls.struck(v)
        forged = [hit]
        assert not straddles or soffs[hit] < ls.xs[k_hit] < soffs[hit] + lens[hit]
        blobs = [bytearray(w) for w in want]
        for i in forged:
            blobs[i][12 + int(lens[i])] ^= 0x40  # the first tag byte
        sealed = far.compose(ls, soffs, blobs)
        po = lo.slots(pslot, 4, (v + 1) % 3, far.out_lines)

        def open_(src, io, out, o):
            return [enc.decrypt_chunks_device(src, io, lens + 28, d_ivs, 16, out, o, far.dev)]

        want_st = [EBADMSG if i in forged else 0 for i in range(n)]
        res = {}
        for near in (True, False):
            got, (st,) = far.run(near, sealed, soffs, po, pslot, open_)
            assert st.tolist() == want_st, (v, near)
            res[near] = [got.take(i, lens[i]) for i in range(n)]
        ref = [bytes(len(c)) if i in forged else c for i, c in enumerate(chunks)]
        assert not _first_wrong(res[False], ref), (v, _first_wrong(res[False], ref))
        assert res[True] == res[False], v


# ------------------------------------------------------------------ compress
COMPRESSORS = ["deflate-default", "gzip", "s2-default", "zstd"]


def _compress_far(far, name, v, near=False):
    ls, lo = far.ls, far.lo
    host, _ = _chunks(far, "mixed")
    bounds = np.array([kc.compress_bound(int(x)) for x in ls.lens], np.int64)
    oo = lo.slots(bounds, 4, v, far.out_lines)
    comp = kc.Compressor(name)

    def call(src, io, out, o):
        return list(comp.compress_chunks_device(src, io, ls.lens, out, o, far.dev))

    got, (ol, ids) = far.run(near, host, ls.offs, oo, bounds, call)
    assert (ol <= bounds).all() and (ol >= 6).all()
    return [got.take(i, ol[i]) for i in range(ls.n)], ol, ids


@pytest.fixture(scope="module")
def own(far):
    """own(name): the device's own contents of the mixed chunks at the far offsets, one compress call
    per name (variant 0, as test_compress checks it against the oracle), kept until the module ends."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _compress_far(far, name, 0)[0]
        return made[name]

    yield get
    made.clear()


@pytest.mark.parametrize("name", COMPRESSORS)
def test_compress(name, far):
    """Every far output decodes through the name's independent decoder to its chunk within its
    bound, the IDs follow the keep-or-drop rule, and the twin's output, lengths and IDs are the
    same: a span's matches depend on its own bytes alone, so two runs of one call agree."""
    ls = far.ls
    _, chunks = _chunks(far, "mixed")
    for v in VARIANTS:
        blobs, ol, ids = _compress_far(far, name, v)
        for i, c in enumerate(chunks):
            assert deflate.decompress(name, blobs[i]) == c, (v, i, len(c))
        assert ids.tolist() == [deflate.kept_header_id(name, len(c), int(ol[i])) for i, c in enumerate(chunks)], v
        assert ids[ls.long_indices()].all()
        nblobs, nol, nids = _compress_far(far, name, v, near=True)
        assert nol.tolist() == ol.tolist() and nids.tolist() == ids.tolist(), v
        assert not _first_wrong(nblobs, blobs), (v, _first_wrong(nblobs, blobs))


# ------------------------------------------------------------------ S2 decompress, inflate
DECODERS = ["s2-default", "deflate-default", "gzip"]


def _foreign(name):
    """(content, decoded bytes) of other writers: Snappy framing and built S2 elements, zlib's streams."""
    if name == sv.NAME:
        data = sv.mixed(65537, 9)
        vs = {v.id: v for v in sv.valid_vectors()}
        # 64 KiB blocks: a content may hold one data chunk per 16 KiB of cap, plus one
        return [(sv.content(sv.snappy_framed(data)), data)] + \
               [(vs[k].blob, vs[k].expected) for k in ("copy2-len64-off65535", "overlap-off3-len300")]
    data = iv.mixed(65538, 9)[:65537]
    return [(iv.content(name, iv.zlib_stream(name, data, level=9)), data),
            (iv.content(name, iv.zlib_stream(name, data[:3000], strategy=iv.zlib.Z_FIXED)), data[:3000]),
            (iv.content(name, iv.zlib_stream(name, data, flush=True)), data)]


def _corrupt_one_byte(name, blob):
    """One byte changed so that the content must be refused: the stored CRC-32C of an S2 content's
    first data chunk (decoded, then refused), a gzip member's CRC-32 (decoded to its end, then
    refused); a raw deflate stream carries no checksum, so its first block's type becomes the
    reserved one."""
    b = bytearray(blob)
    if name == sv.NAME:
        b[4 + len(sv.IDENT_S2) + 4] ^= 0x10
    elif iv.is_gz(name):
        b[-8] ^= 0x10
    else:
        b[4] |= 0x06
    return bytes(b)


@pytest.mark.parametrize("name", DECODERS)
def test_decode(name, far, own):
    """The device's own contents of the far chunks and three foreign ones, read from far offsets
    and decoded into far slots with caps equal to the original lengths.  The long content whose
    compressed bytes straddle a line (far_layout.Layout.struck: where no line has a straddler, the
    one that ends at the first line) has one byte corrupted: KCDC_EBADMSG and length 0 there alone
    (the host model agrees), every other content exact."""
    ls, lo = far.ls, far.lo
    _, chunks = _chunks(far, "mixed")
    foreign = _foreign(name)
    blobs = list(own(name)) + [b for b, _ in foreign]
    plain = list(chunks) + [p for _, p in foreign]
    n = len(blobs)
    in_lines = np.concatenate((ls.line_of, np.arange(len(foreign)) % len(ls.xs)))
    out_lines = in_lines % len(lo.xs)
    clens = np.array([len(b) for b in blobs], np.int64)
    caps = np.array([len(p) for p in plain], np.int64)
    comp = kc.Compressor(name)
    decode = comp.decompress_chunks_device if name == sv.NAME else comp.inflate_chunks_device
    for v in VARIANTS:
        coffs = ls.slots(clens, 1, v, in_lines)
        k_hit, hit, straddles = ls.struck(v)
        bad = [hit]
        assert not straddles or coffs[hit] < ls.xs[k_hit] < coffs[hit] + clens[hit]
        fed = list(blobs)
        for i in bad:
            fed[i] = _corrupt_one_byte(name, blobs[i])
            model = sv.model_decode(fed[i], name, int(caps[i]), sv.room_for(int(caps[i])))[0] if name == sv.NAME \
                else iv.model(name, fed[i], int(caps[i]))[0]
            assert model == EBADMSG, (name, i)
        src = far.compose(ls, coffs, fed)
        oo = lo.slots(caps, 1, (v + 1) % 3, out_lines)

        def call(s, io, out, o):
            return list(decode(s, io, clens, out, o, caps, far.dev))

        want_st = [EBADMSG if i in bad else 0 for i in range(n)]
        res = {}
        for near in (True, False):
            got, (ol, st) = far.run(near, src, coffs, oo, caps, call)
            assert st.tolist() == want_st, (v, near)
            assert ol.tolist() == [0 if want_st[i] else int(caps[i]) for i in range(n)], (v, near)
            res[near] = [got.take(i, ol[i]) for i in range(n)]
        ref = [b"" if want_st[i] else plain[i] for i in range(n)]
        assert not _first_wrong(res[False], ref), (v, _first_wrong(res[False], ref))
        assert res[True] == res[False], v


# ------------------------------------------------------------------ ECC
ECC_OPTS = [(2, 1024), (10, 0)]


def _flip(buf, i):
    buf[i] = 0 if buf[i] >= 128 else 255  # flipByte, ecc_utils_test.go:66-72


def _record(s, kind, block, shard):
    """Offset in a stored chunk of a record (its CRC, then its shard): parity records come first."""
    rec = 4 + s.shard_size
    if kind == "parity":
        return (block * s.parity + shard) * rec
    return s.parity * rec * s.blocks + (block * s.data + shard) * rec


@pytest.mark.parametrize("o,ms", ECC_OPTS)
def test_ecc(o, ms, far):
    """Encode equals the model for every far chunk.  Decode, from stored chunks at far offsets into
    far slots: clean; then with a data shard and a parity CRC damaged in the long chunk whose stored
    bytes straddle a line (far_layout.Layout.struck), and one shard more than its parity lost in the 70,001-byte chunk of the
    line farthest from it (2 GiB away between the offset lines): KCDC_ECC_DAMAGED at those two alone, the repair restores the
    first and refuses the second with a zeroed slot.  The repair finds both chunks' bad-shard masks
    in the workspace by their block prefix, so a mask slot indexed with a chunk's offset would miss."""
    ls, lo = far.ls, far.lo
    n, lens = ls.n, ls.lens
    host, chunks = _chunks(far, "stream")
    m = em.ReedSolomonCrcECC(o, ms)
    a = kecc.CreateAlgorithm(kecc.Options(OverheadPercent=o, MaxShardSize=ms))
    want = [m.encrypt(c) for c in chunks]
    sizes = np.array([a.encoded_size(int(x)) for x in lens], np.int64)
    assert sizes.tolist() == [len(w) for w in want]
    bounds = np.array([a.decoded_bound(int(s)) for s in sizes], np.int64)
    for v in VARIANTS:
        oo = lo.slots(sizes, 1, v, far.out_lines)

        def encode(src, io, out, o_):
            return [a.encrypt_chunks_device(src, io, lens, out, o_, far.dev)]

        res = {}
        for near in (True, False):
            got, (st,) = far.run(near, host, ls.offs, oo, sizes, encode)
            assert st.tolist() == [0] * n, (v, near)
            res[near] = [got.take(i, sizes[i]) for i in range(n)]
        assert not _first_wrong(res[False], want), (v, _first_wrong(res[False], want))
        assert res[True] == res[False], v

        soffs = ls.slots(sizes, 1, v)
        po = lo.slots(bounds, 1, (v + 1) % 3, far.out_lines)
        k_hit, hit, straddles = ls.struck(v)
        k_lost = max(range(len(ls.xs)), key=lambda k: abs(ls.xs[k] - ls.xs[k_hit]))  # the farthest line: 1 GiB away or more
        lost = k_lost * fl.PER_LINE + fl.MID_AT
        assert (not straddles or soffs[hit] < ls.xs[k_hit] < soffs[hit] + sizes[hit]) and abs(int(soffs[hit]) - int(soffs[lost])) >= (1 << 30) - (4 << 20)
        damaged = [bytearray(w) for w in want]
        s = m.sizes_from_original(int(lens[hit]))
        _flip(damaged[hit], _record(s, "data", s.blocks // 2, 3) + 4 + 10)
        _flip(damaged[hit], _record(s, "parity", s.blocks // 2, 1) + 2)
        assert m.decrypt(bytes(damaged[hit])) == chunks[hit]
        s = m.sizes_from_original(int(lens[lost]))
        for k in range(s.parity + 1):
            _flip(damaged[lost], _record(s, "data", s.blocks // 2, 5 + k) + 4 + k)
        with pytest.raises(ValueError):
            m.decrypt(bytes(damaged[lost]))

        def decode(src, io, out, o_):
            dec = a.decrypt_chunks_device(src, io, sizes, out, o_, far.dev)
            first = [dec.status.clone(), dec.out_lens.clone()]
            dec.repair()
            return first + [dec.status, dec.out_lens]

        for label, stored, first_st, last_st in (
                ("clean", want, [0] * n, [0] * n),
                ("damaged", damaged, [DAMAGED if i in (hit, lost) else 0 for i in range(n)],
                 [EBADMSG if i == lost else 0 for i in range(n)])):
            src = far.compose(ls, soffs, stored)
            res = {}
            for near in (True, False):
                got, (st0, ol0, st1, ol1) = far.run(near, src, soffs, po, bounds, decode)
                assert st0.tolist() == first_st and st1.tolist() == last_st, (v, label, near)
                assert ol0.tolist() == [0 if first_st[i] else int(lens[i]) for i in range(n)], (v, label, near)
                assert ol1.tolist() == [0 if last_st[i] else int(lens[i]) for i in range(n)], (v, label, near)
                res[near] = [got.take(i, bounds[i] if last_st[i] else lens[i]) for i in range(n)]
            ref = [bytes(int(bounds[i])) if last_st[i] else chunks[i] for i in range(n)]
            assert not _first_wrong(res[False], ref), (v, label, _first_wrong(res[False], ref))
            assert res[True] == res[False], (v, label)


# ------------------------------------------------------------------ the limits include/kcdc.h states at 2^32
# The buffers really are longer than 4 GiB, so a length of 2^32 describes allocated memory; none of
# these cases reads more than the few bytes put there.
LOW = [(0, 1 << 18)]  # the output window of these calls


def _direct(far, contents, call, out_offs, out_sizes):
    """Put (offset, bytes) contents into the source buffer, run call() -> device vectors, read the
    low output window back and check every other byte of the output buffer and every byte of the
    window outside [out_offs[i], +out_sizes[i]).  Returns (the window's bytes, the vectors)."""
    import torch
    for o, b in contents:
        far.src[o:o + len(b)] = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(far.dev)
    vecs = call()
    torch.cuda.synchronize()
    vecs = [v.cpu().numpy().copy() for v in vecs]
    host = far.get(far.out, LOW)
    rest = far.rest_intact(far.out, LOW)
    far.refill(far.out, LOW)
    if not rest:
        far.out.fill_(FILL)
    assert rest, "a byte of the output buffer outside the low window was written"
    assert fl.outside_intact(host, LOW, out_offs, out_sizes, FILL), "a byte outside the slots was written"
    return host[0], vecs


def test_inflate_length_limits(far):
    """kcdc_inflate_chunks_device, deflate-default: a content of 2^32 bytes gets KCDC_EBADMSG and
    length 0 although a valid stream starts it; one of 2^32 - 1 bytes, the largest accepted, decodes
    (a raw stream ends at its final block, the 4 GiB after it are ignored); a cap of 2^32 + 4096
    counts as 2^32 - 1: the small content decodes and nothing past its length is written."""
    name = "deflate-default"
    data = iv.mixed(5001, 3)[:5000]
    small, big = iv.content(name, iv.zlib_stream(name, data[:300])), iv.content(name, iv.zlib_stream(name, data, level=9))
    at = [(8 << 20) + 3, 0, 4 << 20, (8 << 20) + 4097]
    contents = [(at[0], small), (at[1], big), (at[2], big), (at[3], small)]
    clens = [len(small), G4, G4 - 1, len(small)]
    caps = [300, 5000, 5000, G4 + 4096]
    oo = [8192 + 3, 16384 + 1, 32768 + 5, 0]
    comp = kc.Compressor(name)
    out, (ol, st) = _direct(far, contents, lambda: comp.inflate_chunks_device(far.src.data_ptr(), at, clens, far.out, oo, caps, far.dev),
                            oo, [300, 5000, 5000, 300])
    assert st.tolist() == [0, EBADMSG, 0, 0] and ol.tolist() == [300, 0, 5000, 300]
    for i, want in ((0, data[:300]), (2, data), (3, data[:300])):
        assert out[oo[i]:oo[i] + len(want)].tobytes() == want, i


def test_s2_cap_above_4_gib(far):
    """kcdc_decompress_chunks_device with a cap of 2^32 + 4096 and the workspace
    kcdc_decompress_workspace_size gives for it (a descriptor per 16 KiB of cap): the content decodes,
    nothing past its length is written, its neighbour is exact.  Lengths and caps are 64 bits there."""
    data = sv.mixed(70001, 5)
    blobs = [sv.content(sv.snappy_framed(data[:3000], block_size=1024)), sv.content(sv.snappy_framed(data))]
    at = [(8 << 20) + 1, (8 << 20) + 8192 + 2]
    caps = [G4 + 4096, 70001]
    oo = [0, 65536 + 3]
    comp = kc.Compressor(sv.NAME)
    assert _lib.lib().kcdc_decompress_workspace_size(sum(map(len, blobs)), sum(caps), 2) > (G4 >> 14) * 32
    out, (ol, st) = _direct(far, list(zip(at, blobs)),
                            lambda: comp.decompress_chunks_device(far.src.data_ptr(), at, [len(b) for b in blobs], far.out, oo, caps, far.dev),
                            oo, [3000, 70001])
    assert st.tolist() == [0, 0] and ol.tolist() == [3000, 70001]
    assert out[:3000].tobytes() == data[:3000] and out[oo[1]:oo[1] + 70001].tobytes() == data


@pytest.mark.parametrize("o,ms", ECC_OPTS)
def test_ecc_encode_refuses_4_gib(o, ms, far):
    """kcdc_ecc_encode_chunks_device: chunks of 2^32 - 4 and 2^32 + 5 bytes among normal ones get
    KCDC_EFBIG and not a byte of output (the length prefix is 4 bytes); the host size function
    refuses the same lengths; the neighbours equal the model."""
    m = em.ReedSolomonCrcECC(o, ms)
    a = kecc.CreateAlgorithm(kecc.Options(OverheadPercent=o, MaxShardSize=ms))
    data = coracle.gen_stream(SEED, 60, 80000).tobytes()
    lens = [5000, G4 - 4, 70001, G4 + 5, 33]
    at = [(8 << 20) + 1, 0, (8 << 20) + 8192 + 3, 1 << 20, (8 << 20) + 5]
    chunks = {0: data[:5000], 2: data[5000:75001], 4: data[4:37]}
    contents = [(at[0], data[:5000]), (at[2], data[5000:75001])]  # chunk 4 lies inside chunk 0
    for n in (G4 - 4, G4 + 5):
        with pytest.raises(_lib.KcdcError) as e:
            a.encoded_size(n)
        assert e.value.code == EFBIG
    assert a.encoded_size(G4 - 5) > G4
    want = {i: m.encrypt(c) for i, c in chunks.items()}
    sizes = [len(want[i]) if i in want else 0 for i in range(5)]
    oo, pos = [], 13
    for s in sizes:
        oo.append(pos)
        pos += s + fl.GUARD + 1
    assert pos < LOW[0][1]
    out, (st,) = _direct(far, contents, lambda: [a.encrypt_chunks_device(far.src.data_ptr(), at, lens, far.out, oo, far.dev)], oo, sizes)
    assert st.tolist() == [0, EFBIG, 0, EFBIG, 0]
    for i, w in want.items():
        assert out[oo[i]:oo[i] + len(w)].tobytes() == w, i
