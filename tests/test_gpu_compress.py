"""GPU: deflate / gzip / pgzip content compression of many chunks (kcdc_compress_chunks_device) against the
oracle (oracle/deflate.py: the reference's framing, zlib as the independent RFC 1951 inflater).
Every chunk must inflate back to its bytes behind its 4-byte header ID, carry the content
manager's keep-or-drop ID (content_manager_lock_free.go:64-73), and the reference's own test
properties hold (compressor_test.go:15-87): all-zero data shrinks, random data does not, and
another compressor's reader rejects the stream.  Edge cases: empty chunks, lengths across the
512-byte segment and 32 KiB span boundaries, misaligned offsets, 8 MiB chunks, mixed data."""
import ctypes as C

import numpy as np
import pytest

from kopia_amd import _lib
from kopia_amd import compression as kc
from oracle import coracle, deflate

pytestmark = pytest.mark.gpu
DEFLATE = ["deflate-best-compression", "deflate-best-speed", "deflate-default"]
GZIP = ["gzip", "gzip-best-compression", "gzip-best-speed", "pgzip", "pgzip-best-compression", "pgzip-best-speed"]
S2 = list(deflate.S2_NAMES)  # compressor_s2.go:20-23; decoded by oracle/s2_oracle.c (CRC-32C checked)
ZSTD = list(deflate.ZSTD_NAMES)  # compressor_zstd.go:15-18; decoded by libzstd (the RFC 8878 reference decoder)
ALL = DEFLATE + GZIP + S2 + ZSTD


def _compress(name, host, offs, lens, dev):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    oo, total = kc.compressed_layout(lens)
    out = torch.full((total,), 0xAB, dtype=torch.uint8, device=dev)
    comp = kc.Compressor(name)
    out_lens, ids = comp.compress_chunks_device(d.data_ptr(), offs, lens, out, oo, dev)
    torch.cuda.synchronize()
    return out.cpu().numpy(), oo, out_lens.cpu().numpy(), ids.cpu().numpy()


def _check(name, host, offs, lens, out, oo, out_lens, ids):
    for i, (o, n) in enumerate(zip(offs, lens)):
        blob = out[oo[i]:oo[i] + out_lens[i]].tobytes()
        assert 6 <= out_lens[i] <= kc.compress_bound(int(n)), (i, n, out_lens[i])
        assert deflate.decompress(name, blob) == host[o:o + n].tobytes(), (i, n)
        if name in S2:  # and the blocks through Google's Snappy library (an independent decoder)
            assert deflate.s2_decode_snappy(blob[4:]) == host[o:o + n].tobytes(), (i, n)
        assert ids[i] == deflate.kept_header_id(name, int(n), int(out_lens[i])), i


def _mixed(nbytes, seed):
    """Random, zero, periodic and word-salad stretches (so segments hit every encoder path)."""
    rng = np.random.default_rng(seed)
    words = [b"kopia", b"snapshot", b"content", b"chunk", b"the", b"of", b"blob", b"index", b" ", b"\n"]
    out, size = [], 0
    while size < nbytes:
        kind = int(rng.integers(0, 4))
        n = int(rng.integers(1, 20000))
        if kind == 0:
            s = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            s = bytes(n)
        elif kind == 2:
            p = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            s = (p * (n // len(p) + 1))[:n]
        else:
            s = b"".join(words[int(k)] for k in rng.integers(0, len(words), n // 4 + 1))[:n]
        out.append(s)
        size += len(s)
    return np.frombuffer(b"".join(out)[:nbytes], np.uint8).copy()


@pytest.mark.parametrize("name", ALL)
def test_reference_properties(name, gpu):
    """compressor_test.go:21-84 through the device: 10000 zero bytes shrink (and keep the ID),
    10000 random bytes do not (ID 0, NoCompression), both inflate back; the other deflate
    compressors' readers reject the stream by its header."""
    zeros = np.zeros(10000, np.uint8)
    rnd = np.random.default_rng(5).integers(0, 256, 10000, dtype=np.uint8)
    host = np.concatenate([zeros, rnd])
    offs, lens = [0, 10000], [10000, 10000]
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)
    assert ol[0] < 10000 and ids[0] == deflate.HEADER_IDS[name]
    assert ol[1] >= 10000 and ids[1] == 0
    blob = out[oo[0]:oo[0] + ol[0]].tobytes()
    if name in GZIP:  # the member header as Go's gzip.Writer (and pgzip's) writes it: XFL from the level
        xfl = 2 if name.endswith("best-compression") else 4 if name.endswith("best-speed") else 0
        assert blob[4:14] == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, xfl, 0xFF]), blob[4:14].hex()
    for other in ALL:
        if other != name:
            with pytest.raises(ValueError):
                deflate.decompress(other, blob)


def ragged_corpus():
    """(host bytes, offsets, lengths) of test_ragged_misaligned_chunks; tools/deflate_census.py
    reports which branches of the deflate plan these chunks reach."""
    host = _mixed(24 << 20, 11)
    rng = np.random.default_rng(12)
    edge = [0, 1, 2, 3, 4, 5, 7, 8, 255, 511, 512, 513, 1023, 1024, 1025, 4096, 32767, 32768, 32769,
            65535, 65536, 65537, 100000, (1 << 20) + 3]
    lens = edge + [int(x) for x in rng.integers(0, 300000, 200)]
    offs = [int(rng.integers(0, host.size - L)) for L in lens]
    return host, offs, lens


@pytest.mark.parametrize("name", ["deflate-default", "gzip", "pgzip-best-speed", "s2-default", "s2-better",
                                  "zstd", "zstd-best-compression"])
def test_ragged_misaligned_chunks(name, gpu):
    """Edge lengths around the 512-byte segments and 32 KiB spans at random offsets; for the gzip
    family this exercises the device CRC-32 (end-aligned spans, partial first span)."""
    host, offs, lens = ragged_corpus()
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)
    assert (ids != 0).sum() > len(lens) // 2  # mixed data mostly compresses


@pytest.mark.parametrize("name", DEFLATE + ["gzip-best-compression", "s2-better", "s2-parallel-8", "zstd-fastest",
                                            "zstd-better-compression"])
def test_large_compressible_chunks(name, gpu):
    """The reference benchmark's inputs (compressor_test.go:92-96): a repeated 1..10 pattern and
    zeros, as 8 MiB + odd chunks; both must shrink far below the input."""
    pat = np.tile(np.arange(1, 11, dtype=np.uint8), (8 << 20) // 10 + 2)[:(8 << 20) + 13]
    host = np.concatenate([pat, np.zeros((8 << 20) + 13, np.uint8), _mixed(4 << 20, 3)])
    offs = [0, pat.size, 2 * pat.size]
    lens = [pat.size, pat.size, 4 << 20]
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)
    # Snappy copies carry at most 64 bytes (3 bytes each): the pattern costs S2 ~5 % here
    lim = 0.08 if name in S2 else 0.05
    assert ol[0] < lim * lens[0] and ol[1] < lim * lens[1]


@pytest.mark.parametrize("name", ["deflate-best-speed", "pgzip", "s2-parallel-4", "zstd"])
def test_splitter_chunks_of_mixed_stream(name, gpu):
    """Chunks cut by the oracle's DYNAMIC-128K-BUZHASH over a mixed 32 MiB stream."""
    host = _mixed(32 << 20, 21)
    cuts = [int(c) for c in coracle.split_batch("DYNAMIC-128K-BUZHASH", [host])[0]]
    bounds = [0] + cuts + ([] if cuts and cuts[-1] == host.size else [host.size])
    offs = bounds[:-1]
    lens = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    assert sum(lens) == host.size and len(lens) > 100
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)


@pytest.mark.parametrize("name", ["deflate-default", "gzip"])
def test_random_stream_is_stored(name, gpu):
    """Config-2 bytes (uniform PRNG): every 32 KiB span falls back to ONE stored block (5 + 32768
    bytes: a span whose code would not beat a stored copy is stored whole), the stream is the header
    ID, those blocks and the final empty block (plus the gzip member's 18 bytes), and the ID is
    NoCompression."""
    host = coracle.gen_stream(0x6B6F706961, 0, 8 << 20)
    lens = [1 << 20] * 8
    offs = [i << 20 for i in range(8)]
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)
    assert not ids.any()
    spans = (1 << 20) // 32768
    want = 4 + spans * (5 + 32768) + 2 + (18 if name in GZIP else 0)
    assert all(int(x) == want for x in ol), (want, ol)


def test_workspace_too_small_writes_no_output(gpu):
    import torch
    host = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    offs = torch.tensor([0], dtype=torch.int64, device=gpu)
    lens = torch.tensor([1 << 20], dtype=torch.int64, device=gpu)
    oo = torch.tensor([0], dtype=torch.int64, device=gpu)
    out = torch.zeros(kc.compress_bound(1 << 20), dtype=torch.uint8, device=gpu)
    ol = torch.full((1,), 7, dtype=torch.int64, device=gpu)
    ids = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    need = int(_lib.lib().kcdc_compress_workspace_size(1 << 20, 1))
    work = torch.empty(need // 4, dtype=torch.uint8, device=gpu)
    rc = _lib.lib().kcdc_compress_chunks_device(b"deflate-default", C.c_void_p(host.data_ptr()), offs.data_ptr(),
                                                lens.data_ptr(), 1, out.data_ptr(), oo.data_ptr(), ol.data_ptr(),
                                                ids.data_ptr(), work.data_ptr(), work.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert ol.item() == 0 and ids.item() == 0
    # Too small even for the per-chunk table: refused up front.
    rc = _lib.lib().kcdc_compress_chunks_device(b"deflate-default", C.c_void_p(host.data_ptr()), offs.data_ptr(),
                                                lens.data_ptr(), 1, out.data_ptr(), oo.data_ptr(), ol.data_ptr(),
                                                ids.data_ptr(), work.data_ptr(), 4, None)
    assert rc == _lib.KCDC_EINVAL


def test_s2_random_stream_is_stored(gpu):
    """Config-2 bytes through s2-default: every segment is one stored literal (3-byte header), each
    32 KiB span a framing chunk (8-byte header + 3-byte uvarint), and the ID is NoCompression."""
    host = coracle.gen_stream(0x6B6F706961, 0, 8 << 20)
    lens = [1 << 20] * 8
    offs = [i << 20 for i in range(8)]
    out, oo, ol, ids = _compress("s2-default", host, offs, lens, gpu)
    _check("s2-default", host, offs, lens, out, oo, ol, ids)
    assert not ids.any()
    assert all(int(x) == 4 + 10 + 32 * (8 + 3) + (1 << 20) + 3 * 2048 for x in ol)


def test_zstd_random_stream_is_stored(gpu):
    """Config-2 bytes through zstd: one frame per chunk (magic, descriptor, 4-byte content size),
    every 8 KiB block of 16 segments a Raw_Block (3-byte header), a final empty Raw_Block; ID
    NoCompression."""
    host = coracle.gen_stream(0x6B6F706961, 0, 8 << 20)
    lens = [1 << 20] * 8
    offs = [i << 20 for i in range(8)]
    out, oo, ol, ids = _compress("zstd", host, offs, lens, gpu)
    _check("zstd", host, offs, lens, out, oo, ol, ids)
    assert not ids.any()
    assert all(int(x) == 4 + 9 + 128 * (3 + 8192) + 3 for x in ol)


@pytest.mark.parametrize("name", ["s2-default", "zstd"])
def test_tiny_chunks_frame(name, gpu):
    """Empty and few-byte chunks: a frame with no data block (zstd: header + final empty block;
    S2: the stream identifier alone) still decodes to the empty string."""
    host = np.frombuffer(b"abcabcabcabcabcabcabc", np.uint8).copy()
    offs, lens = [0, 0, 3, 0], [0, 1, 4, 21]
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)


def test_mixed_ratio_does_not_regress(gpu):
    """Pins the device encoders' ratio on text-like data against zlib level 6 on the same 1 MiB
    chunks (DESIGN.md §2.7, round 4 on the bench's mixed data: deflate-default 0.329 = 1.09 x
    zlib-6, best-compression 0.328, s2 0.367, zstd 0.370 = 1.23 x): the levels order as their search
    effort, and each family stays within its margin."""
    import zlib
    host = _mixed(8 << 20, 31)
    z6 = sum(len(zlib.compress(host[i << 20:(i + 1) << 20].tobytes(), 6)) for i in range(8)) / host.size
    offs, lens = [i << 20 for i in range(8)], [1 << 20] * 8
    ratio = {}
    for name in ["deflate-best-speed", "deflate-default", "deflate-best-compression", "s2-default", "zstd"]:
        out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
        _check(name, host, offs, lens, out, oo, ol, ids)
        ratio[name] = float(ol.sum()) / host.size
    assert ratio["deflate-default"] <= ratio["deflate-best-speed"], ratio
    assert ratio["deflate-best-compression"] <= ratio["deflate-default"] + 1e-3, ratio
    assert ratio["deflate-default"] <= 1.12 * z6, (ratio, z6)
    assert ratio["s2-default"] <= 1.25 * z6 and ratio["zstd"] <= 1.26 * z6, (ratio, z6)


def table_carrier_chunks():
    """The chunks of test_zstd_table_carriers (tools/zstd_census.py reports which branches of the span
    encoder they reach)."""
    rng = np.random.default_rng(77)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
    text = lambda n: _mixed(n, int(rng.integers(1 << 30)))[:n]
    words = lambda n: np.frombuffer((b"kopia snapshot content chunk " * (n // 29 + 1))[:n], np.uint8)
    per = np.frombuffer((bytes(range(7, 40)) * (1 + (1 << 16) // 33))[:1 << 16], np.uint8)
    latin = [w.encode("latin-1") for w in ("été", "çà", "über", "naïve", "señor", "ÿ", "æther", " ", "\n")]
    hitext = lambda n: np.frombuffer(b"".join(latin[int(i)] for i in rng.integers(0, len(latin), n))[:n], np.uint8)
    parts = [
        [rnd(8192), words(24576)],                             # block 0 raw, block 1 carries
        [words(8192), rnd(8192), words(16384)],                # a raw block between
        [np.zeros(8192, np.uint8), words(24576)],              # block 0: sequences, few literals
        [rnd(8192), rnd(8192), rnd(8192), words(8192)],        # only the last block compresses
        [per[:32768]],                                         # periodic: repeat offsets
        [words(3000), rnd(5192), words(24576 + 777)],          # ragged last span
        [text(70000)],
        [np.zeros(32768, np.uint8)],                           # one literal symbol: no Huffman
        [hitext(40000)],                                       # literals > 128: FSE-compressed weights
        [rnd(3000), hitext(30000), rnd(100)],                  # every byte value in the span's code
    ]
    return [np.concatenate(p) for p in parts]


def adversarial_parts():
    """The chunks of test_zstd_adversarial_spans (tools/zstd_census.py counts their branches too)."""
    rng = np.random.default_rng(2024)
    vocab = [rng.integers(0, 256, 4, dtype=np.uint8).tobytes() for _ in range(12)]
    tokens = np.frombuffer(b"".join(vocab[int(i)] for i in rng.integers(0, 12, 40000)), np.uint8)
    head = rng.integers(0, 256, 7000, dtype=np.uint8)
    far = np.concatenate([head[:2000], rng.integers(0, 256, 28000, dtype=np.uint8), head[:2768]])
    skew = np.minimum(rng.geometric(0.02, 70000), 255).astype(np.uint8)
    alt = np.tile(np.frombuffer(b"xyzw1234" * 3 + b"ABCD", np.uint8), 4000)
    return [
        tokens[:32768 * 3],                                                 # many 4-byte matches
        np.concatenate([head, head[:500], rng.integers(0, 256, 9000, dtype=np.uint8), head]),  # long carries
        far,                                                                # distances near 32 KiB
        np.tile(np.frombuffer(b"0123456789abcdef" * 64, np.uint8), 70),     # long matches
        skew,                                                               # all byte values, skewed
        alt,                                                                # alternating offsets
        np.concatenate([tokens[:5000], skew[:20000], tokens[5000:30000]]),
    ]


@pytest.mark.parametrize("name", ["zstd", "zstd-best-compression"])
def test_zstd_table_carriers(name, gpu):
    """Spans whose blocks (16 segments each) mix Raw_Blocks with compressed ones: the Huffman tree
    and the FSE tables must ride on the first COMPRESSED block that uses them (a raw block 0, a
    raw block between compressed ones, a literal-free block 0), later blocks reuse them (Treeless
    literals, Repeat_Mode tables), and repeat offsets never reach back across a raw block.  Text
    with literals above 128 takes the FSE-compressed weights description (RFC 8878 §4.2.1.2)."""
    chunks = table_carrier_chunks()
    host = np.concatenate(chunks)
    lens = [c.size for c in chunks]
    offs = list(np.cumsum([0] + lens[:-1]))
    out, oo, ol, ids = _compress(name, host, [int(o) for o in offs], lens, gpu)
    _check(name, host, [int(o) for o in offs], lens, out, oo, ol, ids)
    assert (ids != 0).all(), ol


@pytest.mark.parametrize("name", ["zstd", "zstd-best-compression", "zstd-fastest"])
def test_zstd_adversarial_spans(name, gpu):
    """Spans at the edges of the span writer's limits, each frame decoded by libzstd: the most
    sequences a span can hold (4-byte matches everywhere: up to 8,192 per span, 2,048 per block),
    the longest carries (a block's literals before its first sequence), matches reaching 32 KiB
    back, long matches across whole segments, skewed literals over all 256 byte values, and
    sequences whose offsets alternate (repeat-offset candidates that must not be taken)."""
    parts = adversarial_parts()
    host = np.concatenate(parts)
    lens = [p.size for p in parts]
    offs = [int(x) for x in np.cumsum([0] + lens[:-1])]
    out, oo, ol, ids = _compress(name, host, offs, lens, gpu)
    _check(name, host, offs, lens, out, oo, ol, ids)
