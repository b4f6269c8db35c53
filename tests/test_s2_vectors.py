"""CPU: hand-built S2 vectors for the device decoder (kcdc_decompress_chunks_device), and the
decoder's validity header run over them on the host under AddressSanitizer and UBSan
(tools/s2_decode_host.cpp through kopia_amd/csrc/kcdc_s2_format.h) before any of them reaches a GPU.

This file holds the vector builder: emitters for every element form (literals with the inline and
the 1..4-byte lengths, copy-1, copy-2, copy-4, the eight classes of S2's repeat), a framing
wrapper, and a plain-Python model decoder that defines the expected bytes and status of every
vector.  The model is restated from the published formats (the Snappy framing and block formats,
and klauspost/compress/s2's repeat extension: a copy-1 whose 11-bit offset is 0); no
klauspost-written stream exists here, so the repeat and copy-4 forms are pinned by these vectors
alone ("format, unpinned": DESIGN.md §2.7).  tests/test_gpu_decompress.py imports the vectors."""
import functools
import os
import struct
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from kopia_amd import _lib
from oracle import deflate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "s2-default"
MAX_BLOCK = 4 << 20
EBADMSG, EOVERFLOW, ENOMEM = _lib.KCDC_EBADMSG, _lib.KCDC_EOVERFLOW, _lib.KCDC_ENOMEM


# ------------------------------------------------------------------ element emitters
def uvarint(n):
    out = bytearray()
    while True:
        out.append((n & 127) | (128 if n >= 128 else 0))
        n >>= 7
        if not n:
            return bytes(out)


def literal(data, form=None):
    """form 0: the length in the tag (1..60); 1..4: that many length bytes after tag 60..63."""
    n = len(data)
    assert n >= 1
    if form is None:
        form = 0 if n <= 60 else 1 if n <= 256 else 2 if n <= 65536 else 3 if n <= 1 << 24 else 4
    if form == 0:
        assert n <= 60
        return bytes([(n - 1) << 2]) + bytes(data)
    return bytes([(59 + form) << 2]) + (n - 1).to_bytes(form, "little") + bytes(data)


def copy1(off, n):
    assert 4 <= n <= 11 and 1 <= off <= 2047
    return bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 255])


def copy2(off, n):
    assert 1 <= n <= 64 and 0 <= off <= 65535
    return bytes([2 | ((n - 1) << 2)]) + off.to_bytes(2, "little")


def copy4(off, n):
    assert 1 <= n <= 64 and 0 <= off < 1 << 32
    return bytes([3 | ((n - 1) << 2)]) + off.to_bytes(4, "little")


REPEAT_EXTRA = {5: 1, 6: 2, 7: 3}      # extension bytes of the repeat classes
REPEAT_BASE = {5: 8, 6: 260, 7: 65540}  # and the length they add to


def repeat(cls, ext=0):
    """A copy-1 with offset 0: the previous copy's offset; class 0..4 = lengths 4..8."""
    assert 0 <= cls <= 7
    return bytes([1 | (cls << 2), 0]) + ext.to_bytes(REPEAT_EXTRA.get(cls, 0), "little")


def repeat_len(cls, ext=0):
    return 4 + cls if cls < 5 else REPEAT_BASE[cls] + ext


def block(elements, declared):
    return uvarint(declared) + b"".join(elements)


# ------------------------------------------------------------------ framing
def mask(c):
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


def chunk(kind, payload):
    return bytes([kind]) + len(payload).to_bytes(3, "little") + payload


def data_chunk(blk, decoded, crc=None):
    return chunk(0x00, struct.pack("<I", mask(deflate.crc32c(decoded)) if crc is None else crc) + blk)


def raw_chunk(decoded):
    return chunk(0x01, struct.pack("<I", mask(deflate.crc32c(decoded))) + decoded)


IDENT_S2 = chunk(0xff, b"S2sTwO")
IDENT_SNAPPY = chunk(0xff, b"sNaPpY")


def content(stream, name=NAME):
    return deflate.header(name) + stream


# ------------------------------------------------------------------ the model decoder
class Corrupt(ValueError):
    pass


def model_block(blk):
    """One block (uvarint, elements) -> (bytes, whether a repeat was used); Corrupt on anything
    the format forbids."""
    want, i = 0, 0
    while True:
        if i >= len(blk) or i >= 5:
            raise Corrupt("uvarint")
        b = blk[i]
        want |= (b & 127) << (7 * i)
        i += 1
        if b < 128:
            break
    if want > MAX_BLOCK:
        raise Corrupt("block above 4 MiB")
    out, last, repeats = bytearray(), 0, False
    while i < len(blk):
        tag = blk[i]
        kind = tag & 3
        if kind == 0:
            f, h = tag >> 2, 1
            n = f + 1
            if f >= 60:
                nb = f - 59
                if i + 1 + nb > len(blk):
                    raise Corrupt("literal length past the input")
                n = int.from_bytes(blk[i + 1:i + 1 + nb], "little") + 1
                h = 1 + nb
            if i + h + n > len(blk) or len(out) + n > want:
                raise Corrupt("literal past the input or the declared length")
            out += blk[i + h:i + h + n]
            i += h + n
            continue
        if kind == 1:
            h = 2
            if i + h > len(blk):
                raise Corrupt("copy-1 past the input")
            cls = (tag >> 2) & 7
            n = 4 + cls
            off = ((tag >> 5) << 8) | blk[i + 1]
            if off == 0:
                repeats = True
                off = last
                extra = REPEAT_EXTRA.get(cls, 0)
                if i + h + extra > len(blk):
                    raise Corrupt("repeat past the input")
                if extra:
                    n = REPEAT_BASE[cls] + int.from_bytes(blk[i + 2:i + 2 + extra], "little")
                h += extra
        else:
            h = 3 if kind == 2 else 5
            if i + h > len(blk):
                raise Corrupt("copy past the input")
            n = 1 + (tag >> 2)
            off = int.from_bytes(blk[i + 1:i + h], "little")
        if off == 0 or off > len(out) or len(out) + n > want:
            raise Corrupt("offset 0, offset before the block, or copy past the declared length")
        if off >= n:
            out += out[len(out) - off:len(out) - off + n]
        else:  # the periodic extension
            pat = bytes(out[len(out) - off:])
            out += (pat * (n // off + 1))[:n]
        last = off
        i += h
    if len(out) != want:
        raise Corrupt("block ends short of its declared length")
    return bytes(out), repeats


def model_decode(blob, name, cap, room):
    """(status, bytes, repeats) of a content as include/kcdc.h states them: the framing walk
    first (its first failure in stream order), then every block and its CRC."""
    try:
        if len(blob) < 4 or blob[:4] != deflate.header(name):
            raise Corrupt("header ID")
        i, first, chunks, total = 4, True, [], 0
        while i < len(blob):
            if len(blob) - i < 4:
                raise Corrupt("truncated chunk header")
            kind, n = blob[i], int.from_bytes(blob[i + 1:i + 4], "little")
            i += 4
            if n > len(blob) - i:
                raise Corrupt("chunk past the end")
            body = blob[i:i + n]
            i += n
            if kind == 0xff:
                if body not in (b"S2sTwO", b"sNaPpY"):
                    raise Corrupt("identifier")
                first = False
                continue
            if first:
                raise Corrupt("no identifier first")
            if kind >= 0x80:
                continue
            if kind >= 0x02:
                raise Corrupt("reserved chunk type")
            if n < 4:
                raise Corrupt("no CRC")
            if kind == 0:
                dec, k = 0, 0
                while True:
                    if 4 + k >= n or k >= 5:
                        raise Corrupt("uvarint")
                    dec |= (body[4 + k] & 127) << (7 * k)
                    k += 1
                    if body[4 + k - 1] < 128:
                        break
            else:
                dec = n - 4
            if dec > MAX_BLOCK:
                raise Corrupt("block above 4 MiB")
            if total + dec > cap:
                return EOVERFLOW, b"", False
            if len(chunks) >= room:
                return ENOMEM, b"", False
            chunks.append((kind, body))
            total += dec
        if first:
            raise Corrupt("no identifier")
        out, repeats = [], False
        for kind, body in chunks:
            if kind == 0:
                dec, r = model_block(body[4:])
                repeats = repeats or r
            else:
                dec = body[4:]
            if mask(deflate.crc32c(dec)) != struct.unpack("<I", body[:4])[0]:
                raise Corrupt("CRC")
            out.append(dec)
        return 0, b"".join(out), repeats
    except Corrupt:
        return EBADMSG, b"", False


def room_for(cap):
    """The descriptors a content gets in a workspace of the minimum size."""
    return 1 + (cap >> 14)


# ------------------------------------------------------------------ data
def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def mixed(nbytes, seed):
    """Random, zero, periodic and word-salad stretches (test_gpu_compress._mixed, restated)."""
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
    return b"".join(out)[:nbytes]


# ------------------------------------------------------------------ the vectors
Vector = namedtuple("Vector", "id name blob cap status expected repeats")


def one_block(elements, name=NAME):
    """A content of one compressed block made of `elements`; the model says what it decodes to."""
    body = b"".join(elements)
    n = produced(elements)
    blk = uvarint(n) + body
    decoded, _ = model_block(blk)
    return content(IDENT_S2 + data_chunk(blk, decoded), name)


def produced(elements):
    """Bytes a list of well-formed elements decodes to (from their tags alone)."""
    n = 0
    for e in elements:
        tag, kind = e[0], e[0] & 3
        if kind == 0:
            f = tag >> 2
            n += f + 1 if f < 60 else int.from_bytes(e[1:1 + f - 59], "little") + 1
        elif kind == 1 and ((tag >> 5) << 8 | e[1]) == 0:
            cls = (tag >> 2) & 7
            n += repeat_len(cls, int.from_bytes(e[2:], "little") if cls >= 5 else 0)
        elif kind == 1:
            n += 4 + ((tag >> 2) & 7)
        else:
            n += 1 + (tag >> 2)
    return n


def snappy_framed(data, block_size=1 << 16, ident=None):
    """Google's Snappy blocks (through pyarrow's codec) in the Snappy framing format (or, with
    S2's identifier, in blocks above Snappy's 64 KiB)."""
    import pyarrow as pa
    codec = pa.Codec("snappy")
    out = [IDENT_SNAPPY if ident is None else ident]
    for i in range(0, len(data), block_size):
        part = data[i:i + block_size]
        out.append(data_chunk(codec.compress(part, asbytes=True), part))
    return b"".join(out)


def valid(vid, blob, name=NAME):
    status, expected, repeats = model_decode(blob, name, 1 << 40, 1 << 40)
    assert status == 0, (vid, status)
    cap = len(expected)
    assert model_decode(blob, name, cap, room_for(cap))[0] == 0, f"{vid}: more chunks than a minimum workspace holds"
    return Vector(vid, name, blob, cap, 0, expected, repeats)


@functools.lru_cache(maxsize=None)
def valid_vectors():
    v = []
    # literal length forms
    for n in (1, 60, 61, 256, 257, 65536, 65537):
        v.append(valid(f"literal-{n}", one_block([literal(rand(n, n))])))
    for form in (1, 2, 3, 4):
        v.append(valid(f"literal-300-in-{form}-length-bytes", one_block([literal(rand(40, form), form), literal(rand(300, form), max(form, 2))])))
    v.append(valid("literal-1000-in-4-length-bytes", one_block([literal(rand(1000, 9), 4)])))
    # copy-1 / copy-2 at their smallest and largest lengths and offsets
    for n in (4, 11):
        for off in (1, 2047):
            v.append(valid(f"copy1-len{n}-off{off}", one_block([literal(rand(2047, 1)), copy1(off, n), literal(b"z")])))
    for n in (1, 64):
        for off in (1, 65535):
            v.append(valid(f"copy2-len{n}-off{off}", one_block([literal(rand(65535, 2)), copy2(off, n), literal(b"z")])))
    # copy-4 in a block of exactly 1 MiB
    big = 1 << 20
    v.append(valid("copy4-off65536-and-near-1MiB", one_block(
        [literal(rand(big - 128, 3)), copy4(65536, 64), copy4(big - 100, 64)])))
    # overlapping copies either side of the wave width; 65 and 300 bytes through a repeat
    for off in (1, 2, 3, 63, 64, 65, 127):
        for n in (64, 65, 300):
            el = [literal(rand(127, off))]
            if n == 64:
                el.append(copy2(off, 64))
            elif n == 65:
                el += [copy2(off, 1), repeat(5, 65 - 8)]
            else:
                el += [copy2(off, 1), repeat(6, 300 - 260)]
            v.append(valid(f"overlap-off{off}-len{n}", one_block(el + [literal(b"end")])))
    # every repeat class at its smallest and largest extension (class 7's largest, 65540 + 2^24 - 1,
    # exceeds any block: it is a corrupt vector, and the 4 MiB block below carries the largest that fits)
    for cls in range(5):
        v.append(valid(f"repeat-class{cls}", one_block([literal(rand(100, cls)), copy1(7, 4), repeat(cls)])))
    for cls, top in ((5, 255), (6, 65535)):
        for ext in (0, top):
            v.append(valid(f"repeat-class{cls}-ext{ext}", one_block([literal(rand(100, cls)), copy1(7, 4), repeat(cls, ext)])))
    v.append(valid("repeat-class7-ext0", one_block([literal(rand(100, 7)), copy1(7, 4), repeat(7, 0)])))
    v.append(valid("repeat-after-copy2", one_block([literal(rand(100, 11)), copy2(90, 10), repeat(3), literal(b"q")])))
    v.append(valid("repeat-after-copy4", one_block([literal(rand(100, 12)), copy4(50, 10), repeat(5, 100)])))
    v.append(valid("repeat-after-repeat", one_block([literal(rand(100, 13)), copy1(33, 5), repeat(2), literal(b"mid"),
                                                     repeat(5, 3), repeat(0)])))
    # block lengths either side of 32 KiB, and a multi-block stream of another writer (64 KiB blocks)
    m = mixed(200000, 21)
    for n in (32768, 32769):
        v.append(valid(f"block-{n}", content(deflate.s2_encode(m[:n]))))
    v.append(valid("s2_encode-200000", content(deflate.s2_encode(m))))
    v.append(valid("snappy-framed-200000", content(snappy_framed(m), "s2-better"), "s2-better"))
    # other chunk types among the data: skippable, uncompressed, padding, a second identifier
    import pyarrow as pa
    a, b, c = m[:20000], rand(20000, 5), m[100000:120000]
    codec = pa.Codec("snappy")
    v.append(valid("mixed-chunk-types", content(
        IDENT_S2 + chunk(0x80, b"skip me") + data_chunk(codec.compress(a, asbytes=True), a) + raw_chunk(b) +
        chunk(0xfe, bytes(13)) + IDENT_S2 + data_chunk(codec.compress(c, asbytes=True), c) + chunk(0xfd, b"") +
        chunk(0x99, rand(300, 6)))))
    v.append(valid("identifier-only", content(IDENT_S2)))
    v.append(valid("empty-block", content(IDENT_S2 + data_chunk(uvarint(0), b""))))
    # one 4 MiB block (the CRC is combined from 128 pieces): class 7's largest extension that fits
    head = [literal(rand(300000, 8)), copy4(300000, 64)]
    v.append(valid("block-4MiB", one_block(head + [repeat(7, MAX_BLOCK - 300064 - 65540)])))
    assert len({x.id for x in v}) == len(v)
    return tuple(v)


def _bad_block(blk, crc_of=b""):
    return content(IDENT_S2 + data_chunk(blk, crc_of))


@functools.lru_cache(maxsize=None)
def corrupt_vectors():
    text = b"hello world, hello world, hello world"
    good_blk = block([literal(text[:13]), copy1(13, 11), copy1(13, 11), literal(text[35:])], len(text))
    assert model_block(good_blk)[0] == text
    good = content(IDENT_S2 + data_chunk(good_blk, text))
    assert model_decode(good, NAME, len(text), 1)[:2] == (0, text)
    flip = lambda blob, at, bit=1: blob[:at] + bytes([blob[at] ^ bit]) + blob[at + 1:]  # noqa: E731
    lit8 = literal(b"abcdefgh")
    v = [
        ("wrong-header-id", content(IDENT_S2 + data_chunk(good_blk, text), "s2-better"), 64, EBADMSG),
        ("no-identifier", content(data_chunk(good_blk, text)), 64, EBADMSG),
        ("bad-identifier", content(chunk(0xff, b"S2sTwo") + data_chunk(good_blk, text)), 64, EBADMSG),
        ("truncated-chunk-header", good + b"\x00\x05", 64, EBADMSG),
        ("chunk-past-the-end", good[:-3], 64, EBADMSG),
        ("chunk-type-02", good + chunk(0x02, b"abc"), 64, EBADMSG),
        ("crc-bit", flip(good, 4 + len(IDENT_S2) + 4, 0x10), 64, EBADMSG),
        ("data-bit", flip(good, 4 + len(IDENT_S2) + 8 + 3, 0x04), 64, EBADMSG),
        ("length-above-cap", good, len(text) - 1, EOVERFLOW),
        ("length-above-4MiB", _bad_block(block([lit8], MAX_BLOCK + 1)), 5 << 20, EBADMSG),
        ("literal-past-block-end", _bad_block(uvarint(10) + literal(b"0123456789")[:6]), 64, EBADMSG),
        ("literal-length-bytes-past-block-end", _bad_block(uvarint(300) + bytes([61 << 2, 0x2b])), 512, EBADMSG),
        ("repeat-first", _bad_block(block([lit8, repeat(0)], 12)), 64, EBADMSG),
        ("copy2-offset-0", _bad_block(block([lit8, copy2(0, 4)], 12)), 64, EBADMSG),
        ("copy4-offset-0", _bad_block(block([lit8, copy4(0, 4)], 12)), 64, EBADMSG),
        ("offset-beyond-decoded", _bad_block(block([lit8, copy2(9, 4)], 12)), 64, EBADMSG),
        ("copy-past-block-end", _bad_block(block([lit8], 12) + copy2(4, 4)[:2]), 64, EBADMSG),
        ("element-past-declared-length", _bad_block(block([lit8, copy2(4, 4)], 10)), 64, EBADMSG),
        ("block-short-of-declared-length", _bad_block(block([lit8], 20)), 64, EBADMSG),
        ("uvarint-6-bytes", _bad_block(b"\x88\x80\x80\x80\x80\x00" + lit8), 64, EBADMSG),
        ("repeat-class7-largest-extension", _bad_block(block([literal(rand(100, 7)), copy1(7, 4), repeat(7, 0xFFFFFF)],
                                                             MAX_BLOCK)), MAX_BLOCK, EBADMSG),
        ("1000-chunks-in-a-minimum-workspace",
         content(IDENT_S2 + b"".join(data_chunk(block([literal(bytes([k & 255]))], 1), bytes([k & 255]))
                                     for k in range(1000))), 1000, ENOMEM),
    ]
    out = []
    for vid, blob, cap, status in v:
        got = model_decode(blob, NAME, cap, room_for(cap))
        assert got[0] == status, (vid, got[0])
        out.append(Vector(vid, NAME, blob, cap, status, b"", False))
    assert len({x.id for x in out}) == len(out)
    return tuple(out)


# ------------------------------------------------------------------ the host program
def write_vector_file(path, vectors):
    with open(path, "wb") as f:
        f.write(b"S2VEC1\0\0" + struct.pack("<I", len(vectors)))
        for v in vectors:
            f.write(struct.pack("<IQQiQ", deflate.HEADER_IDS[v.name], v.cap, room_for(v.cap), v.status, len(v.blob)))
            f.write(v.blob)
            f.write(struct.pack("<Q", len(v.expected)))
            f.write(v.expected)


@functools.lru_cache(maxsize=None)
def run_host_program():
    """Build tools/s2_decode_host.cpp with -fsanitize=address,undefined, run every vector through
    it, and return {vector id: (status, decoded length, matched)}.  Raises if a sanitizer fired or
    any vector missed its expectation: no vector goes to a GPU before this has passed."""
    import tempfile
    subprocess.run(["make", "-s", "-C", ROOT, "build/s2_decode_host"], check=True)
    vectors = valid_vectors() + corrupt_vectors()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vectors.bin")
        write_vector_file(path, vectors)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([os.path.join(ROOT, "build", "s2_decode_host"), path], capture_output=True, text=True, env=env)
    assert r.returncode == 0, f"s2_decode_host failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(vectors)
    out = {}
    for v, line in zip(vectors, lines):
        w = line.split()
        out[v.id] = (int(w[2]), int(w[4]), w[5] == "ok")
    return out


# ------------------------------------------------------------------ tests
def test_model_and_oracle_agree_without_repeats():
    """The oracle (oracle/s2_oracle.c: the Snappy subset) decodes every vector that uses no repeat
    to the model's bytes, and refuses every one that does."""
    seen = 0
    for v in valid_vectors():
        if v.repeats:
            with pytest.raises(ValueError):
                deflate.decompress(v.name, v.blob)
            continue
        assert deflate.decompress(v.name, v.blob) == v.expected, v.id
        seen += 1
    assert seen >= 30 and any(v.repeats for v in valid_vectors())


def test_oracle_refuses_every_corrupt_vector():
    """Cap and workspace are not the oracle's business: those two vectors it decodes."""
    for v in corrupt_vectors():
        if v.status == EBADMSG:
            with pytest.raises(ValueError):
                deflate.decompress(v.name, v.blob)
        else:
            assert len(deflate.decompress(v.name, v.blob)) > v.cap or v.status == ENOMEM, v.id


def test_emitters_cover_every_form():
    """Every literal length form, every copy kind and all eight repeat classes occur in the valid
    vectors (read back from the blocks' tags by the model's walk, not from the builder's calls)."""
    tags = set()
    for v in valid_vectors():
        if v.id.startswith(("literal", "copy", "repeat", "overlap", "block-4MiB")):
            blob = v.blob[4 + len(IDENT_S2):]
            blk = blob[8:]
            i = len(uvarint(len(v.expected)))
            while i < len(blk):
                tag, kind = blk[i], blk[i] & 3
                if kind == 0:
                    f = tag >> 2
                    nb = max(f - 59, 0)
                    tags.add(("literal", nb))
                    i += 1 + nb + (f + 1 if f < 60 else int.from_bytes(blk[i + 1:i + 1 + nb], "little") + 1)
                elif kind == 1 and ((tag >> 5) << 8 | blk[i + 1]) == 0:
                    cls = (tag >> 2) & 7
                    tags.add(("repeat", cls))
                    i += 2 + REPEAT_EXTRA.get(cls, 0)
                else:
                    tags.add(("copy", kind))
                    i += {1: 2, 2: 3, 3: 5}[kind]
    assert tags >= {("literal", k) for k in range(5)} | {("copy", k) for k in (1, 2, 3)} | {("repeat", k) for k in range(8)}


def test_host_program_decodes_every_valid_vector():
    res = run_host_program()
    for v in valid_vectors():
        assert res[v.id] == (0, len(v.expected), True), v.id


def test_host_program_refuses_every_corrupt_vector():
    res = run_host_program()
    for v in corrupt_vectors():
        assert res[v.id] == (v.status, 0, True), v.id


def test_decompression_symbols_declared():
    syms = _lib.exported_symbols()
    for s in ("kcdc_decompression_algorithms", "kcdc_decompress_workspace_size", "kcdc_decompress_chunks_device"):
        assert s in syms and hasattr(_lib.lib(), s), s
    from kopia_amd import compression as kc
    assert kc.DecompressibleAlgorithms() == sorted(deflate.S2_NAMES)
    assert set(kc.DecompressibleAlgorithms()) <= set(kc.SupportedAlgorithms())
    # one 32-byte descriptor per content and per 16 KiB of output room, beyond the fixed fields
    ws = _lib.lib().kcdc_decompress_workspace_size
    assert ws(0, 1 << 20, 3) - ws(0, 0, 3) == 64 * 32
    assert ws(0, 0, 1) >= 32


def test_argument_errors_need_no_device():
    """Unknown names and compressors without a device decoder are refused before any device is
    touched; without a device an s2 name fails loudly (no CPU fallback)."""
    L = _lib.lib()
    args = [None] * 3 + [0] + [None] * 6 + [0, None]
    assert L.kcdc_decompress_chunks_device(b"no-such-compressor", *args) == _lib.KCDC_ENOENT
    for name in ("deflate-default", "gzip", "pgzip-best-speed", "zstd"):
        assert L.kcdc_decompress_chunks_device(name.encode(), *args) == _lib.KCDC_EINVAL
        assert name in _lib.last_error()
    if L.kcdc_device_count() == 0:
        assert L.kcdc_decompress_chunks_device(b"s2-default", *args) == _lib.KCDC_ENODEV
