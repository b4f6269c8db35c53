"""Vectors for the device inflate (kcdc_inflate_chunks_device): streams from a foreign writer
(Python's zlib: every block type, level, strategy and flush mode) and hand-built streams at the
decoder's seams, valid and corrupt.  A module, not a test: tests/test_inflate_vectors.py checks its
conditions and runs every vector through the sanitizer-built host program
(tools/inflate_host.cpp), tests/test_gpu_inflate.py sends them to the device.

Holds an LSB-first bit writer, a canonical-code builder, emitters for the three block types and a
model of the contract in include/kcdc.h (header ID, members, trailers, cap) over
tests/deflate_model.py's inflate.  The expected bytes of every valid vector come from zlib, never
from the code under test, and every corrupt vector (but the cap and header-ID ones, which are this
library's own rules) is one that zlib refuses too.  Cases where zlib and Go's readers differ
(reserved FLG bits, a missing length for symbol 256, ...) are left out: nothing here can arbitrate
them."""
import functools
import os
import struct
import subprocess
import zlib
from collections import namedtuple

import deflate_model as dm
from kopia_amd import _lib
from oracle import deflate
from test_s2_vectors import mixed, rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBADMSG, EOVERFLOW = _lib.KCDC_EBADMSG, _lib.KCDC_EOVERFLOW
RAW, GZ, PGZ = "deflate-default", "gzip", "pgzip-best-speed"
FAMILIES = (RAW, GZ, PGZ)
NINE = sorted(["deflate-best-speed", "deflate-default", "deflate-best-compression", "gzip", "gzip-best-speed",
               "gzip-best-compression", "pgzip", "pgzip-best-speed", "pgzip-best-compression"])
SIZES = (0, 1, 300, (64 << 10) + 1, (1 << 20) + 3)
MAX_DECODED = (1 << 20) + 3

Vector = namedtuple("Vector", "id name blob cap status expected")


def is_gz(name):
    return not name.startswith("deflate")


# ------------------------------------------------------------------ bits and codes
class Bits:
    """LSB-first bit writer (RFC 1951 3.1.1): fields low bit first, Huffman codes high bit first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, v, n):
        assert 0 <= v < 1 << n
        self.acc |= v << self.n
        self.n += n

    def code(self, c):
        code, n = c
        self.bits(int(format(code, f"0{n}b")[::-1], 2), n)

    def align(self):
        self.n = (self.n + 7) & ~7

    def raw(self, data):
        assert self.n % 8 == 0
        for b in data:
            self.bits(b, 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canon(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2)."""
    out, code = {}, 0
    for n in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


def complete(symbols, size):
    """Lengths (a list of `size`) of a complete code over `symbols` (two or more), near-balanced."""
    k = len(symbols)
    assert k >= 2
    m = (k - 1).bit_length()
    lens = [0] * size
    for i, s in enumerate(sorted(symbols)):
        lens[s] = m - 1 if i < (1 << m) - k else m
    return lens


FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canon([5] * 32)


def len_sym(n):
    if n == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if dm.LEN_BASE[i] <= n)
    return 257 + s, n - dm.LEN_BASE[s], dm.LEN_EXTRA[s]


def dist_sym(d):
    s = max(i for i in range(30) if dm.DIST_BASE[i] <= d)
    return s, d - dm.DIST_BASE[s], dm.DIST_EXTRA[s]


def tokens(w, toks, lit, dist, eob=True):
    """Literal bytes (ints), matches (length, distance) and raw symbols ("L", sym) / ("D", sym)."""
    for t in toks:
        if isinstance(t, int):
            w.code(lit[t])
        elif t[0] == "L":
            w.code(lit[t[1]])
        elif t[0] == "D":
            w.code(dist[t[1]])
        else:
            s, x, xb = len_sym(t[0])
            w.code(lit[s])
            w.bits(x, xb)
            s, x, xb = dist_sym(t[1])
            w.code(dist[s])
            w.bits(x, xb)
    if eob:
        w.code(lit[256])


def fixed(w, toks, final=True, eob=True):
    w.bits(final, 1)
    w.bits(1, 2)
    tokens(w, toks, FIXED_LIT, FIXED_DIST, eob)


def stored(w, data, final=True, nlen=None):
    w.bits(final, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    w.raw(data)


CL_LENS = [4] * 13 + [5] * 6  # a complete code over all 19 code-length symbols
CL_CODE = canon(CL_LENS)


def rle(seq):
    """Code-length symbols (symbol, extra value) for the lengths, runs wherever they pay."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


def dynamic(w, lit_lens, dist_lens, toks, final=True, eob=True, cl_syms=None, hlit=None, hdist=None, body=True):
    """A dynamic block: lit_lens (257..288 lengths) and dist_lens (1..32) as given, the header's
    lengths run-length coded over their concatenation (so a run may cross from one to the other)."""
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
    w.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
    w.bits(19 - 4, 4)
    for s in dm.CL_ORDER:
        w.bits(CL_LENS[s], 3)
    for s, x in rle(list(lit_lens) + list(dist_lens)) if cl_syms is None else cl_syms:
        w.code(CL_CODE[s])
        if s >= 16:
            w.bits(x, dm.CL_EXTRA[s])
    if body:
        tokens(w, toks, canon(lit_lens), canon(dist_lens), eob)


def content(name, stream):
    return deflate.header(name) + stream


def gzip_member(raw, data, flg=0, extra=b"", fname=b"", comment=b"", crc=None, isize=None, magic=b"\x1f\x8b", cm=8,
                hcrc=None):
    h = magic + bytes([cm, flg]) + bytes(4) + b"\x00\xff"
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += fname + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) if hcrc is None else hcrc)
    return h + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc,
                                 (len(data) & 0xFFFFFFFF) if isize is None else isize)


# ------------------------------------------------------------------ zlib: the reference decoder
def zlib_decode(name, blob):
    """(bytes, clean): what zlib makes of the stream after the header ID; clean is False when zlib
    raises, or ends without reaching a final block or a whole trailer."""
    data, out = blob[4:], b""
    try:
        if not is_gz(name):
            d = zlib.decompressobj(-15)
            out = d.decompress(data)
            return out, d.eof
        while True:
            d = zlib.decompressobj(31)
            out += d.decompress(data)
            if not d.eof:
                return out, False
            data = d.unused_data
            if not data:
                return out, True
    except zlib.error:
        return out, False


# ------------------------------------------------------------------ the model of the contract
def model(name, blob, cap):
    """(status, bytes) as include/kcdc.h states them, over tests/deflate_model.py's inflate (which
    follows zlib: the vectors avoid the cases where Go differs)."""
    try:
        if len(blob) < 4 or blob[:4] != deflate.header(name):
            raise dm.InflateError("header ID")
        out, pos = b"", 4

        def raw_at(pos):
            part, blocks = dm.inflate_blocks(blob[pos:])
            return part, pos + (blocks[-1].bit_off + blocks[-1].bit_len + 7) // 8

        if not is_gz(name):
            out, pos = raw_at(pos)
        else:
            while True:
                h = blob[pos:pos + 10]
                if len(h) < 10 or h[:3] != b"\x1f\x8b\x08":
                    raise dm.InflateError("member header")
                flg, i = h[3], pos + 10
                if flg & 4:
                    if len(blob) - i < 2:
                        raise dm.InflateError("FEXTRA")
                    i += 2 + int.from_bytes(blob[i:i + 2], "little")
                for f in (8, 16):
                    if flg & f:
                        z = blob.find(b"\0", i)
                        if z < 0:
                            raise dm.InflateError("FNAME / FCOMMENT")
                        i = z + 1
                if flg & 2:
                    if len(blob) - i < 2 or int.from_bytes(blob[i:i + 2], "little") != zlib.crc32(blob[pos:i]) & 0xFFFF:
                        raise dm.InflateError("FHCRC")
                    i += 2
                if i > len(blob):
                    raise dm.InflateError("member header past the end")
                part, pos = raw_at(i)
                if len(blob) - pos < 8:
                    raise dm.InflateError("trailer")
                crc, isize = struct.unpack("<II", blob[pos:pos + 8])
                if crc != zlib.crc32(part) or isize != len(part) & 0xFFFFFFFF:
                    raise dm.InflateError("CRC-32 / ISIZE")
                out += part
                pos += 8
                if pos == len(blob):
                    break
    except dm.InflateError:
        return EBADMSG, b""
    return (EOVERFLOW, b"") if len(out) > cap else (0, out)


# ------------------------------------------------------------------ foreign writer
def zlib_stream(name, data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flush=False):
    c = zlib.compressobj(level, zlib.DEFLATED, 31 if is_gz(name) else -15, mem, strategy)
    if not flush:
        return c.compress(data) + c.flush()
    a, b = len(data) // 3, 2 * len(data) // 3
    return (c.compress(data[:a]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[a:b]) + c.flush(zlib.Z_FULL_FLUSH) +
            c.compress(data[b:]) + c.flush())


@functools.lru_cache(maxsize=None)
def foreign_vectors():
    out = []
    for name in FAMILIES:
        for size in SIZES:
            data = mixed(size + 1, 7 + size % 11)[:size]
            kinds = [(f"level{lv}", data, dict(level=lv)) for lv in (1, 6, 9, 0)]
            kinds += [("fixed", data, dict(strategy=zlib.Z_FIXED)), ("huffman-only", data, dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                      ("rle", data, dict(strategy=zlib.Z_RLE)), ("memlevel1", data, dict(mem=1)),
                      ("flushes", data, dict(flush=True)), ("random", rand(size, 3), {}), ("zeros", bytes(size), {})]
            for kind, d, kw in kinds:
                blob = content(name, zlib_stream(name, d, **kw))
                out.append(Vector(f"zlib-{name}-{kind}-{size}", name, blob, len(d), 0, d))
    return tuple(out)


# ------------------------------------------------------------------ hand-built, valid
def _valid(vid, name, stream):
    blob = content(name, stream)
    expected, clean = zlib_decode(name, blob)
    assert clean, vid
    return Vector(vid, name, blob, len(expected), 0, expected)


def _phase_prefix(w, phase):
    """Non-final fixed blocks of 10 bits (empty) and 19 bits (one 9-bit literal) until the next
    block header starts at the given bit phase."""
    for nine in range(8):
        for empty in range(8):
            if (19 * nine + 10 * empty) % 8 == phase:
                for _ in range(nine):
                    fixed(w, [200], final=False)
                for _ in range(empty):
                    fixed(w, [], final=False)
                return
    raise AssertionError(phase)


@functools.lru_cache(maxsize=None)
def built_valid_vectors():
    v = []
    text = list(rand(40, 11))
    w = Bits()
    fixed(w, text + [(n, 7) for n in (3, 10, 11, 257, 258)])
    v.append(_valid("match-lengths-3-10-11-257-258", RAW, w.bytes()))
    w = Bits()
    fixed(w, [120, (258, 1)])
    v.append(_valid("distance-1-length-258", RAW, w.bytes()))
    for d in (63, 64, 65):
        w = Bits()
        fixed(w, list(rand(100, d)) + [(d - 10, d), (d + 30, d), (d, d), (258, d)])
        v.append(_valid(f"distance-{d}-lengths-either-side", RAW, w.bytes()))
    w = Bits()
    stored(w, rand(32768, 12), final=False)
    fixed(w, [(100, 32768), 7, (258, 32768)])
    v.append(_valid("distance-32768-from-byte-32768", RAW, w.bytes()))
    w = Bits()
    fixed(w, [1, 2, 3, 4, 5, (20, 5), (33, 25)])
    v.append(_valid("distance-equal-to-produced", RAW, w.bytes()))
    w = Bits()
    stored(w, rand(50, 13), final=False)
    lits = sorted(set(rand(30, 14)))
    dynamic(w, complete(lits + [256], 257), [0], list(rand(30, 14)), final=False)
    fixed(w, [(30, 75), (10, 20), (40, 120)])
    v.append(_valid("fixed-match-into-stored-and-dynamic", RAW, w.bytes()))
    # a 15-bit code: lengths 1..14 on fourteen literals, 15 on the end of block and on length 3
    ll = [0] * 258
    for k in range(14):
        ll[65 + k] = k + 1
    ll[256] = ll[257] = 15
    w = Bits()
    dynamic(w, ll, [1], [65 + k for k in range(14)] * 3 + [(3, 1), 78, (3, 1)])
    v.append(_valid("dynamic-15-bit-code", RAW, w.bytes()))
    w = Bits()
    dynamic(w, complete([97, 98, 256, 260], 261), [0, 0, 1], [97, 98, 97, (6, 3), 98])
    v.append(_valid("dynamic-single-one-bit-distance-code", RAW, w.bytes()))
    w = Bits()
    dynamic(w, complete([97, 98, 99, 256], 257), [0], [97, 98, 99, 99, 98])
    v.append(_valid("dynamic-no-distance-code", RAW, w.bytes()))
    w = Bits()  # lengths 2 at the end of the literal/length lengths and the start of the distance lengths: one 16 run
    ll = complete([97, 98, 256, 285], 286)
    syms = rle(ll + [2, 2, 2, 2])
    assert syms[-2:] == [(2, 0), (16, 1)]
    dynamic(w, ll, [2, 2, 2, 2], [97, (258, 1), 98, (258, 4), (258, 2), (258, 3)])
    v.append(_valid("length-run-16-crosses-into-distances", RAW, w.bytes()))
    w = Bits()  # zeros at the end of 260 literal/length lengths and the start of the distance lengths: one 17 run
    ll = complete([97, 256, 257], 258) + [0, 0]
    syms = rle(ll + [0, 0, 0, 0, 1])
    assert syms[-2:] == [(17, 3), (1, 0)] and any(s == 18 for s, _ in syms)
    dynamic(w, ll, [0, 0, 0, 0, 1], [97] * 6 + [(3, 5), (3, 6)])
    v.append(_valid("length-runs-17-18-cross-into-distances", RAW, w.bytes()))
    w = Bits()
    fixed(w, [104, 105, (9, 2)], final=False)
    stored(w, b"")
    v.append(_valid("empty-final-stored-block", RAW, w.bytes()))
    w = Bits()
    fixed(w, [33], final=False)
    stored(w, rand(65535, 20), final=False)
    fixed(w, [(258, 65535 - 40000), 34])
    v.append(_valid("stored-block-65535", RAW, w.bytes()))
    w = Bits()
    fixed(w, list(rand(65, 15)) + [(70, 65), 9, (5, 1)])
    v.append(_valid("65-literals-then-a-match", RAW, w.bytes()))
    for phase in range(8):
        w = Bits()
        _phase_prefix(w, phase)
        assert w.n % 8 == phase
        stored(w, rand(37, 16 + phase), final=False)
        fixed(w, [(37, 37), 1])
        v.append(_valid(f"stored-block-at-bit-phase-{phase}", RAW, w.bytes()))
    data = mixed(5000, 17)[:5000]
    raw = zlib_stream(RAW, data)
    v.append(_valid("gzip-fextra-fname-fcomment-fhcrc", GZ,
                    gzip_member(raw, data, flg=2 | 4 | 8 | 16, extra=b"\x41\x42\x03\x00xyz", fname=b"name.bin", comment=b"a comment")))
    d2 = mixed(70000, 18)[:70000]
    v.append(_valid("gzip-two-members", GZ, gzip_member(raw, data) + gzip_member(zlib_stream(RAW, d2), d2)))
    v.append(_valid("gzip-empty-member", GZ, gzip_member(zlib_stream(RAW, b""), b"")))
    v.append(_valid("gzip-empty-member-after-data", PGZ, gzip_member(raw, data) + gzip_member(zlib_stream(RAW, b""), b"")))
    v.append(_valid("literal-run-100-fixed", RAW, literal_run_fixed()))
    v.append(_valid("literal-run-100-sub-table-codes", RAW, literal_run_long_codes()))
    v.append(_valid("raw-stream-then-5-junk-bytes", RAW, raw + b"\xde\xad\xbe\xef\x00"))
    assert len({x.id for x in v}) == len(v)
    return tuple(v)


RUN = 100


def literal_run_fixed():
    """A fixed block of 100 literals, 8-bit and 9-bit codes mixed."""
    w = Bits()
    fixed(w, [(37 * k) & 255 for k in range(RUN)])
    return w.bytes()


def literal_run_long_codes():
    """A dynamic block of 100 literals whose codes are 1 to 14 bits long (those above 9 bits sit
    in sub-tables), after the 15-bit end of block's neighbour: dynamic-15-bit-code's lengths."""
    ll = [0] * 258
    for k in range(14):
        ll[65 + k] = k + 1
    ll[256] = ll[257] = 15
    w = Bits()
    dynamic(w, ll, [1], [65 + (5 * k) % 14 if k % 3 else 75 + k % 4 for k in range(RUN)])
    return w.bytes()


def valid_vectors():
    return foreign_vectors() + built_valid_vectors()


# ------------------------------------------------------------------ hand-built, corrupt
@functools.lru_cache(maxsize=None)
def corrupt_vectors():
    v = []

    def bad(vid, name, stream, cap=4096, status=EBADMSG, blob=None):
        v.append(Vector(vid, name, content(name, stream) if blob is None else blob, cap, status, b""))

    ok_ll, toks = complete([97, 98, 256, 257], 258), [97, 98, (3, 2)]

    def dyn(**kw):
        w = Bits()
        dynamic(w, kw.pop("ll", ok_ll), kw.pop("dl", [1, 1]), toks, **kw)
        return w.bytes()

    assert zlib_decode(RAW, content(RAW, dyn()))[1]
    # the refuse list
    bad("hlit-287", RAW, dyn(hlit=30, body=False) + bytes(64))
    bad("hdist-31", RAW, dyn(hdist=30, body=False) + bytes(64))
    over = [0] * 257
    over[97] = over[98] = over[256] = 1
    bad("over-subscribed-lengths", RAW, dyn(ll=over, body=False) + bytes(8))
    inc = [0] * 257
    inc[97] = inc[256] = 2
    bad("incomplete-lengths", RAW, dyn(ll=inc, body=False) + bytes(8))
    bad("incomplete-distance-lengths", RAW, dyn(dl=[2, 2, 2], body=False) + bytes(8))
    bad("code-16-with-no-previous-length", RAW, dyn(cl_syms=[(16, 0)] + rle(ok_ll + [1, 1]), body=False) + bytes(8))
    bad("length-run-past-hlit-plus-hdist", RAW, dyn(cl_syms=rle(ok_ll + [1]) + [(16, 3)], body=False) + bytes(8))
    for s in (286, 287):
        w = Bits()
        fixed(w, [97, 98, 99, ("L", s), ("D", 0)])
        bad(f"literal-length-symbol-{s}", RAW, w.bytes())
    for s in (30, 31):
        w = Bits()
        fixed(w, [97, 98, 99, ("L", 257), ("D", s)])
        bad(f"distance-symbol-{s}", RAW, w.bytes() + bytes(4))
    w = Bits()
    stored(w, b"stored bytes", nlen=(12 ^ 0xFFFF) ^ 0x100)
    bad("len-not-complement-of-nlen", RAW, w.bytes())
    w = Bits()
    fixed(w, [97], final=False)
    w.bits(1, 1)
    w.bits(3, 2)
    bad("btype-3", RAW, w.bytes() + bytes(4))
    w = Bits()
    fixed(w, [97, 98, 99, (3, 4)])
    bad("distance-beyond-produced", RAW, w.bytes())
    w = Bits()
    stored(w, b"abc", final=False)
    fixed(w, [(3, 4)])
    bad("distance-beyond-produced-across-blocks", RAW, w.bytes())
    # truncation at each structural point
    good_raw = zlib_stream(RAW, mixed(3000, 19)[:3000])
    bad("truncated-inside-the-id", RAW, b"", blob=deflate.header(RAW)[:2])
    bad("truncated-no-stream", RAW, b"")
    w = Bits()
    stored(w, b"", final=False)
    bad("truncated-at-the-block-header", RAW, w.bytes())
    for left in (2, 1):  # the content ends with two bits, and with one bit, of a 3-bit block header
        w = Bits()
        _phase_prefix(w, 8 - left)
        cut = (w.n + left) // 8
        assert w.n + left == 8 * cut
        fixed(w, [97])
        bad("truncated-inside-the-block-header" + ("" if left == 2 else "-1-bit"), RAW, w.bytes()[:cut])
    bad("truncated-inside-hclen-lengths", RAW, dyn()[:4])
    bad("truncated-inside-the-code-lengths", RAW, dyn()[:14])
    w = Bits()
    fixed(w, [97])
    bad("truncated-inside-a-symbol", RAW, w.bytes()[:1])
    for pad in range(8):
        w = Bits()
        w.bits(1, 1)
        w.bits(1, 2)
        tokens(w, [200] * pad, FIXED_LIT, FIXED_DIST, eob=False)  # 9-bit literals move the phase
        w.code(FIXED_LIT[281])  # length 131..162: 5 extra bits
        lo = w.n
        w.bits(17, 5)
        if lo < 8 * ((lo + 7) // 8) < w.n:
            bad("truncated-inside-extra-bits", RAW, w.bytes()[:(lo + 7) // 8])
            break
    else:
        raise AssertionError("no byte boundary inside the extra bits")
    w = Bits()
    stored(w, bytes(range(100)))
    bad("truncated-inside-a-stored-block", RAW, w.bytes()[:55])
    bad("truncated-inside-len-nlen", RAW, w.bytes()[:3])
    w = Bits()
    fixed(w, [97, 98, 99, 100, 101], eob=False)
    assert w.n % 8 == 3  # 43 bits; the last byte's padding is 00000: the start of a code, never an end of block
    bad("truncated-before-the-end-of-block", RAW, w.bytes())
    bad("truncated-zlib-stream", RAW, good_raw[:-1])
    data = mixed(3000, 19)[:3000]
    good_gz = gzip_member(good_raw, data)
    assert zlib_decode(GZ, content(GZ, good_gz)) == (data, True)
    bad("truncated-inside-the-gzip-header", GZ, good_gz[:5])
    bad("truncated-inside-fname", GZ, gzip_member(good_raw, data, flg=8, fname=b"name")[:13])
    bad("truncated-inside-the-trailer", GZ, good_gz[:-3])
    bad("truncated-no-trailer", PGZ, good_gz[:-8])
    # header IDs and families
    bad("wrong-header-id", RAW, b"", blob=content("deflate-best-speed", good_raw))
    bad("wrong-header-id-gzip", GZ, b"", blob=content(PGZ, good_gz))
    bad("gzip-member-under-a-deflate-name", RAW, good_gz)
    bad("raw-stream-under-a-gzip-name", GZ, good_raw)
    # members
    bad("gzip-bad-magic", GZ, gzip_member(good_raw, data, magic=b"\x1f\x8c"))
    bad("gzip-cm-7", GZ, gzip_member(good_raw, data, cm=7))
    hc = gzip_member(good_raw, data, flg=2)
    bad("gzip-bad-fhcrc", GZ, gzip_member(good_raw, data, flg=2, hcrc=(zlib.crc32(hc[:10]) & 0xFFFF) ^ 0x8000))
    bad("gzip-crc32-off-by-one-bit", GZ, gzip_member(good_raw, data, crc=zlib.crc32(data) ^ 0x00010000))
    bad("gzip-isize-off-by-one", PGZ, gzip_member(good_raw, data, isize=len(data) + 1))
    bad("gzip-data-bit-flipped", GZ, gzip_member(zlib_stream(RAW, data, level=0)[:200] + b"\x01" +
                                                 zlib_stream(RAW, data, level=0)[201:], data))
    bad("gzip-junk-after-the-trailer", GZ, good_gz + b"junk")
    bad("gzip-second-member-crc32", GZ, good_gz + gzip_member(good_raw, data, crc=zlib.crc32(data) ^ 1), cap=8192)
    w = Bits()
    fixed(w, [(10, 100), 1, 2])  # a distance that only the first member's bytes could serve
    bad("gzip-second-member-distance-into-the-first", GZ, good_gz + gzip_member(w.bytes(), data[-100:-90] + b"\1\2"), cap=8192)
    bad("gzip-second-member-truncated", GZ, good_gz + good_gz[:-1], cap=8192)
    # a cap one byte short: reached by a literal, by a match and by a stored block
    w = Bits()
    fixed(w, [97, 98, 99, (5, 3), 100])
    bad("cap-reached-by-a-literal", RAW, w.bytes(), cap=8, status=EOVERFLOW)
    w = Bits()
    fixed(w, [97, 98, 99, (5, 3)])
    bad("cap-reached-by-a-match", RAW, w.bytes(), cap=7, status=EOVERFLOW)
    w = Bits()
    fixed(w, [97, 98, 99], final=False)
    stored(w, b"0123456789")
    bad("cap-reached-by-a-stored-block", RAW, w.bytes(), cap=12, status=EOVERFLOW)
    # ... and by a literal inside a run of literals, which the decoder takes several at a time: the
    # third (the first one taken that way), one in the middle of a look, the 65th and the last
    for what, stream in (("fixed", literal_run_fixed()), ("sub-table-codes", literal_run_long_codes())):
        for k in (3, 6, 65, 100):
            bad(f"cap-reached-by-literal-{k}-of-a-run-{what}", RAW, stream, cap=k - 1, status=EOVERFLOW)
    bad("cap-reached-in-a-gzip-member", GZ, good_gz, cap=len(data) - 1, status=EOVERFLOW)
    bad("cap-zero", RAW, good_raw, cap=0, status=EOVERFLOW)
    assert len({x.id for x in v}) == len(v)
    return tuple(v)


def all_vectors():
    return valid_vectors() + corrupt_vectors()


# ------------------------------------------------------------------ the host program
def write_vector_file(path, vectors):
    with open(path, "wb") as f:
        f.write(b"INFVEC1\0" + struct.pack("<I", len(vectors)))
        for v in vectors:
            f.write(struct.pack("<IIQiQ", deflate.HEADER_IDS[v.name], int(is_gz(v.name)), v.cap, v.status, len(v.blob)))
            f.write(v.blob)
            f.write(struct.pack("<Q", len(v.expected)))
            f.write(v.expected)


@functools.lru_cache(maxsize=None)
def run_host_program():
    """Build tools/inflate_host.cpp with -fsanitize=address,undefined, run every vector through it,
    and return {vector id: (status, decoded length, matched)}.  Raises if a sanitizer fired or the
    program found a mismatch: no vector goes to a GPU before this has passed."""
    import tempfile
    subprocess.run(["make", "-s", "-C", ROOT, "build/inflate_host"], check=True)
    vectors = all_vectors()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vectors.bin")
        write_vector_file(path, vectors)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([os.path.join(ROOT, "build", "inflate_host"), path], capture_output=True, text=True, env=env)
    bad = [f"{v.id}: {line}" for v, line in zip(vectors, r.stdout.splitlines()) if not line.endswith(" ok")]
    assert r.returncode == 0, f"inflate_host failed ({r.returncode}):\n" + "\n".join(bad[:40]) + "\n" + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(vectors)
    out = {}
    for v, line in zip(vectors, lines):
        w = line.split()
        out[v.id] = (int(w[2]), int(w[4]), w[5] == "ok")
    return out
