"""Vectors for the device zstd decoder (kcdc_zstd_decode_chunks_device): frames from a foreign
writer (libzstd through ctypes: levels, window sizes, checksums, content-size widths, flushes,
block splitting, uncompressed literals, several frames) and hand-built frames at the decoder's
seams, valid and corrupt.  A module, not a test: tests/test_zstd_vectors.py checks its conditions and
runs every vector through the sanitizer-built host program (tools/zstd_decode_host.cpp),
tests/test_gpu_zstd_decode.py sends them to the device.

The expected bytes of every valid vector come from libzstd's ZSTD_decompress, never from the code
under test, and every corrupt vector is one that libzstd refuses too, except where the rule is this
library's own (OWN_RULES).  tests/zstd_model.py, a decoder restated from RFC 8878, is the second
opinion and reads the vectors' structure."""
import ctypes as C
import functools
import os
import struct
import subprocess
from collections import namedtuple

import zstd_model as zm
from kopia_amd import _lib
from test_s2_vectors import mixed, rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBADMSG, EOVERFLOW, ENOMEM = _lib.KCDC_EBADMSG, _lib.KCDC_EOVERFLOW, _lib.KCDC_ENOMEM
FOUR = ["zstd", "zstd-best-compression", "zstd-better-compression", "zstd-fastest"]  # sorted
HEADER_IDS = {"zstd": 0x1100, "zstd-fastest": 0x1101, "zstd-better-compression": 0x1102, "zstd-best-compression": 0x1103}
SIZES = (0, 1, 300, (64 << 10) + 1, 128 << 10, (128 << 10) + 1, (1 << 20) + 3)
MAX_DECODED = (1 << 20) + 3
MAGIC = struct.pack("<I", 0xFD2FB528)

# extra: descriptors beyond the workspace rule's 4 + cap / 1 KiB (a larger work_bytes)
# why (corrupt vectors): what tests/zstd_model.py says when it refuses the stream; a vector refused for
# another reason than the one it is named for does not pass
Vector = namedtuple("Vector", "id name blob cap status expected extra why", defaults=(None,))

# ------------------------------------------------------------------ libzstd
Z = C.CDLL("libzstd.so.1")
Z.ZSTD_createCCtx.restype = C.c_void_p
Z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
Z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
Z.ZSTD_CCtx_setParameter.restype = C.c_size_t
Z.ZSTD_CCtx_setPledgedSrcSize.argtypes = [C.c_void_p, C.c_ulonglong]
Z.ZSTD_CCtx_setPledgedSrcSize.restype = C.c_size_t
Z.ZSTD_compressBound.argtypes = [C.c_size_t]
Z.ZSTD_compressBound.restype = C.c_size_t
Z.ZSTD_isError.argtypes = [C.c_size_t]
Z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
Z.ZSTD_decompress.restype = C.c_size_t
P_LEVEL, P_WINDOW_LOG, P_CONTENT_SIZE, P_CHECKSUM, P_LIT_MODE, P_TARGET_CBLOCK = 100, 101, 200, 201, 1002, 1003
E_CONTINUE, E_FLUSH, E_END = 0, 1, 2


class _Buf(C.Structure):  # ZSTD_inBuffer / ZSTD_outBuffer
    _fields_ = [("p", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


Z.ZSTD_compressStream2.argtypes = [C.c_void_p, C.POINTER(_Buf), C.POINTER(_Buf), C.c_int]
Z.ZSTD_compressStream2.restype = C.c_size_t


def zstd_frame(data, level=3, window_log=None, content_size=True, checksum=False, lit_mode=None, target_cblock=None,
               flush_at=(), streamed=False):
    """One frame by libzstd.  streamed: the input arrives before the end is announced, so the frame
    header holds no content size; flush_at: input positions at which the stream is flushed."""
    cctx = Z.ZSTD_createCCtx()
    try:
        params = [(P_LEVEL, level), (P_CONTENT_SIZE, int(content_size)), (P_CHECKSUM, int(checksum))]
        if window_log is not None:
            params.append((P_WINDOW_LOG, window_log))
        if lit_mode is not None:
            params.append((P_LIT_MODE, lit_mode))
        if target_cblock is not None:
            params.append((P_TARGET_CBLOCK, target_cblock))
        for k, v in params:
            assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(cctx, k, v)), (k, v)
        room = Z.ZSTD_compressBound(len(data)) + 64 * (len(flush_at) + 2) + (len(data) >> 6) + 1024
        dst = C.create_string_buffer(room)
        out = _Buf(C.cast(dst, C.c_void_p), room, 0)
        src = C.create_string_buffer(bytes(data), max(len(data), 1))
        cuts = sorted({min(c, len(data)) for c in flush_at}) + [len(data)]
        at = 0
        for i, cut in enumerate(cuts):
            inb = _Buf(C.cast(src, C.c_void_p), cut, at)
            final = i == len(cuts) - 1
            mode = E_FLUSH if not final else (E_CONTINUE if streamed else E_END)
            while True:
                r = Z.ZSTD_compressStream2(cctx, C.byref(out), C.byref(inb), mode)
                assert not Z.ZSTD_isError(r)
                if (mode == E_CONTINUE and inb.pos == cut) or (mode != E_CONTINUE and r == 0):
                    break
            at = cut
        if streamed:
            inb = _Buf(C.cast(src, C.c_void_p), len(data), len(data))
            while Z.ZSTD_compressStream2(cctx, C.byref(out), C.byref(inb), E_END) != 0:
                pass
        return dst.raw[:out.pos]
    finally:
        Z.ZSTD_freeCCtx(cctx)


def zstd_decode(stream, room=MAX_DECODED + 64):
    """(bytes, True) as ZSTD_decompress decodes `stream` (frames, no header ID), or (b"", False)."""
    dst = C.create_string_buffer(max(room, 1))
    src = C.create_string_buffer(bytes(stream), max(len(stream), 1))
    r = Z.ZSTD_decompress(dst, room, src, len(stream))
    if Z.ZSTD_isError(r):
        return b"", False
    return dst.raw[:r], True


def header(name):
    return struct.pack(">I", HEADER_IDS[name])


def content(name, stream):
    return header(name) + stream


def skippable(payload, nibble=0):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + payload


def _valid(vid, name, stream, extra=0):
    got, ok = zstd_decode(stream)
    assert ok, vid
    return Vector(vid, name, content(name, stream), len(got), 0, got, extra)


# ------------------------------------------------------------------ the foreign writer's frames
def periodic(n):
    return (bytes(range(251)) * (n // 251 + 1))[:n]


FOREIGN_KINDS = ("level-5", "level1", "level3", "level9", "level19", "random", "zeros", "checksum", "streamed",
                 "streamed-checksum", "windowlog10", "flushes", "targetcblock2000", "literals-off", "two-frames")


def foreign_stream(kind, size):
    data = mixed(size, 100 + size % 97)
    if kind.startswith("level"):
        return zstd_frame(data, level=int(kind[5:]))
    if kind == "random":
        return zstd_frame(rand(size, 7), checksum=True)
    if kind == "zeros":
        return zstd_frame(bytes(size))
    if kind == "checksum":
        return zstd_frame(data, checksum=True)
    if kind == "streamed":
        return zstd_frame(data, streamed=True)
    if kind == "streamed-checksum":
        return zstd_frame(data, streamed=True, checksum=True, level=1)
    if kind == "windowlog10":
        return zstd_frame(data, window_log=10, streamed=True, checksum=True)
    if kind == "flushes":
        return zstd_frame(data, flush_at=[size // 7, size // 3, size // 3 + 1, (3 * size) // 4], checksum=True)
    if kind == "targetcblock2000":
        return zstd_frame(data, target_cblock=2000, level=5)
    if kind == "literals-off":
        return zstd_frame(data, lit_mode=2)
    if kind == "two-frames":
        return (zstd_frame(data[:size // 3], checksum=True) + skippable(b"between the frames", 7) +
                zstd_frame(data[size // 3:], level=1))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def foreign_vectors():
    out = []
    k = 0
    for kind in FOREIGN_KINDS:
        for size in SIZES:
            name = FOUR[k % 4]
            k += 1
            out.append(_valid(f"libzstd-{kind}-{size}", name, foreign_stream(kind, size)))
    # one-shot single-segment frames at each content-size width libzstd writes (1, 2, 4 bytes)
    for size in (0, 255, 256, 65791, 65792):
        out.append(_valid(f"libzstd-single-segment-{size}", FOUR[size % 4], zstd_frame(periodic(size) if size % 2 else mixed(size, 3))))
    return out


# ------------------------------------------------------------------ the host program
def write_vector_file(path, vectors):
    with open(path, "wb") as f:
        f.write(b"ZSTVEC1\0" + struct.pack("<I", len(vectors)))
        for v in vectors:
            f.write(struct.pack("<IQQiQ", HEADER_IDS[v.name], v.cap, v.extra, v.status, len(v.blob)))
            f.write(v.blob)
            f.write(struct.pack("<Q", len(v.expected)))
            f.write(v.expected)


@functools.lru_cache(maxsize=None)
def run_host_program():
    """Build tools/zstd_decode_host.cpp with -fsanitize=address,undefined, run every vector through
    it, and return {vector id: (status, decoded length, matched)}.  Raises if a sanitizer fired or
    the program found a mismatch: no vector goes to a GPU before this has passed."""
    import tempfile
    subprocess.run(["make", "-s", "-C", ROOT, "build/zstd_decode_host"], check=True)
    vectors = all_vectors()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vectors.bin")
        write_vector_file(path, vectors)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([os.path.join(ROOT, "build", "zstd_decode_host"), path], capture_output=True, text=True, env=env)
    bad = [f"{v.id}: {line}" for v, line in zip(vectors, r.stdout.splitlines()) if not line.endswith(" ok")]
    assert r.returncode == 0, f"zstd_decode_host failed ({r.returncode}):\n" + "\n".join(bad[:40]) + "\n" + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(vectors)
    out = {}
    for v, line in zip(vectors, lines):
        w = line.split()
        out[v.id] = (int(w[2]), int(w[4]), w[5] == "ok")
    return out


# ------------------------------------------------------------------ hand-built frames
import sys  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
import zstd_span_model as zsm  # noqa: E402  (FSE, Huffman and bit writers)


class _Rle:
    """An RLE-mode table: one symbol, no bits."""
    al = 0

    def init(self, s):
        return 0

    def enc(self, w, v, s):
        return 0


PRE = [(0, zsm.CTable(zsm.LL_NORM, 6), b""), (0, zsm.CTable(zsm.OF_NORM, 5), b""), (0, zsm.CTable(zsm.ML_NORM, 6), b"")]


def fse_tab(norm, al):
    """(mode 2, encoder, description) of a table with these normalized counts."""
    last = max(s for s in range(len(norm)) if norm[s])
    return (2, zsm.CTable(list(norm), al), zsm.write_ncount(list(norm[:last + 1]), al))


def rle_tab(sym):
    return (1, _Rle(), bytes([sym]))


def repeat(tab):
    return (3, tab[1], b"")


def count_bytes(n, width=None):
    width = width or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    return bytes([n]) if width == 1 else bytes([128 + (n >> 8), n & 255]) if width == 2 else b"\xff" + struct.pack("<H", n - 0x7F00)


def seq_section(seqs, tabs=PRE, width=None):
    """The sequences section of (ll, ml, offset_value) triples; tabs: (mode, encoder, description)
    for LL, OF, ML."""
    n = len(seqs)
    if n == 0:
        return count_bytes(0, width)
    (mLL, tLL, dLL), (mOF, tOF, dOF), (mML, tML, dML) = tabs
    hdr = count_bytes(n, width) + bytes([(mLL << 6) | (mOF << 4) | (mML << 2)]) + dLL + dOF + dML
    w = zsm.BitW()
    for k in range(n - 1, -1, -1):
        ll, ml, ov = seqs[k]
        llc, llb, llx = zsm.ll_code(ll)
        mlc, mlb, mlx = zsm.ml_code(ml)
        ofc = ov.bit_length() - 1
        if k == n - 1:
            sML, sOF, sLL = tML.init(mlc), tOF.init(ofc), tLL.init(llc)
        else:
            sOF = tOF.enc(w, sOF, ofc)
            sML = tML.enc(w, sML, mlc)
            sLL = tLL.enc(w, sLL, llc)
        w.put(llx, llb)
        w.put(mlx, mlb)
        w.put(ov - (1 << ofc), ofc)
    w.put(sML, tML.al)
    w.put(sOF, tOF.al)
    w.put(sLL, tLL.al)
    return hdr + w.close()


def raw_lits(lits, hlen=None):
    n = len(lits)
    hlen = hlen or (1 if n < 32 else 2 if n < 4096 else 3)
    return ((n << 3) if hlen == 1 else 0b0100 | (n << 4) if hlen == 2 else 0b1100 | (n << 4)).to_bytes(hlen, "little") + bytes(lits)


def rle_lits(byte, n, hlen=None):
    hlen = hlen or (1 if n < 32 else 2 if n < 4096 else 3)
    return (1 | ((n << 3) if hlen == 1 else 0b0100 | (n << 4) if hlen == 2 else 0b1100 | (n << 4))).to_bytes(hlen, "little") + bytes([byte])


def block(btype, body, size=None, last=False):
    size = len(body) if size is None else size
    return ((size << 3) | (btype << 1) | int(last)).to_bytes(3, "little") + body


def raw_block(data, last=False):
    return block(0, bytes(data), last=last)


def rle_block(byte, n, last=False):
    return block(1, bytes([byte]), size=n, last=last)


def comp_block(lits, seqs, last=False, tabs=PRE, width=None, lit_section=None):
    return block(2, (raw_lits(lits) if lit_section is None else lit_section) + seq_section(seqs, tabs, width), last=last)


def frame(blocks, window_log=None, fcs=None, fcs_bytes=0, checksum=None, did_bytes=0, did=0, reserved=0):
    """A frame of these blocks (the last one is flagged here).  window_log None: Single_Segment
    (fcs required); checksum: the decoded bytes to sum."""
    single = window_log is None
    if single and not fcs_bytes:
        fcs_bytes = 1
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    fhd = (flag << 6) | (int(single) << 5) | (reserved << 3) | (int(checksum is not None) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    out = MAGIC + bytes([fhd])
    if not single:
        out += bytes([(window_log - 10) << 3])
    out += did.to_bytes(did_bytes, "little")
    if fcs_bytes:
        out += (fcs - 256 if fcs_bytes == 2 else fcs).to_bytes(fcs_bytes, "little")
    blocks = list(blocks)
    blocks[-1] = bytes([blocks[-1][0] | 1]) + blocks[-1][1:]
    out += b"".join(blocks)
    if checksum is not None:
        out += struct.pack("<I", zm.xxh64(bytes(checksum)) & 0xFFFFFFFF)
    return out


def alphabet(n, seed=0):
    """n literal bytes with no repeats a match finder would care about."""
    return bytes((seed + 7 * i + (i >> 3)) & 255 for i in range(n))


def descriptors(stream):
    """One per block and one per frame: what the index pass writes for this stream."""
    return sum(1 + len(f.blocks) for f in zm.walk(stream) if not f.skippable)


def _hv(vid, stream, k=[0]):
    """A hand-built valid vector; with more blocks than 4 + cap / 1 KiB, the descriptors it needs beyond them."""
    k[0] += 1
    v = _valid(vid, FOUR[k[0] % 4], stream)
    return v._replace(extra=max(0, descriptors(stream) - (4 + v.cap // 1024)))


def huff_literals(lits, lens=None, fse=False, treeless=False, streams=None, jump=None, comp=None):
    """A Compressed (or Treeless) literals section of `lits` under code lengths `lens`, in 1 stream or
    in 4 with their 6-byte jump table.  jump: the three sizes to write instead of the true ones;
    comp: the compressed size to claim (the body is cut to it)."""
    if lens is None:
        lens = zsm.huff_lengths(_freq(lits))
    codes = zsm.huff_table_any(lens)[0]
    desc = b"" if treeless else (zsm.huff_desc_fse(lens) if fse else zsm.huff_table(lens)[1])
    assert desc is not None
    n, typ = len(lits), 3 if treeless else 2
    if streams is None:
        streams = 1 if n <= 1023 else 4
    if streams == 1:
        body = desc + zsm.huff_stream(list(lits), codes)
        assert n <= 1023 and len(body) <= 1023
        return (typ | (n << 4) | (len(body) << 14)).to_bytes(3, "little") + body
    seg = (n + 3) // 4
    parts = [zsm.huff_stream(list(lits[k * seg:(k + 1) * seg if k < 3 else n]), codes) for k in range(4)]
    sizes = jump or [len(x) for x in parts[:3]]
    body = desc + b"".join(struct.pack("<H", x) for x in sizes) + b"".join(parts)
    if comp is not None:
        body = body[:comp]
    c = len(body)
    sf = 1 if n <= 1023 and c <= 1023 else 2 if n <= 16383 and c <= 16383 else 3
    v = typ | (sf << 2) | (n << 4) | (c << (4 + (10, 14, 18)[sf - 1]))
    return v.to_bytes(sf + 2, "little") + body


def _freq(lits):
    f = [0] * 256
    for c in lits:
        f[c] += 1
    return f


def ncount(norm, al):
    """The FSE description of these counts (-1: less than 1) as RFC 8878 4.1.1 writes them, whether or
    not they sum to the table: zeros take their 2-bit repeat flags."""
    w = zsm.BitW()
    w.put(al - 5, 4)
    remaining, thr, nb, i = (1 << al) + 1, 1 << al, al + 1, 0
    while i < len(norm):
        c = norm[i]
        i += 1
        mx, x = 2 * thr - 1 - remaining, c + 1
        if x < mx:
            w.put(x, nb - 1)
        else:
            w.put(x if x < thr else x + mx, nb)
        remaining -= abs(c)
        if c == 0:
            z = 0
            while i < len(norm) and norm[i] == 0:
                z, i = z + 1, i + 1
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
        while 1 < remaining < thr:
            nb, thr = nb - 1, thr >> 1
    if w.nb:
        w.put(0, 8 - w.nb)
    return bytes(w.out)


@functools.lru_cache(maxsize=None)
def built_valid_vectors():
    out = []
    HIST = raw_block(alphabet(40, 1))  # something for the first offsets to reach
    # repeat codes, with literals and without, and the rotation after each
    hist = [(8, 4, 3 + 5), (4, 4, 3 + 9), (4, 4, 3 + 13)]  # offsets 5, 9, 13: rep = 13, 9, 5
    for code in (1, 2, 3):
        for ll in (0, 2):
            seqs = hist + [(ll, 5, code), (1, 4, 1), (1, 4, 2), (1, 4, 3), (0, 3, 1), (0, 3, 2), (0, 3, 3)]
            lits = alphabet(sum(s[0] for s in seqs) + 3, code)
            out.append(_hv(f"repeat-code-{code}-ll-{ll}-and-rotation", frame([comp_block(lits, seqs)], window_log=10)))
    # the initial offsets 1, 4, 8 at the start of a frame
    out.append(_hv("initial-repeat-offsets-1-4-8", frame([comp_block(alphabet(30), [(9, 4, 3), (2, 5, 2), (3, 6, 1), (0, 4, 2)])],
                                                          window_log=10)))
    # repeats carried across a compressed, a raw and an RLE block, reset at a new frame
    carry = [comp_block(alphabet(20), [(12, 4, 3 + 7), (2, 4, 3 + 11)]), raw_block(alphabet(9, 3)),
             comp_block(alphabet(6, 9), [(2, 4, 1), (1, 4, 2), (1, 5, 3)]), rle_block(0x55, 10),
             comp_block(alphabet(4, 1), [(0, 6, 1), (2, 4, 1)])]
    out.append(_hv("repeats-carried-across-compressed-raw-rle-blocks", frame(carry, window_log=10)))
    out.append(_hv("repeats-reset-at-a-new-frame", frame(carry, window_log=10) +
                   frame([comp_block(alphabet(12, 5), [(9, 4, 3), (1, 4, 2), (2, 3, 1)])], window_log=10)))
    # offset 1
    for ml in (3, 64, 65, 65536):
        out.append(_hv(f"offset-1-length-{ml}", frame([comp_block(b"Q" + alphabet(3), [(1, ml, 4)])], window_log=17)))
    # offsets 63, 64, 65 with lengths on either side
    for off in (63, 64, 65):
        seqs = [(70, off - 1, off + 3), (1, off, off + 3), (1, off + 1, off + 3), (1, 3 * off + 7, off + 3)]
        out.append(_hv(f"offset-{off}-lengths-either-side", frame([comp_block(alphabet(80, off), seqs)], window_log=12)))
    # the executor's batch seams: 64 sequences to a batch
    filler = [(1, 3, 3 + 1)] * 64  # a first batch of 256 bytes
    out.append(_hv("match-source-inside-its-own-batch",
                   frame([comp_block(alphabet(100), filler + [(4, 8, 3 + 3), (2, 5, 3 + 9), (0, 4, 3 + 2)])], window_log=12)))
    out.append(_hv("match-source-straddles-the-batch-start",
                   frame([comp_block(alphabet(100), filler + [(4, 12, 3 + 10), (0, 20, 3 + 30)])], window_log=12)))
    out.append(_hv("match-source-ends-at-the-batch-start",
                   frame([comp_block(alphabet(100), filler + [(4, 10, 3 + 14), (0, 16, 3 + 30), (1, 5, 3 + 36)])], window_log=12)))
    out.append(_hv("every-match-reads-the-previous-match",
                   frame([comp_block(alphabet(80), [(8, 5, 3 + 6)] + [(0, 5, 3 + 5)] * 70 + [(1, 9, 3 + 4)] * 60)], window_log=12)))
    for n in (63, 64, 65, 128, 129):
        seqs = [(3, 4, 3 + 2)] + [(k % 3, 3 + k % 5, 3 + 1 + k % 7) for k in range(n - 1)]
        out.append(_hv(f"{n}-sequences-in-a-block", frame([comp_block(alphabet(sum(s[0] for s in seqs) + 5, n), seqs)], window_log=12)))
    out.append(_hv("offset-equal-to-the-bytes-produced", frame([comp_block(alphabet(40), [(17, 9, 3 + 17), (3, 40, 3 + 29)])], window_log=10)))
    out.append(_hv("match-into-the-previous-block-back-to-the-first-byte",
                   frame([comp_block(alphabet(50), [(20, 6, 3 + 20)]), raw_block(alphabet(10, 8)),
                          comp_block(alphabet(5, 2), [(2, 30, 3 + 68), (0, 7, 3 + 9)])], window_log=10)))
    out.append(_hv("block-with-no-sequences", frame([comp_block(alphabet(45), [])], window_log=10)))
    out.append(_hv("two-byte-empty-compressed-block-then-data", frame([comp_block(alphabet(1), []), raw_block(b"xyz")], window_log=10)))
    out.append(_hv("block-with-no-literals", frame([raw_block(alphabet(30)), comp_block(b"", [(0, 9, 3 + 30), (0, 4, 3 + 2)])], window_log=10)))
    out.append(_hv("trailing-literals-after-the-last-sequence", frame([comp_block(alphabet(90), [(10, 5, 3 + 4)])], window_log=10)))
    out.append(_hv("two-byte-count-for-5-sequences", frame([comp_block(alphabet(20), [(2, 3, 3 + 1)] * 5, width=2)], window_log=10)))
    out.append(_hv("three-byte-count-0x7f00-sequences", frame([comp_block(b"ab", [(2, 3, 3 + 2)] + [(0, 3, 3 + 2)] * (0x7F00 - 1))], window_log=17)))
    out.append(_hv("three-byte-count-0x7f05-sequences", frame([comp_block(b"abc", [(3, 3, 3 + 3)] + [(0, 3, 3 + 3)] * (0x7F05 - 1))], window_log=17)))
    out.append(_hv("two-byte-count-0x7eff-sequences", frame([comp_block(b"abcd", [(4, 3, 3 + 4)] + [(0, 3, 3 + 4)] * (0x7EFF - 1))], window_log=17)))
    big = alphabet(65536 + 40)
    out.append(_hv("ll-code-35-and-ml-code-52", frame([comp_block(big, [(65536, 3, 3 + 7), (4, 9, 3 + 65536)]),
                                                       comp_block(alphabet(9), [(2, 65539 + 1000, 3 + 5)])], window_log=18)))
    # modes: RLE for each table, FSE_Compressed at both accuracy limits, Repeat, less-than-1, zero-repeat flags
    same = [(2, 5, 8 + 1), (2, 5, 8 + 3), (2, 5, 8 + 6)]  # LL code 2, ML code 2, OF code 3 throughout
    out.append(_hv("rle-mode-for-each-table", frame([HIST, comp_block(alphabet(20), same, tabs=[rle_tab(2), rle_tab(3), rle_tab(2)])], window_log=10)))
    for t, sym in ((0, 2), (1, 3), (2, 2)):
        tabs = list(PRE)
        tabs[t] = rle_tab(sym)
        out.append(_hv(f"rle-mode-for-table-{t}-alone", frame([HIST, comp_block(alphabet(20), same, tabs=tabs)], window_log=10)))
    ll5, of5, ml5 = [8, 8, 8, 8], [4, 4, 8, 8, 8], [0, 0, 16, 16]
    lo = [fse_tab(ll5, 5), fse_tab(of5, 5), fse_tab(ml5, 5)]
    mixed_seqs = [(k % 4, 5 + k % 2, (1 << (2 + k % 3)) + 1) for k in range(30)]
    lits30 = alphabet(sum(s[0] for s in mixed_seqs) + 2)
    out.append(_hv("fse-compressed-accuracy-log-5-then-repeat-mode",
                   frame([HIST, comp_block(lits30, mixed_seqs, tabs=lo), comp_block(lits30, mixed_seqs, tabs=[repeat(t) for t in lo]),
                          comp_block(alphabet(3), []), raw_block(b"between"),
                          comp_block(lits30, mixed_seqs, tabs=[repeat(lo[0]), PRE[1], repeat(lo[2])]),
                          comp_block(lits30, mixed_seqs, tabs=[PRE[0], repeat(PRE[1]), rle_tab(2)][:2] + [repeat(lo[2])])], window_log=12)))
    hi = [fse_tab([128] * 4, 9), fse_tab([32, 32, 64, 64, 64], 8), fse_tab([0, 0, 256, 256], 9)]
    out.append(_hv("fse-compressed-accuracy-logs-9-8-9", frame([HIST, comp_block(lits30, mixed_seqs, tabs=hi)], window_log=12)))
    less = [fse_tab([10, 10, 6, 5, -1], 5), fse_tab([0, 0, 12, 12, 7, -1], 5), fse_tab([0, 0, 20, 11, 0, 0, 0, 0, 0, -1], 5)]
    seqs_less = mixed_seqs + [(4, 12, 32 + 5)]  # LL code 4, ML code 9, OF code 5: the less-than-1 symbols
    out.append(_hv("less-than-1-symbols-and-zero-repeat-flags", frame([HIST, comp_block(alphabet(80), seqs_less, tabs=less)], window_log=12)))
    rep_after = [PRE[0], rle_tab(3), PRE[2]]
    out.append(_hv("repeat-mode-after-predefined-and-rle",
                   frame([HIST, comp_block(alphabet(20), same, tabs=rep_after), comp_block(alphabet(20), same, tabs=[repeat(t) for t in rep_after])],
                         window_log=10)))
    # Huffman literals
    text = b"the quick brown fox jumps over the lazy dog; " * 20
    out.append(_hv("huffman-1-stream-direct-weights", frame([block(2, huff_literals(text[:600]) + seq_section([]))], window_log=10)))
    out.append(_hv("huffman-4-streams-fse-weights", frame([block(2, huff_literals(rand(3000, 2), fse=True) + seq_section([]))], window_log=12)))
    out.append(_hv("huffman-4-streams-for-few-literals", frame([block(2, huff_literals(text[:40], streams=4) + seq_section([]))], window_log=10)))
    out.append(_hv("huffman-4-streams-18-bit-sizes", frame([block(2, huff_literals((text * 23)[:20000]) + seq_section([]))], window_log=15)))
    lens11 = [0] * 256
    for s, ln in enumerate([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11]):
        lens11[s] = ln
    skew = bytes([0] * 40 + list(range(12)) * 3 + [11, 10, 11])
    out.append(_hv("huffman-11-bit-codes-even-weight-count", frame([block(2, huff_literals(skew, lens11) + seq_section([]))], window_log=10)))
    lens_odd = [0] * 256
    for s, ln in enumerate([1, 2, 3, 4, 5, 5]):
        lens_odd[2 * s] = ln  # symbols 0, 2, .., 10: ten weights listed, the eleventh implied
    odd = bytes([0, 2, 4, 6, 8, 10] * 9)
    out.append(_hv("huffman-odd-symbol-count-with-gaps", frame([block(2, huff_literals(odd, lens_odd) + seq_section([]))], window_log=10)))
    lens_t = [0] * 256
    for s, ln in enumerate([2, 2, 2, 3, 3]):
        lens_t[s] = ln
    t_lits = bytes([0, 1, 2, 3, 4] * 12)
    out.append(_hv("treeless-after-a-raw-literals-block",
                   frame([block(2, huff_literals(t_lits, lens_t) + seq_section([(3, 4, 3 + 2)])), comp_block(alphabet(9), [(4, 4, 3 + 1)]),
                          block(2, huff_literals(t_lits[:33], lens_t, treeless=True) + seq_section([(1, 5, 2)])),
                          block(2, huff_literals(t_lits[:41], lens_t, treeless=True, streams=4) + seq_section([]))], window_log=10)))
    short = bytes([0, 1, 2, 3] * 3 + [4])  # 13 literals in 4 streams: 4, 4, 4 and 1
    out.append(_hv("huffman-4-streams-one-short-stream", frame([block(2, huff_literals(short, lens_t, streams=4) + seq_section([]))], window_log=10)))
    out.append(_hv("huffman-4-streams-of-2-2-2-and-0-literals", frame([block(2, huff_literals(short[:6], lens_t, streams=4) + seq_section([]))], window_log=10)))
    out.append(_hv("rle-literals-in-every-size-format",
                   frame([block(2, rle_lits(65, 20) + seq_section([])), block(2, rle_lits(66, 20, 2) + seq_section([(5, 4, 3 + 1)])),
                          block(2, rle_lits(67, 5000) + seq_section([])), block(2, raw_lits(alphabet(20), 3) + seq_section([])),
                          block(2, raw_lits(alphabet(20), 2) + seq_section([]))], window_log=13)))
    # frames
    one = frame([raw_block(b"payload")], window_log=10)
    out.append(_hv("skippable-frames-of-size-0-at-the-start-and-the-end", skippable(b"") + one + skippable(b"", 15)))
    out.append(_hv("only-skippable-frames", skippable(b"abc") + skippable(b"")))
    out.append(_hv("no-frame-at-all", b""))
    for nb in (1, 2, 4):
        out.append(_hv(f"dictionary-id-field-of-{nb}-bytes-holding-0", frame([raw_block(b"no dictionary")], window_log=10, did_bytes=nb)))
    out.append(_hv("content-size-of-8-bytes", frame([raw_block(alphabet(300))], window_log=10, fcs=300, fcs_bytes=8)))
    out.append(_hv("single-segment-content-size-of-8-bytes", frame([raw_block(alphabet(300))], fcs=300, fcs_bytes=8)))
    out.append(_hv("content-size-of-2-bytes-with-its-256", frame([raw_block(alphabet(256))], window_log=10, fcs=256, fcs_bytes=2)))
    out.append(_hv("window-size-with-a-mantissa", MAGIC + bytes([0, (1 << 3) | 5]) + raw_block(alphabet(1500), last=True)))
    out.append(_hv("empty-raw-last-block-after-data", frame([raw_block(b"data"), raw_block(b"")], window_log=10, checksum=b"data")))
    out.append(_hv("rle-block-of-128-kib", frame([rle_block(7, 128 << 10)], window_log=17)))
    for n in CHECKSUMMED:
        out.append(_hv(f"checksummed-frame-of-{n}-bytes", zstd_frame(mixed(n, n), checksum=True)))
    return out


CHECKSUMMED = (0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97)


def valid_vectors():
    # a flushed 300-byte stream has more blocks than 4 + cap / 1 KiB: it takes extra descriptors
    return [v._replace(extra=max(0, descriptors(v.blob[4:]) - (4 + v.cap // 1024))) for v in foreign_vectors()] + built_valid_vectors()


# ------------------------------------------------------------------ corrupt contents
OWN_RULES = ("wrong-header-id", "frame-under-another-zstd-name", "cap-", "dictionary-id-", "offset-beyond-the-window",
             "offset-0-from-rep1-minus-1", "more-empty-raw-blocks-than-descriptors", "block-decodes-past-",
             "offset-into-the-previous-frame", "raw-block-over-", "rle-block-over-", "reserved-bits-of-the-modes-byte",
             "sequence-stream-not-consumed-exactly", "huffman-code-of-12-bits")
# libzstd 1.4.8's one-shot decoder does not hold a block to Block_Maximum_Size, ignores the modes
# byte's reserved bits, leaves bits of a sequence stream unread, decodes a 12-bit Huffman code and
# turns the offset 0 of rep1 - 1 into 1; RFC 8878 refuses all of these, and so does the library.


def _bad(vid, name, stream, why, status=EBADMSG, cap=None, extra=0):
    return Vector(vid, name, content(name, stream), 4096 if cap is None else cap, status, b"", extra, why)


@functools.lru_cache(maxsize=None)
def corrupt_vectors():
    out = []
    Z0, Z1, Z2, Z3 = FOUR
    data = mixed(3000, 11)
    base = zstd_frame(data, checksum=True, level=3)              # Single_Segment, 2-byte content size
    streamed = zstd_frame(data, checksum=True, streamed=True)    # Window_Descriptor, no content size
    # truncation at every structural point of the frame
    for what, stream, at, why in (("magic", base, 2, "truncated magic"), ("frame-header", base, 5, "truncated frame header"),
                                  ("window-descriptor", streamed, 5, "truncated frame header"),
                                  ("block-header", base, 8, "truncated block header"),
                                  ("literals-header", base, 11, "truncated or oversized compressed block"),
                                  ("before-the-checksum", base, len(base) - 4, "truncated checksum"),
                                  ("the-checksum", base, len(base) - 2, "truncated checksum"),
                                  ("the-last-byte-of-the-sequences", base, len(base) - 5, "truncated or oversized compressed block")):
        out.append(_bad(f"truncated-inside-{what}", Z0, stream[:at], why))
    # ... and of a block: the block header tells the truth about the bytes that are left
    text = b"the quick brown fox jumps over the lazy dog; " * 20
    lens_t = [0] * 256
    for sym, ln in enumerate([2, 2, 2, 3, 3]):
        lens_t[sym] = ln
    short = bytes([0, 1, 2, 3] * 3 + [4])  # 13 literals: streams of 4, 4, 4 and 1
    lit4 = huff_literals(short, lens_t, streams=4)
    tree = len(zsm.huff_table(lens_t)[1])
    sizes = [int.from_bytes(lit4[3 + tree + k:5 + tree + k], "little") for k in (0, 2, 4)]
    streams_bytes = len(lit4) - 3 - tree - 6

    def lit_block(section, seqs=()):
        return frame([block(2, section + seq_section(list(seqs)))], window_log=10)

    def cut_block(section_prefix):
        return frame([block(2, section_prefix)], window_log=10)
    out.append(_bad("truncated-inside-the-one-byte-literals-header", Z1, cut_block(lit4[:1]), "truncated or oversized compressed block"))
    out.append(_bad("truncated-inside-the-three-byte-literals-header", Z1, cut_block(lit4[:2]), "truncated literals header"))
    out.append(_bad("truncated-inside-jump-table", Z1, cut_block(lit4[:3 + tree + 4]), "literals section larger than the block"))
    out.append(_bad("section-ends-inside-its-jump-table", Z1, lit_block(huff_literals(short, lens_t, streams=4, comp=tree + 4)),
                    "truncated jump table"))
    out.append(_bad("truncated-inside-the-weight-description", Z1, cut_block(lit4[:3 + tree - 2]), "literals section larger than the block"))
    out.append(_bad("section-ends-inside-its-weight-description", Z1, lit_block(huff_literals(short, lens_t, streams=4, comp=tree - 1)),
                    "truncated weights"))
    out.append(_bad("truncated-inside-a-huffman-stream", Z1, cut_block(lit4[:-2]), "literals section larger than the block"))
    claims_more = (int.from_bytes(lit4[:3], "little") + (4 << 14)).to_bytes(3, "little") + lit4[3:]  # 4 bytes more than the block holds
    out.append(_bad("literals-section-larger-than-the-block", Z2, lit_block(claims_more), "literals section larger than the block"))
    fse_lits = huff_literals(rand(3000, 2), fse=True)
    out.append(_bad("truncated-inside-the-fse-weights", Z2, cut_block(fse_lits[:9]), "literals section larger than the block"))
    cut_fse = bytearray(fse_lits)
    cut_fse[4] = 1  # the weights' description claims 1 byte: it ends inside its FSE table description
    out.append(_bad("weight-description-ends-inside-its-fse-description", Z2, frame([block(2, bytes(cut_fse) + seq_section([]))], window_log=12),
                    "truncated FSE description"))
    seqs = [(2, 5, 8 + 1), (2, 5, 8 + 3), (2, 5, 8 + 6)]
    hist = raw_block(alphabet(40, 1))
    good_tabs = [fse_tab([8, 8, 8, 8], 5), fse_tab([4, 4, 8, 8, 8], 5), fse_tab([0, 0, 16, 16], 5)]
    raw20 = raw_lits(alphabet(20))
    sec = raw20 + seq_section(seqs, good_tabs)
    out.append(_bad("truncated-inside-an-fse-description", Z3, frame([hist, block(2, sec[:len(raw20) + 3])], window_log=10),
                    "truncated FSE description"))
    many = [(k % 4, 5 + k % 2, (1 << (2 + k % 3)) + 1) for k in range(30)]
    long_sec = raw_lits(alphabet(60)) + seq_section(many)
    at = len(raw_lits(alphabet(60))) + 2  # the count and the modes byte, then the stream: its first bytes are read last
    out.append(_bad("truncated-inside-the-sequence-bit-stream", Z3, frame([hist, block(2, long_sec[:at] + long_sec[at + 3:])], window_log=10),
                    "sequence stream too short"))
    out.append(_bad("sequences-header-missing", Z0, frame([hist, block(2, raw20)], window_log=10), "truncated sequences header"))
    out.append(_bad("truncated-inside-the-two-byte-sequence-count", Z0, frame([hist, block(2, raw20 + b"\x80")], window_log=10),
                    "truncated sequences header"))
    out.append(_bad("modes-byte-missing", Z0, frame([hist, block(2, raw20 + b"\x03")], window_log=10), "truncated sequences header"))
    out.append(_bad("bytes-after-an-empty-sequences-section", Z0, frame([hist, block(2, raw20 + b"\x00\x00")], window_log=10),
                    "bytes after an empty sequences section"))
    out.append(_bad("truncated-inside-a-raw-block", Z0, frame([raw_block(b"0123456789")], window_log=10)[:-3], "truncated raw block"))
    out.append(_bad("truncated-before-an-rle-block-byte", Z0, frame([rle_block(1, 9)], window_log=10)[:-1], "truncated RLE block"))
    out.append(_bad("truncated-skippable-frame", Z1, skippable(b"abcdef")[:-2], "truncated skippable frame"))
    out.append(_bad("no-last-block", Z1, MAGIC + bytes([0, 0]) + raw_block(b"abc"), "truncated block header"))
    out.append(_bad("junk-after-the-frame", Z1, base + b"\x01\x02\x03\x04\x05", "bad magic"))
    # blocks
    out.append(_bad("block-type-3", Z2, frame([block(3, b"abc")], window_log=10), "block type 3"))
    out.append(_bad("raw-block-over-block-maximum-size", Z2, frame([raw_block(alphabet(1025))], window_log=10), "block over Block_Maximum_Size"))
    out.append(_bad("rle-block-over-block-maximum-size", Z2, frame([rle_block(3, 1025)], window_log=10), "block over Block_Maximum_Size"))
    out.append(_bad("rle-block-over-128-kib", Z2, frame([rle_block(3, (128 << 10) + 1)], window_log=20), "block over Block_Maximum_Size",
                    cap=200000))
    out.append(_bad("block-decodes-past-128-kib", Z3, frame([comp_block(b"Q" + alphabet(3), [(1, 70000, 4), (1, 70000, 4)])], window_log=20),
                    "block decodes past its maximum", cap=200000))
    out.append(_bad("block-decodes-past-block-maximum-size-by-a-match", Z3, frame([comp_block(alphabet(10), [(1, 600, 4), (1, 600, 4)])], window_log=10),
                    "block decodes past its maximum"))
    out.append(_bad("block-decodes-past-block-maximum-size-by-trailing-literals", Z3,
                    frame([comp_block(alphabet(600), [(100, 500, 4)])], window_log=10), "block decodes past its maximum"))
    out.append(_bad("block-decodes-past-block-maximum-size-by-its-headers", Z3,
                    frame([comp_block(alphabet(1000), [(1, 3, 4)] * 9)], window_log=10), "block decodes past its maximum"))
    # Huffman weights: a Compressed section of 4 literals in one stream under these direct weights
    def weights_block(desc, stream=b"\x01"):
        return lit_block((2 | (4 << 4) | ((len(desc) + len(stream)) << 14)).to_bytes(3, "little") + desc + stream)
    # weights 1, 1, 3, 3: 1 + 1 + 4 + 4 = 10, and 6 are left of 16.  Were the implied weight taken as 3 all the
    # same, the code would lack two of its 16 cells and the stream's bits 01 01 01 01 would decode as four
    # symbols and end exactly: the weights alone refuse this content
    out.append(_bad("weights-do-not-complete-a-power-of-two", Z0, weights_block(bytes([127 + 4, 0x11, 0x33]), b"\x55\x01"),
                    "weights do not complete a power of two"))
    out.append(_bad("weight-over-11", Z0, weights_block(bytes([127 + 2, 0xC1])), "weight over 11"))
    # weight 2 and an implied 2: a complete 1-bit code, which four bits 0101 would decode exactly, but no weight 1
    out.append(_bad("weights-without-a-pair-of-weight-1-symbols", Z0, weights_block(bytes([127 + 1, 0x20]), b"\x15"), "weight-1 symbols"))
    out.append(_bad("weights-all-zero", Z0, weights_block(bytes([127 + 2, 0x00])), "no weights"))
    # weights 11, 11, 11, 10, .., 2, 1 and an implied 1: complete, two of weight 1, and 12 bits long
    out.append(_bad("huffman-code-of-12-bits", Z0, weights_block(bytes([127 + 13, 0xBB, 0xBA, 0x98, 0x76, 0x54, 0x32, 0x10]), b"\x55\x01"),
                    "code over 11 bits"))
    # FSE-compressed weights from a one-symbol table: no state ever reads a bit, the weights never end
    out.append(_bad("fse-weights-that-never-end", Z0, weights_block(bytes([4]) + ncount([32], 5) + b"\x00\x10"), "too many weights"))
    out.append(_bad("fse-weights-without-a-stream", Z0, weights_block(bytes([2]) + ncount([32], 5)), "no weight stream"))
    # FSE descriptions and symbols
    for t, (name, maxlog, maxsym) in enumerate((("ll", 9, 35), ("of", 8, 31), ("ml", 9, 52))):
        def with_table(desc):
            tabs = list(good_tabs)
            tabs[t] = desc if isinstance(desc, tuple) else (2, good_tabs[t][1], desc)
            return frame([hist, comp_block(alphabet(20), seqs, tabs=tabs)], window_log=10)
        out.append(_bad(f"{name}-accuracy-log-over-its-limit", FOUR[t], with_table(bytes([maxlog + 1 - 5]) + b"\x00\x00\x00"),
                        "accuracy log over its limit"))
        out.append(_bad(f"{name}-rle-symbol-beyond-its-table", FOUR[t], with_table(rle_tab(maxsym + 1)), "RLE symbol beyond the table"))
        norm = [0] * (maxsym + 2)
        norm[0], norm[maxsym + 1] = 31, 1
        # 31 of 32 for symbol 0, the last 1 for a symbol the table does not have: the symbols end with 1 missing
        out.append(_bad(f"{name}-fse-symbol-beyond-its-table", FOUR[t], with_table(ncount(norm, 5)), "FSE description does not sum"))
        # 16 of 32, then a run of zeros whose repeat flags pass the last symbol
        out.append(_bad(f"{name}-zero-repeat-flags-beyond-its-table", FOUR[t], with_table(ncount([16] + [0] * (maxsym + 4) + [16], 5)),
                        "symbol beyond the table"))
        # every symbol "less than 1" under accuracy log 6: the symbols run out before the counts fill the table
        out.append(_bad(f"{name}-fse-description-short-of-its-table", FOUR[t], with_table(ncount([-1] * (maxsym + 1), 6)),
                        "FSE description does not sum"))
        out.append(_bad(f"{name}-repeat-mode-in-the-first-block", FOUR[t], with_table((3, good_tabs[t][1], b"")), "Repeat_Mode without a table"))
    out.append(_bad("treeless-literals-in-the-first-block", Z1, lit_block(huff_literals(text[:40], treeless=True)),
                    "Treeless literals without a tree"))
    out.append(_bad("reserved-bits-of-the-modes-byte", Z1, frame([hist, block(2, raw20 + b"\x03\x01" + seq_section(seqs)[2:])], window_log=10),
                    "reserved mode bits"))
    # streams
    for k, what in enumerate(("first", "second", "third")):
        jump = list(sizes)
        jump[k] = streams_bytes - sum(sizes[:k]) + 1  # one more than what the sizes before it leave
        out.append(_bad(f"jump-table-larger-than-its-section-by-the-{what}-size", Z2, lit_block(huff_literals(short, lens_t, streams=4, jump=jump)),
                        "jump table larger than its section"))
    out.append(_bad("four-streams-for-5-literals", Z2, lit_block(huff_literals(short[:5], lens_t, streams=4)), "4 streams for too few literals"))
    out.append(_bad("four-streams-for-1-literal", Z2, lit_block(huff_literals(short[:1], lens_t, streams=4)), "4 streams for too few literals"))
    shifted = [sizes[0] + 1, sizes[1] - 1, sizes[2]]  # inside the section, but not where the streams end
    out.append(_bad("jump-table-sizes-off-by-one", Z2, lit_block(huff_literals(short, lens_t, streams=4, jump=shifted)), "Huffman stream"))
    zero_last = bytearray(lit4)
    zero_last[-1] = 0
    out.append(_bad("huffman-stream-with-a-zero-last-byte", Z2, lit_block(bytes(zero_last)), "no final-bit marker"))
    one = huff_literals(text[:40], streams=1)
    longer = bytearray(one)
    longer[0:3] = (int.from_bytes(one[:3], "little") + (1 << 4)).to_bytes(3, "little")  # one more literal than the stream holds
    out.append(_bad("huffman-stream-not-consumed-exactly-too-short", Z3, lit_block(bytes(longer)), "Huffman stream not consumed exactly"))
    shorter = bytearray(one)
    shorter[0:3] = (int.from_bytes(one[:3], "little") - (1 << 4)).to_bytes(3, "little")
    out.append(_bad("huffman-stream-not-consumed-exactly-bits-left", Z3, lit_block(bytes(shorter)), "Huffman stream not consumed exactly"))
    s_ok = seq_section(seqs)
    out.append(_bad("sequence-stream-with-a-zero-last-byte", Z0, frame([hist, block(2, raw20 + s_ok[:-1] + b"\x00")], window_log=10),
                    "no final-bit marker"))
    out.append(_bad("sequence-stream-not-consumed-exactly", Z0, frame([hist, block(2, raw20 + s_ok[:2] + b"\x55" + s_ok[2:])], window_log=10),
                    "sequence stream not consumed exactly"))
    out.append(_bad("sequences-need-more-literals-than-the-block-has", Z1, frame([hist, comp_block(alphabet(5), seqs)], window_log=10),
                    "sequences need more literals than the block has"))
    # offsets
    out.append(_bad("offset-0-from-rep1-minus-1", Z1, frame([comp_block(alphabet(30), [(9, 4, 3), (2, 5, 2), (3, 6, 1), (0, 4, 3)])], window_log=10),
                    "offset 0"))
    out.append(_bad("offset-beyond-the-bytes-produced", Z2, frame([comp_block(alphabet(30), [(9, 4, 3 + 10)])], window_log=10),
                    "offset beyond the bytes the frame has produced"))
    out.append(_bad("offset-beyond-the-bytes-produced-by-one-in-a-later-block", Z2,
                    frame([raw_block(alphabet(20)), comp_block(alphabet(30), [(9, 4, 3 + 30)])], window_log=10),
                    "offset beyond the bytes the frame has produced"))
    first = frame([raw_block(alphabet(100))], window_log=10)
    out.append(_bad("offset-into-the-previous-frame", Z2, first + frame([comp_block(alphabet(30), [(9, 4, 3 + 10)])], window_log=10),
                    "offset beyond the bytes the frame has produced"))
    out.append(_bad("offset-beyond-the-window", Z3, frame([raw_block(alphabet(1024)), raw_block(alphabet(400, 3)),
                                                           comp_block(alphabet(30), [(9, 4, 3 + 1025)])], window_log=10), "offset beyond the window"))
    # the frame header
    ok300 = alphabet(300)
    out.append(_bad("frame-content-size-one-short", Z0, frame([raw_block(ok300)], window_log=10, fcs=299, fcs_bytes=2), "Frame_Content_Size mismatch"))
    out.append(_bad("frame-content-size-one-over", Z0, frame([raw_block(ok300)], window_log=10, fcs=301, fcs_bytes=4), "Frame_Content_Size mismatch"))
    out.append(_bad("single-segment-content-size-one-over", Z0, frame([raw_block(ok300)], fcs=301, fcs_bytes=2), "Frame_Content_Size mismatch"))
    out.append(_bad("reserved-bit", Z1, frame([raw_block(ok300)], window_log=10, reserved=1), "reserved bit"))
    for nb in (1, 2, 4):
        out.append(_bad(f"dictionary-id-of-{nb}-bytes-not-zero", FOUR[nb % 4], frame([raw_block(ok300)], window_log=10, did_bytes=nb, did=1 << (8 * nb - 1)),
                        "a dictionary is asked for"))
    out.append(_bad("bad-magic", Z2, b"\x27" + base[1:], "bad magic"))
    for n in CHECKSUMMED:
        f = bytearray(zstd_frame(mixed(n, n), checksum=True))
        f[-1 - n % 4] ^= 1 << (n % 8)
        out.append(_bad(f"checksummed-frame-of-{n}-bytes-one-checksum-bit-flipped", FOUR[n % 4], bytes(f), "checksum mismatch"))
    flipped = bytearray(zstd_frame(rand(5000, 3), checksum=True))
    flipped[2000] ^= 0x10  # a byte of a raw block: the checksum alone can tell
    out.append(_bad("raw-block-byte-flipped-under-a-checksum", Z3, bytes(flipped), "checksum mismatch", cap=5000))
    # this library's own framing
    out.append(Vector("wrong-header-id", Z0, b"\x00\x00\x11\x04" + base, 4096, EBADMSG, b"", 0))
    out.append(Vector("frame-under-another-zstd-name", Z0, content(Z1, base), 4096, EBADMSG, b"", 0))
    out.append(Vector("wrong-header-id-truncated", Z0, header(Z0)[:3], 4096, EBADMSG, b"", 0))
    # the cap: the streams are valid (why None) and longer than the cap.  The first five are answered
    # by the executor (the literal room and the sequence room hold what the headers ask for)
    crossing = frame([comp_block(alphabet(15), [(1, 40, 3 + 1), (10, 3, 3 + 2)])], window_log=10)  # 41, then 10 literals, a match, 4 more
    out.append(_bad("cap-reached-by-literals", Z0, crossing, None, EOVERFLOW, cap=45))
    out.append(_bad("cap-reached-by-a-match", Z1, crossing, None, EOVERFLOW, cap=30))
    out.append(_bad("cap-reached-by-the-last-byte-of-a-match", Z1, crossing, None, EOVERFLOW, cap=53))
    out.append(_bad("cap-reached-by-trailing-literals", Z0, crossing, None, EOVERFLOW, cap=57))
    out.append(_bad("cap-reached-in-the-second-batch", Z3, frame([comp_block(alphabet(100), [(1, 3, 3 + 1)] * 64 + [(4, 8, 3 + 3)])], window_log=12),
                    None, EOVERFLOW, cap=262))
    out.append(_bad("cap-reached-by-a-raw-block", Z2, frame([raw_block(alphabet(50))], window_log=10), None, EOVERFLOW, cap=49))
    out.append(_bad("cap-reached-by-an-rle-block", Z3, frame([raw_block(b"ab"), rle_block(9, 50)], window_log=10), None, EOVERFLOW, cap=51))
    out.append(_bad("cap-reached-by-the-second-frame", Z2, first + first, None, EOVERFLOW, cap=199))
    # ... and these by the index pass: the headers alone ask for more than the cap grants
    out.append(_bad("cap-below-the-literals-of-a-block", Z0, frame([comp_block(alphabet(50), [(40, 5, 3 + 4)])], window_log=10), None, EOVERFLOW, cap=39))
    out.append(_bad("cap-below-a-third-of-the-sequences", Z0, frame([comp_block(b"ab", [(2, 3, 3 + 2)] + [(0, 3, 3 + 2)] * 19)], window_log=10),
                    None, EOVERFLOW, cap=50))
    out.append(_bad("cap-below-the-content-size", Z1, base, None, EOVERFLOW, cap=2999))
    # descriptor room
    out.append(_bad("more-empty-raw-blocks-than-descriptors", Z0, frame([raw_block(b"")] * 8 + [raw_block(b"end")], window_log=10), None, ENOMEM, cap=3))
    # the four names in turn, so that every call of the GPU tests has its share (the header-ID vectors keep theirs)
    for i, v in enumerate(out):
        if v.blob[:4] == header(v.name):
            out[i] = v._replace(name=FOUR[i % 4], blob=header(FOUR[i % 4]) + v.blob[4:])
    return out


def enomem_twin():
    """The KCDC_ENOMEM content with the descriptors it asks for: the same bytes decode."""
    v = next(v for v in corrupt_vectors() if v.id == "more-empty-raw-blocks-than-descriptors")
    return Vector("empty-raw-blocks-with-descriptors-for-them", v.name, v.blob, 3, 0, b"end", 8)


def all_vectors():
    return valid_vectors() + corrupt_vectors() + [enomem_twin()]


def model_reason(stream):
    """What tests/zstd_model.py says when it refuses `stream` (frames, no header ID); None if it decodes."""
    try:
        zm.decode(stream)
    except zm.Bad as e:
        return str(e)
    return None


def model(name, blob, cap, extra=0):
    """The contract of include/kcdc.h over tests/zstd_model.py: (status, bytes)."""
    if len(blob) < 4 or blob[:4] != header(name):
        return EBADMSG, b""
    try:
        got, frames = zm.decode(blob[4:])
    except zm.Bad:
        try:  # a content size above the cap is found before any block is read
            frames = []
            zm.decode(blob[4:], entropy=False)
        except zm.Bad:
            pass
        return EBADMSG, b""
    if len(got) > cap:
        return EOVERFLOW, b""
    if descriptors(blob[4:]) > 4 + cap // 1024 + extra:
        return ENOMEM, b""
    return 0, got
