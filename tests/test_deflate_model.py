"""CPU: pins tests/deflate_model.py (the structural RFC 1951 reader and the code-length references
behind tests/test_gpu_deflate_edges.py) against zlib: its inflate on zlib's own streams of every
block type, its refusals on hand-built bad streams, and its length limiter (gen_bitlen) through
Z_HUFFMAN_ONLY streams of Fibonacci-count data, whose Huffman tree is deeper than 15."""
import zlib

import numpy as np
import pytest

import deflate_model as dm


def _inputs():
    rng = np.random.default_rng(1951)
    words = [b"kopia", b"snapshot", b"content", b"chunk", b"the", b"of", b"blob", b"index", b" ", b"\n"]
    return {
        "empty": b"",
        "one": b"k",
        "zeros": bytes(70000),
        "random": rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(),
        "text": b"".join(words[int(k)] for k in rng.integers(0, len(words), 30000)),
    }


INPUTS = _inputs()
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE}


def _raw(data, level, strategy, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("what", sorted(INPUTS))
def test_model_inflates_zlib_streams(what, level, strategy):
    data = INPUTS[what]
    raw = _raw(data, level, STRATEGIES[strategy])
    assert zlib.decompress(raw, -15) == data
    got, blocks = dm.inflate_blocks(raw)
    assert got == data
    assert blocks[-1].bfinal and not any(b.bfinal for b in blocks[:-1])
    assert blocks[-1].bit_off + blocks[-1].bit_len <= 8 * len(raw) < blocks[-1].bit_off + blocks[-1].bit_len + 8
    assert sum(b.out_len for b in blocks) == len(data)
    if level == 0:
        assert all(b.btype == 0 for b in blocks)
    elif strategy == "fixed":
        assert all(b.btype != 2 for b in blocks)  # fixed, or stored where that is shorter
    for b, nxt in zip(blocks, blocks[1:] + [None]):
        assert nxt is None or nxt.bit_off == b.bit_off + b.bit_len
        if b.btype == 0:
            assert b.stored_len == b.out_len
            continue
        assert b.bit_len == b.header_bits + dm.token_bits(b) + b.eob_bits
        assert b.lit_hist[dm.EOB] == 1 and sum(b.dist_hist) == len(b.matches)
        if b.btype == 2:  # what zlib sends is what the model's restatements of zlib give
            assert [s for s, _ in dm.rle_lengths(b.lens[:b.hlit])] + [s for s, _ in dm.rle_lengths(
                b.lens[dm.NLIT:dm.NLIT + b.hdist])] == [s for s, _ in b.cl_syms]  # zlib codes the two sets apart
            assert dm.code_cost(b.lit_hist, b.lens[:dm.NLIT]) == dm.code_cost(
                b.lit_hist, dm.zlib_limit(b.lit_hist, 15))
            assert dm.code_cost(b.cl_hist, b.cl_lens) == dm.code_cost(b.cl_hist, dm.zlib_limit(b.cl_hist, 7))
            if strategy == "huffman":
                assert not b.matches and b.lens[dm.NLIT:dm.NLIT + 2] == [1, 1]


# ---- hand-built bad streams
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= v << self.n
        self.n += n
        return self

    def code(self, code, n):  # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8 + 2, "little")  # two spare zero bytes after the stream


def _canon(lens):
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


CL8 = {s: 3 for s in (0, 1, 2, 3, 4, 16, 17, 18)}  # a complete code-length code


def _dyn(cl_syms, tokens=(), hlit=257, hdist=1, cl=CL8):
    """A final dynamic block: the code-length symbols as given, then tokens as (lit/len or
    distance code table index, symbol[, extra value, extra bits])."""
    cl_lens = [cl.get(s, 0) for s in range(19)]
    hclen = max(i for i, s in enumerate(dm.CL_ORDER) if cl_lens[s]) + 1
    w = Bits().put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(max(hclen, 4) - 4, 4)
    for i in range(max(hclen, 4)):
        w.put(cl_lens[dm.CL_ORDER[i]], 3)
    cc = _canon(cl_lens)
    seq = []
    for s, x in cl_syms:
        w.code(*cc[s])
        if s >= 16:
            w.put(x, dm.CL_EXTRA[s])
        seq += [s] if s < 16 else [seq[-1] if seq else 0] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x)
    seq += [0] * (hlit + hdist - len(seq))
    codes = (_canon(seq[:hlit]), _canon(seq[hlit:hlit + hdist]))
    for t in tokens:
        w.code(*codes[t[0]][t[1]])
        if len(t) > 2:
            w.put(t[2], t[3])
    return w.bytes()


Z254 = [(18, 127), (18, 105)]  # 254 zero lengths
GOOD = [(2, 0), (2, 0)] + Z254 + [(2, 0), (2, 0), (1, 0)]  # literals 0 and 1, end of block, length 3; one distance code
BAD = {
    "over-subscribed": _dyn([], cl={s: 1 for s in (16, 17, 18, 0)}),
    "incomplete code-length code": _dyn([], cl={0: 1, 18: 2}),
    "incomplete literal/length code": _dyn([(2, 0), (2, 0)] + Z254 + [(2, 0), (0, 0)], [(0, 256)]),
    "incomplete distance code": _dyn([(2, 0), (2, 0)] + Z254 + [(2, 0), (2, 0), (2, 0)], [(0, 256)]),
    "repeat without previous": _dyn([(16, 0)] + GOOD[1:]),
    "run past HLIT + HDIST": _dyn([(2, 0), (2, 0)] + Z254 + [(2, 0), (17, 0)], [(0, 256)]),
    "missing end of block": _dyn([(2, 0)] * 4 + [(18, 127), (18, 103), (0, 0), (0, 0)], [(0, 0)]),
    "distance beyond the output": _dyn(GOOD, [(0, 257), (1, 0), (0, 256)], hlit=258),
    "distance beyond the output, fixed": Bits().put(1, 1).put(1, 2).code(1, 7).code(0, 5).code(0, 7).bytes(),
    "LEN/NLEN mismatch": bytes([1, 3, 0, 0xFD, 0xFF, 1, 2, 3]),
    "block type 3": bytes([7, 0, 0]),
    "literal/length symbol 286": Bits().put(1, 1).put(1, 2).code(0b11000110, 8).code(0, 7).bytes(),
    "truncated": _raw(INPUTS["text"], 6, zlib.Z_DEFAULT_STRATEGY)[:-7],
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_model_rejects_what_zlib_rejects(what):
    raw = BAD[what]
    with pytest.raises(zlib.error):
        d = zlib.decompressobj(-15)
        d.decompress(raw)
        if not d.eof:
            raise zlib.error("incomplete stream")
    with pytest.raises(dm.InflateError):
        dm.inflate_blocks(raw.rstrip(b"\0") if what == "truncated" else raw)


def test_model_accepts_the_single_distance_code():
    """The builder's control: the one incomplete code inflaters take, a lone 1-bit distance code."""
    raw = _dyn(GOOD, [(0, 0), (0, 257), (1, 0), (0, 1), (0, 256)], hlit=258)
    assert zlib.decompress(raw, -15) == b"\0\0\0\0\1"
    got, (b,) = dm.inflate_blocks(raw)
    assert got == b"\0\0\0\0\1" and b.tokens == [0, (3, 1, 257, 0), 1]
    assert (b.hlit, b.hdist, b.hclen) == (258, 1, 18) and b.lens[dm.NLIT:dm.NLIT + 2] == [1, 0]
    assert b.cl_syms == GOOD


# ---- the code-length references
def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _fib_data(nsym, seed):
    rng = np.random.default_rng(seed)
    syms = rng.permutation(256)[:nsym]
    data = np.repeat(syms.astype(np.uint8), _fib(nsym + 1)[1:])  # 1, 2, 3, 5, ...: the end of block is the other 1
    rng.shuffle(data)
    return data.tobytes()


@pytest.mark.parametrize("nsym", [16, 17, 18, 19, 20])
def test_zlib_limit_is_zlibs(nsym):
    """Z_HUFFMAN_ONLY makes no matches, so the block's histogram is the data's plus the end of
    block; with memLevel 9 fewer than 32,768 bytes are one block.  Fibonacci counts make the
    unrestricted tree as deep as it has symbols: zlib's limiter runs, and the restatement agrees."""
    data = _fib_data(nsym, nsym)
    assert len(data) < 32768
    raw = _raw(data, 6, zlib.Z_HUFFMAN_ONLY, mem=9)
    got, blocks = dm.inflate_blocks(raw)
    assert got == data and len(blocks) == 1 and blocks[0].btype == 2
    b = blocks[0]
    hist = [int(x) for x in np.bincount(np.frombuffer(data, np.uint8), minlength=dm.NLIT)]
    hist[dm.EOB] = 1
    assert b.lit_hist == hist
    opt, depth = dm.huffman_cost(hist)
    assert depth == nsym > 15
    assert max(b.lens[:dm.NLIT]) == 15
    want = dm.zlib_limit(hist, 15)
    assert max(want) == 15 and dm.kraft(want)[0] == dm.kraft(want)[1]
    cost = dm.code_cost(hist, b.lens[:dm.NLIT])
    assert cost == dm.code_cost(hist, want)
    pm = dm.package_merge(hist, 15)
    assert max(pm) <= 15 and dm.kraft(pm)[0] == dm.kraft(pm)[1]
    assert opt < dm.code_cost(hist, pm) <= cost


def _histograms():
    rng = np.random.default_rng(7)
    out = [_fib(n) for n in (2, 3, 9, 12, 19, 25)]
    out += [[int(x) for x in rng.geometric(p, 60)] for p in (0.5, 0.05, 0.001)]
    out += [[int(x) for x in rng.integers(0, 4, 286)], [1] * 286, [1 << k for k in range(20)],
            [0, 0, 7, 0], [0] * 5, [3, 0, 3], [int(x) for x in np.bincount(np.minimum(rng.geometric(0.03, 30000), 285))]]
    return out


@pytest.mark.parametrize("maxb", [5, 7, 9, 11, 15])
def test_package_merge_bounds(maxb):
    """package_merge is complete, within the limit, never costlier than zlib's heuristic, and is
    the Huffman optimum whenever the optimal tree of least depth fits the limit."""
    bit = 0
    for h in _histograms():
        used = sum(1 for c in h if c)
        if used > 1 << maxb:
            continue
        pm = dm.package_merge(h, maxb)
        opt, depth = dm.huffman_cost(h)
        cost = dm.code_cost(h, pm)
        assert max(pm, default=0) <= maxb and all((l > 0) == (c > 0) for c, l in zip(h, pm))
        if used >= 2:
            assert dm.kraft(pm)[0] == dm.kraft(pm)[1]
            zl = dm.zlib_limit(h, maxb)
            assert max(zl) <= maxb and dm.kraft(zl)[0] == dm.kraft(zl)[1]
            assert cost <= dm.code_cost(h, zl)
        assert cost >= opt
        if depth <= maxb:
            assert cost == opt
        else:
            assert cost > opt
            bit += 1
    assert bit >= 2, "the limit never bit"


def test_rle_lengths_edges():
    z = lambda n: [0] * n
    assert dm.rle_lengths(z(2)) == [(0, 0), (0, 0)]
    assert dm.rle_lengths(z(3)) == [(17, 0)] and dm.rle_lengths(z(10)) == [(17, 7)]
    assert dm.rle_lengths(z(11)) == [(18, 0)] and dm.rle_lengths(z(138)) == [(18, 127)]
    assert dm.rle_lengths(z(139)) == [(18, 127), (0, 0)]
    assert dm.rle_lengths(z(141)) == [(18, 127), (17, 0)] and dm.rle_lengths(z(149)) == [(18, 127), (18, 0)]
    assert dm.rle_lengths([5] * 3) == [(5, 0)] * 3 and dm.rle_lengths([5] * 4) == [(5, 0), (16, 0)]
    assert dm.rle_lengths([5] * 7) == [(5, 0), (16, 3)] and dm.rle_lengths([5] * 8) == [(5, 0), (16, 3), (5, 0)]
    assert dm.rle_lengths([5] * 10) == [(5, 0), (16, 3), (16, 0)]
    assert dm.rle_lengths([3, 3, 0, 0, 0, 4]) == [(3, 0), (3, 0), (17, 0), (4, 0)]
