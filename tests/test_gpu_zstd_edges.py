"""GPU: the zstd span encoder's blocks, tables and limits, asserted structurally.

tests/test_gpu_compress.py asks of every zstd frame whether libzstd decodes it back; that is blind
to the branches its inputs never reach and to valid but wasteful streams.  Here every case is read
back with tests/zstd_model.py's detail records and asserts, in this order:
  1. libzstd, the model and the device decoder (status 0) each return the input; the header ID is
     the content manager's keep-or-drop one, the length within compress_bound;
  2. the regime: the branch the input was built for shows in the records (tests/zstd_structure.py
     regimes(); a case that misses its branch fails);
  3. the invariants of tests/zstd_structure.py on every span.
run() is step 1, the test's own assertions step 2, invariants() step 3; what the invariants return
(a span's length-limit side, its tree description sizes) is asserted after them.
Every case runs at lead 0 and at an odd lead (the span staged misaligned: stage_span's d).

The planner facts the inputs rely on (kcdc_compress.hip): a span is 32 KiB, a segment 512 bytes; a
match is >= 4 bytes, ends with its segment and finds its source in the span alone: at the latest
position of its 6-bit hash in the segment, at the previous match's distance, among the 32 nearest
distances at a segment's start, at the three previous segments' latest entries and at the span's
first position of its 11-bit hash (ftab).  So a span's first segment (its head) is the source these
inputs copy from: a copy of the head's first bytes is always found (position 0 is the first of its
hash), and so is each 4-byte token of the head that is the first of its own hash (Build places
them so, on the CPU).  A parse position is skipped after 32 (zstd) or 256 (zstd-best-compression)
literals without a match, one more per that many: literal runs here end where both still look.
A span's four blocks are runs of segments of about equal cost, a sequence 1 and a segment 4
(plan() restates the cut; the builders assert their intent against it on the CPU)."""
import random

import numpy as np
import pytest

import zstd_structure as zs
from kopia_amd import compression as kc
from oracle import deflate

pytestmark = pytest.mark.gpu
SPAN, SEG = zs.SPAN, zs.SEG
NAMES = ("zstd", "zstd-best-compression")
LEADS = (0, 37)
both = pytest.mark.parametrize("name,lead", [(n, ld) for n in NAMES for ld in LEADS])
leads = pytest.mark.parametrize("lead", LEADS)
EFFORT = {"zstd-fastest": 0, "zstd": 1, "zstd-best-compression": 2, "zstd-better-compression": 2}


# ------------------------------------------------------------------ running and reading back
def compress(name, chunks, dev, lead=0):
    """Compress the chunks in one launch, the first at byte `lead` of the device buffer (so spans
    start misaligned); returns each chunk's content (header ID and frame) as bytes."""
    import torch
    host = np.concatenate([np.zeros(lead, np.uint8)] + [np.frombuffer(c, np.uint8) for c in chunks] + [np.zeros(8, np.uint8)])
    lens = [len(c) for c in chunks]
    offs = [lead + int(x) for x in np.cumsum([0] + lens[:-1])]
    d = torch.from_numpy(host).to(dev)
    oo, total = kc.compressed_layout(lens)
    out = torch.full((total,), 0xAB, dtype=torch.uint8, device=dev)
    ol, ids = kc.Compressor(name).compress_chunks_device(d.data_ptr(), offs, lens, out, oo, dev)
    torch.cuda.synchronize()
    out, ol, ids = out.cpu().numpy(), ol.cpu().numpy(), ids.cpu().numpy()
    blobs = []
    for i, n in enumerate(lens):
        blob = out[oo[i]:oo[i] + ol[i]].tobytes()
        assert ids[i] == deflate.kept_header_id(name, n, len(blob)), i
        assert len(blob) <= kc.compress_bound(n), (i, n, len(blob))
        blobs.append(blob)
    return blobs


def device_decode(name, blobs, lens, dev):
    import torch
    comp = np.frombuffer(b"\0" + b"".join(blobs), np.uint8).copy()
    bo = [1 + int(x) for x in np.cumsum([0] + [len(b) for b in blobs[:-1]])]
    oo = [int(x) for x in np.cumsum([0] + lens[:-1])]
    d_out = torch.full((sum(lens) + 8,), 0xCD, dtype=torch.uint8, device=dev)
    d_comp = torch.from_numpy(comp).to(dev)  # (kept until the call has finished)
    ln, st = kc.Compressor(name).zstd_decode_chunks_device(d_comp.data_ptr(), bo, [len(b) for b in blobs], d_out, oo, lens, dev)
    torch.cuda.synchronize()
    del d_comp
    assert not st.cpu().numpy().any(), st
    assert ln.cpu().numpy().tolist() == lens
    return d_out.cpu().numpy()[:sum(lens)].tobytes()


def run(name, lead, chunks, dev):
    """Step 1 for every chunk: the device decoder, libzstd and the model (zs.read) return the input;
    returns their Readings.  The test asserts its regime on them, then calls invariants()."""
    chunks = [bytes(c) for c in chunks]
    assert sum(len(c) for c in chunks) <= 1 << 20
    blobs = compress(name, chunks, dev, lead)
    assert device_decode(name, blobs, [len(c) for c in chunks], dev) == b"".join(chunks)
    out = []
    for data, blob in zip(chunks, blobs):
        assert deflate.decompress(name, blob) == data
        r = zs.read(blob[4:], data)
        r.effort = EFFORT[name]
        out.append(r)
    return out


def invariants(readings):
    """Step 3: every invariant of tests/zstd_structure.py on every span (each span's length-limit
    regime and tree description sizes are left in span.limit and span.desc)."""
    for r in readings:
        zs.check_reading(r, r.effort)


def reached(readings):
    """(all regimes, per chunk: per span its regimes)."""
    per = [[zs.regimes(sp) for sp in r.spans] for r in readings]
    return set().union(*[s for c in per for s in c]), per


def lit_counts(readings):
    return [[[len(b.lits) for b in sp.coded] for sp in r.spans] for r in readings]


# ------------------------------------------------------------------ inputs
def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def skewed(seed, lo=32, rate=0.05, hi=230):
    """A source of text-like bytes: lo + a geometric step, at most hi."""
    r = random.Random(seed)
    return lambda: min(hi, lo + int(r.expovariate(rate)))


def uniform(seed):
    r = random.Random(seed)
    return lambda: r.randrange(256)


def no_repeat(n, draw, seen=None, tail=b""):
    """n bytes from draw() in which no 4 bytes occur twice (nor in `seen`): nothing for a match."""
    seen = set() if seen is None else seen
    out = bytearray(tail)
    k0 = len(out)
    while len(out) - k0 < n:
        for _ in range(200):
            c = draw()
            g = bytes(out[-3:]) + bytes([c])
            if len(g) < 4 or g not in seen:
                break
        else:
            raise AssertionError("no byte left that makes a new 4-gram")
        out.append(c)
        if len(g) == 4:
            seen.add(g)
    return bytes(out[k0:])


KMUL = 0x1E35A7BD


def bucket(b4):
    return ((int.from_bytes(b4, "little") * KMUL) & 0xFFFFFFFF) >> 21


def looked_at(skip):
    """The positions of a segment the parse looks at while it finds no match."""
    x, out = 0, set()
    while x <= SEG - 4:
        out.add(x)
        x += 1 + (x >> skip)
    return out


RUNS = sorted(looked_at(5) & looked_at(8))  # literal runs that end where both efforts look


def split_run(n, k):
    """n literals as k runs of RUNS (each at most 508: room for the copy that ends the segment)."""
    if k == 1:
        assert n in RUNS, n
        return [n]
    for j in sorted((j for j in RUNS if j <= min(n, 508)), key=lambda j: abs(j - n // k)):
        if n - j <= 508 * (k - 1):
            try:
                return [j] + split_run(n - j, k - 1)
            except AssertionError:
                continue
    raise AssertionError((n, k))


def plan(costs):
    """The segments' block numbers, as zstd_emit_kernel cuts a span: a segment belongs to block q while
    its middle lies within q + 1 quarters of the span's cost (each block at least one segment)."""
    tot, ci, mids = sum(costs), 0, []
    for c in costs:
        ci += c
        mids.append(2 * ci - c)
    b = [sum(1 for m in mids if 2 * m <= q * tot) for q in (1, 2, 3)]
    b[0] = min(max(b[0], 1), 61)
    b[1] = min(max(b[1], b[0] + 1), 62)
    b[2] = min(max(b[2], b[1] + 1), 63)
    return [sum(1 for e in b if i >= e) for i in range(len(costs))]


class Build:
    """One span, segment by segment.  Its head (segment 0) is 512 literals that no later literal run
    repeats a 4-gram of; its first bytes are the tokens, each the first position of its ftab hash."""

    def __init__(self, draw, ntok=0):
        self.draw, self.seen = draw, set()
        self.tok = []
        head = bytearray()
        firsts, taken = set(), set()
        for t in range(ntok):
            for _ in range(4000):
                cand = bytes([draw() for _ in range(4)])
                trial = bytes(head[-3:]) + cand
                grams = [trial[i:i + 4] for i in range(len(trial) - 3)]
                if cand[0] in firsts or any(g in self.seen for g in grams) or bucket(cand) in taken or len(set(grams)) < len(grams):
                    continue
                if len({bucket(g) for g in grams} | taken) < len(grams) + len(taken):
                    continue
                break
            else:
                raise AssertionError("no token left")
            head += cand
            firsts.add(cand[0])
            for g in grams:
                self.seen.add(g)
                taken.add(bucket(g))
            self.tok.append(cand)
        self.head = bytes(head) + no_repeat(SEG - len(head), draw, self.seen, bytes(head[-3:]))
        assert len(self.head) == SEG
        self.data = bytearray(self.head)
        self.costs, self.lits, self.want = [4], [SEG], []
        self.walk = None

    def _run(self, n):
        return no_repeat(n, self.draw, self.seen, bytes(self.data[-3:]))

    def using(self, draw):
        """The literals from here on come from `draw`."""
        self.draw = draw
        return self

    def units(self, specs, pad=True):
        """(ll, ml) pairs: ll fresh literals, then the head's first ml bytes (the byte after them is not the
        head's next one, so the match ends there); a unit does not cross a segment, and the span's
        last segment is filled with literals."""
        for ll, ml in specs:
            room = SEG - len(self.data) % SEG
            if room < ll + ml + 1:
                self.data += self._run(room)
            self.data += self._run(ll) + self.head[:ml]
            for _ in range(100):
                c = self._run(1)
                if c[0] != self.head[ml]:
                    break
            self.data += c
        if pad and len(self.data) % SEG:
            self.data += self._run(SEG - len(self.data) % SEG)
        return self

    def literal(self, k=1):
        for _ in range(k):
            self.data += self._run(SEG)
            self.costs.append(4)
            self.lits.append(SEG)
        return self

    def part(self, j):
        """j literals, then the head's first bytes to the segment's end: one match."""
        self.data += self._run(j) + self.head[:SEG - j]
        self.costs.append(5)
        self.lits.append(j)
        return self

    def parts(self, n, k):
        for j in split_run(n, k):
            self.part(j)
        return self

    def copies(self, k):
        for _ in range(k):
            self.part(0)
        return self

    def dense(self, k=1, ntok=128):
        """k segments of ntok tokens (and literals to the segment's end), no pair of tokens twice in
        the span nor next to each other in the head: matches of 4 bytes."""
        n = len(self.tok)
        if self.walk is None:
            assert n > 2 and all(n % p for p in range(2, n)), "a prime number of tokens"
            self.walk = (self.tok[(i * d) % n] for d in range(2, n - 1) for i in range(n))
        for _ in range(k):
            seg = b"".join(next(self.walk) for _ in range(ntok))
            self.data += seg + self._run(SEG - len(seg))
            self.costs.append(4 + ntok)
            self.lits.append(SEG - len(seg))
        return self

    def blocks(self):
        """Per planned block: (segments, literals)."""
        p = plan(self.costs)
        return [(p.count(q), sum(n for n, b in zip(self.lits, p) if b == q)) for q in range(4) if q in p]

    def bytes(self):
        return bytes(self.data)


# ------------------------------------------------------------------ literal counts per block
@both
def test_raw_literals_header_at_31_32(name, lead, gpu):
    """kcdc_compress.hip:1825 (rawlh) and :2019 on: the raw literals header grows from 1 to 2 bytes at
    32 literals.  Four one-segment blocks: the head, then 31, 32 and 34 uniform literals before a copy
    (zstd does not look at position 33 of a run)."""
    b = Build(uniform(3)).part(31).part(32).part(34)
    assert [n for _, n in b.blocks()] == [512, 31, 32, 34]
    rd = run(name, lead, [b.bytes()], gpu)
    sp = rd[0].spans[0]
    assert sp.kinds == "Rrrr", sp.kinds
    assert [(len(x.lits), x.lit_hlen, len(x.seqs)) for x in sp.coded] == [(31, 1, 1), (32, 2, 1), (34, 2, 1)]
    invariants(rd)


@both
def test_raw_literals_header_at_4095_4096(name, lead, gpu):
    """kcdc_compress.hip:1825: the raw literals header grows from 2 to 3 bytes at 4096 literals.
    Uniform literals (try_huff is false, :1469), so the blocks keep them raw: block 0 holds the
    head, literal segments and runs to 4095 (4096) literals, then copies that make it smaller than
    its bytes; the other three blocks are copies."""
    spans = []
    for n in (4095, 4096):
        b = Build(uniform(n)).literal(5).parts(n - 6 * 512, 3).copies(7)
        b.copies(48)
        assert b.blocks()[0][1] == n and len(b.costs) == 64, b.blocks()
        spans.append(b.bytes())
    rd = run(name, lead, spans, gpu)
    got = [(len(r.spans[0].coded[0].lits), r.spans[0].coded[0].lit_hlen, r.spans[0].coded[0].lit_type) for r in rd]
    assert got == [(4095, 2, 0), (4096, 3, 0)], (got, lit_counts(rd))
    assert all("literals: no Huffman in the span" in zs.regimes(r.spans[0]) for r in rd)
    invariants(rd)


@both
def test_huffman_streams_at_1023_1024_1025(name, lead, gpu):
    """kcdc_compress.hip:1629 (nstr) and :1830 (hlh): 1 stream up to 1023 literals, 4 from 1024 (each of
    the first three a quarter rounded up, :1630; 1025 leaves a ragged last one).  Text-like
    literals; block 0 is the head and runs to the count, then copies."""
    spans = []
    for n in (1023, 1024, 1025):
        b = Build(skewed(n)).parts(n - 512, 2).copies(13)
        b.copies(48)
        assert b.blocks()[0][1] == n and len(b.costs) == 64, b.blocks()
        spans.append(b.bytes())
    rd = run(name, lead, spans, gpu)
    got = [(len(r.spans[0].coded[0].lits), r.spans[0].coded[0].streams, r.spans[0].coded[0].lit_hlen, r.spans[0].kinds[0]) for r in rd]
    assert got == [(1023, 1, 3, "h"), (1024, 4, 4, "h"), (1025, 4, 4, "h")], (got, lit_counts(rd))
    assert "literals: ragged last stream" in zs.regimes(rd[2].spans[0])
    invariants(rd)
    assert all(r.spans[0].full and r.spans[0].limit == "optimal" for r in rd)


@both
def test_huffman_header_at_16383_16384(name, lead, gpu):
    """kcdc_compress.hip:1830: the 4-stream literals header grows from 4 to 5 bytes past 16383 literals.
    A cost-skewed span: the head and literal segments first (4 a segment), token-dense segments last
    (132 a segment), so block 0 takes more than half the span's bytes: 16383, 16384 and about 17000
    literals in it (a token-dense segment may add one of its own)."""
    spans = []
    for n in (16383, 16384, 17000):
        k = n // 512 - 2
        b = Build(skewed(n), ntok=67).literal(k).parts(n - 512 * (k + 1), 3)
        b.dense(64 - len(b.costs))
        assert b.blocks()[0][1] == n and len(b.costs) == 64, b.blocks()
        spans.append(b.bytes())
    rd = run(name, lead, spans, gpu)
    got = [(len(r.spans[0].coded[0].lits), r.spans[0].coded[0].streams, r.spans[0].coded[0].lit_hlen) for r in rd]
    assert got[:2] == [(16383, 4, 4), (16384, 4, 5)] and got[2][1:] == (4, 5) and 16384 < got[2][0] < 17100, (got, lit_counts(rd))
    assert all(r.spans[0].kinds[0] == "h" for r in rd)
    invariants(rd)


# ------------------------------------------------------------------ literals kinds
def words(n, seed=0):
    r = random.Random(seed)
    w = [b"kopia", b"snapshot", b"content", b"chunk", b"the", b"of", b"blob", b"index", b"manifest", b"epoch"]
    out = bytearray()
    while len(out) < n:
        out += r.choice(w) + (b" " if r.random() < 0.8 else b",\n")
    return bytes(out[:n])


@both
def test_literals_kinds(name, lead, gpu):
    """kcdc_compress.hip:1469 (try_huff), :1827-1835 (the Huffman section against the raw one, the tree on
    the first block that uses it) and :2007 (Compressed / Treeless): one literal symbol and
    near-uniform literals take no Huffman code; the tree rides on block 1 after a Raw_Block 0
    (16 segments of uniform literals, then text-like ones: blocks of 16 match-free segments); on
    block 2 after a literal-free block 1 (zeros; a span's first byte is a literal, so block 0
    cannot be literal-free: it keeps its one literal raw); a Raw_Block lies between two Huffman
    blocks; every later block is Treeless; a block of 6 literals keeps them raw beside its
    Huffman neighbours."""
    tiny = Build(skewed(5)).literal(15).copies(6).part(6).copies(6).copies(13).literal(16)
    assert tiny.blocks() == [(16, 8192), (13, 6), (13, 0), (16, 8192)], tiny.blocks()
    chunks = [
        bytes(SPAN),                                                                           # 0: one literal symbol
        Build(uniform(9)).literal(15).copies(48).bytes(),                                     # 1: near-uniform literals
        Build(uniform(10)).literal(15).using(skewed(10)).literal(48).bytes(),                 # 2: Raw_Block 0
        bytes(16384) + Build(skewed(11)).literal(31).bytes(),                                  # 3: literal-free block 1
        Build(skewed(12)).literal(15).using(uniform(12)).literal(16).using(skewed(13)).literal(32).bytes(),  # 4: a Raw_Block between
        tiny.bytes(),                                                                          # 5: raw literals beside the tree
    ]
    rd = run(name, lead, chunks, gpu)
    _, per = reached(rd)
    want = [{"literals: no Huffman in the span"}, {"literals: no Huffman in the span", "literals: raw, 3-byte header"},
            {"tree: after a Raw_Block", "tree: Treeless after it"}, {"tree: after a literal-free block", "tree: Treeless after it"},
            {"tree: a Raw_Block between Huffman blocks", "tree: Treeless after it"}, {"tree: raw literals kept beside it", "tree: Treeless after it"}]
    for k, (w, got) in enumerate(zip(want, per)):
        assert w <= got[0], (k, rd[k].spans[0].kinds, sorted(w - got[0]), lit_counts(rd)[k])
    assert rd[2].spans[0].kinds == "Rhtt" and rd[4].spans[0].kinds == "hRtt", [r.spans[0].kinds for r in rd]
    assert rd[5].spans[0].kinds == "hrrt" and [len(b.lits) for b in rd[5].spans[0].coded] == [8192, 6, 0, 8192]
    assert sum(rd[0].spans[0].H) == rd[0].spans[0].H[0] <= 64
    invariants(rd)


# ------------------------------------------------------------------ weights
def over_alphabet(top, n, seed, lo=0):
    """n no-repeat literals over lo..top, geometric from the bottom, every value present."""
    r = random.Random(seed)
    vals = list(range(lo, top + 1))

    def draw():
        return vals[min(len(vals) - 1, int(r.expovariate((2.5 if len(vals) < 48 else 12.0) / len(vals))))]
    body = no_repeat(min(n if len(vals) < 48 else 4 * n, len(vals) ** 4 // 6) - len(vals), draw)
    if len(vals) < 48:
        return bytes(r.sample(vals, len(vals))) + body
    out = list(body)  # every value once, spread out (at the start they would make block 0 a Raw_Block)
    for k, v in enumerate(r.sample(vals, len(vals))):
        out.insert(k * len(out) // len(vals), v)
    return bytes(out)


@both
def test_weights_direct_and_fse(name, lead, gpu):
    """kcdc_compress.hip:1520-1577: direct weights or FSE-compressed ones, the smaller (:1569); above
    symbol 128 FSE alone (:1524).  A sweep of alphabets 0..top: the smallest top at which FSE wins
    shows as the first FSE tree, the one before it direct; top 129, 130, 254 and 255 force FSE over
    an odd and an even count of weights (the two-state start, :1551-1560).
    The FSE stream cannot pass 127 bytes (:1533, :1566): the weights 0..11 of a complete code obey
    Kraft's sum, so at most 2^k symbols have one of the k + 1 heaviest weights; the 255 weights of
    the largest tree then carry under 2.6 bits of entropy each, about 85 bytes with the table's
    rounding, and the description adds at most 10."""
    tops = list(range(6, 40)) + [129, 130, 254, 255]
    chunks = [over_alphabet(t, 1500, t) for t in tops]
    rd = run(name, lead, chunks, gpu)
    kinds = []
    for t, r in zip(tops, rd):
        assert len(r.spans) == 1 and r.spans[0].full and r.spans[0].tree is not None, (t, r.spans[0].kinds)
        sp = r.spans[0]
        assert len(sp.tree.weights) - 1 == t
        kinds.append(sp.tree.tree_kind)
    assert kinds[-4:] == ["fse"] * 4
    got, _ = reached(rd[-4:])
    assert {"weights: FSE over an odd count", "weights: FSE over an even count", "weights: FSE, top > 128"} <= got
    small = kinds[:-4]
    assert "direct" in small and "fse" in small, list(zip(tops, kinds, [r.spans[0].desc for r in rd]))
    first = small.index("fse")
    assert first > 0 and set(small[:first]) == {"direct"}, list(zip(tops, kinds))
    assert "weights: FSE, top <= 128" in reached(rd[:-4])[0]
    invariants(rd)
    assert all(r.spans[0].desc[0] == k for r, k in zip(rd, kinds))
    d = rd[first].spans[0].desc  # the switch: there both forms exist and FSE is the smaller, one symbol before it is not
    assert d[2] < d[1] and rd[first - 1].spans[0].desc[2] >= rd[first - 1].spans[0].desc[1]


# ------------------------------------------------------------------ length limit
def with_counts(counts, seed):
    """Literals with exactly these counts per byte value, no 4 bytes twice: no match, so the span's
    histogram is the counts."""
    r = random.Random(seed)
    for _ in range(50):
        left = dict(counts)
        seen, out = set(), bytearray()
        ok = True
        while left:
            vals = list(left)
            wts = [left[v] for v in vals]
            for _ in range(60):
                c = r.choices(vals, wts)[0]
                g = bytes(out[-3:]) + bytes([c])
                if len(g) < 4 or g not in seen:
                    break
            else:
                ok = False
                break
            out.append(c)
            seen.add(g)
            left[c] -= 1
            if not left[c]:
                del left[c]
        if ok:
            return bytes(out)
    raise AssertionError("no arrangement without a repeated 4-gram")


def deep_counts(tail, flat, each):
    """Fibonacci-like counts (a chain `tail` deep) under `flat` symbols of `each`: the flat top keeps
    4-grams from repeating, the chain sets the depth."""
    fib = [1, 1]
    while len(fib) < tail:
        fib.append(fib[-1] + fib[-2])
    c = {40 + k: v for k, v in enumerate(fib)}
    c.update({80 + k: each for k in range(flat)})
    return c


@both
def test_length_limit(name, lead, gpu):
    """kcdc_compress.hip:1473 (huff_lengths(..., 11, ...)): a histogram whose optimal tree is deeper than 11
    is limited (cost between package-merge and zlib's limiter), one whose optimum is exactly 11
    deep is kept (cost equal).  No 4 bytes occur twice, so nothing matches, every block is a
    literal-only Compressed_Block (:1838, the single byte 0) and H is the planted counts."""
    deep, edge = deep_counts(13, 24, 100), deep_counts(9, 8, 60)
    assert zs.dm.huffman_cost(list(deep.values()))[1] > 11 and zs.dm.huffman_cost(list(edge.values()))[1] == 11
    chunks = [with_counts(deep, 1), with_counts(edge, 2)]
    rd = run(name, lead, chunks, gpu)
    for r, c in zip(rd, (deep, edge)):
        assert all(sp.full for sp in r.spans)
        for sp in r.spans:
            assert set(sp.kinds) <= {"h", "t"} and not sp.seqs, sp.kinds
        H = [sum(sp.H[s] for sp in r.spans) for s in range(256)]
        assert H == [c.get(s, 0) for s in range(256)]
    assert len(rd[0].spans) == 1 and len(rd[1].spans) == 1
    a, b = rd[0].spans[0], rd[1].spans[0]
    assert a.tree.maxbits == 11 and "code: optimum deeper than 11" in zs.regimes(a)
    assert b.tree.maxbits == 11 and "code: optimum depth 11" in zs.regimes(b)
    assert "sequences: none in a block" in zs.regimes(a)
    invariants(rd)
    assert a.limit == "limited" and b.limit == "optimal"  # (which side of the cost rule each span was held to)


# ------------------------------------------------------------------ sequence counts per block
@both
def test_sequence_counts(name, lead, gpu):
    """kcdc_compress.hip:1838 (sh: Number_of_Sequences in 1 byte under 128, else 2) and :2036 on: blocks of
    1, 127 and 128 sequences (one segment each: a copy; 127 and 128 four-byte tokens), and the most
    a span holds: 63 segments of 128 tokens behind the head, 8064 sequences, 2016 or more a block."""
    b = Build(uniform(7), ntok=97).dense(1, 127).dense(1, 128).part(0)
    assert [s for s, _ in b.blocks()] == [1, 1, 1, 1]
    full = Build(uniform(8), ntok=97).dense(63)
    rd = run(name, lead, [b.bytes(), full.bytes()], gpu)
    sp = rd[0].spans[0]
    assert [len(x.seqs) for x in sp.coded] == [127, 128, 1], (sp.kinds, [len(x.seqs) for x in sp.coded])
    assert [x.nseq_bytes for x in sp.coded] == [1, 2, 1]
    sp = rd[1].spans[0]
    assert sp.nseq == 63 * 128 and "sequences: 2000 or more in a block" in zs.regimes(sp), (sp.kinds, [len(x.seqs) for x in sp.coded])
    assert all(q[1] == 4 for q in sp.seqs)
    invariants(rd)


# ------------------------------------------------------------------ table modes and shapes
def pool():
    """Spans for the table tests: (name of the case, bytes, the regimes it is built to reach[, the one
    compressor under which it must])."""
    T, N, D = "tables: ", "normalisation: ", "description: zero run of "
    out = []
    # copies of the head alone: one match length; literal lengths 0 and 512 only, codes far apart
    out.append(("copies", Build(uniform(20)).copies(63).bytes(),
                {T + "ML RLE", T + "ML Repeat after RLE", T + "LL log 5", T + "OF log 5", D + "24 or more"}))
    # 3 sequences in blocks 1 to 3 (block 0, the head, is a Raw_Block)
    out.append(("three-parts", Build(uniform(21)).part(31).part(32).part(33).bytes(),
                {T + "LL Predefined", T + "LL Repeat after Predefined", T + "carried by a later block"}))
    # 8064 matches of 4 bytes
    out.append(("tokens", Build(uniform(22), ntok=97).dense(63).bytes(),
                {T + "LL FSE_Compressed", T + "LL Repeat after FSE_Compressed", T + "OF FSE_Compressed", T + "OF Repeat after FSE_Compressed",
                 T + "LL log 9", T + "OF log 8", N + "deficit of several", D + "24 or more"}))
    out.append(("words", words(SPAN, 5),
                {T + "ML FSE_Compressed", T + "ML Repeat after FSE_Compressed", T + "ML log 9", D + "1-2", D + "3-23"}))
    # 40 sequences, 40 match length codes: no description pays
    out.append(("forty", ml_forty(11), {T + "ML Predefined", T + "ML Repeat after Predefined", T + "carried by a later block"}))
    # the head itself 16 literals and 16 bytes of it again, and so on: one LL code, one ML code
    x = Build(uniform(13))
    x.data = bytearray()
    # (a unit's first literal is no other's nor the head's first byte, which follows the source at 0: the
    # match ends at 16; its last literal is no other's nor the head's 16th: no match begins a byte early)
    firsts = [v for v in range(256) if v != x.head[0]]
    lasts = [v for v in range(256) if v != x.head[15]]
    for k in range(254):
        first = bytes([firsts[k]])
        x.data += (x.head[:16] if k == 0 else first + no_repeat(14, x.draw, x.seen, first) + bytes([lasts[k]])) + x.head[:16]
    out.append(("ll-ml-one-code", x.bytes(), {T + "LL RLE", T + "LL Repeat after RLE", T + "ML RLE"}))
    # each token of the head once, 9 KiB and more behind it: one OF code (no distance twice); 4 bytes
    # each (one ML code), or 8 and 16 bytes behind 0 to 15 literals
    r = random.Random(14)
    far = Build(uniform(14), ntok=97).literal(18)
    three = Build(uniform(15), ntok=97).literal(18)
    for k in range(30):
        far.data += far._run(12) + far.tok[k]
        three.data += three._run(r.randrange(16)) + three.head[16 * (k % 24):16 * (k % 24) + (8 if k % 3 else 16)]
        for b in (far, three):
            b.data += b._run(1)
    for b in (far, three):
        b.data += b._run(SEG - len(b.data) % SEG)
        b.literal(4)
    out.append(("of-one-code", far.bytes(), {T + "OF RLE", T + "ML RLE", T + "carried by a later block"}))
    out.append(("of-one-code-ml-two", three.bytes(),
                {T + "OF RLE", T + "OF Repeat after RLE", T + "LL Predefined", T + "ML FSE_Compressed", T + "ML log 5",
                 T + "three different modes in the carrier"}))
    # 6 sequences, 6 offset codes
    sp = Build(uniform(16)).part(31)
    for k in (1, 2, 4, 8, 16):
        sp.literal(k).part(31)
    out.append(("spread-offsets", sp.bytes(), {T + "OF Predefined", T + "OF Repeat after Predefined"}))
    # 200 matches of 20 and one of each of 43 other ML codes: more codes than a table of 32 cells holds
    mix = [(1, 20)] * 200 + [(1, m) for m in list(range(4, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131]]
    random.Random(17).shuffle(mix)
    out.append(("ml-43-codes", Build(uniform(17)).units(mix).bytes(), {T + "log raised for the used codes", T + "ML log 6"}))
    out.append(("ml-two-codes", Build(uniform(18)).units([(1, 20), (1, 24), (2, 20)] * 40).bytes(),
                {T + "LL log 5", T + "OF log 5", T + "ML log 5"}))
    # the rounding surplus hangs on the parse: copies of every length behind one literal reach it under
    # zstd, literal lengths 0..22 before matches of 6 to 8 under zstd-best-compression (each alone)
    out.append(("lengths", ml_mix(9), {N + "surplus"}, "zstd"))
    out.append(("ll-spread", Build(uniform(19)).units([(k % 23, 6 + k % 3) for k in range(300)]).bytes(), {N + "surplus"},
                "zstd-best-compression"))
    return out


def ml_mix(seed):
    """Copies of the head of every length 4..130 behind one literal each."""
    b = Build(uniform(seed))
    r = random.Random(seed)
    data = bytearray(b.head)
    m = 4
    while len(data) + 140 < SPAN:
        room = SEG - len(data) % SEG
        if room < m + 1:
            data += no_repeat(room, b.draw, b.seen, bytes(data[-3:]))
            continue
        data += no_repeat(1, b.draw, b.seen, bytes(data[-3:])) + b.head[:m]
        m = 4 + (m - 3 + r.randrange(3)) % 127
    return bytes(data)


def ml_forty(seed):
    """About 40 sequences over more than 31 match length codes: the log is raised to hold them."""
    b = Build(uniform(seed))
    data = bytearray(b.head)
    for m in list(range(4, 36)) + [37, 39, 41, 43, 47, 51, 59, 67]:
        room = SEG - len(data) % SEG
        if room < m + 2:
            data += no_repeat(room, b.draw, b.seen, bytes(data[-3:]))
        data += no_repeat(1, b.draw, b.seen, bytes(data[-3:])) + b.head[:m]
    data += no_repeat(SEG - len(data) % SEG, b.draw, b.seen, bytes(data[-3:]))
    return bytes(data)


MODES = [f"tables: {f} {m}" for f in zs.FIELD for m in zs.MODE[:3]]
AFTER = [f"tables: {f} Repeat after {m}" for f in zs.FIELD for m in zs.MODE[:3]]
SHAPES = ["tables: LL log 5", "tables: OF log 5", "tables: ML log 5", "tables: LL log 9", "tables: OF log 8", "tables: ML log 9",
          "tables: log raised for the used codes", "normalisation: surplus", "normalisation: deficit of several",
          "description: zero run of 1-2", "description: zero run of 3-23", "description: zero run of 24 or more"]


def pooled(name, lead, gpu, listed):
    """The pool in one launch: each case reaches the regimes it was built for (those of `listed`),
    and the cases together every regime of `listed`; then the invariants."""
    cases = [c for c in pool() if len(c) == 3 or c[3] == name]
    rd = run(name, lead, [c[1] for c in cases], gpu)
    _, per = reached(rd)
    for (case, _, want, *_), got, r in zip(cases, per, rd):
        assert len(got) == 1 and want & set(listed) <= got[0], (case, r.spans[0].kinds, r.spans[0].nseq, sorted(want & set(listed) - got[0]))
    planted = set().union(*[c[2] for c in cases])
    assert set(listed) <= planted, sorted(set(listed) - planted)
    invariants(rd)


@both
def test_table_modes(name, lead, gpu):
    """kcdc_compress.hip:1598-1618 (the mode of least estimated cost: RLE for one code, Predefined when its
    cost is within the description's, else FSE_Compressed), :1837 (the carrier: the first coded block
    with sequences) and :2036-2042 (Repeat_Mode after it): every mode of every field in a carrier,
    Repeat_Mode after each, a carrier of three different modes, a carrier that is not block 0;
    pool() names the case that must reach each."""
    pooled(name, lead, gpu, MODES + AFTER + ["tables: three different modes in the carrier", "tables: carried by a later block"])


@both
def test_table_shapes(name, lead, gpu):
    """kcdc_compress.hip:1078-1098 (zstd_table): log 5 with few sequences and the largest log of each field
    (9, 8, 9) with thousands; the log raised because used + 1 > 2^log (:1080); the rounding surplus
    given to the largest count (:1092) and a deficit of several taken one at a time (:1095); zero
    runs in the descriptions (:1148-1160) of 1-2, of 3-23 and of 24 or more (literal lengths 0 and 512
    alone: the codes between them unused); pool() names the case that must reach each."""
    pooled(name, lead, gpu, SHAPES)


# ------------------------------------------------------------------ offsets and the widest sequence
@both
def test_offsets(name, lead, gpu):
    """zstd_ov (kcdc_compress.hip:1232-1239): offset value 1 with literals before it, and without them
    (periodic data across segments: match length 512, no literals, the same distance three times
    running); alternating distances take no repeat; the first sequence after a Raw_Block names its
    offset (the invariant, on a span that has one); distances 1, 32763 and 32764: a match is 4 bytes
    inside the span, so 32764 is the largest there is (32766 and 32767 cannot occur)."""
    per10 = (bytes(range(7, 17)) * 3300)[:SPAN]  # a period of 10: found among the 32 nearest at each segment's start
    holes = bytearray(per10)
    for k in range(45, SPAN, 50):
        holes[k] = 128 + k % 120  # a literal every 50 bytes, the match after it at the distance before it
    alt = (b"xyzw1234" * 3 + b"ABCD") * 1170

    def far(d):  # the head's first 4 bytes again at d, behind a copy of the bytes after them
        b = Build(uniform(d), ntok=3).literal(62)
        n = d - 63 * SEG
        b.data += b.head[4:4 + n] + b.head[:4] + no_repeat(SEG - n - 4, b.draw, b.seen)
        return b.bytes()
    chunks = [per10, bytes(holes), alt[:SPAN], Build(uniform(9)).literal(19).bytes() + per10[:22528],
              bytes(SPAN), far(32763), far(32764)]
    rd = run(name, lead, chunks, gpu)
    _, per = reached(rd)
    assert "offsets: repeat without literals" in per[0][0], sorted(per[0][0])
    assert any(q[0] == 0 and q[1] == 512 and q[2] == 1 for q in rd[0].spans[0].seqs)
    assert "offsets: repeat with literals" in per[1][0]
    assert any(q[2] == 1 and q[0] > 0 for q in rd[1].spans[0].seqs)
    assert rd[3].spans[0].kinds[0] == "R" and rd[3].spans[0].seqs and rd[3].spans[0].seqs[0][2] > 3
    assert "offsets: distance 1" in per[4][0]
    for k, d in ((5, 32763), (6, 32764)):
        assert d in {q[3] for q in rd[k].spans[0].seqs}, (d, rd[k].spans[0].kinds, rd[k].spans[0].seqs[-3:])
    a = rd[2].spans[0]  # alternating distances: explicit offsets among the sequences
    assert sum(1 for q in a.seqs if q[2] > 3) > 1 and len({q[3] for q in a.seqs}) >= 2
    invariants(rd)


@both
def test_widest_sequence_and_code_switches(name, lead, gpu):
    """put64 (kcdc_compress.hip:1709-1718, :1791-1795): one sequence with 16384 or more literals (a carry over
    33 match-free segments, :1386), a match of 259 or more and an offset beyond 16 KiB (code >= 14):
    22 + 15 extra bits beside the state bits.  The code tables switch to the computed codes at
    match length 131 (m = 128, :1743-1750) and literal length 64 (:1742-1747): match lengths 130, 131,
    511 and 512 and literal lengths 63 and 64 each occur."""
    wide = Build(skewed(41), ntok=67).literal(33)
    wide.part(12)  # 17 420 literals (the head, 33 segments, 12), then 500 bytes of the head: 17 408 + 12 back
    wide.copies(2).dense(27)  # (costly segments behind it, so block 0 reaches past the 35th segment)
    assert plan(wide.costs)[34] == 0 and len(wide.costs) == 64
    edge = Build(uniform(42))
    data = bytearray(edge.head)

    def fresh(n, avoid=None):
        for _ in range(100):
            c = no_repeat(n, edge.draw, edge.seen, bytes(data[-3:]))
            if avoid is None or n == 0 or c[0] != avoid:
                return c
    # (tail literals of one segment, a run at the start of the next, the match after them): the literal
    # length is the sum (zstd looks at position 32 of a run, not at 63); copies between keep each pair
    # inside one block
    costs = [4]
    for t, r, m, pad in ((31, 32, 130, 5), (32, 32, 131, 4), (0, 1, 511, 3), (0, 0, 512, 0)):
        data += edge.head * pad
        costs += [5] * pad
        data += edge.head[:SEG - t] + fresh(t, edge.head[(SEG - t) % SEG])
        data += fresh(r) + edge.head[:m]
        rest = SEG - r - m
        if rest:
            data += fresh(1, edge.head[m]) + edge.head[:rest - 1]
        costs += [5, 6 if rest else 5]
        assert plan(costs + [5] * (64 - len(costs)))[len(costs) - 2] == plan(costs + [5] * (64 - len(costs)))[len(costs) - 1]
    data += edge.head * (64 - len(costs))
    assert len(data) == SPAN
    rd = run(name, lead, [wide.bytes(), bytes(data)], gpu)
    w = [q for q in rd[0].spans[0].seqs if q[0] >= 16384]
    assert w and w[0][1] >= 259 and zs.of_code(w[0][2]) >= 14, (rd[0].spans[0].kinds, rd[0].spans[0].seqs[:3])
    seqs = rd[1].spans[0].seqs
    assert {130, 131, 511, 512} <= {q[1] for q in seqs}, sorted({q[1] for q in seqs})
    assert {(63, 130), (64, 131)} <= {q[:2] for q in seqs}, sorted({q[:2] for q in seqs})
    invariants(rd)


# ------------------------------------------------------------------ fallbacks and frame forms
@both
def test_raw_fallback_beside_coded_blocks(name, lead, gpu):
    """kcdc_compress.hip:1840 (body < B.raw): a block whose coded body would not be smaller than its bytes is a
    Raw_Block while its neighbours are coded.  The `over` path (:1796: the bitstream past the
    block's region) is not reached from inputs: a sequence costs at most 63 bits and covers at
    least 4 bytes, and a block whose sequences average more than 32 bits on 4 bytes fails :1840
    long before its stream passes the region of 576 bytes a segment."""
    chunks = [Build(skewed(51)).literal(15).using(uniform(51)).literal(16).using(skewed(52)).literal(32).bytes(),
              Build(uniform(53)).literal(31).using(skewed(53)).literal(32).bytes()]
    rd = run(name, lead, chunks, gpu)
    assert rd[0].spans[0].kinds[1] == "R" and rd[0].spans[0].kinds[0] in "ht" and rd[0].spans[0].kinds[2] in "ht"
    assert rd[1].spans[0].kinds[:2] == "RR" and rd[1].spans[0].kinds[2] in "ht"
    invariants(rd)


@both
def test_frame_forms(name, lead, gpu):
    """zstd_frame_header (kcdc_compress.hip:2483-2494): the Frame_Content_Size field of 1, 2 and 4 bytes at
    chunk lengths 0, 1, 255, 256, 65791 and 65792; spans of 1, 2 and 3 segments (the b1 / b2 / b3
    clamps of :1345-1347 leave empty blocks, which are not written); a last span of one byte."""
    text = words(65792 + 32769, 8)
    lens = [0, 1, 255, 256, 65791, 65792, 512, 1024, 1536, 700, 1300, 32769]
    chunks, at = [], 0
    for n in lens:
        chunks.append(text[at % 999:at % 999 + n])
        at += 131
    rd = run(name, lead, chunks, gpu)
    assert [r.frame.fcs_bytes for r in rd] == [1, 1, 1, 2, 2, 4, 2, 2, 2, 2, 2, 2]
    assert [len(r.blocks) for r in rd[:2]] == [1, 2]
    assert [len(r.spans[0].blocks) for r in rd[6:11]] == [1, 2, 3, 2, 3]
    assert len(rd[11].spans) == 2 and rd[11].spans[1].kinds == "R" and rd[11].spans[1].blocks[0].out_len == 1
    invariants(rd)


# ------------------------------------------------------------------ zstd-fastest
def hash6(b4):
    return ((int.from_bytes(b4, "little") * KMUL) & 0xFFFFFFFF) >> 26


def short_repeats(n, seed):
    """A segment of uniform literals with n 4-byte repeats near its start, each 5 bytes behind its
    source, where zstd-fastest's segment table still holds it (no position between has its hash)."""
    for s in range(seed, seed + 400):
        r = random.Random(s)
        seen = set()
        out = bytearray()
        for _ in range(n):
            a = no_repeat(4, lambda: r.randrange(256), seen, bytes(out[-3:]))
            f = no_repeat(1, lambda: r.randrange(256), seen, bytes((out + a)[-3:]))
            out += a + f + a
        out += no_repeat(SEG - len(out), lambda: r.randrange(256), seen, bytes(out[-3:]))
        ok = True
        for k in range(n):
            at = 9 * k
            ok &= all(hash6(out[x:x + 4]) != hash6(out[at:at + 4]) for x in range(at + 1, at + 5))
            ok &= out[at + 9] != out[at + 4]
        if ok:
            return bytes(out)
    raise AssertionError("no seed")


def parse_fastest(seg):
    """zstd-fastest's parse of one segment, restated (kcdc_compress.hip:2177-2275 at effort 0): at each
    position it looks at, the latest one of the same 6-bit hash is the only candidate; a position
    inside a match is not entered; after 16 literals it skips.  Returns [(ll, ml, distance)]."""
    tab, x, lit, seqs = {}, 0, 0, []
    while x + 4 <= len(seg):
        v = seg[x:x + 4]
        c = tab.get(hash6(v))
        tab[hash6(v)] = x
        n = 0
        if c is not None and seg[c:c + 4] == v:
            n = 4
            while x + n < len(seg) and seg[x + n] == seg[c + n]:
                n += 1
        if n:
            seqs.append((x - lit, n, x - c))
            x += n
            lit = x
        else:
            x += 1 + ((x - lit) >> 4)
    return seqs


def most_sequences(seed):
    """A segment of 4 literals and 127 matches of 4 bytes: the four rotations of its first 4 bytes (of 4
    different hashes), each next one chosen so that the match before it ends after 4 bytes (a
    search over the restated parse)."""
    import sys
    r = random.Random(seed)
    while True:
        a = bytes(r.sample(range(256), 4))
        rots = [a[i:] + a[:i] for i in range(4)]
        if len({hash6(g) for g in rots}) == 4:
            break
    seg = bytearray(a)

    def grow():
        if len(seg) == SEG:
            return True
        for g in r.sample(rots, 4):
            seg.extend(g)
            q = parse_fastest(bytes(seg))
            if len(q) == len(seg) // 4 - 1 and all(m == 4 for _, m, _ in q) and grow():
                return True
            del seg[-4:]
        return False
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 2000))
    try:
        assert grow()
    finally:
        sys.setrecursionlimit(limit)
    return bytes(seg)


@leads
def test_fastest(lead, gpu):
    """zstd-fastest (kcdc_compress.hip:2286-2297, zstd_seqs): one block a segment, predefined tables, the
    2-byte raw literals header at every literal count, never a repeat offset (zeros with a
    literal every 50 bytes included).  Its matches come from the segment's own table alone (:2190), so a block has at
    least one literal (zeros: exactly 1; 0 literals cannot occur) and at most 127 sequences: a match
    is 4 bytes or more and its source lies at a position of the segment the parse has looked at, so
    the first 4 bytes are literals and 508 are left (128 cannot occur); most_sequences() builds
    the segment of 4 literals and 127 matches, Number_of_Sequences still in 1 byte.  A sweep of
    literal runs before and inside a period of 8 places 31 and 32 literals (a run of its own does
    not: after 16 literals the parse looks at every second position).  A segment with one 4-byte repeat
    fails total >= seg_len + 3 (:2290), one with two returns kZOver (:985: 8 bytes of headers and
    one coded sequence pass the 8 bytes the matches save); both are stored, like random bytes."""
    per = bytearray(2048)
    for k in range(45, 2048, 50):
        per[k] = 1 + k % 250  # a literal every 50 zeros: the match behind it starts 50 after the one before, its source
    seg = lambda j, s: rnd(j, s) + (rnd(8, s + 1) * 64)[:SEG - j]  # noqa: E731

    def two_runs(j, s):  # 10 literals, a period of 8 (8 more), j literals, the period again: 18 + j literals
        p = rnd(8, s + 1)
        return rnd(10, s) + p * 8 + rnd(j, s + 2) + (p * 64)[:SEG - 74 - j]
    sweep = b"".join(seg(j, 100 + j) for j in range(0, 9)) + b"".join(two_runs(j, 200 + 7 * j + k) for j in range(9, 17) for k in (0, 1))
    dense = most_sequences(1)
    assert [q[:2] for q in parse_fastest(dense)] == [(4, 4)] + [(0, 4)] * 126
    chunks = [per, bytes(2048), sweep, rnd(1024, 6) + words(1024, 1), words(4096, 3),
              short_repeats(1, 1) + short_repeats(2, 500) + bytes(SEG), dense]
    rd = run("zstd-fastest", lead, chunks, gpu)
    blocks = [b for r in rd for sp in r.spans for b in sp.coded]
    counts = sorted({len(b.lits) for b in blocks})
    assert {1, 31, 32} <= set(counts) and counts[-1] > 32, counts
    assert all(len(b.lits) == 1 and len(b.seqs) == 1 for b in rd[1].spans[0].coded) and rd[1].spans[0].kinds == "rrrr"
    assert rd[3].spans[0].kinds[:2] == "RR"
    assert rd[5].spans[0].kinds == "RRr", rd[5].spans[0].kinds
    assert all(len(b.seqs) >= 3 for b in rd[0].spans[0].coded)
    most = rd[6].spans[0].blocks[0]
    assert (most.type, len(most.lits), len(most.seqs), most.nseq_bytes) == (2, 4, 127, 1), (most.type, len(most.lits), len(most.seqs))
    assert all(q[1] == 4 for q in most.seqs) and max(len(b.seqs) for b in blocks) == 127
    invariants(rd)
