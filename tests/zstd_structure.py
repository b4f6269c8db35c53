"""The span reader and invariant checker of the device's zstd frames (kcdc_compress.hip: zstd_table,
zstd_ov, zstd_emit_kernel, zstd_seqs).  Plain Python over tests/zstd_model.py's detail records:
importable without torch and without the library.

read(stream, data) decodes one frame with the model, checks it against `data` and groups its blocks
into the 32 KiB spans the encoder works in; check(stream, data, effort) also runs every invariant
below and raises Violation(group, what) at the first one that does not hold.  The groups, each a
restatement of what the encoder promises (never of how it computes it):

  frame     magic, Single_Segment, the smallest Frame_Content_Size field (zstd_frame_header), no
            checksum, no dictionary ID, one frame, closed by the empty last Raw_Block 01 00 00;
  block     a Compressed_Block is smaller than the Raw_Block of its content; a block stays in a span;
  literals  stream count and header sizes by the literal count, no RLE literals, one tree per span on
            its first Huffman block and Treeless after, the tree ending at the last used symbol;
  tree      the tree description the smaller of direct and FSE-compressed weights (the latter
            restated here: accuracy log 5, two interleaved states), direct only up to symbol 128;
  lengths   the code's cost over the span's literal histogram: the Huffman optimum when that fits 11
            bits, else between package-merge and zlib's limiter (tests/deflate_model.py);
  tables    one carrier block per span and Repeat_Mode after, RLE iff one code, valid counts, the
            accuracy log rule, the description byte-identical to RFC 8878 4.1.1 re-encoded here;
  offsets   the repeat-offset rule from the decoder's side: offset value 1 exactly where the
            previous sequence's offset returns under the conditions zstd_ov names, never 2 or 3;
  fastest   (effort 0) one segment per block, predefined tables, no repeats, 2-byte raw literals.

A Raw_Block hides its literals and sequences from the reader, and the encoder counted them: the
rules that need the span's full counts (lengths; tables' log, RLE and unused codes; the tree's top)
are exact on a span without one (Span.full) and one-sided otherwise."""
import deflate_model as dm
import zstd_model as zm

SPAN, SEG = 32768, 512
MAXBITS = 11
GROUPS = ("frame", "block", "literals", "tree", "lengths", "tables", "offsets")
NSYM = (36, 32, 53)  # LL, OF, ML codes


class Violation(AssertionError):
    def __init__(self, group, what):
        super().__init__(f"{group}: {what}")
        self.group, self.what = group, what


def must(cond, group, what):
    if not cond:
        raise Violation(group, what)


# ------------------------------------------------------------------ codes
def ll_code(ll):
    if ll < 16:
        return ll
    return max(c for c in range(16, 36) if zm.LL_BASE[c] <= ll)


def ml_code(ml):
    if ml < 35:
        return ml - 3
    return max(c for c in range(32, 53) if zm.ML_BASE[c] <= ml)


def of_code(ov):
    return ov.bit_length() - 1


# ------------------------------------------------------------------ RFC 8878 4.1.1, the writer's side
class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, x, nb):
        assert 0 <= x < (1 << nb) or nb == 0 and x == 0
        self.v |= x << self.n
        self.n += nb

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def write_ncount(norm, log):
    """The description of these normalized counts (-1: less than 1): Accuracy_Log - 5 in 4 bits, each
    count + 1 in the fewest bits its range allows (the small values one bit shorter), after a zero
    count the run of further zeros in 2-bit flags (3: three more and another flag), up to the last
    non-zero count; zero padding to a byte."""
    last = max(s for s, c in enumerate(norm) if c)
    w = _Bits()
    w.put(log - 5, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    s = 0
    while s <= last:
        c = norm[s]
        s += 1
        small = 2 * threshold - 1 - remaining  # values below it take nb - 1 bits
        x = c + 1
        if x < small:
            w.put(x, nb - 1)
        else:
            w.put(x if x < threshold else x + small, nb)
        remaining -= abs(c)
        if c == 0:
            z = 0
            while s <= last and norm[s] == 0:
                z, s = z + 1, s + 1
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
        while 1 < remaining < threshold:
            nb, threshold = nb - 1, threshold >> 1
    assert remaining == 1, "counts do not sum to the table"
    return w.bytes()


def zero_runs(norm):
    """The lengths of the runs of zero counts a description spells out (those before its last count)."""
    last = max(s for s, c in enumerate(norm) if c)
    runs, z = [], 0
    for c in norm[:last + 1]:
        if c == 0:
            z += 1
        elif z:
            runs.append(z)
            z = 0
    return runs


def table_log(nseq, used, maxlog):
    """The encoder's Accuracy_Log: log2(N - 1) - 2 within 5..maxlog, raised while 2^log < used + 1."""
    log = (nseq - 1).bit_length() - 1 - 2 if nseq > 4 else 0
    log = max(5, min(maxlog, log))
    while (1 << log) < used + 1 and log < maxlog:
        log += 1
    return log


def normalize(counts, log):
    """(normalized counts, rounding difference) as zstd_table rounds: each used count to the nearest
    share of 2^log, at least 1; a surplus goes to the largest entry at once, a deficit is taken from
    the largest one at a time (the lowest symbol among equals).  The difference tells the branch:
    > 0 surplus, < 0 that many deficit steps."""
    total, size = sum(counts), 1 << log
    v = [max(1, (c * size + total // 2) // total) if c else 0 for c in counts]
    diff = size - sum(v)
    d = diff
    while d:
        k = v.index(max(v))
        if d > 0:
            v[k] += d
            d = 0
        else:
            v[k] -= 1
            d += 1
    return v, diff


class FseEncoder:
    """The encoding side of one table (zstd's FSE_buildCTable formulation over the model's decoding
    cells): states in [size, 2 size); a symbol's states in ascending order."""

    def __init__(self, norm, log):
        self.log, self.size, self.norm = log, 1 << log, norm
        cells = zm.fse_table(norm, log)
        self.states = {}
        for u, (s, _, _) in enumerate(cells):
            self.states.setdefault(s, []).append(self.size + u)

    def _dnb(self, s):
        c = abs(self.norm[s])
        if c == 1:
            return (self.log << 16) - self.size
        mbo = self.log - ((c - 1).bit_length() - 1)
        return (mbo << 16) - (c << mbo)

    def init(self, s):
        dnb = self._dnb(s)
        nb = (dnb + (1 << 15)) >> 16
        return self.states[s][(((nb << 16) - dnb) >> nb) - abs(self.norm[s])]

    def step(self, w, x, s):
        nb = (x + self._dnb(s)) >> 16
        w.put(x & ((1 << nb) - 1), nb)
        return self.states[s][(x >> nb) - abs(self.norm[s])]


def fse_weights(weights):
    """The FSE-compressed description of a tree (RFC 8878 4.2.1.2) as the encoder writes it, or None
    where it writes none: the weights of symbols 0..top-1 (top's is implied) over one table of
    accuracy log 5, two interleaved states from the last weight backwards, under 128 bytes."""
    w = list(weights[:-1])
    top = len(w)
    cnt = [w.count(x) for x in range(12)]
    if top < 3 or max(cnt) == top:
        return None
    norm, _ = normalize(cnt, 5)
    desc = write_ncount(norm, 5)
    t, b = FseEncoder(norm, 5), _Bits()
    i = top
    if top & 1:
        s1 = t.init(w[i - 1])
        s2 = t.init(w[i - 2])
        s1 = t.step(b, s1, w[i - 3])
        i -= 3
    else:
        s2 = t.init(w[i - 1])
        s1 = t.init(w[i - 2])
        i -= 2
    two = True
    while i > 0:
        i -= 1
        if two:
            s2 = t.step(b, s2, w[i])
        else:
            s1 = t.step(b, s1, w[i])
        two = not two
    b.put(s2 - 32, 5)
    b.put(s1 - 32, 5)
    b.put(1, 1)
    body = desc + b.bytes()
    if len(body) >= 127:  # the header byte and the body stay under 128 bytes
        return None
    return bytes([len(body)]) + body


def code_lengths(weights, maxbits):
    return [maxbits + 1 - w if w else 0 for w in weights] + [0] * (256 - len(weights))


# ------------------------------------------------------------------ the span reader
class Span:
    """One 32 KiB span of a frame: its blocks' Details; kinds, a letter per block (R Raw_Block, L
    RLE_Block, and per Compressed_Block its literals: r raw, l RLE, h Huffman with the tree, t
    Treeless); H, the histogram of its visible literals; counts, the LL / OF / ML code counts of its
    visible sequences; the tree's and the tables' carrier blocks (indices, None without one)."""

    def __init__(self, blocks, at):
        self.blocks, self.at = blocks, at
        self.kinds = "".join("RL"[b.type] if b.type < 2 else "rlht"[b.lit_type] for b in blocks)
        self.coded = [b for b in blocks if b.type == 2]
        self.full = len(self.coded) == len(blocks)
        self.H = [0] * 256
        for b in self.coded:
            for c in b.lits:
                self.H[c] += 1
        self.seqs = [q for b in self.coded for q in b.seqs]
        self.nseq = len(self.seqs)
        self.counts = [[0] * n for n in NSYM]
        for ll, ml, ov, _ in self.seqs:
            self.counts[0][ll_code(ll)] += 1
            self.counts[1][of_code(ov)] += 1
            self.counts[2][ml_code(ml)] += 1
        huff = [k for k, b in enumerate(blocks) if b.type == 2 and b.lit_type >= 2]
        self.huff = huff
        self.tree_carrier = next((k for k in huff if blocks[k].lit_type == 2), None)
        with_seqs = [k for k, b in enumerate(blocks) if b.type == 2 and b.seqs]
        self.with_seqs = with_seqs
        self.table_carrier = next((k for k in with_seqs if any(f.mode != 3 for f in blocks[k].fields)), None)
        self.tree = blocks[self.tree_carrier] if self.tree_carrier is not None else None
        self.tables = blocks[self.table_carrier].fields if self.table_carrier is not None else None

    def lengths(self):
        return code_lengths(self.tree.weights, self.tree.maxbits)

    def cost(self):
        return dm.code_cost(self.H, self.lengths())


class Reading:
    def __init__(self, stream, data, frame, blocks, spans):
        self.stream, self.data, self.frame, self.blocks, self.spans = stream, data, frame, blocks, spans


def read(stream, data):
    """Decode one frame with the model (it must give `data`) and group its blocks into spans; the
    frame's last block is kept apart (Reading.blocks has it, no span does)."""
    stream, data = bytes(stream), bytes(data)
    got, frames, details = zm.decode(stream, detail=True)
    must(got == data, "frame", "the model does not decode the input")
    must(len(frames) == 1 and not frames[0].skippable, "frame", "not exactly one frame")
    blocks = details[0]
    must(frames[0].blocks[-1].last and not any(b.last for b in frames[0].blocks[:-1]), "frame", "Last_Block flags")
    must(all(b.out_len for b in blocks[:-1]), "frame", "an empty block before the last")
    spans, cur, have, at = [], [], 0, 0
    for b in blocks[:-1]:
        want = min(SPAN, len(data) - SPAN * len(spans))
        cur.append(b)
        have += b.out_len
        must(have <= want, "block", "a block crosses a span")
        if have == want:
            spans.append(Span(cur, at))
            at += have
            cur, have = [], 0
    must(not cur, "block", "blocks after the content")
    return Reading(stream, data, frames[0], blocks, spans)


# ------------------------------------------------------------------ the invariants
def check_frame(r):
    s, n = r.stream, len(r.data)
    must(s[:4] == b"\x28\xb5\x2f\xfd", "frame", "magic")
    fhd = s[4]
    must(fhd & 0x20, "frame", "Single_Segment flag not set")
    must(fhd & 0x04 == 0, "frame", "a checksum")
    must(fhd & 0x03 == 0, "frame", "a dictionary ID")
    must(fhd & 0x18 == 0, "frame", "unused or reserved descriptor bits")
    want = 1 if n < 256 else 2 if n < 65536 + 256 else 4 if n < 1 << 32 else 8
    must(r.frame.fcs_bytes == want, "frame", f"Frame_Content_Size in {r.frame.fcs_bytes} bytes, the smallest is {want}")
    fcs = int.from_bytes(s[5:5 + want], "little") + (256 if want == 2 else 0)
    must(fcs == n, "frame", "Frame_Content_Size")
    last = r.blocks[-1]
    must(last.type == 0 and last.size == 0, "frame", "the last block is not an empty Raw_Block")
    must(s[-3:] == b"\x01\x00\x00", "frame", "the stream does not end with 01 00 00")
    must(5 + want + sum(3 + (b.size if b.type != 1 else 1) for b in r.blocks) == len(s), "frame", "bytes after the last block")


def check_blocks(sp):
    for b in sp.blocks:
        must(b.type != 1, "block", "an RLE_Block: the encoder writes none")
        must(b.out_len <= SPAN, "block", "block content over one span")
        if b.type == 2:
            must(b.size < b.out_len, "block", f"a Compressed_Block of {b.size} bytes for {b.out_len} bytes of content")


def check_literals(sp):
    for b in sp.coded:
        n = len(b.lits)
        must(b.lit_type != 1, "literals", "an RLE literals block: the encoder writes none")
        # (each of the first three of 4 streams holds ceil(n / 4) literals: the model decodes them with
        # that split and every stream must end exactly on its last bit, so a frame that read() returned
        # has it; Detail.jump keeps the three sizes for the record)
        if b.lit_type == 0:
            must(b.lit_hlen == (1 if n < 32 else 2 if n < 4096 else 3), "literals", f"raw header of {b.lit_hlen} bytes for {n} literals")
        else:
            must((b.streams == 1) == (n <= 1023), "literals", f"{b.streams} stream(s) for {n} literals")
            if b.streams == 1:
                must(b.lit_hlen == 3, "literals", "single-stream header")
            else:
                must((b.lit_hlen == 4) == (n <= 16383 and b.lit_comp <= 16383), "literals",
                     f"4-stream header of {b.lit_hlen} bytes for {n} literals in {b.lit_comp} bytes")
    if not sp.huff:
        return
    must(sp.tree_carrier == sp.huff[0], "literals", "the span's first Huffman block carries no tree")
    must(all(sp.blocks[k].lit_type == 3 for k in sp.huff[1:]), "literals", "a tree sent twice in a span")
    t = sp.tree
    top = len(t.weights) - 1
    seen = max(s for s in range(256) if sp.H[s])
    must(top == seen if sp.full else top >= seen, "literals", f"the tree ends at symbol {top}, the literals at {seen}")
    if sp.full:
        must(all((w != 0) == (c != 0) for w, c in zip(t.weights, sp.H)), "literals", "a code for an unused symbol, or none for a used one")


def check_tree(sp):
    """Returns (chosen kind, direct size or None, FSE size or None), or None without a tree."""
    t = sp.tree
    if t is None:
        return None
    top = len(t.weights) - 1
    direct = 1 + (top + 1) // 2 if top <= 128 else None
    fse = fse_weights(t.weights)
    must(direct is not None or fse is not None, "tree", "no description the encoder writes fits this tree")
    want = "fse" if fse is not None and (direct is None or len(fse) < direct) else "direct"
    must(t.tree_kind == want, "tree", f"{t.tree_kind} weights where {want} is the smaller description")
    must(t.tree_bytes == (len(fse) if want == "fse" else direct), "tree", "the tree description's size")
    return want, direct, None if fse is None else len(fse)


def check_lengths(sp):
    """Returns None (no tree, or a Raw_Block hides literals), 'optimal' or 'limited'."""
    if sp.tree is None:
        return None
    must(sp.tree.maxbits <= MAXBITS, "lengths", "a code over 11 bits")
    if not sp.full:
        return None
    cost = sp.cost()
    best, depth = dm.huffman_cost(sp.H)
    if depth <= MAXBITS:
        must(cost == best, "lengths", f"the code costs {cost} bits, the Huffman optimum {best}")
        return "optimal"
    lo = dm.code_cost(sp.H, dm.package_merge(sp.H, MAXBITS))
    hi = dm.code_cost(sp.H, dm.zlib_limit(sp.H, MAXBITS))
    must(lo <= cost <= hi, "lengths", f"the limited code costs {cost} bits, outside package-merge {lo} .. zlib {hi}")
    return "limited"


def check_tables(sp):
    for b in sp.coded:
        n = len(b.seqs)
        must(b.nseq_bytes == (1 if n < 128 else 2), "tables", f"Number_of_Sequences in {b.nseq_bytes} bytes for {n}")
    if not sp.with_seqs:
        return
    must(sp.table_carrier == sp.with_seqs[0], "tables", "the span's first block with sequences carries no tables")
    must(all(f.mode != 3 for f in sp.tables), "tables", "Repeat_Mode in the carrier")
    for k in sp.with_seqs[1:]:
        must(all(f.mode == 3 for f in sp.blocks[k].fields), "tables", "a later block is not Repeat_Mode x 3")
    for k, f in enumerate(sp.tables):
        cnt = sp.counts[k]
        used = [s for s, c in enumerate(cnt) if c]
        if f.mode == 1:
            must(used == [f.rle], "tables", "RLE for a field with more than one code")
            continue
        must(not (sp.full and len(used) == 1), "tables", "a one-code field is not RLE")
        norm = list(f.norm) + [0] * (NSYM[k] - len(f.norm))
        must(all(norm[s] != 0 for s in used), "tables", "a used code without cells")
        if f.mode == 0:
            continue
        maxlog = 8 if k == 1 else 9
        must(all(c >= 0 for c in norm) and sum(norm) == 1 << f.log, "tables", "counts of an FSE_Compressed table")
        must(5 <= f.log <= maxlog, "tables", "accuracy log out of range")
        must(write_ncount(f.norm, f.log) == f.desc, "tables", "the description is not the RFC's minimal one")
        if sp.full:
            must(all(norm[s] == 0 for s in range(NSYM[k]) if not cnt[s]), "tables", "cells for an unused code")
            want = table_log(sp.nseq, len(used), maxlog)
            must(f.log == want, "tables", f"accuracy log {f.log}, the rule gives {want}")


def check_offsets(sp):
    for b in sp.coded:
        for i, (ll, ml, ov, off) in enumerate(b.seqs):
            must(ov == 1 or ov > 3, "offsets", f"offset value {ov}")
            rep = False
            if i > 0 and b.seqs[i - 1][3] == off:
                rep = ll > 0 or (b.seqs[i - 1][0] == 0 and i >= 2 and b.seqs[i - 2][3] == off)
            must((ov == 1) == rep, "offsets", f"sequence {i} (ll {ll}, offset {off}) has offset value {ov}, repeat due: {rep}")


def check_fastest(sp):
    """zstd-fastest: every block one segment, coded by zstd_seqs."""
    for b in sp.blocks:
        must(b.out_len <= SEG and b.at % SEG == 0, "fastest", "a block is not one segment")
        if b.type != 2:
            continue
        must(len(b.seqs) <= SEG // 4, "fastest", "over 128 sequences")
        must(b.lit_type == 0 and b.lit_hlen == 2, "fastest", "not the 2-byte raw literals header")
        must(b.nseq_bytes == (1 if len(b.seqs) < 128 else 2), "fastest", "Number_of_Sequences width")
        must(all(f.mode == 0 for f in b.fields), "fastest", "a mode other than Predefined")
        must(all(ov > 3 for _, _, ov, _ in b.seqs), "fastest", "a repeat offset")


def check(stream, data, effort=1, groups=GROUPS):
    """read() and every invariant of `groups` (effort 0: frame, block and fastest); returns the
    Reading, each span's length-limit regime in span.limit and its tree description's (kind, direct
    size, FSE size) in span.desc."""
    return check_reading(read(stream, data), effort, groups)


def check_reading(r, effort=1, groups=GROUPS):
    """The invariants of `groups` on a Reading of read(); returns it."""
    if "frame" in groups:
        check_frame(r)
    for sp in r.spans:
        sp.limit = sp.desc = None
        if "block" in groups:
            check_blocks(sp)
        if effort == 0:
            check_fastest(sp)
            continue
        if "literals" in groups:
            check_literals(sp)
        if "tree" in groups:
            sp.desc = check_tree(sp)
        if "lengths" in groups:
            sp.limit = check_lengths(sp)
        if "tables" in groups:
            check_tables(sp)
        if "offsets" in groups:
            check_offsets(sp)
    return r


# ------------------------------------------------------------------ which branches a span reached
FIELD = ("LL", "OF", "ML")
MODE = ("Predefined", "RLE", "FSE_Compressed", "Repeat")


def regimes(sp):
    """The names of the encoder branches this span's records show (tests/test_gpu_zstd_edges.py plants
    each on purpose; tools/zstd_census.py counts them over the corpora of tests/test_gpu_compress.py)."""
    r = set()
    k = sp.kinds
    r.add("span: all Raw_Blocks" if set(k) == {"R"} else "span: a Raw_Block beside compressed ones" if "R" in k else "span: no Raw_Block")
    for b in sp.coded:
        n = len(b.lits)
        if b.lit_type == 0:
            r.add(f"literals: raw, {b.lit_hlen}-byte header")
        elif b.streams == 1:
            r.add("literals: Huffman, 1 stream")
        else:
            r.add(f"literals: Huffman, 4 streams, {b.lit_hlen}-byte header")
            if n % 4:
                r.add("literals: ragged last stream")
        if n == 0:
            r.add("literals: none in a block")
        ns = len(b.seqs)
        r.add("sequences: none in a block" if ns == 0 else "sequences: 1 in a block" if ns == 1 else
              "sequences: 127 in a block" if ns == 127 else "sequences: 128 in a block" if ns == 128 else
              "sequences: 2000 or more in a block" if ns >= 2000 else "sequences: some")
        for i, (ll, ml, ov, off) in enumerate(b.seqs):
            if ov == 1:
                r.add("offsets: repeat with literals" if ll else "offsets: repeat without literals")
            if off == 1 or off >= 32760:
                r.add("offsets: distance 1" if off == 1 else "offsets: distance 32760 or more")
            if ll >= 16384:
                r.add("sequence: literal length 16384 or more")
            if ml >= 259:
                r.add("sequence: match length 259 or more")
            if ov > 3 and of_code(ov) >= 14:
                r.add("sequence: offset code 14 or more")
    if not sp.huff:
        r.add("literals: no Huffman in the span")
    else:
        t, c = sp.tree, sp.tree_carrier
        if c > 0:
            r.add("tree: carried by a later block")
            r.add("tree: after a Raw_Block" if "R" in k[:c] else "tree: after a compressed block")
            if any(b.type == 2 and not b.lits for b in sp.blocks[:c]):
                r.add("tree: after a literal-free block")
        if "t" in k:
            r.add("tree: Treeless after it")
        if "r" in k[c:] and any(len(b.lits) for b in sp.blocks[c:] if b.type == 2 and b.lit_type == 0):
            r.add("tree: raw literals kept beside it")
        if "R" in k[c:sp.huff[-1]]:
            r.add("tree: a Raw_Block between Huffman blocks")
        top = len(t.weights) - 1
        if t.tree_kind == "direct":
            r.add("weights: direct")
        else:
            r.add("weights: FSE, top <= 128" if top <= 128 else "weights: FSE, top > 128")
            r.add("weights: FSE over an odd count" if top & 1 else "weights: FSE over an even count")
        r.add(f"code: longest {t.maxbits}")
        if sp.full:
            depth = dm.huffman_cost(sp.H)[1]
            r.add("code: optimum deeper than 11" if depth > MAXBITS else f"code: optimum depth {depth}" if depth == MAXBITS else "code: optimum under 11")
    if sp.tables is not None:
        c = sp.table_carrier
        if c > 0:
            r.add("tables: carried by a later block")
        modes = [f.mode for f in sp.tables]
        if len(set(modes)) == 3:
            r.add("tables: three different modes in the carrier")
        for f_, f in zip(FIELD, sp.tables):
            r.add(f"tables: {f_} {MODE[f.mode]}")
            if len(sp.with_seqs) > 1:
                r.add(f"tables: {f_} Repeat after {MODE[f.mode]}")
            if f.mode != 2:
                continue
            r.add(f"tables: {f_} log {f.log}")
            for z in zero_runs(f.norm):
                r.add("description: zero run of 1-2" if z < 3 else "description: zero run of 3-23" if z < 24 else "description: zero run of 24 or more")
            if sp.full:
                cnt = sp.counts[FIELD.index(f_)]
                maxlog = 8 if f_ == "OF" else 9
                if table_log(sp.nseq, 0, maxlog) < f.log:
                    r.add("tables: log raised for the used codes")
                diff = normalize(cnt, f.log)[1]
                r.add("normalisation: exact" if diff == 0 else "normalisation: surplus" if diff > 0 else
                      "normalisation: deficit of 1" if diff == -1 else "normalisation: deficit of several")
    return r
