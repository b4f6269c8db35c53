"""A structural reader of raw DEFLATE streams (RFC 1951) and references for code lengths; CPU only.

inflate_blocks() inflates a stream and records, block by block, what the encoder chose: block
types, the dynamic header's fields and its run-length symbols, every code length and every token.
It is written from the RFC and rejects what zlib's inflate rejects (inftrees.c's completeness
rule included: an incomplete code is an error unless it is a literal/length or distance code whose
longest length is 1).  The tests of the device's deflate plan assert on these records.

Code-length references:
  huffman_cost(counts)          the optimal unrestricted cost and the depth of the optimal tree of
                                least depth (two queues, leaves before internal nodes on ties);
  package_merge(counts, maxb)   optimal lengths under a length limit (Larmore and Hirschberg);
  zlib_limit(counts, maxb)      zlib's trees.c restated: build_tree's heap and gen_bitlen's
                                overflow repair;
  rle_lengths(seq)              RFC 1951 section 3.2.7's run-length symbols, greedily.
"""
from __future__ import annotations

from dataclasses import dataclass, field

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
NLIT, NDIST, EOB = 286, 30, 256


class InflateError(ValueError):
    pass


@dataclass
class Block:
    bfinal: int
    btype: int                  # 0 stored, 1 fixed, 2 dynamic
    bit_off: int                # of the 3-bit block header
    bit_len: int = 0            # header bits, padding, LEN/NLEN and data included
    out_off: int = 0            # output bytes before / of this block
    out_len: int = 0
    stored_len: int | None = None
    hlit: int | None = None     # 257..286, 1..30, 4..19 (the counts, not the fields)
    hdist: int | None = None
    hclen: int | None = None
    cl_lens: list | None = None   # 19 code-length-code lengths, by symbol
    cl_syms: list | None = None   # [(symbol 0..18, extra value)]
    cl_hist: list | None = None   # 19
    lens: list | None = None      # 286 + 30 code lengths (0 past HLIT / HDIST)
    header_bits: int = 0          # the 3 header bits + everything before the first token
    tokens: list = field(default_factory=list)  # a literal byte (int), or (length, distance, lsym, dsym)
    lit_hist: list | None = None  # 286, end of block counted
    dist_hist: list | None = None  # 30
    eob_bits: int = 0

    @property
    def matches(self):
        return [t for t in self.tokens if not isinstance(t, int)]


def kraft(lens):
    """(sum of 2^(maxlen - l) over used lengths, 2^maxlen): equal when the code is complete."""
    used = [l for l in lens if l]
    if not used:
        return 0, 1
    m = max(used)
    return sum(1 << (m - l) for l in used), 1 << m


def _decode_table(lens, what, may_be_single):
    """(table, maxlen): table[peek of maxlen bits] = (symbol, length) or None.  Checks the code as
    inftrees.c does."""
    used = [l for l in lens if l]
    if not used:
        if not may_be_single:
            raise InflateError(f"{what}: no code at all")
        return [None, None], 1
    if max(used) > 15:
        raise InflateError(f"{what}: length > 15")
    s, full = kraft(lens)
    m = max(used)
    if s > full:
        raise InflateError(f"{what}: over-subscribed code")
    if s < full and not (may_be_single and m == 1):
        raise InflateError(f"{what}: incomplete code")
    table = [None] * (1 << m)
    code = 0
    for l in range(1, m + 1):
        for sym, sl in enumerate(lens):
            if sl == l:
                r = int(format(code, f"0{l}b")[::-1], 2)  # codes are packed most significant bit first
                for k in range(r, 1 << m, 1 << l):
                    table[k] = (sym, l)
                code += 1
        code <<= 1
    return table, m


_FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED = None


def inflate_blocks(raw: bytes):
    """Inflate a raw DEFLATE stream up to and including its final block: (bytes, [Block]).
    Raises InflateError on anything zlib's inflate refuses."""
    global _FIXED
    data = bytes(raw) + b"\0" * 8
    nbits_total = 8 * len(raw)
    pos = 0
    out = bytearray()
    blocks = []

    def get(n):
        nonlocal pos
        if pos + n > nbits_total:
            raise InflateError("unexpected end of stream")
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def sym(table, m):
        nonlocal pos
        e = table[(int.from_bytes(data[pos >> 3:(pos >> 3) + 3], "little") >> (pos & 7)) & ((1 << m) - 1)]
        if e is None:
            raise InflateError("invalid code")
        pos += e[1]
        if pos > nbits_total:
            raise InflateError("unexpected end of stream")
        return e

    while True:
        b = Block(bfinal=0, btype=0, bit_off=pos, out_off=len(out))
        b.bfinal = get(1)
        b.btype = get(2)
        if b.btype == 3:
            raise InflateError("invalid block type")
        if b.btype == 0:
            pos = (pos + 7) & ~7
            ln, nln = get(16), get(16)
            if ln != (nln ^ 0xFFFF):
                raise InflateError("invalid stored block lengths")
            if pos + 8 * ln > nbits_total:
                raise InflateError("unexpected end of stream")
            out += data[pos >> 3:(pos >> 3) + ln]
            pos += 8 * ln
            b.stored_len = ln
        else:
            if b.btype == 1:
                if _FIXED is None:
                    _FIXED = (_decode_table(_FIXED_LENS, "fixed", False), _decode_table([5] * 32, "fixed dist", False))
                (lt, lm), (dt, dm) = _FIXED
            else:
                b.hlit, b.hdist, b.hclen = get(5) + 257, get(5) + 1, get(4) + 4
                if b.hlit > 286 or b.hdist > 30:
                    raise InflateError("too many length or distance symbols")
                b.cl_lens = [0] * 19
                for i in range(b.hclen):
                    b.cl_lens[CL_ORDER[i]] = get(3)
                ct, cm = _decode_table(b.cl_lens, "code lengths set", False)
                seq, b.cl_syms, b.cl_hist = [], [], [0] * 19
                nt = b.hlit + b.hdist
                while len(seq) < nt:
                    s, _ = sym(ct, cm)
                    x = get(CL_EXTRA[s]) if s >= 16 else 0
                    b.cl_syms.append((s, x))
                    b.cl_hist[s] += 1
                    if s < 16:
                        seq.append(s)
                        continue
                    if s == 16:
                        if not seq:
                            raise InflateError("invalid bit length repeat (no previous length)")
                        v, r = seq[-1], 3 + x
                    else:
                        v, r = 0, (3 if s == 17 else 11) + x
                    if len(seq) + r > nt:
                        raise InflateError("invalid bit length repeat (past HLIT + HDIST)")
                    seq += [v] * r
                if seq[EOB] == 0:
                    raise InflateError("invalid code -- missing end-of-block")
                b.lens = seq[:b.hlit] + [0] * (NLIT - b.hlit) + seq[b.hlit:] + [0] * (NDIST - b.hdist)
                lt, lm = _decode_table(b.lens[:NLIT], "literal/lengths set", True)
                dt, dm = _decode_table(b.lens[NLIT:], "distances set", True)
            b.header_bits = pos - b.bit_off
            b.lit_hist, b.dist_hist = [0] * NLIT, [0] * NDIST
            lh, dh, toks = b.lit_hist, b.dist_hist, b.tokens
            while True:
                s, sl = sym(lt, lm)
                if s < 256:
                    lh[s] += 1
                    out.append(s)
                    toks.append(s)
                    continue
                if s == EOB:
                    lh[EOB] += 1
                    b.eob_bits = sl
                    break
                if s >= NLIT:
                    raise InflateError("invalid literal/length code")
                n = LEN_BASE[s - 257] + get(LEN_EXTRA[s - 257])
                ds, _ = sym(dt, dm)
                if ds >= NDIST:
                    raise InflateError("invalid distance code")
                dist = DIST_BASE[ds] + get(DIST_EXTRA[ds])
                if dist > len(out):
                    raise InflateError("invalid distance too far back")
                lh[s] += 1
                dh[ds] += 1
                toks.append((n, dist, s, ds))
                if dist >= n:
                    out += out[len(out) - dist:len(out) - dist + n]
                else:
                    for _ in range(n):
                        out.append(out[-dist])
        b.bit_len = pos - b.bit_off
        b.out_len = len(out) - b.out_off
        blocks.append(b)
        if b.bfinal:
            return bytes(out), blocks


def code_cost(counts, lens):
    """Sum of count * length; every counted symbol must have a length."""
    assert all(l for c, l in zip(counts, lens) if c), "a counted symbol has no code"
    return sum(c * l for c, l in zip(counts, lens))


def token_bits(block: Block):
    """A coded block's token bits recomputed from its histograms and code lengths (end of block
    excluded), independently of the positions the reader walked."""
    ll = block.lens[:NLIT] if block.btype == 2 else _FIXED_LENS[:NLIT]
    dl = block.lens[NLIT:] if block.btype == 2 else [5] * NDIST
    bits = sum(c * ll[s] for s, c in enumerate(block.lit_hist) if s != EOB)
    bits += sum(c * LEN_EXTRA[s - 257] for s, c in enumerate(block.lit_hist) if s > EOB)
    bits += sum(c * (dl[s] + DIST_EXTRA[s]) for s, c in enumerate(block.dist_hist))
    return bits


def huffman_cost(counts):
    """(optimal sum of count * length, depth) over the non-zero counts, with no length limit.  A
    single used symbol costs one bit each.  Two queues with leaves taken before internal nodes of
    equal weight: among the optimal trees this one has the least depth."""
    leaves = sorted(c for c in counts if c)
    if not leaves:
        return 0, 0
    if len(leaves) == 1:
        return leaves[0], 1
    inner, li, ii, cost = [], 0, 0, 0  # inner: (weight, height)

    def take():
        nonlocal li, ii
        if li < len(leaves) and (ii >= len(inner) or leaves[li] <= inner[ii][0]):
            li += 1
            return leaves[li - 1], 0
        ii += 1
        return inner[ii - 1]
    for _ in range(len(leaves) - 1):
        (w1, h1), (w2, h2) = take(), take()
        inner.append((w1 + w2, max(h1, h2) + 1))
        cost += w1 + w2
    return cost, inner[-1][1]


def package_merge(counts, maxb):
    """Optimal code lengths (0 for unused symbols) with no length above maxb."""
    used = sorted((c, i) for i, c in enumerate(counts) if c)
    lens = [0] * len(counts)
    if len(used) == 1:
        lens[used[0][1]] = 1
    if len(used) < 2:
        return lens
    assert len(used) <= 1 << maxb, "no code of that depth holds these symbols"
    leaves = [(c, (i,)) for c, i in used]
    prev = list(leaves)
    for _ in range(maxb - 1):
        packs = [(prev[k][0] + prev[k + 1][0], prev[k][1] + prev[k + 1][1]) for k in range(0, len(prev) - 1, 2)]
        prev = sorted(leaves + packs, key=lambda t: t[0])
    for _, syms in prev[:2 * len(used) - 2]:
        for i in syms:
            lens[i] += 1
    return lens


def zlib_limit(counts, maxb):
    """zlib's code lengths for these counts: trees.c's build_tree (its heap, ties by subtree depth)
    and gen_bitlen with max_length = maxb (depths clamped, then leaves moved down from the deepest
    level that has one until the overflow is gone, lengths reassigned by frequency)."""
    n = len(counts)
    size = 2 * n + 1
    freq = list(counts) + [0] * (n + 1)
    dad, depth, ln = [0] * size, [0] * size, [0] * size
    heap, heap_len, heap_max, max_code = [0] * (size + 1), 0, size, -1
    for i in range(n):
        if freq[i]:
            heap_len += 1
            heap[heap_len] = max_code = i
    while heap_len < 2:  # zlib forces two codes
        if max_code < 2:
            max_code += 1
            node = max_code
        else:
            node = 0
        heap_len += 1
        heap[heap_len] = node
        freq[node] = 1

    def smaller(a, b):
        return freq[a] < freq[b] or (freq[a] == freq[b] and depth[a] <= depth[b])

    def down(k):
        v, j = heap[k], k << 1
        while j <= heap_len:
            if j < heap_len and smaller(heap[j + 1], heap[j]):
                j += 1
            if smaller(v, heap[j]):
                break
            heap[k] = heap[j]
            k, j = j, j << 1
        heap[k] = v
    for k in range(heap_len // 2, 0, -1):
        down(k)
    node = n
    while True:
        a = heap[1]
        heap[1] = heap[heap_len]
        heap_len -= 1
        down(1)
        b = heap[1]
        heap_max -= 1
        heap[heap_max] = a
        heap_max -= 1
        heap[heap_max] = b
        freq[node] = freq[a] + freq[b]
        depth[node] = max(depth[a], depth[b]) + 1
        dad[a] = dad[b] = node
        heap[1] = node
        node += 1
        down(1)
        if heap_len < 2:
            break
    heap_max -= 1
    heap[heap_max] = heap[1]
    # gen_bitlen
    bl = [0] * (maxb + 2)
    overflow = 0
    ln[heap[heap_max]] = 0
    for h in range(heap_max + 1, size):
        m = heap[h]
        bits = ln[dad[m]] + 1
        if bits > maxb:
            bits = maxb
            overflow += 1
        ln[m] = bits
        if m <= max_code:
            bl[bits] += 1
    if overflow > 0:
        while overflow > 0:
            bits = maxb - 1
            while bl[bits] == 0:
                bits -= 1
            bl[bits] -= 1
            bl[bits + 1] += 2
            bl[maxb] -= 1
            overflow -= 2
        h = size
        for bits in range(maxb, 0, -1):
            k = bl[bits]
            while k:
                h -= 1
                m = heap[h]
                if m > max_code:
                    continue
                ln[m] = bits
                k -= 1
    return [ln[i] if freq[i] else 0 for i in range(n)]


def rle_lengths(seq):
    """Section 3.2.7's symbols for a sequence of code lengths, greedily: [(symbol, extra value)].
    Zero runs: 18 for 11..138 at a time, then 17 for 3..10, then single zeros.  Other runs: the
    length once, then 16 for 3..6 repeats at a time, then single lengths."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        r, i = j - i, j
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
                r -= k
            if r >= 3:
                out.append((17, r - 3))
                r = 0
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                r -= k
        out += [(v, 0)] * r
    return out
