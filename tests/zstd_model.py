"""A zstd decoder restated from RFC 8878, for the tests: the second opinion on the hand-built vectors
of tests/zstd_vectors.py (libzstd is the first) and the reader of every vector's structure.  Plain
Python over bytes, one symbol at a time; nothing here is shared with the code under test.

decode(stream) -> (bytes, [Frame]) or raises Bad; walk(stream) -> [Frame] from the headers alone
(no entropy decoding, so it is quick on the megabyte vectors); decode(stream, detail=True) ->
(bytes, [Frame], [[Detail]]): one Detail per block with everything the block's sections hold
(tests/zstd_structure.py checks the span encoder's choices on them).  The choices the library makes where
readers differ (kopia_amd/csrc/kcdc_zstd_format.h lists them) are made here too: a non-zero
Dictionary_ID is refused, an offset may not pass the frame's own output or Window_Size, a block may
not decode past Block_Maximum_Size."""
from collections import namedtuple

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
DEFAULTS = ((LL_DEFAULT, 6), (OF_DEFAULT, 5), (ML_DEFAULT, 6))
MAX_LOG = (9, 8, 9)
MAX_SYM = (35, 31, 52)
BLOCK_MAX = 128 << 10


class Bad(Exception):
    pass


Block = namedtuple("Block", "type size last lit_type streams size_format weights modes nseq reps decoded")
Frame = namedtuple("Frame", "single fcs_bytes window checksum did_bytes blocks skippable")
# One block in full (decode(detail=True)).  Every block: type (0 raw, 1 RLE, 2 compressed), size (the
# header's Block_Size), at / out_len (its bytes in the frame's output).  A compressed block besides:
#   lit_type, lits (the literal bytes), lit_hlen (header bytes), lit_comp (Compressed_Size; the
#   section's bytes after the header), streams, jump (the three jump-table sizes, or None);
#   weights (with the implied last one), maxbits (the longest code), tree_bytes (the description's
#   bytes, header byte included), tree_kind ('direct' | 'fse'): None / 0 without a tree;
#   fields: for LL, OF, ML a Field(mode, log, norm, rle, desc_bytes, desc): the accuracy log and counts
#   of a Predefined or FSE_Compressed table, the symbol of an RLE one, None for what Repeat_Mode keeps;
#   desc: the description's bytes (the RLE symbol's byte), desc_bytes their number;
#   seqs: [(ll, ml, offset value, resolved offset)]; nseq_bytes (Number_of_Sequences), seq_hlen (that,
#   the modes byte and the descriptions), bitstream (the bytes after them).
Field = namedtuple("Field", "mode log norm rle desc_bytes desc")
Detail = namedtuple("Detail", "type size at out_len lit_type lits lit_hlen lit_comp streams jump weights maxbits "
                    "tree_bytes tree_kind fields seqs nseq_bytes seq_hlen bitstream",
                    defaults=(None, b"", 0, 0, 0, None, None, 0, 0, None, (), (), 0, 0, 0))


def need(cond, what):
    if not cond:
        raise Bad(what)


class Fwd:
    """Little-endian bit reader, first bit first (FSE descriptions)."""

    def __init__(self, data):
        self.v, self.n, self.bit = int.from_bytes(data, "little"), 8 * len(data), 0

    def peek(self, nb):
        return (self.v >> self.bit) & ((1 << nb) - 1)

    def skip(self, nb):
        self.bit += nb
        need(self.bit <= self.n, "truncated FSE description")


class Back:
    """The backward bit stream: from the final-bit marker of the last byte down."""

    def __init__(self, data):
        need(len(data) > 0 and data[-1] != 0, "no final-bit marker")
        self.v = int.from_bytes(data, "little")
        self.pos = 8 * (len(data) - 1) + data[-1].bit_length() - 1

    def read(self, nb):
        v = self.peek(nb)
        self.pos -= nb
        return v

    def peek(self, nb):
        lo = self.pos - nb
        if lo >= 0:
            return (self.v >> lo) & ((1 << nb) - 1)
        if self.pos <= 0:
            return 0
        return (self.v & ((1 << self.pos) - 1)) << -lo  # zeros below the first bit


def read_fse(data, max_log, max_sym):
    """(normalized counts, accuracy log, bytes used)."""
    b = Fwd(data)
    log = b.peek(4) + 5
    b.skip(4)
    need(log <= max_log, "accuracy log over its limit")
    remaining, norm = (1 << log) + 1, []
    threshold, nb = 1 << log, log + 1
    while remaining > 1 and len(norm) <= max_sym:
        mx = 2 * threshold - 1 - remaining
        low = b.peek(nb - 1)
        if low < mx:
            count = low
            b.skip(nb - 1)
        else:
            count = b.peek(nb)
            if count >= threshold:
                count -= mx
            b.skip(nb)
        count -= 1
        remaining -= abs(count)
        norm.append(count)
        if count == 0:
            while True:
                r = b.peek(2)
                b.skip(2)
                norm += [0] * r
                need(len(norm) <= max_sym + 1, "symbol beyond the table")
                if r != 3:
                    break
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    need(remaining == 1 and len(norm) <= max_sym + 1, "FSE description does not sum")
    return norm, log, (b.bit + 7) // 8


def fse_table(norm, log):
    """[(symbol, bits, baseline)] of 1 << log states."""
    size = 1 << log
    cells, high = [None] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            cells[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            cells[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    need(pos == 0 and None not in cells, "FSE spread")
    nxt = [1 if c == -1 else c for c in norm]
    table = []
    for s in cells:
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


def read_weights(data):
    """(weights with the implied last one, longest code, bytes used, 'direct' | 'fse')."""
    need(len(data) >= 1, "truncated weights")
    hb = data[0]
    if hb >= 128:
        n = hb - 127
        need(len(data) >= 1 + (n + 1) // 2, "truncated weights")
        w = [(data[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
        used, kind = 1 + (n + 1) // 2, "direct"
    else:
        need(hb > 0 and len(data) >= 1 + hb, "truncated weights")
        norm, log, used_f = read_fse(data[1:1 + hb], 6, 255)
        table = fse_table(norm, log)
        need(used_f < hb, "no weight stream")
        b = Back(data[1 + used_f:1 + hb])
        s1, s2 = b.read(log), b.read(log)
        need(b.pos >= 0, "weights stream too short")
        w = []
        while True:
            need(len(w) <= 253, "too many weights")
            sym, nb, base = table[s1]
            w.append(sym)
            s1 = base + b.read(nb)
            if b.pos < 0:
                w.append(table[s2][0])
                break
            s1, s2 = s2, s1
        used, kind = 1 + hb, "fse"
    need(all(x <= 11 for x in w), "weight over 11")
    total = sum(1 << (x - 1) for x in w if x)
    need(total > 0, "no weights")
    log = total.bit_length()
    need(log <= 11, "code over 11 bits")
    rest = (1 << log) - total
    need(rest & (rest - 1) == 0, "weights do not complete a power of two")
    w.append(rest.bit_length())
    ones = w.count(1)
    need(ones >= 2 and ones % 2 == 0, "weight-1 symbols")
    return w, log, used, kind


def huffman_table(w, log):
    table = []
    for wt in range(1, log + 1):
        for s, x in enumerate(w):
            if x == wt:
                table += [(s, log + 1 - wt)] * (1 << (wt - 1))
    return table


def huffman_stream(data, table, log, count):
    b = Back(data)
    out = bytearray()
    for _ in range(count):
        s, nb = table[b.peek(log)]
        out.append(s)
        b.pos -= nb
    need(b.pos == 0, "Huffman stream not consumed exactly")
    return bytes(out)


def lit_header(blk):
    need(len(blk) >= 1, "truncated literals header")
    b0 = blk[0]
    t, sf = b0 & 3, (b0 >> 2) & 3
    if t < 2:
        hlen = 2 if sf == 1 else 3 if sf == 3 else 1
        need(len(blk) >= hlen, "truncated literals header")
        v = int.from_bytes(blk[:hlen], "little")
        regen = v >> 3 if hlen == 1 else v >> 4
        comp, streams = (regen if t == 0 else 1), 1
    else:
        hlen = 3 if sf < 2 else sf + 2
        need(len(blk) >= hlen, "truncated literals header")
        v = int.from_bytes(blk[:hlen], "little") >> 4
        nb = {3: 10, 4: 14, 5: 18}[hlen]
        regen, comp = v & ((1 << nb) - 1), v >> nb
        streams = 1 if sf == 0 else 4
    need(regen <= BLOCK_MAX and hlen + comp <= len(blk), "literals section larger than the block")
    return t, sf, hlen, regen, comp, streams


def seq_header(sec):
    need(len(sec) >= 1, "truncated sequences header")
    b0 = sec[0]
    if b0 < 128:
        n, h = b0, 1
    elif b0 < 255:
        need(len(sec) >= 2, "truncated sequences header")
        n, h = ((b0 - 128) << 8) + sec[1], 2
    else:
        need(len(sec) >= 3, "truncated sequences header")
        n, h = sec[1] + (sec[2] << 8) + 0x7F00, 3
    if n == 0:
        need(len(sec) == h, "bytes after an empty sequences section")
        return 0, h, None
    need(len(sec) > h, "truncated sequences header")
    m = sec[h]
    need(m & 3 == 0, "reserved mode bits")
    return n, h + 1, (m >> 6, (m >> 4) & 3, (m >> 2) & 3)


class State:
    """What a frame carries from block to block."""

    def __init__(self):
        self.huf = None
        self.tables = [None, None, None]
        self.rep = [1, 4, 8]


def decode_block(blk, st, out, frame_at, window, block_max, entropy=True, rec=None):
    """A compressed block: appends to out, returns its Block (rec: a list that takes its Detail)."""
    t, sf, hlen, regen, comp, streams = lit_header(blk)
    weights = None
    d = {"lit_type": t, "lit_hlen": hlen, "lit_comp": comp, "streams": streams}
    body = blk[hlen:hlen + comp]
    if t == 0:
        lits = body
    elif t == 1:
        lits = body * regen
    else:
        if t == 2:
            w, log, used, weights = read_weights(body)
            st.huf = (huffman_table(w, log), log)
            d.update(weights=w, maxbits=log, tree_bytes=used, tree_kind=weights)
            body = body[used:]
        need(st.huf is not None, "Treeless literals without a tree")
        lits = None
        if entropy:
            table, log = st.huf
            if streams == 1:
                lits = huffman_stream(body, table, log, regen)
            else:
                need(len(body) >= 6, "truncated jump table")
                l1, l2, l3 = (int.from_bytes(body[k:k + 2], "little") for k in (0, 2, 4))
                need(l1 + l2 + l3 <= len(body) - 6, "jump table larger than its section")
                seg = (regen + 3) // 4
                need(3 * seg <= regen, "4 streams for too few literals")
                d["jump"] = (l1, l2, l3)
                at, lits = 6, b""
                for k, ln in enumerate((l1, l2, l3, len(body) - 6 - l1 - l2 - l3)):
                    lits += huffman_stream(body[at:at + ln], table, log, seg if k < 3 else regen - 3 * seg)
                    at += ln
    sec = blk[hlen + comp:]
    nseq, h, modes = seq_header(sec)
    reps = set()
    start = len(out)
    fields, seqs = [], []
    d.update(lits=lits, fields=fields, seqs=seqs, nseq_bytes=h - (1 if nseq else 0), seq_hlen=h)

    def done(b):
        if rec is not None:
            rec.append(Detail(2, len(blk), start - frame_at, len(out) - start, **d))
        return b
    if nseq:
        need(regen + 3 * nseq <= block_max, "block decodes past its maximum")
        at = h
        for k in range(3):
            if modes[k] == 0:
                st.tables[k] = (fse_table(*DEFAULTS[k]), DEFAULTS[k][1])
                fields.append(Field(0, DEFAULTS[k][1], list(DEFAULTS[k][0]), None, 0, b""))
            elif modes[k] == 1:
                need(len(sec) > at and sec[at] <= MAX_SYM[k], "RLE symbol beyond the table")
                st.tables[k] = ([(sec[at], 0, 0)], 0)
                fields.append(Field(1, 0, None, sec[at], 1, sec[at:at + 1]))
                at += 1
            elif modes[k] == 2:
                norm, log, used = read_fse(sec[at:], MAX_LOG[k], MAX_SYM[k])
                st.tables[k] = (fse_table(norm, log), log)
                fields.append(Field(2, log, norm, None, used, sec[at:at + used]))
                at += used
            else:
                need(st.tables[k] is not None, "Repeat_Mode without a table")
                fields.append(Field(3, None, None, None, 0, b""))
        d.update(seq_hlen=at, bitstream=len(sec) - at)
        if not entropy:
            return done(Block(2, len(blk), 0, t, streams, sf, weights, modes, nseq, reps, None))
        b = Back(sec[at:])
        (lt, ll_log), (ot, of_log), (mt, ml_log) = st.tables
        ls, os_, ms = b.read(ll_log), b.read(of_log), b.read(ml_log)
        lp = 0
        for i in range(nseq):
            oc, mc, lc = ot[os_][0], mt[ms][0], lt[ls][0]
            ofv = (1 << oc) + b.read(oc)
            ml = ML_BASE[mc] + b.read(ML_BITS[mc])
            ll = LL_BASE[lc] + b.read(LL_BITS[lc])
            if i + 1 < nseq:
                ls = lt[ls][2] + b.read(lt[ls][1])
                ms = mt[ms][2] + b.read(mt[ms][1])
                os_ = ot[os_][2] + b.read(ot[os_][1])
            need(b.pos >= 0, "sequence stream too short")
            need(lp + ll <= regen, "sequences need more literals than the block has")
            out += lits[lp:lp + ll]
            lp += ll
            rep = st.rep
            if ofv > 3:
                off = ofv - 3
                st.rep = [off, rep[0], rep[1]]
            else:
                reps.add((ofv, ll == 0))
                idx = ofv - 1 + (1 if ll == 0 else 0)
                if idx == 0:
                    off = rep[0]
                else:
                    off = rep[0] - 1 if idx == 3 else rep[idx]
                    need(off != 0, "offset 0")
                    st.rep = [off, rep[0], rep[2]] if idx == 1 else [off, rep[0], rep[1]]
            need(off <= len(out) - frame_at, "offset beyond the bytes the frame has produced")
            need(off <= window, "offset beyond the window")
            need(len(out) - start + ml <= block_max, "block decodes past its maximum")
            seqs.append((ll, ml, ofv, off))
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                for _ in range(ml):
                    out.append(out[-off])
        need(b.pos == 0, "sequence stream not consumed exactly")
        out += lits[lp:]
    else:
        if not entropy:
            return done(Block(2, len(blk), 0, t, streams, sf, weights, modes, 0, reps, None))
        out += lits
    need(len(out) - start <= block_max, "block decodes past its maximum")
    return done(Block(2, len(blk), 0, t, streams, sf, weights, modes, nseq, reps, len(out) - start))


def xxh64(data):
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    M = (1 << 64) - 1
    rotl = lambda v, r: ((v << r) | (v >> (64 - r))) & M  # noqa: E731
    rnd = lambda a, v: (rotl((a + v * P2) & M, 31) * P1) & M  # noqa: E731
    n, at = len(data), 0
    if n >= 32:
        v = [(P1 + P2) & M, P2, 0, (-P1) & M]
        while at + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[at + 8 * k:at + 8 * k + 8], "little"))
            at += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = P5
    h = (h + n) & M
    while at + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[at:at + 8], "little")), 27) * P1 + P4) & M
        at += 8
    if at + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[at:at + 4], "little") * P1) & M, 23) * P2 + P3) & M
        at += 4
    while at < n:
        h = (rotl(h ^ (data[at] * P5) & M, 11) * P1) & M
        at += 1
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    return h ^ (h >> 32)


def decode(stream, entropy=True, detail=False):
    """(decoded bytes, [Frame]).  entropy=False: the headers alone (bytes are not produced).
    detail=True: (decoded bytes, [Frame], [[Detail] per frame]), one Detail per block."""
    stream = bytes(stream)
    out, frames, pos, n = bytearray(), [], 0, len(stream)
    details = []
    while pos < n:
        need(n - pos >= 4, "truncated magic")
        magic = int.from_bytes(stream[pos:pos + 4], "little")
        pos += 4
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            need(n - pos >= 4, "truncated skippable frame")
            size = int.from_bytes(stream[pos:pos + 4], "little")
            need(size <= n - pos - 4, "truncated skippable frame")
            pos += 4 + size
            frames.append(Frame(0, 0, 0, 0, 0, [], True))
            details.append([])
            continue
        need(magic == 0xFD2FB528, "bad magic")
        need(n - pos >= 1, "truncated frame header")
        fhd = stream[pos]
        pos += 1
        need(fhd & 8 == 0, "reserved bit")
        single, checksum = (fhd >> 5) & 1, (fhd >> 2) & 1
        window = 0
        if not single:
            need(n - pos >= 1, "truncated frame header")
            wd = stream[pos]
            pos += 1
            base = 1 << (10 + (wd >> 3))
            window = base + (base >> 3) * (wd & 7)
        did_bytes = (0, 1, 2, 4)[fhd & 3]
        need(n - pos >= did_bytes, "truncated frame header")
        need(not any(stream[pos:pos + did_bytes]), "a dictionary is asked for")
        pos += did_bytes
        fcs_bytes = (single, 2, 4, 8)[fhd >> 6]
        need(n - pos >= fcs_bytes, "truncated frame header")
        fcs = int.from_bytes(stream[pos:pos + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0) if fcs_bytes else None
        pos += fcs_bytes
        if single:
            window = fcs
        block_max = min(window, BLOCK_MAX)
        st, blocks, frame_at = State(), [], len(out)
        rec = []
        while True:
            need(n - pos >= 3, "truncated block header")
            bh = int.from_bytes(stream[pos:pos + 3], "little")
            pos += 3
            last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
            need(btype != 3, "block type 3")
            need(size <= block_max, "block over Block_Maximum_Size")
            if btype == 0:
                need(size <= n - pos, "truncated raw block")
                rec.append(Detail(0, size, len(out) - frame_at, size))
                out += stream[pos:pos + size]
                pos += size
                blocks.append(Block(0, size, last, None, 0, None, None, None, 0, set(), size))
            elif btype == 1:
                need(n - pos >= 1, "truncated RLE block")
                rec.append(Detail(1, size, len(out) - frame_at, size))
                out += stream[pos:pos + 1] * size
                pos += 1
                blocks.append(Block(1, size, last, None, 0, None, None, None, 0, set(), size))
            else:
                need(2 <= size <= n - pos and size < BLOCK_MAX, "truncated or oversized compressed block")
                b = decode_block(stream[pos:pos + size], st, out, frame_at, window, block_max, entropy, rec)
                blocks.append(b._replace(last=last))
                pos += size
            if last:
                break
        if entropy:
            need(fcs is None or fcs == len(out) - frame_at, "Frame_Content_Size mismatch")
        if checksum:
            need(n - pos >= 4, "truncated checksum")
            if entropy:
                need(int.from_bytes(stream[pos:pos + 4], "little") == xxh64(bytes(out[frame_at:])) & 0xFFFFFFFF, "checksum mismatch")
            pos += 4
        frames.append(Frame(single, fcs_bytes, window, checksum, did_bytes, blocks, False))
        details.append(rec)
    if detail:
        return bytes(out), frames, details
    return bytes(out), frames


def walk(stream):
    return decode(stream, entropy=False)[1]
