"""CPU: the detail records of tests/zstd_model.py and the span checker of tests/zstd_structure.py,
before either reads a frame the device wrote (tests/test_gpu_zstd_edges.py).

The records are pinned on frames of a foreign writer (libzstd, oracle.deflate.zstd_encode) and on
the hand-built vectors of tests/zstd_vectors.py: the sequences re-executed over the literals give
the block's bytes, the sizes add up to the block, counts sum to 2^log, weights complete a power of
two.  The checker is shown to bite: per invariant group one frame that libzstd and the model
decode but that breaks the group's promise is refused, by that group, while its well-formed twin
passes.  The host model of the layout (tools/zstd_span_model.py encode_chunk_t) passes the frame,
block, literals and offsets rules."""
import os
import random
import sys

import pytest

import zstd_model as zm
import zstd_structure as zs
import zstd_vectors as zv
from oracle import deflate

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import zstd_span_model as zsm  # noqa: E402


def text(n, seed):
    rnd = random.Random(seed)
    words = [b"kopia", b"snapshot", b"content", b"chunk", b"the", b"of", b"blob", b"index", b"manifest", b"epoch"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + (b" " if rnd.random() < 0.8 else b",\n")
        if rnd.random() < 0.1:
            out += b"%d" % rnd.randrange(100000)
    return bytes(out[:n])


def libzstd_frames():
    rnd = random.Random(4)
    skew = bytes(min(255, int(rnd.expovariate(0.03))) for _ in range(50000))
    return [deflate.zstd_encode(d, lv) for d, lv in ((text(70000, 1), 3), (text(20000, 2), 19), (skew, 1),
                                                     (text(3000, 3) + skew[:9000] + bytes(5000), 5), (b"", 3), (b"abc", 3))]


def check_details(stream):
    out, frames, details = zm.decode(stream, detail=True)
    assert (out, frames) == zm.decode(stream), "detail=True changes what decode returns"
    assert len(frames) == len(details)
    seen = {"seqs": 0, "fse": 0, "weights": 0}
    base = 0
    for f, ds in zip(frames, details):
        assert len(ds) == len(f.blocks)
        got = bytearray()
        for b, d in zip(f.blocks, ds):
            assert (d.type, d.size, d.at) == (b.type, b.size, len(got))
            if d.type != 2:
                assert d.out_len == b.decoded and not d.seqs and not d.fields
                got += out[base + d.at:base + d.at + d.out_len]
                continue
            assert (d.lit_type, d.streams, len(d.seqs)) == (b.lit_type, b.streams, b.nseq)
            # the block's bytes: header, literals section, sequences header, bitstream
            assert d.lit_hlen + d.lit_comp + d.seq_hlen + d.bitstream == d.size
            assert d.seq_hlen == d.nseq_bytes + (1 + sum(x.desc_bytes for x in d.fields) if d.seqs else 0)
            assert (d.bitstream > 0) == bool(d.seqs)
            if d.jump is not None:
                assert d.streams == 4 and 6 + sum(d.jump) < d.lit_comp - (d.tree_bytes if d.lit_type == 2 else 0)
            # the sequences over the literals give the block's bytes
            lp = 0
            for ll, ml, ov, off in d.seqs:
                assert ov >= 1 and 1 <= off <= len(got) + ll
                got += d.lits[lp:lp + ll]
                lp += ll
                for _ in range(ml):
                    got.append(got[-off])
                seen["seqs"] += 1
            got += d.lits[lp:]
            assert len(got) - d.at == d.out_len == b.decoded
            for k, x in enumerate(d.fields):
                assert x.mode == b.modes[k] and len(x.desc) == x.desc_bytes
                if x.mode in (0, 2):
                    assert sum(abs(c) for c in x.norm) == 1 << x.log
                if x.mode == 2:
                    assert zm.read_fse(x.desc, zm.MAX_LOG[k], zm.MAX_SYM[k]) == (x.norm, x.log, x.desc_bytes)
                    assert zs.write_ncount(x.norm, x.log) == x.desc  # libzstd writes the minimal description too
                    seen["fse"] += 1
                if x.mode == 1:
                    assert x.desc == bytes([x.rle])
                if x.mode == 3:
                    assert x.norm is None and x.desc_bytes == 0
            if d.lit_type == 2:
                assert d.tree_kind == b.weights and d.tree_bytes > 1
                assert sum(1 << (w - 1) for w in d.weights if w) == 1 << d.maxbits and d.weights[-1]
                assert max(zs.code_lengths(d.weights, d.maxbits)) == d.maxbits <= 11
                seen["weights"] += 1
            else:
                assert d.weights is None and d.tree_bytes == 0
        assert bytes(got) == out[base:base + len(got)]
        base += len(got)
    assert base == len(out)
    return seen


def test_detail_records_on_libzstd_frames():
    seen = {"seqs": 0, "fse": 0, "weights": 0}
    for s in libzstd_frames():
        for k, v in check_details(s).items():
            seen[k] += v
    assert seen["seqs"] > 1000 and seen["fse"] >= 6 and seen["weights"] >= 4, seen


def test_detail_records_on_hand_built_vectors():
    seen = {"seqs": 0, "fse": 0, "weights": 0}
    vectors = [v for v in zv.built_valid_vectors() if v.cap <= 64 << 10]  # (the megabyte ones test the device's room, not the reader)
    for v in vectors:
        for k, n in check_details(v.blob[4:]).items():
            seen[k] += n
    assert len(vectors) > 50 and seen["seqs"] > 100 and seen["fse"] >= 3 and seen["weights"] >= 5, seen


def test_description_writer_against_the_reader():
    """write_ncount and fse_weights (the checker's restatements of the writer's side) read back through
    the model: every zero-run length 0..40, less-than-one counts, and trees of 3..256 symbols."""
    for run in range(41):
        norm = [20, 0, 3] + [0] * run + [8, -1]
        assert sum(abs(c) for c in norm) == 32
        d = zs.write_ncount(norm, 5)
        assert zm.read_fse(d, 9, 52) == (norm, 5, len(d))
        assert d == zsm.write_ncount(norm, 5)
        assert zs.zero_runs(norm) == [1] + ([run] if run else [])
    rnd = random.Random(9)
    both = 0
    for trial in range(300):
        n = rnd.choice((3, 4, 5, 17, 64, 128, 129, 130, 131, 200, 255, 256))
        hi = rnd.choice((100, 129, 256))  # top <= 128: the trees that have a direct description too
        syms = sorted(rnd.sample(range(hi), min(n, hi)))
        freq = [0] * 256
        for s in syms:
            freq[s] = 1 + int(rnd.expovariate(0.02))
        lens = zsm.huff_lengths(freq)
        top, maxb = syms[-1], max(lens)
        w = [maxb + 1 - x if x else 0 for x in lens[:top + 1]]
        d = zs.fse_weights(w)
        if d is None:
            continue
        assert d[0] == len(d) - 1 < 127
        got = zm.read_weights(d)
        assert (got[0], got[1], got[2], got[3]) == (w, maxb, len(d), "fse")
        both += top <= 128
    assert both > 20


def test_table_log_rule():
    assert [zs.table_log(n, 2, 9) for n in (1, 4, 5, 129, 257, 513, 1025, 2049, 4097, 8192)] == [5, 5, 5, 5, 6, 7, 8, 9, 9, 9]
    assert zs.table_log(8192, 2, 8) == 8 and zs.table_log(40, 31, 9) == 5 and zs.table_log(40, 32, 9) == 6
    assert zs.normalize([10, 1, 1, 1], 5) == ([26, 2, 2, 2], 1)  # 25 + 3 x 2: the surplus branch
    assert zs.normalize([1000] + [1] * 20, 5)[1] == -19  # many count-1 codes: the deficit branch


# ------------------------------------------------------------------ the host model passes
@pytest.mark.parametrize("G", [16, 64])
def test_host_model_frames_pass(G):
    data = text(50000, 6) + bytes(range(7, 40)) * 700 + text(20000, 7)
    blob = zsm.encode_chunk_t(data, G)
    assert deflate.zstd_decode(blob) == data
    r = zs.check(blob, data, 1, ("frame", "block", "literals", "offsets"))  # (not "tree": the model writes direct weights only)
    kinds = "".join(sp.kinds for sp in r.spans)
    assert "h" in kinds and ("t" in kinds or G == 64)
    reps = [q for sp in r.spans for q in sp.seqs if q[2] == 1]
    assert any(q[0] > 0 for q in reps) and any(q[0] == 0 for q in reps)


# ------------------------------------------------------------------ the checker bites
END = zv.raw_block(b"")


def one_frame(blocks, n):
    return zv.frame(list(blocks) + [END], fcs=n, fcs_bytes=1 if n < 256 else 2 if n < 65792 else 4)


def refused(stream, data, group):
    """libzstd and the model decode it, the checker's `group` refuses it; returns the reason."""
    assert zv.zstd_decode(stream) == (data, True)
    assert zm.decode(stream)[0] == data
    with pytest.raises(zs.Violation) as e:
        zs.check(stream, data, 1, (group,))
    assert e.value.group == group
    return e.value.what


def test_refuses_frame_forms():
    data = zv.alphabet(300, 3)
    good = one_frame([zv.raw_block(data)], 300)
    zs.check(good, data)
    assert "smallest" in refused(zv.frame([zv.raw_block(data), END], fcs=300, fcs_bytes=4), data, "frame")
    assert "Single_Segment" in refused(zv.frame([zv.raw_block(data), END], window_log=10), data, "frame")
    assert "checksum" in refused(zv.frame([zv.raw_block(data), END], fcs=300, fcs_bytes=2, checksum=data), data, "frame")
    assert "last block" in refused(zv.frame([zv.raw_block(data)], fcs=300, fcs_bytes=2), data, "frame")
    assert "empty block" in refused(one_frame([zv.raw_block(data), zv.raw_block(b"")], 300), data, "frame")
    refused(deflate.zstd_encode(data, 3), data, "frame")  # libzstd closes with the data block itself
    with pytest.raises(zs.Violation):  # bytes after the frame: a second (skippable) frame
        zs.check(good + zv.skippable(b"x"), data)
    with pytest.raises(zs.Violation):
        zs.check(good, data[:-1] + b"!")


def test_refuses_a_compressed_block_larger_than_its_content():
    data = zv.alphabet(200, 5)
    hist = zv.alphabet(300, 8)  # (a frame of the one block alone would pass its own Block_Maximum_Size)
    assert "Compressed_Block" in refused(one_frame([zv.raw_block(hist), zv.comp_block(data, [])], 500), hist + data, "block")
    assert "RLE_Block" in refused(one_frame([zv.rle_block(7, 200)], 200), bytes([7]) * 200, "block")
    big = zv.alphabet(40000, 1)
    assert "crosses" in refused(one_frame([zv.raw_block(big)], 40000), big, "block")
    shrunk = bytes(180) + zv.alphabet(20, 5)  # its twin: one zero, a match of 179, 20 literals
    zs.check(one_frame([zv.comp_block(bytes(1) + zv.alphabet(20, 5), [(1, 179, 3 + 1)])], 200), shrunk, 1, ("frame", "block"))


def skewed(n, seed, top=90):
    rnd = random.Random(seed)
    return bytes(min(top, 32 + int(rnd.expovariate(0.12))) for _ in range(n))


def huff_section(lits, desc, lens=None):
    """A one-stream Compressed_Literals section with this tree description."""
    stream = zv.huff_literals(lits, lens=lens, treeless=True)[3:]
    body = desc + stream
    return (2 | (len(lits) << 4) | (len(body) << 14)).to_bytes(3, "little") + body


LIT = ("frame", "block", "literals", "lengths")


def test_refuses_literals_forms():
    lits = skewed(1000, 1)
    good = one_frame([zv.comp_block(lits, [], lit_section=zv.huff_literals(lits))], 1000)
    zs.check(good, lits, 1, LIT)
    four = one_frame([zv.comp_block(lits, [], lit_section=zv.huff_literals(lits, streams=4))], 1000)
    assert "4 stream" in refused(four, lits, "literals")
    # a tree sent twice; its well-formed twin sends it once and goes Treeless
    a, b = skewed(900, 2), skewed(800, 3)
    lens = zsm.huff_lengths(zv._freq(a + b))
    twice = [zv.comp_block(x, [], lit_section=zv.huff_literals(x, lens=lens)) for x in (a, b)]
    once = [twice[0], zv.comp_block(b, [], lit_section=zv.huff_literals(b, lens=lens, treeless=True))]
    zs.check(one_frame(once, 1700), a + b, 1, LIT)
    assert "twice" in refused(one_frame(twice, 1700), a + b, "literals")
    # a wide raw literals header, an RLE literals section
    wide = one_frame([zv.block(2, zv.raw_lits(zv.alphabet(20), hlen=2) + zv.seq_section([(20, 30, 3 + 20)]))], 50)
    assert "raw header" in refused(wide, zv.alphabet(20) + (zv.alphabet(20) * 2)[:30], "literals")
    rle = one_frame([zv.raw_block(zv.alphabet(50)), zv.block(2, zv.rle_lits(65, 100) + zv.seq_section([]))], 150)
    assert "RLE literals" in refused(rle, zv.alphabet(50) + b"A" * 100, "literals")


def test_refuses_the_larger_tree_description():
    """Direct weights where the FSE-compressed ones are smaller and the reverse; the twins carry the
    checker's own restatement of the encoder's FSE description, which libzstd and the model read."""
    def weights(lits):
        lens = zsm.huff_lengths(zv._freq(lits))
        return [max(lens) + 1 - x if x else 0 for x in lens[:max(lits) + 1]]
    many = skewed(1000, 1)  # 43 symbols up to 84: 43 bytes of direct weights
    fse = zs.fse_weights(weights(many))
    assert len(fse) < 43
    r = zs.check(one_frame([zv.comp_block(many, [], lit_section=huff_section(many, fse))], 1000), many, 1, LIT + ("tree",))
    assert r.spans[0].desc == ("fse", 43, len(fse))
    direct = one_frame([zv.comp_block(many, [], lit_section=zv.huff_literals(many))], 1000)
    assert "fse is the smaller" in refused(direct, many, "tree")
    low = bytes([2, 3, 4, 5, 6] * 30 + [2] * 100 + [3] * 40)  # symbols 2..6: 4 bytes direct, the FSE form is longer
    good = one_frame([zv.comp_block(low, [], lit_section=zv.huff_literals(low))], len(low))
    r = zs.check(good, low, 1, LIT + ("tree",))
    kind, dsz, fsz = r.spans[0].desc
    assert kind == "direct" and dsz == 4 and fsz is not None
    assert len(zs.fse_weights(weights(low))) > 4
    bad = one_frame([zv.comp_block(low, [], lit_section=huff_section(low, zs.fse_weights(weights(low))))], len(low))
    assert "direct is the smaller" in refused(bad, low, "tree")


def test_refuses_code_lengths_off_the_optimum():
    lits = skewed(1000, 4)
    flat = zsm.huff_lengths([1 if c else 0 for c in zv._freq(lits)])
    bad = one_frame([zv.comp_block(lits, [], lit_section=zv.huff_literals(lits, lens=flat))], 1000)
    assert "optimum" in refused(bad, lits, "lengths")
    # a histogram whose optimum is 13 bits deep: package-merge passes, a cruder limiter does not
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377]
    deep = b"".join(bytes([48 + k]) * c for k, c in enumerate(fib))
    deep = bytes(random.Random(5).sample(list(deep), len(deep)))
    r = zs.check(one_frame([zv.comp_block(deep, [], lit_section=zv.huff_literals(deep))], len(deep)), deep, 1, ("lengths",))
    assert r.spans[0].limit == "limited" and r.spans[0].tree.maxbits == 11
    # the same histogram under a 10-bit package-merge code: complete and decodable, but dearer than
    # zlib's limiter at 11 bits
    short = zs.dm.package_merge(zv._freq(deep), 10)
    worse = one_frame([zv.comp_block(deep, [], lit_section=zv.huff_literals(deep, lens=short))], len(deep))
    assert "package-merge" in refused(worse, deep, "lengths")


def split_zero_runs(norm, log):
    """A valid but non-minimal description: every zero of a run with a repeat flag of its own."""
    w = zs._Bits()
    w.put(log - 5, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    for c in norm:
        small, x = 2 * threshold - 1 - remaining, c + 1
        if x < small:
            w.put(x, nb - 1)
        else:
            w.put(x if x < threshold else x + small, nb)
        remaining -= abs(c)
        if c == 0:
            w.put(0, 2)
        while 1 < remaining < threshold:
            nb, threshold = nb - 1, threshold >> 1
    return w.bytes()


def table_case(ml_tab=None, ll_tab=None, count_width=None, later=None):
    """40 sequences, literal lengths 1 and 2, match lengths 4 and 40, offsets 8 and 40, in one block
    (or two: later = the second block's tables)."""
    seqs = [(1 + k % 2, 4 if k % 3 else 40, 3 + (8 if k % 5 else 40)) for k in range(40)]
    norm = [0] * 35
    norm[1], norm[34] = 19, 13
    ml = ml_tab or zv.fse_tab(norm, 5)
    tabs = [ll_tab or zv.PRE[0], zv.PRE[1], ml]
    hist = zv.alphabet(60, 9)
    blocks, data = [zv.raw_block(hist)], bytearray(hist)

    def add(sq, tb):
        lits = zv.alphabet(sum(s[0] for s in sq), len(data))
        blocks.append(zv.comp_block(lits, sq, tabs=tb, width=count_width))
        lp = 0
        for ll, m, ov in sq:
            data.extend(lits[lp:lp + ll])
            lp += ll
            for _ in range(m):
                data.append(data[-(ov - 3)])
    if later is None:
        add(seqs, tabs)
    else:
        add(seqs[:20], tabs)
        add(seqs[20:], later(tabs))
    return one_frame(blocks, len(data)), bytes(data), norm


def test_refuses_table_forms():
    good, data, norm = table_case()
    # (the raw history block hides nothing here, but the span is not `full`: the one-sided rules)
    zs.check(good, data, 1, ("frame", "block", "tables"))
    bad, data, _ = table_case(ml_tab=(2, zv.fse_tab(norm, 5)[1], split_zero_runs(norm, 5)))
    assert zm.decode(bad, detail=True)[2][0][1].fields[2].norm == norm
    assert "minimal" in refused(bad, data, "tables")
    wide, data, _ = table_case(count_width=2)
    assert "Number_of_Sequences" in refused(wide, data, "tables")
    again, data, _ = table_case(later=lambda t: t)
    assert "Repeat_Mode" in refused(again, data, "tables")
    rep, data, _ = table_case(later=lambda t: [zv.repeat(x) for x in t])
    zs.check(rep, data, 1, ("frame", "block", "tables"))
    rle = [(3, 4, 3 + 8), (3, 4, 3 + 20)] * 3  # one literal length, one match length, two offset codes
    lits, hist = zv.alphabet(18, 2), zv.alphabet(60, 9)
    body = execute(hist, lits, rle)
    full = one_frame([zv.comp_block(hist, []), zv.comp_block(lits, rle, tabs=[zv.rle_tab(3), zv.PRE[1], zv.rle_tab(1)])], len(body))
    r = zs.check(full, body, 1, ("tables",))
    assert r.spans[0].full and r.spans[0].table_carrier == 1
    pre = one_frame([zv.comp_block(hist, []), zv.comp_block(lits, rle)], len(body))
    assert "RLE" in refused(pre, body, "tables")


def execute(hist, lits, seqs):
    """The bytes a decoder makes of `hist` and then these (ll, ml, offset value) sequences."""
    data, lp, rep = bytearray(hist), 0, [1, 4, 8]
    for ll, ml, ov in seqs:
        data += lits[lp:lp + ll]
        lp += ll
        if ov > 3:
            off = ov - 3
            rep = [off] + rep[:2]
        else:
            idx = ov - 1 + (ll == 0)
            off = rep[0] - 1 if idx == 3 else rep[idx]
            if idx:
                rep = [off] + [x for k, x in enumerate(rep) if k != min(idx, 2)]
        for _ in range(ml):
            data.append(data[-off])
    return bytes(data + lits[lp:])


def offsets_case(seqs):
    hist = zv.alphabet(64, 3)
    lits = zv.alphabet(sum(s[0] for s in seqs) + 2, 77)
    data = execute(hist, lits, seqs)
    return one_frame([zv.raw_block(hist), zv.comp_block(lits, seqs)], len(data)), data


def test_refuses_offset_choices():
    taken = [(3, 5, 3 + 20), (2, 4, 1), (0, 6, 3 + 9), (0, 4, 3 + 9), (0, 4, 1), (1, 4, 3 + 30)]
    zs.check(*offsets_case(taken), 1, zs.GROUPS)
    missed = [(3, 5, 3 + 20), (2, 4, 3 + 20)]
    assert "repeat due: True" in refused(*offsets_case(missed), "offsets")
    missed0 = [(1, 6, 3 + 9), (0, 4, 3 + 9), (0, 4, 3 + 9)]
    assert "repeat due: True" in refused(*offsets_case(missed0), "offsets")
    first = [(3, 5, 1)]
    assert "repeat due: False" in refused(*offsets_case(first), "offsets")
    for ov in (2, 3):
        assert f"offset value {ov}" in refused(*offsets_case([(3, 5, 3 + 20), (2, 4, ov)]), "offsets")


def test_refuses_fastest_forms():
    """The zstd-fastest rules on hand-built one-segment blocks."""
    hist = zv.alphabet(512, 1)
    lits = zv.alphabet(40, 200)

    def case(seqs, hlen=2, tabs=zv.PRE, split=False):
        data = execute(hist, lits, seqs)
        blocks = [zv.raw_block(hist[:256]), zv.raw_block(hist[256:])] if split else [zv.raw_block(hist)]
        return one_frame(blocks + [zv.block(2, zv.raw_lits(lits, hlen=hlen) + zv.seq_section(seqs, tabs))], len(data)), data
    seqs = [(20, 236, 3 + 512), (20, 236, 3 + 300)]
    zs.check(*case(seqs), 0)
    for bad, why in ((case(seqs, hlen=3), "2-byte"), (case([seqs[0], (20, 236, 1)]), "repeat offset"),
                     (case(seqs, tabs=[zv.PRE[0], zv.PRE[1], zv.rle_tab(43)]), "Predefined"), (case(seqs, split=True), "one segment")):
        assert deflate.zstd_decode(bad[0]) == bad[1]
        with pytest.raises(zs.Violation) as e:
            zs.check(*bad, 0)
        assert e.value.group == "fastest" and why in e.value.what, e.value
