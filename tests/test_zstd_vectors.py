"""CPU: the vectors of tests/zstd_vectors.py keep their conditions (libzstd is the judge of every
expectation, tests/zstd_model.py the second opinion), the zstd decoder's validity header decodes or
refuses each of them on the host under AddressSanitizer and UBSan (tools/zstd_decode_host.cpp
through kopia_amd/csrc/kcdc_zstd_format.h) before any reaches a GPU, the kcdc_zstd_decode_* entry
points are declared and answer their argument errors without a device, and the zstd kernels' code
objects hold what DESIGN.md 2.7d says of them."""
import os
import re
import subprocess

import pytest

import zstd_model as zm
import zstd_vectors as zv
from kopia_amd import _lib
from kopia_amd import compression as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 << 10   # gfx950
WAVES_PER_CU = 16        # the entropy grid is 16 waves for each CU
SYMBOLS = ("kcdc_zstd_decode_algorithms", "kcdc_zstd_decode_workspace_size", "kcdc_zstd_decode_chunks_device")


@pytest.fixture(autouse=True, scope="module")
def decoder_present():
    """The vectors are the decoder's: their conditions say nothing without the entry points they are for."""
    syms = _lib.exported_symbols()
    assert all(s in syms for s in SYMBOLS), "the library has no kcdc_zstd_decode_* entry points"


# ------------------------------------------------------------------ the vectors' conditions
def test_expected_bytes_come_from_libzstd():
    for v in zv.valid_vectors() + [zv.enomem_twin()]:
        got, clean = zv.zstd_decode(v.blob[4:])
        assert clean and got == v.expected and v.status == 0 and v.cap >= len(v.expected), v.id
        assert len(v.expected) <= zv.MAX_DECODED and v.blob[:4] == zv.header(v.name), v.id


def test_libzstd_refuses_every_corrupt_vector():
    """But where the rule is this library's own (zv.OWN_RULES): the header ID, the cap, a non-zero
    Dictionary_ID, the window, the descriptor room, and what RFC 8878 refuses and libzstd 1.4.8 lets
    pass."""
    seen = set()
    for v in zv.corrupt_vectors():
        assert v.expected == b"" and v.status in (zv.EBADMSG, zv.EOVERFLOW, zv.ENOMEM), v.id
        got, clean = zv.zstd_decode(v.blob[4:])
        if v.status == zv.EOVERFLOW:
            assert clean and len(got) > v.cap and v.id.startswith("cap-"), v.id
        elif v.status == zv.ENOMEM:
            assert clean and zv.descriptors(v.blob[4:]) > 4 + v.cap // 1024 + v.extra, v.id
        elif not any(v.id.startswith(rule) for rule in zv.OWN_RULES):
            assert not clean, v.id
        seen.add(v.status)
    assert seen == {zv.EBADMSG, zv.EOVERFLOW, zv.ENOMEM}
    assert len(zv.corrupt_vectors()) >= 60
    ids = [v.id for v in zv.all_vectors()]
    assert len(set(ids)) == len(ids)


def test_model_agrees_on_the_built_vectors():
    """The model of the contract (header ID, cap, descriptors over tests/zstd_model.py's decoder)
    gives every hand-built vector its status and bytes; no expectation rests on it alone."""
    for v in zv.built_valid_vectors() + zv.corrupt_vectors() + [zv.enomem_twin()]:
        assert zv.model(v.name, v.blob, v.cap, v.extra) == (v.status, v.expected), v.id


def test_every_corrupt_vector_is_refused_for_its_own_reason():
    """A vector named for one defect and refused for another tests nothing: the model's reason for
    refusing each malformed stream is the one the vector was built for.  The cap, descriptor and
    header-ID vectors hold well-formed streams (why is None): the model decodes them."""
    for v in zv.corrupt_vectors():
        got = zv.model_reason(v.blob[4:])
        if v.why is None:
            assert got is None or v.id.startswith(("wrong-header-id", "frame-under")), (v.id, got)
            assert v.status != zv.EBADMSG or v.blob[:4] != zv.header(v.name) or len(v.blob) < 4, v.id
        else:
            assert v.status == zv.EBADMSG and got is not None and v.why in got, (v.id, v.why, got)
    reasons = {v.why for v in zv.corrupt_vectors()} - {None}
    assert len(reasons) >= 40, sorted(reasons)


def test_four_stream_vectors_hold_four_streams():
    """The small 4-stream sections are what their names say: (type, streams, regenerated size) read
    from the literals header, the jump-table vectors' included."""
    def lits(vid, block=-1):
        v = next(v for v in zv.all_vectors() if v.id == vid)
        frames = [f for f in zm.walk(v.blob[4:]) if not f.skippable]
        b = frames[0].blocks[block]
        return b.lit_type, b.streams
    assert lits("huffman-4-streams-one-short-stream") == (2, 4)
    assert lits("huffman-4-streams-of-2-2-2-and-0-literals") == (2, 4)
    assert lits("huffman-4-streams-for-few-literals") == (2, 4)
    assert lits("treeless-after-a-raw-literals-block") == (3, 4) and lits("treeless-after-a-raw-literals-block", 2) == (3, 1)
    for vid in ("jump-table-larger-than-its-section-by-the-first-size", "jump-table-larger-than-its-section-by-the-second-size",
                "jump-table-larger-than-its-section-by-the-third-size", "section-ends-inside-its-jump-table",
                "four-streams-for-5-literals", "four-streams-for-1-literal", "jump-table-sizes-off-by-one",
                "huffman-stream-with-a-zero-last-byte"):
        assert lits(vid) == (2, 4), vid


def test_model_agrees_on_the_small_foreign_vectors():
    for v in zv.foreign_vectors():
        if len(v.expected) <= (64 << 10) + 1:
            assert zm.decode(v.blob[4:])[0] == v.expected, v.id


def test_xxh64_of_the_model():
    assert zm.xxh64(b"") == 0xEF46DB3751D8E999 and zm.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert zm.xxh64(b"abc") == 0x44BC2CF5AD770999


def test_vector_set_covers_the_list():
    ids = {v.id for v in zv.all_vectors()}
    for kind in zv.FOREIGN_KINDS:
        for size in zv.SIZES:
            assert f"libzstd-{kind}-{size}" in ids
    assert zv.SIZES == (0, 1, 300, (64 << 10) + 1, 128 << 10, (128 << 10) + 1, (1 << 20) + 3)
    want = {f"repeat-code-{c}-ll-{ll}-and-rotation" for c in (1, 2, 3) for ll in (0, 2)}
    want |= {f"offset-1-length-{n}" for n in (3, 64, 65, 65536)}
    want |= {f"offset-{o}-lengths-either-side" for o in (63, 64, 65)}
    want |= {f"{n}-sequences-in-a-block" for n in (63, 64, 65, 128, 129)}
    want |= {f"checksummed-frame-of-{n}-bytes" for n in zv.CHECKSUMMED}
    want |= {f"checksummed-frame-of-{n}-bytes-one-checksum-bit-flipped" for n in zv.CHECKSUMMED}
    # an over-full FSE description cannot be written (kcdc_zstd_format.h, fse_read): its reachable
    # neighbours are a description short of its table and zero-repeat flags that pass the last symbol
    want |= {f"{t}-{what}" for t in ("ll", "of", "ml") for what in ("accuracy-log-over-its-limit", "rle-symbol-beyond-its-table",
                                                                   "fse-symbol-beyond-its-table", "fse-description-short-of-its-table",
                                                                   "zero-repeat-flags-beyond-its-table", "repeat-mode-in-the-first-block")}
    want |= {f"jump-table-larger-than-its-section-by-the-{k}-size" for k in ("first", "second", "third")}
    want |= {"initial-repeat-offsets-1-4-8", "repeats-carried-across-compressed-raw-rle-blocks", "repeats-reset-at-a-new-frame",
             "match-source-inside-its-own-batch", "match-source-straddles-the-batch-start", "match-source-ends-at-the-batch-start",
             "every-match-reads-the-previous-match", "offset-equal-to-the-bytes-produced",
             "match-into-the-previous-block-back-to-the-first-byte", "block-with-no-sequences", "block-with-no-literals",
             "trailing-literals-after-the-last-sequence", "two-byte-count-for-5-sequences", "three-byte-count-0x7f00-sequences",
             "ll-code-35-and-ml-code-52", "rle-mode-for-each-table", "fse-compressed-accuracy-log-5-then-repeat-mode",
             "fse-compressed-accuracy-logs-9-8-9", "less-than-1-symbols-and-zero-repeat-flags", "huffman-11-bit-codes-even-weight-count",
             "huffman-odd-symbol-count-with-gaps", "huffman-4-streams-18-bit-sizes", "treeless-after-a-raw-literals-block", "huffman-4-streams-one-short-stream",
             "skippable-frames-of-size-0-at-the-start-and-the-end", "dictionary-id-field-of-1-bytes-holding-0", "content-size-of-8-bytes",
             "truncated-inside-magic", "truncated-inside-frame-header", "truncated-inside-block-header", "truncated-inside-literals-header",
             "truncated-inside-jump-table", "truncated-inside-a-huffman-stream", "truncated-inside-the-weight-description",
             "truncated-inside-an-fse-description", "truncated-inside-the-sequence-bit-stream", "truncated-inside-before-the-checksum",
             "truncated-inside-the-checksum", "block-type-3", "raw-block-over-block-maximum-size", "block-decodes-past-128-kib",
             "weights-do-not-complete-a-power-of-two", "section-ends-inside-its-jump-table", "huffman-stream-with-a-zero-last-byte",
             "four-streams-for-5-literals", "weights-without-a-pair-of-weight-1-symbols", "huffman-code-of-12-bits", "fse-weights-that-never-end",
             "block-decodes-past-block-maximum-size-by-a-match", "block-decodes-past-block-maximum-size-by-trailing-literals",
             "cap-reached-by-the-last-byte-of-a-match", "cap-below-the-literals-of-a-block", "cap-below-a-third-of-the-sequences",
             "huffman-4-streams-of-2-2-2-and-0-literals",
             "sequence-stream-with-a-zero-last-byte", "sequence-stream-not-consumed-exactly", "huffman-stream-not-consumed-exactly-bits-left",
             "sequences-need-more-literals-than-the-block-has", "offset-0-from-rep1-minus-1", "offset-beyond-the-bytes-produced",
             "offset-into-the-previous-frame", "offset-beyond-the-window", "frame-content-size-one-short", "frame-content-size-one-over",
             "reserved-bit", "dictionary-id-of-1-bytes-not-zero", "wrong-header-id", "frame-under-another-zstd-name",
             "cap-reached-by-literals", "cap-reached-by-a-match", "cap-reached-by-a-raw-block", "cap-reached-by-an-rle-block",
             "cap-reached-by-trailing-literals", "cap-below-the-content-size", "more-empty-raw-blocks-than-descriptors",
             "empty-raw-blocks-with-descriptors-for-them"}
    assert want <= ids, sorted(want - ids)


def test_vectors_hold_every_structure():
    """Read back with the model: every block type, literals type, stream count and size format,
    direct and FSE-compressed weights, each mode of each table, each repeat code with and without
    literals, every content-size width, and the 1 KiB-block stream exactly at the descriptor rule."""
    block_types, lit_types, streams, formats, weights, reps, fcs = set(), set(), set(), set(), set(), set(), set()
    modes = [set(), set(), set()]
    for v in zv.valid_vectors():
        small = len(v.expected) <= 4096 or v in zv.built_valid_vectors()
        frames = zm.decode(v.blob[4:])[1] if small else zm.walk(v.blob[4:])
        for f in frames:
            if f.skippable:
                continue
            fcs.add((f.single, f.fcs_bytes))
            for b in f.blocks:
                block_types.add(b.type)
                if b.type != 2:
                    continue
                lit_types.add(b.lit_type)
                formats.add((b.lit_type >= 2, b.size_format))
                if b.lit_type >= 2:
                    streams.add(b.streams)
                if b.weights:
                    weights.add(b.weights)
                if b.modes:
                    for t in range(3):
                        modes[t].add(b.modes[t])
                reps |= b.reps
    assert block_types == {0, 1, 2} and lit_types == {0, 1, 2, 3} and streams == {1, 4}
    assert formats >= {(False, 0), (False, 1), (False, 3), (True, 0), (True, 1), (True, 2), (True, 3)}
    assert weights == {"direct", "fse"}
    assert all(m == {0, 1, 2, 3} for m in modes), modes
    assert reps == {(c, z) for c in (1, 2, 3) for z in (False, True)}
    assert fcs >= {(0, 0), (1, 1), (1, 2), (1, 4), (0, 8), (1, 8), (0, 2)}
    by = {v.id: v for v in zv.valid_vectors()}
    v = by[f"libzstd-windowlog10-{(1 << 20) + 3}"]
    # 1 KiB blocks: a frame, 1,025 blocks (the last holds 3 bytes): two short of the rule's room, and no extra asked
    assert 0 <= 4 + v.cap // 1024 - zv.descriptors(v.blob[4:]) <= 2 and v.extra == 0
    assert sum(1 for f in zm.walk(by["libzstd-two-frames-300"].blob[4:]) if not f.skippable) == 2


# ------------------------------------------------------------------ the host program
def test_host_program_decodes_every_valid_vector():
    res = zv.run_host_program()
    for v in zv.valid_vectors() + [zv.enomem_twin()]:
        assert res[v.id] == (0, len(v.expected), True), v.id


def test_host_program_refuses_every_corrupt_vector():
    res = zv.run_host_program()
    for v in zv.corrupt_vectors():
        assert res[v.id] == (v.status, 0, True), v.id


MUTATIONS = {  # a bound of kcdc_zstd_format.h -> (its line, the line without it, the vectors that reach it alone)
    "jump table": ("if (l1 > body || l2 > body - l1 || l3 > body - l1 - l2) {", "if (false) {",
                   ("jump-table-larger-than-its-section-by-the-first-size", "jump-table-larger-than-its-section-by-the-second-size",
                    "jump-table-larger-than-its-section-by-the-third-size")),
    "four streams": ("if (left < 6u || 3u * seg > regen) {", "if (false) {",
                     ("section-ends-inside-its-jump-table", "four-streams-for-5-literals", "four-streams-for-1-literal")),
    "power of two": ("if (rest & (rest - 1u)) return kBadMsg;", "", ("weights-do-not-complete-a-power-of-two",)),
    "weight-1 pair": ("if (ones < 2u || (ones & 1u)) return kBadMsg;", "", ("weights-without-a-pair-of-weight-1-symbols",)),
    "code length": ("if (log > kHufLog) return kBadMsg;", "", ("huffman-code-of-12-bits",)),
    "literals against the cap": ("if (r.ll > cap - at || r.ml > cap - at - r.ll) {", "if (r.ml > cap - at - r.ll) {",
                                 ("cap-reached-by-literals",)),
    "match against the cap": ("if (r.ll > cap - at || r.ml > cap - at - r.ll) {", "if (r.ll > cap - at) {",
                              ("cap-reached-by-a-match", "cap-reached-by-the-last-byte-of-a-match")),
    "trailing literals against the cap": ("if (trail > cap - o) return kOverflow;", "", ("cap-reached-by-trailing-literals",)),
    "offset against the frame": ("if (off > at + r.ll - frame_at || off > window) {", "if (off > window) {",
                                 ("offset-beyond-the-bytes-produced", "offset-into-the-previous-frame")),
}


def test_each_bound_is_held_by_its_vectors(tmp_path):
    """With one bound taken out of a copy of kcdc_zstd_format.h, the sanitizer-built host program no
    longer gives that bound's vectors their status (or the sanitizers report): every vector below
    reaches the check it is named for, and nothing else catches what the check lets through."""
    from concurrent.futures import ThreadPoolExecutor
    src = open(os.path.join(ROOT, "kopia_amd", "csrc", "kcdc_zstd_format.h")).read()
    by = {v.id: v for v in zv.all_vectors()}

    def run(item):
        what, (line, without, ids) = item
        assert src.count(line) == 1, what
        d = tmp_path / what.replace(" ", "_")
        d.mkdir()
        (d / "kcdc_zstd_format.h").write_text(src.replace(line, without))
        exe = str(d / "host")
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(d), os.path.join(ROOT, "tools", "zstd_decode_host.cpp"),
                        "-o", exe], check=True)
        held = []
        for vid in ids:
            zv.write_vector_file(str(d / "v.bin"), [by[vid]])
            held.append(subprocess.run([exe, str(d / "v.bin")], capture_output=True).returncode == 0)
        return what, held

    with ThreadPoolExecutor(4) as ex:
        for what, held in ex.map(run, MUTATIONS.items()):
            assert not any(held), (what, held)


# ------------------------------------------------------------------ the entry points
def test_zstd_decode_symbols_declared():
    syms = _lib.exported_symbols()
    for s in SYMBOLS:
        assert s in syms and hasattr(_lib.lib(), s), s
    from test_lib_host import header_symbols
    assert set(SYMBOLS) <= set(header_symbols())
    assert kc.ZstdDecodableAlgorithms() == zv.FOUR
    assert not set(kc.ZstdDecodableAlgorithms()) & (set(kc.DecompressibleAlgorithms()) | set(kc.InflatableAlgorithms()))
    assert set(kc.ZstdDecodableAlgorithms()) <= set(kc.SupportedAlgorithms())
    assert {n: kc.HeaderID(n) for n in zv.FOUR} == zv.HEADER_IDS


def test_argument_errors_need_no_device():
    L = _lib.lib()
    args = [None] * 3 + [0] + [None] * 6 + [0, None]
    assert L.kcdc_zstd_decode_chunks_device(b"no-such-compressor", *args) == _lib.KCDC_ENOENT
    assert L.kcdc_zstd_decode_chunks_device(None, *args) == _lib.KCDC_ENOENT
    for name in ("s2-default", "s2-parallel-8", "gzip", "deflate-default", "pgzip-best-speed"):
        assert L.kcdc_zstd_decode_chunks_device(name.encode(), *args) == _lib.KCDC_EINVAL
        assert name in _lib.last_error()
    if L.kcdc_device_count() == 0:
        for name in zv.FOUR:
            assert L.kcdc_zstd_decode_chunks_device(name.encode(), *args) == _lib.KCDC_ENODEV


def test_workspace_size_follows_the_rule():
    """Monotone in the cap total and the count; the compressed total does not enter; per cap byte: a
    literal byte, a third of a 12-byte sequence record and 1/1024 of a 32-byte descriptor; per
    content: a record, 4 descriptors and 36 bytes of bookkeeping."""
    ws = _lib.lib().kcdc_zstd_decode_workspace_size
    assert ws.argtypes == [_lib.C.c_uint64, _lib.C.c_uint64, _lib.C.c_uint32]
    caps = [0, 1, 2, 3, 1023, 1024, 3072, 1 << 20, (1 << 32) - 1, 1 << 40]
    for n in (1, 2, 64, 5000):
        sizes = [ws(0, c, n) for c in caps]
        assert sizes == sorted(sizes), n
        assert len({ws(k, 1 << 20, n) for k in (0, 1, 1 << 30)}) == 1
    counts = [ws(0, 1 << 20, n) for n in (0, 1, 2, 3, 64, 4096, 5000, 1 << 20)]
    assert counts == sorted(counts) and len(set(counts)) == len(counts)
    assert ws(0, 3072, 1) - ws(0, 0, 1) == 3072 + 12 * 1024 + 32 * 3
    assert ws(0, 3 << 20, 7) - ws(0, 0, 7) == (3 << 20) + 12 * (1 << 20) + 32 * 3072
    # per content: 12 + 4 * 32 + 5 arrays of 8 or 4 bytes, between the 256-byte steps of those arrays
    assert ws(0, 0, 5000) - ws(0, 0, 4936) == 64 * (12 + 128 + 36)
    assert ws(0, 0, 0) >= 8


# ------------------------------------------------------------------ the code objects
@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel: {field: int}} from the code object metadata of kcdc_zstd.hip for gfx950."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("zstd_asm") / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "kopia_amd", "csrc", "kcdc_zstd.hip"), "-o", str(out)], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return kernels


def test_zstd_kernels_do_not_spill(metadata):
    names = sorted(metadata)
    assert len(names) == 7 and all("zsdev" in n for n in names), names
    for what in ("zstd_scan_kernel", "zstd_index_kernel", "zstd_entropy_kernel", "zstd_execute_kernel", "zstd_checksum_kernel",
                 "zstd_final_kernel"):
        assert any(what in n for n in names), what
    for n, m in metadata.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)


def test_entropy_kernel_lds_allows_the_claimed_waves(metadata):
    """16 single-wave workgroups of the entropy kernel per CU (its tables, build scratch and held
    arguments), and far more of the execute kernel (a batch plan)."""
    for n, m in metadata.items():
        lds = m["group_segment_fixed_size"]
        if "zstd_entropy_kernel" in n:
            assert 0 < lds * WAVES_PER_CU <= LDS_PER_CU, (n, lds)
        elif "zstd_execute_kernel" in n:
            assert 0 < lds * WAVES_PER_CU * 2 <= LDS_PER_CU, (n, lds)
        elif "zstd_scan_kernel" in n:
            assert 0 < lds <= 32 << 10, (n, lds)
        else:
            assert lds == 0, (n, lds)
