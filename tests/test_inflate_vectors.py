"""CPU: the vectors of tests/inflate_vectors.py keep their conditions (zlib is the judge of every
expectation), the inflate decoder's validity header decodes or refuses each of them on the host
under AddressSanitizer and UBSan (tools/inflate_host.cpp through
kopia_amd/csrc/kcdc_inflate_format.h) before any reaches a GPU, the kcdc_inflate_* entry points are
declared and answer their argument errors without a device, and the inflate kernels' code objects
hold what DESIGN.md 2.7c says of them."""
import os
import re
import subprocess

import pytest

import inflate_vectors as iv
from kopia_amd import _lib
from kopia_amd import compression as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 << 10   # gfx950
WAVES_PER_CU = 16        # the inflate grid is 16 waves for each CU


# ------------------------------------------------------------------ the vectors' conditions
def test_expected_bytes_come_from_zlib():
    for v in iv.valid_vectors():
        got, clean = iv.zlib_decode(v.name, v.blob)
        assert clean and got == v.expected and v.status == 0 and v.cap >= len(v.expected), v.id
        assert len(v.expected) <= iv.MAX_DECODED, v.id


def test_zlib_refuses_every_corrupt_vector():
    """But the cap ones and the header-ID ones: those are this library's rules, not the format's."""
    seen = set()
    for v in iv.corrupt_vectors():
        assert v.expected == b"" and v.status in (iv.EBADMSG, iv.EOVERFLOW), v.id
        if v.status == iv.EOVERFLOW:
            got, clean = iv.zlib_decode(v.name, v.blob)
            assert clean and len(got) > v.cap, v.id
        elif v.id.startswith("wrong-header-id"):
            assert v.blob[:4] != iv.deflate.header(v.name)
        else:
            assert not iv.zlib_decode(v.name, v.blob)[1], v.id
        seen.add(v.status)
    assert seen == {iv.EBADMSG, iv.EOVERFLOW}


def test_model_agrees_on_the_built_vectors():
    """The model of the contract (header ID, members, trailers, cap over tests/deflate_model.py's
    inflate) gives every hand-built vector its status and bytes; no expectation rests on it alone."""
    for v in iv.built_valid_vectors() + iv.corrupt_vectors():
        assert iv.model(v.name, v.blob, v.cap) == (v.status, v.expected), v.id


def test_vector_set_covers_the_list():
    ids = {v.id for v in iv.all_vectors()}
    for name in iv.FAMILIES:
        for size in iv.SIZES:
            for kind in ("level0", "level1", "level6", "level9", "fixed", "huffman-only", "rle", "memlevel1", "flushes",
                         "random", "zeros"):
                assert f"zlib-{name}-{kind}-{size}" in ids
    want = {"match-lengths-3-10-11-257-258", "distance-1-length-258", "distance-63-lengths-either-side",
            "distance-64-lengths-either-side", "distance-65-lengths-either-side", "distance-32768-from-byte-32768",
            "distance-equal-to-produced", "fixed-match-into-stored-and-dynamic", "dynamic-15-bit-code",
            "dynamic-single-one-bit-distance-code", "dynamic-no-distance-code", "length-run-16-crosses-into-distances",
            "length-runs-17-18-cross-into-distances", "empty-final-stored-block", "65-literals-then-a-match", "stored-block-65535",
            "gzip-fextra-fname-fcomment-fhcrc", "gzip-two-members", "gzip-empty-member", "raw-stream-then-5-junk-bytes",
            "hlit-287", "hdist-31", "over-subscribed-lengths", "incomplete-lengths", "code-16-with-no-previous-length",
            "literal-length-symbol-286", "literal-length-symbol-287", "distance-symbol-30", "distance-symbol-31",
            "len-not-complement-of-nlen", "btype-3", "distance-beyond-produced", "truncated-before-the-end-of-block",
            "truncated-inside-the-id", "truncated-inside-the-block-header", "truncated-inside-hclen-lengths",
            "truncated-inside-a-symbol", "truncated-inside-extra-bits", "truncated-inside-a-stored-block",
            "truncated-inside-the-gzip-header", "truncated-inside-the-trailer", "wrong-header-id",
            "gzip-member-under-a-deflate-name", "raw-stream-under-a-gzip-name", "gzip-bad-magic", "gzip-cm-7",
            "gzip-bad-fhcrc", "gzip-crc32-off-by-one-bit", "gzip-isize-off-by-one", "gzip-junk-after-the-trailer",
            "cap-reached-by-a-literal", "cap-reached-by-a-match", "cap-reached-by-a-stored-block",
            "truncated-inside-the-block-header-1-bit", "literal-run-100-fixed", "literal-run-100-sub-table-codes"}
    want |= {f"cap-reached-by-literal-{k}-of-a-run-{w}" for k in (3, 6, 65, 100) for w in ("fixed", "sub-table-codes")}
    want |= {f"stored-block-at-bit-phase-{p}" for p in range(8)}
    assert want <= ids, sorted(want - ids)


def test_zlib_streams_hold_every_block_type():
    """The foreign streams are what their names say: stored blocks split at 65,535, fixed-only,
    literal-only and many-block streams (read back by tests/deflate_model.py's inflate)."""
    by = {v.id: v for v in iv.foreign_vectors()}
    size = iv.SIZES[3]
    blocks = lambda kind: iv.dm.inflate_blocks(by[f"zlib-{iv.RAW}-{kind}-{size}"].blob[4:])[1]  # noqa: E731
    lv0 = blocks("level0")
    # zlib fills a stored block to its pending buffer: 65,535 bytes less a few; the hand-built
    # stored-block-65535 holds the format's maximum itself
    assert {b.btype for b in lv0} == {0} and 65000 < lv0[0].stored_len <= 65535 and len(lv0) == 2
    assert {b.btype for b in blocks("fixed")} == {1}
    assert not any(b.matches for b in blocks("huffman-only"))
    assert all(m[1] == 1 for b in blocks("rle") for m in b.matches) and any(b.matches for b in blocks("rle"))
    assert len(blocks("memlevel1")) > 4 * len(blocks("level6")) and {b.btype for b in blocks("level6")} >= {2}
    assert sum(1 for b in blocks("flushes") if b.btype == 0 and b.stored_len == 0) >= 2


# ------------------------------------------------------------------ the host program
def test_host_program_decodes_every_valid_vector():
    res = iv.run_host_program()
    for v in iv.valid_vectors():
        assert res[v.id] == (0, len(v.expected), True), v.id


def test_host_program_refuses_every_corrupt_vector():
    res = iv.run_host_program()
    for v in iv.corrupt_vectors():
        assert res[v.id] == (v.status, 0, True), v.id


# ------------------------------------------------------------------ the entry points
def test_inflate_symbols_declared():
    syms = _lib.exported_symbols()
    for s in ("kcdc_inflate_algorithms", "kcdc_inflate_workspace_size", "kcdc_inflate_chunks_device"):
        assert s in syms and hasattr(_lib.lib(), s), s
    from test_lib_host import header_symbols
    assert {"kcdc_inflate_algorithms", "kcdc_inflate_workspace_size", "kcdc_inflate_chunks_device"} <= set(header_symbols())
    assert kc.InflatableAlgorithms() == iv.NINE
    assert not set(kc.InflatableAlgorithms()) & set(kc.DecompressibleAlgorithms())
    assert set(kc.InflatableAlgorithms()) <= set(kc.SupportedAlgorithms())


def test_argument_errors_need_no_device():
    L = _lib.lib()
    args = [None] * 3 + [0] + [None] * 6 + [0, None]
    assert L.kcdc_inflate_chunks_device(b"no-such-compressor", *args) == _lib.KCDC_ENOENT
    assert L.kcdc_inflate_chunks_device(None, *args) == _lib.KCDC_ENOENT
    for name in ("s2-default", "s2-parallel-8", "zstd", "zstd-fastest"):
        assert L.kcdc_inflate_chunks_device(name.encode(), *args) == _lib.KCDC_EINVAL
        assert name in _lib.last_error()
    if L.kcdc_device_count() == 0:
        for name in iv.NINE:
            assert L.kcdc_inflate_chunks_device(name.encode(), *args) == _lib.KCDC_ENODEV


def test_workspace_size_depends_on_the_count_alone():
    ws = _lib.lib().kcdc_inflate_workspace_size
    sizes = [ws(n) for n in (0, 1, 2, 3, 64, 4096, 5000, 1 << 20, (1 << 32) - 1)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(2) - ws(1) == ws(5000) - ws(4999) == 32 and ws(0) >= 8
    assert ws.argtypes == [_lib.C.c_uint32]  # nothing else to depend on


# ------------------------------------------------------------------ the code objects
@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel: {field: int}} from the code object metadata of kcdc_inflate.hip for gfx950."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("inflate_asm") / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "kopia_amd", "csrc", "kcdc_inflate.hip"), "-o", str(out)], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return kernels


def test_inflate_kernels_do_not_spill(metadata):
    names = sorted(metadata)
    assert len(names) == 4 and all("infdev" in n for n in names), names
    for what in ("inflate_init_kernel", "inflate_kernel", "inflate_crc_kernel", "inflate_final_kernel"):
        assert any(what in n for n in names), what
    for n, m in metadata.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)


def test_inflate_kernel_lds_allows_the_claimed_waves(metadata):
    """16 single-wave workgroups of the inflate kernel per CU; the CRC kernel's byte table (32
    copies, 32 KiB) leaves its four-wave workgroups four to a CU, 16 waves again."""
    for n, m in metadata.items():
        lds = m["group_segment_fixed_size"]
        if "inflate_kernel" in n:
            assert 0 < lds * WAVES_PER_CU <= LDS_PER_CU, (n, lds)
        elif "inflate_crc_kernel" in n:
            assert 0 < lds * (WAVES_PER_CU // 4) <= LDS_PER_CU, (n, lds)
        else:
            assert lds == 0, (n, lds)
