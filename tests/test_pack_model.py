"""CPU: the pack plan's decisions (kopia_amd/csrc/kcdc_pack_format.h, run by the stand-alone
build/pack_plan_host under the host sanitizers) against the literal loop of addToPackUnlocked in
tests/pack_model.py, on the placement seams, the masks, the refusals, the ECC thresholds and 200
seeded random vectors; kcdc_pack_bounds against what the model needs; the refusals the library makes
before it touches a device; and a check that the GPU tests' own inputs reach every alignment."""
import ctypes as C
import os
import re
import subprocess

import pytest

import pack_cases as pc
import pack_model as pm
from conftest import ROOT
from kopia_amd import _lib

HOST = os.path.join(ROOT, "build", "pack_plan_host")
NO_CAP = (1 << 63) - 1
ENC = b"CHACHA20-POLY1305-HMAC-SHA256"


def vector_text(vecs) -> str:
    out = ["PACKVEC1", str(len(vecs))]
    for v in vecs:
        e = pc.ecc_of(v.ecc)
        info = e.info() if e else (0,) * 7
        out.append(" ".join(str(int(x)) for x in (
            v.max_pack_size, v.lead, v.open_fill, (1 << 40) if v.max_total is None else v.max_total,
            NO_CAP if v.pack_cap is None else v.pack_cap, 0xFFFFFFFF if v.packs_cap is None else v.packs_cap,
            v.header_id, 1 if e else 0, *info, len(v.lengths))))
        keep = v.keep or [1] * len(v.lengths)
        comp = v.comp_lens or [0] * len(v.lengths)
        out.extend(f"{int(n)} {int(k)} {int(c)}" for n, k, c in zip(v.lengths, keep, comp))
    return "\n".join(out) + "\n"


def run_host(vecs, tmp_path):
    """[(header dict, entries, packs)] of the host program over these vectors; any sanitizer report
    (a non-zero exit, or anything on stderr) fails."""
    assert os.path.exists(HOST), "build/pack_plan_host is not built (make all)"
    path = tmp_path / "vectors.txt"
    path.write_text(vector_text(vecs))
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    p = subprocess.run([HOST, str(path)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    res = []
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "v":
            res.append((dict(zip(f[2::2], map(int, f[3::2]))), [], []))
        elif f[0] == "e":
            res[-1][1].append(tuple(int(x) for x in f[1:]))
        else:
            res[-1][2].append(tuple(int(x) for x in f[1:]))
    assert len(res) == len(vecs)
    return res


def check(vecs, tmp_path):
    for v, (hdr, entries, packs) in zip(vecs, run_host(vecs, tmp_path)):
        want = v.model()
        assert entries == want.entries, v.tag
        assert packs == want.packs, v.tag
        assert (hdr["packs"], hdr["bytes"]) == want.totals, v.tag
    # the header's bounds, from a true bound on the total, cover what the model needs
    free = [pc.Vec(**{**v.__dict__, "max_total": v.true_total()}) for v in vecs
            if v.max_total is None and v.pack_cap is None and v.packs_cap is None]
    for v, (b, _, _) in zip(free, run_host(free, tmp_path)):
        want = v.model()
        assert b["bound_stored"] >= want.stored_total, v.tag
        assert b["bound_packs"] >= want.totals[0], v.tag
        assert b["bound_bytes"] >= want.totals[1], v.tag


def test_seams(tmp_path):
    vecs = pc.seam_vectors()
    check(vecs, tmp_path)
    by = {v.tag: v.model() for v in vecs}
    # the shapes are what they are named after
    assert [p[3] for p in by["exact64-lead0-fill0"].packs] == [64, 64, 64, 8]
    assert [p[3] for p in by["exact128-lead0-fill0"].packs] == [128, 128, 44]
    assert by["short1-lead0-fill0"].packs[0][1:] == (4095 + 64, 0, 65)
    assert by["large-lead0-fill0"].packs[0][1] > 4096
    assert by["many-lead0-fill0"].totals[0] == 100 > 64
    assert by["closed-lead0-fill0"].packs[-1][1] == 4096 and by["open-lead0-fill0"].packs[-1][1] == 64
    assert by["exact64-lead0-fill4032"].packs[0][3] == 1  # the first content closes the continued pack
    assert by["exact64-lead37-fill4095"].entries[0][1] == 4095


def test_masks_refusals_ecc(tmp_path):
    vecs = pc.mask_vectors() + pc.refusal_vectors() + pc.ecc_vectors()
    check(vecs, tmp_path)
    by = {v.tag: v.model() for v in vecs}
    assert by["all-skipped"].totals == (0, 0) and {e[5] for e in by["all-skipped"].entries} == {pm.SKIPPED}
    assert {e[5] for e in by["enomem"].entries} == {pm.ENOMEM} and by["total-exact"].totals[0] > 0
    assert {e[5] for e in by["pack-cap-short"].entries} == {pm.EOVERFLOW} == {e[5] for e in by["packs-cap-short"].entries}
    assert by["pack-cap-exact"].totals[0] > 0 and by["packs-cap-exact"].totals[0] > 0
    assert [e[5] for e in by["efbig"].entries] == [0, pm.EFBIG, 0, 0]


def test_random_vectors(tmp_path):
    vecs = pc.random_vectors()
    assert len(vecs) == 200
    check(vecs, tmp_path)
    kinds = {e[5] for v in vecs for e in v.model().entries}
    assert kinds >= {pm.PACKED, pm.SKIPPED, pm.EFBIG, pm.ENOMEM, pm.EOVERFLOW}


def params(v, max_total, compression=None, encryption=ENC, secret=b"k" * 32):
    return _lib.PackParams(compression, encryption, secret, len(secret) if secret else 0,
                           b"REED-SOLOMON-CRC32" if v.ecc else None, v.ecc[0] if v.ecc else 0, v.ecc[1] if v.ecc else 0,
                           v.max_pack_size, v.lead, v.open_fill, max_total)


def bounds(p, n):
    pb, mp, wb = C.c_uint64(), C.c_uint32(), C.c_uint64()
    rc = _lib.lib().kcdc_pack_bounds(C.byref(p), n, C.byref(pb), C.byref(mp), C.byref(wb))
    return rc, pb.value, mp.value, wb.value


def test_library_bounds_cover_the_model():
    for v in pc.all_vectors():
        if v.max_total is not None or v.pack_cap is not None or v.packs_cap is not None:
            continue
        want = v.model()
        rc, pb, mp, wb = bounds(params(v, v.true_total(), b"zstd" if v.comp_lens else None), len(v.lengths))
        assert rc == 0, v.tag
        assert pb >= want.totals[1] and mp >= want.totals[0], v.tag
        assert wb >= 8 * len(v.lengths), v.tag


def test_refusals_before_any_device():
    L = _lib.lib()
    v = pc.Vec([10], 4096)
    ok = params(v, 10)
    assert bounds(ok, 1)[0] == 0
    assert bounds(params(v, 10, compression=b"nosuch"), 1)[0] == _lib.KCDC_ENOENT
    assert bounds(params(v, 10, encryption=b"nosuch"), 1)[0] == _lib.KCDC_ENOENT
    assert bounds(params(v, 10, encryption=None), 1)[0] == _lib.KCDC_ENOENT
    bad_ecc = params(v, 10)
    bad_ecc.ecc = b"nosuch"
    assert bounds(bad_ecc, 1)[0] == _lib.KCDC_ENOENT
    bad_ecc.ecc, bad_ecc.ecc_overhead_percent = b"REED-SOLOMON-CRC32", 0
    assert bounds(bad_ecc, 1)[0] == _lib.KCDC_EINVAL
    assert bounds(params(v, 10, secret=b""), 1)[0] == _lib.KCDC_EINVAL
    assert bounds(params(v, 10, secret=b"k" * 65), 1)[0] == _lib.KCDC_EINVAL
    assert bounds(params(pc.Vec([10], 0), 10), 1)[0] == _lib.KCDC_EINVAL
    assert bounds(params(pc.Vec([10], (1 << 30) + 1), 10), 1)[0] == _lib.KCDC_EINVAL
    assert bounds(params(pc.Vec([10], 1 << 30), 10), 1)[0] == 0
    assert bounds(params(pc.Vec([10], 4096, open_fill=4096), 10), 1)[0] == _lib.KCDC_EINVAL
    assert bounds(params(v, (1 << 40) + 1), 1)[0] == _lib.KCDC_EINVAL
    assert L.kcdc_pack_bounds(None, 1, None, None, None) == _lib.KCDC_EINVAL
    # the chunk call: argument checks come before the device is looked at
    _, pb, mp, wb = bounds(ok, 1)
    P = C.c_void_p
    fake = P(1 << 20)  # never dereferenced: every call below is refused on the host

    def call(p=ok, data=fake, totals=fake, work=fake, work_bytes=wb, id_len=16, id_stride=16, n=1):
        return L.kcdc_pack_chunks_device(C.byref(p), data, fake, fake, None, n, fake, id_len, id_stride, fake, fake, pb,
                                         fake, fake, mp, totals, work, work_bytes, None)

    assert call(data=None) == _lib.KCDC_EINVAL
    assert call(totals=None) == _lib.KCDC_EINVAL
    assert call(work=None) == _lib.KCDC_EINVAL
    assert call(work=P((1 << 20) + 4)) == _lib.KCDC_EINVAL
    assert call(work_bytes=wb - 1) == _lib.KCDC_EINVAL
    assert call(id_len=0) == _lib.KCDC_EINVAL and call(id_len=65) == _lib.KCDC_EINVAL
    assert call(id_len=16, id_stride=8, n=2, work_bytes=1 << 40) == _lib.KCDC_EINVAL
    assert call(p=params(v, 10, encryption=b"nosuch")) == _lib.KCDC_ENOENT


def test_gpu_inputs_reach_every_alignment():
    """The byte-exact GPU case: the model's pack offsets cover all 16 residues mod 16 (the gather's
    destinations), and so do the source offsets."""
    _, offs = pc.sources(pc.EXACT_LENS)
    assert {int(o) % 16 for o in offs} == set(range(16))
    for mps in pc.EXACT_PACK_SIZES:
        r = pc.Vec(pc.EXACT_LENS, mps, lead=37).model()
        assert {(r.packs[e[0]][0] + e[1]) % 16 for e in r.entries} == set(range(16)), mps
    assert len(pc.Vec(pc.EXACT_LENS, 4096, lead=37).model().packs) > 3


# ------------------------------------------------------------------ the code objects
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def pack_asm(tmp_path_factory):
    """The gfx950 assembly of kcdc_pack.hip."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("pack_asm") / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "kopia_amd", "csrc", "kcdc_pack.hip"), "-o", str(out)], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def test_pack_kernels_do_not_spill(pack_asm):
    meta = pack_asm[pack_asm.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    for what in ("init_kernel", "plan0_lens_kernel", "plan0_slots_kernel", "scan_kernel", "plan1_sizes_kernel",
                 "plan1_chain_kernel", "plan1_entries_kernel", "gather_kernel"):
        assert any(what in n for n in kernels), what
    assert len(kernels) == 8 and all("packdev" in n for n in kernels), sorted(kernels)
    for n, m in kernels.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)


def test_gather_moves_16_bytes_per_store(pack_asm):
    """The gather's body: 16-byte loads from 4-byte aligned sources and 16-byte stores; the only
    narrower stores are the byte stores of a part's head and tail."""
    start = pack_asm.index("gather_kernel")
    body = pack_asm[start:pack_asm.index("s_endpgm", start)]
    stores = set(re.findall(r"\b(?:global|flat)_store_(\w+)", body))
    assert stores == {"dwordx4", "byte"}, stores
    assert re.search(r"\b(?:global|flat)_load_dwordx4\b", body)
