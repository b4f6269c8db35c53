"""CPU: the content-ID set's decisions (kopia_amd/csrc/kcdc_dedup_format.h, run sequentially by the
stand-alone build/dedup_host under the host sanitizers, every table of its exact size) against the
literal loop of tests/dedup_model.py, on the vectors the GPU tests use and on seeded random call
sequences; kcdc_dedup_bytes, the home slot and the refusals the library makes before it touches a
device; and the kernels' code objects."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dedup_cases as dc
import dedup_model as dm
from conftest import ROOT
from kopia_amd import _lib

HOST = os.path.join(ROOT, "build", "dedup_host")


def lib_home(id_len, max_keys, prefix, one):
    return _lib.lib().kcdc_test_dedup_home(id_len, max_keys, prefix, one)


def vector_text(vecs, homes) -> str:
    out = ["DEDUPVEC1", str(len(vecs))]
    for v in vecs:
        mine = homes.get(v.tag, [])
        out.append(f"{v.id_len} {v.max_keys} {len(v.calls) + len(mine)}")
        out.extend(f"home {prefix} {one.hex()}" for prefix, one in mine)
        for c in v.calls:
            if c.op == "clear":
                out.append("clear")
            elif c.op == "grow":
                out.append(f"grow {c.max_keys}")
            else:
                out.append(f"{c.op} {c.prefix} {c.stride or v.id_len} {c.offset} {len(c.ids)} "
                           f"{dc.buffer_of(c, v.id_len).tobytes().hex() or '-'}")
    return "\n".join(out) + "\n"


def run_host(vecs, homes=None):
    """Per vector ({bytes, slots}, [home slots], results in dedup_model.run's form) of the host
    program, fed through stdin; any sanitizer report (a non-zero exit, or anything on stderr) fails."""
    assert os.path.exists(HOST), "build/dedup_host is not built (make all)"
    homes = homes or {}
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    p = subprocess.run([HOST], input=vector_text(vecs, homes), capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines()]
    at, out = 0, []

    def take(kind, count):
        nonlocal at
        rows = lines[at:at + count]
        assert len(rows) == count and all(r[0] == kind for r in rows), (kind, count, rows[:3])
        at += count
        return [[int(x) for x in r[1:]] for r in rows]

    for v in vecs:
        assert lines[at][0] == "v"
        hdr = dict(zip(lines[at][2::2], map(int, lines[at][3::2])))
        at += 1
        slots = [r[0] for r in take("h", len(homes.get(v.tag, [])))]
        res = []
        for c in v.calls:
            if c.op == "lookup":
                res.append(("l", [r[0] for r in take("l", len(c.ids))]))
            elif c.op == "clear":
                take("c", 1)
                res.append(("c",))
            else:
                t = tuple(take("t", 1)[0])
                if c.op == "claim":
                    rows = take("k", len(c.ids))
                    res.append(("t", *t, [r[0] for r in rows], [r[1] for r in rows]))
                else:
                    res.append(("t", *t))
        out.append((hdr, slots, res))
    assert at == len(lines)
    return out


@pytest.fixture(scope="module")
def vectors():
    return dc.small_vectors(lib_home)


def test_host_program_matches_the_model(vectors):
    for v, (_, _, got) in zip(vectors, run_host(vectors)):
        assert got == dm.run(v), v.tag


def test_the_cases_are_what_they_are_named_after(vectors):
    by = {v.tag: dm.run(v) for v in vectors}
    for n in (64, 200):  # only index 0 is kept, first is 0 for all
        assert by[f"copies{n}"][0][1:] == (0, 1, 1, [1] + [0] * (n - 1), [0] * n)
    _, status, new, stored, keep, first = by["shuffled"][0]
    ids = dm.id_list(dc.shuffled_ids())
    lowest = {}
    for i, one in enumerate(ids):
        lowest.setdefault(one, i)
    assert (status, new, stored, sum(keep)) == (0, 512, 512, 512) and len(ids) == 4096
    assert first == [lowest[one] for one in ids] and [i for i, k in enumerate(keep) if k] == sorted(lowest.values())
    second, third = by["repeat"][1], by["repeat"][2]
    assert second[5].count(dm.KNOWN) == 150 and sum(second[4]) == 150
    assert sum(third[4]) == 0 and set(third[5]) == {dm.KNOWN}
    for tag in ("twins-len32", "twins-len28"):
        r = by[tag]
        n = len(r[0][4]) // 2
        assert r[0][4] == [1] * n + [0] * n and r[0][5] == list(range(n)) * 2  # twins are distinct, copies equal
        assert sum(r[1][4]) == n and sum(r[2][4]) == n and sum(r[3][4]) == 0  # prefixes tell keys apart
        assert r[4][1] == [0] * n and r[6][1] == [1] * n and r[7][1] == [0] * n
    full = by["full"]
    assert [c[1] for c in full if c[0] == "t"] == [0, 0, dm.ENOSPC, dm.ENOSPC, dm.ENOSPC, 0, 0]
    assert full[2][3] == 1000 and full[3][1] == [1] * 1000 and full[6][1] == [1, 0]
    assert full[8][1:4] == (0, 1, 1001) and full[9][1] == [1] * 1001
    look = by["lookup"]
    assert look[1] == look[2] and look[3][5][:100] == [dm.KNOWN] * 100 and sum(look[3][4]) == 200
    clear = by["clear"]
    assert clear[2][1] == [0] * 500 and clear[3][2] == 400 and sum(clear[4][4]) == 100


def test_one_home_chain_wraps(vectors):
    """Case 6's IDs share one home within the table's last 8 slots, by the library and by the host
    program alike; 300 of them fill the slots to the end and go on from slot 0."""
    ids, slot = dc.one_home_ids(lib_home)
    slots = dc.slot_count(512)
    assert len(ids) == 300 and len(set(dm.id_list(ids))) == 300 and slots - 8 <= slot < slots
    v = next(v for v in vectors if v.tag == "one-home")
    hdr, homes, _ = run_host([v], {v.tag: [(0, one) for one in dm.id_list(ids)]})[0]
    assert hdr["slots"] == slots and homes == [slot] * 300
    # other prefixes and shapes agree too
    rng = np.random.default_rng(11)
    for id_len, max_keys in ((16, 1), (28, 1000), (32, 5000)):
        keys = [(int(p), one) for p, one in zip(rng.integers(0, 256, 50), dm.id_list(dc.rand_ids(rng, 50, id_len)))]
        got = run_host([dc.Vec("homes", id_len, max_keys)], {"homes": keys})[0][1]
        assert got == [lib_home(id_len, max_keys, p, one) for p, one in keys] and len(set(got)) > 1


def random_vectors(count=60):
    vecs = []
    for k in range(count):
        rng = np.random.default_rng(1000 + k)
        id_len = int(rng.choice([16, 17, 20, 28, 31, 32]))
        max_keys = int(rng.choice([1, 7, 64, 300]))
        pool = dc.rand_ids(rng, int(rng.integers(1, 2 * max_keys + 2)), id_len)
        if k % 3 == 0:
            pool[:, :16] = pool[0, :16]  # one home and one fingerprint for all
        v = dc.Vec(f"random{k}", id_len, max_keys)
        for _ in range(int(rng.integers(1, 9))):
            op = str(rng.choice(["claim", "claim", "claim", "insert", "lookup", "clear", "grow"]))
            if op == "grow":
                v.calls.append(dc.Call("grow", max_keys=int(rng.choice([1, 7, 64, 300, 700]))))
                continue
            if op == "clear":
                v.calls.append(dc.Call("clear"))
                continue
            n = int(rng.integers(0, max_keys + 3))
            stride = id_len + int(rng.integers(0, 9))
            v.calls.append(dc.Call(op, pool[rng.integers(0, len(pool), n)], prefix=int(rng.choice([0, 0, 107, 120])),
                                   stride=stride, offset=int(rng.integers(0, 5))))
        vecs.append(v)
    return vecs


def test_random_call_sequences():
    vecs = random_vectors()
    statuses = set()
    for v, (_, _, got) in zip(vecs, run_host(vecs)):
        want = dm.run(v)
        assert got == want, v.tag
        statuses |= {c[1] for c in want if c[0] == "t"}
    assert statuses == {0, dm.ENOSPC}


def test_dedup_bytes_and_host_refusals():
    L = _lib.lib()
    host = run_host([dc.Vec("a", 16, 1000), dc.Vec("b", 32, 1), dc.Vec("c", 28, 4097)])
    for (id_len, max_keys), (hdr, _, _) in zip(((16, 1000), (32, 1), (28, 4097)), host):
        b = L.kcdc_dedup_bytes(id_len, max_keys)
        assert b == hdr["bytes"] and b % 256 == 0
        stride = (id_len + 1 + 3) // 4 * 4
        assert b >= 8 * hdr["slots"] + stride * max_keys + 8 * max_keys and hdr["slots"] >= 2 * max_keys
    assert L.kcdc_dedup_bytes(16, 1 << 31) > (1 << 32) * 8
    for id_len, max_keys in ((15, 10), (33, 10), (0, 10), (16, 0), (16, (1 << 31) + 1)):
        assert L.kcdc_dedup_bytes(id_len, max_keys) == 0 and "id_len" in _lib.last_error()
        assert not L.kcdc_dedup_new(0, id_len, max_keys) and "id_len" in _lib.last_error()
        assert L.kcdc_test_dedup_home(id_len, max_keys, 0, bytes(32)) == (1 << 64) - 1
    assert L.kcdc_test_dedup_home(16, 10, 0, None) == (1 << 64) - 1
    # null arguments are refused before any device is looked at
    fake = C.c_void_p(1 << 20)  # never dereferenced
    assert L.kcdc_dedup_claim_device(None, 0, fake, 16, 1, fake, fake, fake, None) == _lib.KCDC_EINVAL
    assert L.kcdc_dedup_insert_device(None, 0, fake, 16, 1, fake, None) == _lib.KCDC_EINVAL
    assert L.kcdc_dedup_lookup_device(None, 0, fake, 16, 1, fake, None) == _lib.KCDC_EINVAL
    assert L.kcdc_dedup_grow_device(None, None, fake, None) == _lib.KCDC_EINVAL
    assert L.kcdc_dedup_clear_device(None, None) == _lib.KCDC_EINVAL
    assert L.kcdc_dedup_count(None, None) == _lib.KCDC_EINVAL
    L.kcdc_dedup_free(None)


def test_device_entry_points_fail_loudly_without_device():
    if _lib.lib().kcdc_device_count() > 0:
        pytest.skip("a gfx950 device is present")
    from kopia_amd import dedup
    L = _lib.lib()
    assert not L.kcdc_dedup_new(0, 16, 1000)
    assert "device" in _lib.last_error().lower()
    with pytest.raises(_lib.KcdcError):
        dedup.ContentSet("cuda:0", 16, 1000)
    # no set can exist, so every *_device call is refused for its null set: none runs on the CPU instead
    fake = C.c_void_p(1 << 20)
    for rc in (L.kcdc_dedup_claim_device(None, 0, fake, 16, 1, fake, None, fake, None),
               L.kcdc_dedup_insert_device(None, 0, fake, 16, 1, fake, None),
               L.kcdc_dedup_lookup_device(None, 0, fake, 16, 1, fake, None),
               L.kcdc_dedup_grow_device(None, None, fake, None), L.kcdc_dedup_clear_device(None, None)):
        assert rc == _lib.KCDC_EINVAL and "null" in _lib.last_error()
    assert dedup.set_bytes(16, 1000) == L.kcdc_dedup_bytes(16, 1000)


# ------------------------------------------------------------------ the code objects
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def dedup_asm(tmp_path_factory):
    """The gfx950 assembly of kcdc_dedup.hip."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("dedup_asm") / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "kopia_amd", "csrc", "kcdc_dedup.hip"), "-o", str(out)], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def test_dedup_kernels_do_not_spill(dedup_asm):
    meta = dedup_asm[dedup_asm.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    for what in ("probe_kernel", "outcome_kernel", "scan_tile_sums_kernel", "scan_sums_kernel", "scan_tiles_kernel",
                 "commit_kernel", "finish_kernel", "lookup_kernel", "clear_kernel"):
        assert any(what in n for n in kernels), what
    assert len(kernels) == 9 and all("dedupdev" in n for n in kernels), sorted(kernels)
    for n, m in kernels.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)


def test_slot_words_are_touched_by_atomics(dedup_asm):
    """The probe takes an empty slot with a 64-bit compare-and-swap and converges duplicates with a
    64-bit unsigned minimum; the lookup kernel has no atomic but its ticket add."""
    def body(kernel):
        start = dedup_asm.index(kernel + "ENS0_4ArgsE:")
        return dedup_asm[start:dedup_asm.index("s_endpgm", start)]

    atomics = lambda text: set(re.findall(r"\bglobal_atomic_(\w+)", text))
    assert atomics(body("probe_kernel")) == {"cmpswap_x2", "umin_x2", "add_x2"}
    assert atomics(body("lookup_kernel")) == {"add_x2"}
    assert atomics(body("commit_kernel")) == {"add_x2"}
