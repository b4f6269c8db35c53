"""bench.py's own multi-process launcher (`--gpus N` without torchrun): N spawned rank
processes, gloo barrier / max / gather (no RCCL), whole-job aggregation.  CPU only: the
ranks report made-up timings through bench.launcher_selftest."""
import json

import numpy as np

import bench


def test_aggregate_weak_scaling():
    per = [{"bytes_per_step": 1 << 30, "elapsed_s": 2.0, "own_s": 1.0},
           {"bytes_per_step": 1 << 30, "elapsed_s": 4.0, "own_s": 2.0}]
    a = bench.aggregate(per, 4)
    assert a["value"] == 2.0  # 8 GiB over the slowest rank's 4 s
    assert a["ms_per_step"] == 1000.0
    assert a["per_gpu_gib_s"] == [4.0, 2.0]


def test_spawn_gloo_world2(tmp_path):
    out = tmp_path / "agg.json"
    bench.spawn_ranks(2, [str(out)], entry="launcher_selftest")
    d = json.loads(out.read_text())
    assert d["world"] == 2
    assert d["max"] == 1.0
    # (1 + 2) GiB per step x 2 steps over max elapsed 2 s
    assert d["agg"]["value"] == 3.0
    assert d["agg"]["per_gpu_gib_s"] == [4.0, round(2 * 2 / 1.5, 3)]


def test_parse_config4_shape():
    a = bench.parse(["--config", "4", "--gpus", "8"])
    assert (a.streams, a.stream_mib, a.gpus) == (8192, 8, 8)


def test_parse_plain_and_full():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs(tmp_path, monkeypatch):
    cuts = [np.array([5, 9, 1 << 40], dtype=np.int64), np.zeros(0, np.int64), np.array([3], dtype=np.int64)]
    bench.dump_outputs(str(tmp_path / "a"), cuts)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("streams", "counts", "cuts")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["streams"].tolist() == [0, 1, 2] and got["counts"].tolist() == [3, 0, 1]
    assert got["cuts"].tolist() == [5, 9, 1 << 40, 3]
    # over the limit: the same sample of whole streams every time, within the limit; ranks share it
    monkeypatch.setattr(bench, "DUMP_LIMIT", 8 * (64 + 40))
    many = [np.arange(1, 4, dtype=np.int64) * (i + 1) for i in range(20)]  # 5 entries a stream with its index and count
    for d, world, k in (("b", 1, 8), ("c", 1, 8), ("r", 2, 0)):
        bench.dump_outputs(str(tmp_path / d), many, rank=world - 1, world=world)
        tag = ".rank1" if world > 1 else ""
        s, c, v = (np.load(tmp_path / d / f"{n}{tag}.npy") for n in ("streams", "counts", "cuts"))
        assert s.size == k and np.all(np.diff(s) > 0) and c.tolist() == [3] * k
        assert v.tolist() == [x for i in s for x in many[int(i)].tolist()]
    assert np.array_equal(np.load(tmp_path / "b" / "streams.npy"), np.load(tmp_path / "c" / "streams.npy"))


def test_host_cpu_info():
    info = bench.host_cpu_info()
    assert info["logical_cores"] >= 1 and 1 <= info["threads_all"] <= info["logical_cores"]
