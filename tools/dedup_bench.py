"""Timing of kcdc_dedup_claim_device (kopia_amd.dedup) beside the two things it stands between.
One JSON line per condition, printed and appended to profiles/dedup/dedup_bench.jsonl:
  claim_ms       device time of one claim (between two events, the median of --reps calls, each with
                 IDs it has not seen): batches of 5,705 IDs (the chunks of one config-2 batch) and of
                 2^20 IDs; 0 %, 50 % and 99 % of a batch already in the set (the rest are new and
                 distinct; IDs are uniform random bytes, as hash outputs are); sets preloaded with
                 2^20 and with 2^26 keys
  roundtrip_ms   what the claim replaces, in the same process: synchronise, copy the n digests to
                 pinned host memory, copy an n-byte mask back, synchronise (wall clock, the median).
                 The host's map lookups between the two copies are NOT included: this is the floor
                 of the host path, whatever the map costs.
  hash_ms        kcdc_hash_chunks_device("BLAKE3-256-128") over a batch of as many chunks: the 5,705
                 chunks DYNAMIC-4M-BUZHASH cuts from 4,096 streams of 4 MiB, and the same 16 GiB as
                 2^20 chunks of 16 KiB (device time, tables already on the device)
Not a parity test: tests/test_gpu_dedup.py is.

The driver holds no GPU: every preload size runs in a child process of its own under `timeout`, and
the first child that fails, faults or times out ends the run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "dedup", "dedup_bench.jsonl")
BATCHES = (5705, 1 << 20)
DUP_PERCENT = (0, 50, 99)
ID_LEN = 16
HASH = "BLAKE3-256-128"


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def preload(torch, dev, cs, keys, gen):
    """Insert `keys` random IDs, 2^22 per call; returns the first 2^20 of them (the known pool)."""
    pool, left = None, keys
    while left:
        n = min(left, 1 << 22)
        ids = torch.randint(0, 256, (n, ID_LEN), dtype=torch.uint8, device=dev, generator=gen)
        cs.insert(ids)
        if pool is None:
            pool = ids[:1 << 20].clone()
        left -= n
    torch.cuda.synchronize()
    assert cs.count() == keys, "random 16-byte IDs collided"
    return pool


def claim_times(torch, dev, cs, pool, n, dup, reps, gen):
    """Device ms of `reps` claims of n IDs, dup % of them from the pool of stored keys."""
    known = n * dup // 100
    times, kept = [], None
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    totals = torch.empty(3, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    for r in range(reps + 1):  # the first call warms up
        ids = torch.randint(0, 256, (n, ID_LEN), dtype=torch.uint8, device=dev, generator=gen)
        if known:
            where = torch.randperm(n, device=dev, generator=gen)[:known]
            ids[where] = pool[torch.randint(0, pool.shape[0], (known,), device=dev, generator=gen)]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = cs.claim_raw(ids, ID_LEN, n, keep, first, totals, st)
        e1.record()
        assert rc == 0
        torch.cuda.synchronize()
        t = totals.cpu().tolist()
        assert t[0] == 0 and t[1] == n - known == int(keep.sum().item()), t
        kept = t[1]
        if r:
            times.append(e0.elapsed_time(e1))
    return median(times), kept


def roundtrip_times(torch, dev, n, reps):
    """Wall ms of synchronise + D2H of n digests + H2D of an n-byte mask + synchronise."""
    ids = torch.randint(0, 256, (n, ID_LEN), dtype=torch.uint8, device=dev)
    h_ids = torch.empty((n, ID_LEN), dtype=torch.uint8).pin_memory()
    h_mask = torch.ones(n, dtype=torch.uint8).pin_memory()
    d_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    times = []
    for r in range(reps + 1):
        ids.add_(1)  # work in flight on the stream, as after a hash launch
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        h_ids.copy_(ids, non_blocking=True)
        torch.cuda.synchronize()  # the host reads the digests here
        d_mask.copy_(h_mask, non_blocking=True)
        torch.cuda.synchronize()
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    return median(times)


def hash_tables(torch, dev):
    """The 16 GiB of a config-2 batch and its two chunk tables: {n: (offsets, lengths)}."""
    from kopia_amd import batch
    from kopia_amd import hashing as kh
    name, ns, L = "DYNAMIC-4M-BUZHASH", 4096, 4 << 20
    data = torch.empty(ns * L, dtype=torch.uint8, device=dev)
    batch.fill_prng(data, L, ns, L, 0x6B6F706961, 0)
    b = batch.make_device_batch(name, [data.data_ptr() + i * L for i in range(ns)], [L] * ns, dev)
    batch.split_batch_device(name, b)
    torch.cuda.synchronize()
    offs, lens = kh.chunk_table([i * L for i in range(ns)], batch.read_cuts(b))
    m = 1 << 20
    piece = ns * L // m
    return data, {len(offs): (offs, lens), m: (np.arange(m, dtype=np.int64) * piece, np.full(m, piece, np.int64))}


def hash_times(torch, dev, data, offs, lens, reps):
    from kopia_amd import _lib
    n = len(offs)
    d_offs, d_lens = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    d_order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    out = torch.empty((n, ID_LEN), dtype=torch.uint8, device=dev)
    key = bytes(range(32))
    st = torch.cuda.current_stream(dev)
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.lib().kcdc_hash_chunks_device(HASH.encode(), C.c_void_p(data.data_ptr()), d_offs.data_ptr(),
                                                     d_lens.data_ptr(), d_order.data_ptr(), n, key, len(key),
                                                     out.data_ptr(), ID_LEN, C.c_void_p(st.cuda_stream)))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return median(times)


def worker(args):
    import torch
    from kopia_amd import dedup as kd
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(17)
    if args.kind == "context":  # the two yardsticks, once
        data, tables = hash_tables(torch, dev)
        for n, (offs, lens) in tables.items():
            emit({"kind": "context", "ids": n, "hash": HASH, "hash_bytes": int(lens.sum()),
                  "hash_ms": round(hash_times(torch, dev, data, offs, lens, args.reps), 3),
                  "roundtrip_ms": round(roundtrip_times(torch, dev, n, args.reps), 3),
                  "roundtrip_excludes": "the host map lookups"})
        return
    keys = int(args.kind)
    room = sum(BATCHES) * len(DUP_PERCENT) * (args.reps + 1)
    cs = kd.ContentSet(dev, ID_LEN, keys + room)
    pool = preload(torch, dev, cs, keys, gen)
    for n in BATCHES:
        for dup in DUP_PERCENT:
            before = cs.count()
            ms, kept = claim_times(torch, dev, cs, pool, n, dup, args.reps, gen)
            emit({"kind": "claim", "preloaded": keys, "stored_before": before, "max_keys": cs.max_keys,
                  "set_bytes": kd.set_bytes(ID_LEN, cs.max_keys), "ids": n, "dup_percent": dup, "kept": kept,
                  "claim_ms": round(ms, 4), "ids_per_us": round(n / ms / 1e3, 2)})
    cs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kinds", default="context,1048576,67108864", help="context, or a preload size")
    ap.add_argument("--kind", default="", help="(worker) run this kind in this process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    args = ap.parse_args()
    if args.kind:
        return worker(args)
    for kind in args.kinds.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--kind", kind, "--reps", str(args.reps)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps({"kind": kind, "failed": rc}), flush=True)
            sys.exit(rc)  # start nothing more on the GPU after a step that failed


if __name__ == "__main__":
    main()
