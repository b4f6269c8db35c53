"""Timing of kcdc_pack_chunks_device (kopia_amd.packing) over the chunks of a config-2-shaped batch
(streams of 4 MiB split by DYNAMIC-4M-BUZHASH, as tools/ecc_bench.py), on mixed and on random data,
for deflate-default, s2-default, zstd and no compressor, both encryptors, ECC off and 2 %.
One JSON line per configuration:
  pack_ms      the one call (device time between two events)
  stages_ms    the same work through the existing entry points on the same inputs in the same
               process: compress, seal (kept contents from the compress slots, dropped ones in place),
               ECC encode; the decisions between them are read back on the host and not timed
  overhead     (pack_ms - sum of stages_ms) / pack_ms: plan + gather + launch gaps
  kernels_ms   per-kernel device time inside the call from the profiler (plan = the plan and scan
               kernels, gather), when the profiler is available
  copy_ms      a device-to-device copy of the sealed bytes in one piece, the gather's yardstick
and one line for the plan alone at 2^20 one-KiB chunks.  Not a parity test: tests/test_gpu_pack.py is.

The driver holds no GPU: every data kind runs in a child process of its own under `timeout`, and the
first child that fails, faults or times out ends the run."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COMPS = (None, "deflate-default", "s2-default", "zstd")
MAX_PACK = 20 << 20  # the reference's default MaxPackSize


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_times(torch, fn):
    """{plan, gather, other} device ms of one call, from the profiler; None without it."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {"plan": 0.0, "gather": 0.0, "other": 0.0}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            if not t:
                continue
            key = "gather" if "gather_kernel" in ev.key else "plan" if "packdev" in ev.key else "other"
            out[key] += t / 1e3
        return {k: round(v, 3) for k, v in out.items()} if out["plan"] else None
    except Exception as e:  # no profiler in this build: the event times stand alone
        return {"unavailable": type(e).__name__}


def mixed_fill(torch, data, seed):
    """Half of every 64 KiB text-like (a 4 KiB phrase table repeated with a per-block twist), half PRNG."""
    g = torch.Generator(device=data.device).manual_seed(seed)
    words = torch.randint(97, 123, (4096,), dtype=torch.uint8, device=data.device, generator=g)
    view = data.view(-1, 65536)
    view[:, :32768] = words.repeat(8)[None, :]
    view[:, 0:32768:257] = torch.randint(0, 256, (view.shape[0], len(range(0, 32768, 257))), dtype=torch.uint8,
                                         device=data.device, generator=g)


def one_config(torch, dev, data, offs, lens, ids, nonces, comp, alg, ecc_pct, reps):
    from kopia_amd import compression as kc
    from kopia_amd import ecc as kecc
    from kopia_amd import encryption as ke
    from kopia_amd import packing as kp
    n = len(lens)
    packer = kp.Packer(alg, ke.derive_key(bytes(range(32))), MAX_PACK, compression=comp,
                       ecc=kecc.DefaultAlgorithm if ecc_pct else None, ecc_overhead_percent=ecc_pct, pack_lead=37)
    call = lambda: packer.pack_chunks_device(data.data_ptr(), offs, lens, ids, nonces, dev)
    d_pack, entries, packs, totals = call()
    torch.cuda.synchronize()
    ent = kp.entries_numpy(entries)
    assert not ent["status"].any()
    tot = totals.cpu().tolist()
    del d_pack, entries, packs, totals
    pack_ms = timed(torch, call, reps)
    kern = kernel_times(torch, call)

    # the stages through the existing entry points
    stages = {}
    enc = ke.Encryptor(alg, bytes(range(32)))
    plain_lens = np.asarray(lens, np.int64)
    src = np.asarray(offs, np.int64)
    if comp:
        c = kc.Compressor(comp)
        co, ctotal = kc.compressed_layout(lens)
        d_comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        stages["compress"] = timed(torch, lambda: c.compress_chunks_device(data.data_ptr(), offs, lens, d_comp, co, dev), reps)
        ol, hid = c.compress_chunks_device(data.data_ptr(), offs, lens, d_comp, co, dev)
        ol, hid = ol.cpu().numpy(), hid.cpu().numpy()
        kept = hid != 0
        assert (ent["header_id"] == hid.astype(np.uint32)).all()
        plain_lens = np.where(kept, ol, plain_lens)
        # kept contents are read from the compress buffer: offsets relative to the data pointer, modulo 2^64
        rel = (np.asarray(co, np.int64) + (d_comp.data_ptr() - data.data_ptr())).astype(np.int64)
        src = np.where(kept, rel, src)
    so, stotal = ke.sealed_layout(plain_lens, alg)
    sealed = torch.empty(stotal, dtype=torch.uint8, device=dev)
    nb = bytes(nonces.cpu().numpy().tobytes())
    stages["seal"] = timed(torch, lambda: enc.encrypt_chunks_device(data.data_ptr(), src, plain_lens, ids, ids.shape[1],
                                                                    sealed, so, dev, nonces=nb, iv_len=16), reps)
    slens = plain_lens + 28
    if ecc_pct:
        a = kecc.CreateEncryptor(kecc.DefaultAlgorithm, ecc_pct)
        eo, esizes, etotal = a.stored_layout(slens)
        stored = torch.empty(etotal, dtype=torch.uint8, device=dev)
        stages["ecc"] = timed(torch, lambda: a.encrypt_chunks_device(sealed.data_ptr(), so, slens, stored, eo, dev), reps)
        assert (ent["packed_length"] == esizes.astype(np.uint32)).all()
    else:
        assert (ent["packed_length"] == slens.astype(np.uint32)).all()
    dst = torch.empty(int(slens.sum()), dtype=torch.uint8, device=dev)
    one = sealed[:int(slens.sum())]
    copy_ms = timed(torch, lambda: dst.copy_(one), reps)
    ssum = sum(stages.values())
    row = {"compression": comp, "encryption": alg, "ecc_percent": ecc_pct, "chunks": n, "bytes": int(np.sum(lens)),
           "kept": int((ent["header_id"] != 0).sum()), "packs": tot[0], "pack_bytes": tot[1],
           "pack_ms": round(pack_ms, 3), "stages_ms": {k: round(v, 3) for k, v in stages.items()},
           "overhead": round((pack_ms - ssum) / pack_ms, 3), "kernels_ms": kern, "sealed_bytes": int(slens.sum()),
           "copy_ms": round(copy_ms, 3), "copy_gb_s": round(slens.sum() / copy_ms / 1e6, 1)}
    if kern and kern.get("gather"):
        row["gather_gb_s"] = round(slens.sum() / kern["gather"] / 1e6, 1)
        row["gather_vs_copy"] = round(copy_ms / kern["gather"], 3)
    return row


def worker(args):
    import torch
    from kopia_amd import batch
    from kopia_amd import encryption as ke
    from kopia_amd import hashing as kh
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    if args.kind == "plan":  # the plan alone: 2^20 chunks of 1 KiB
        n = 1 << 20
        data = torch.empty(n << 10, dtype=torch.uint8, device=dev)
        batch.fill_prng(data, n << 10, 1, n << 10, 0x6B6F706961, 0)
        offs, lens = np.arange(n, dtype=np.int64) << 10, np.full(n, 1024, np.int64)
        ids = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).to(dev)
        nonces = torch.from_numpy(rng.integers(0, 256, (n, 12), dtype=np.uint8)).to(dev)
        row = one_config(torch, dev, data, offs, lens, ids, nonces, None, ke.ChaCha20Poly1305, 0, args.reps)
        row["kind"] = "plan-2^20x1KiB"
        print(json.dumps(row), flush=True)
        return
    name, ns, L = "DYNAMIC-4M-BUZHASH", args.streams, 4 << 20
    data = torch.empty(ns * L, dtype=torch.uint8, device=dev)
    batch.fill_prng(data, L, ns, L, 0x6B6F706961, 0)
    if args.kind == "mixed":
        mixed_fill(torch, data, 7)
    b = batch.make_device_batch(name, [data.data_ptr() + i * L for i in range(ns)], [L] * ns, dev)
    batch.split_batch_device(name, b)
    offs, lens = kh.chunk_table([i * L for i in range(ns)], batch.read_cuts(b))
    ids = kh.hash_chunks_device(kh.DefaultAlgorithm, data.data_ptr(), offs, lens, bytes(range(32)), dev).contiguous()
    ids = ids[:, -16:].contiguous()
    nonces = torch.from_numpy(rng.integers(0, 256, (len(lens), 12), dtype=np.uint8)).to(dev)
    for comp in COMPS:
        for alg in (ke.Aes256Gcm, ke.ChaCha20Poly1305):
            for ecc_pct in (0, 2):
                row = one_config(torch, dev, data, offs, lens, ids, nonces, comp, alg, ecc_pct, args.reps)
                row["kind"] = args.kind
                print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512, help="4 MiB streams (config 2 has 4096)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kinds", default="mixed,random,plan")
    ap.add_argument("--kind", default="", help="(worker) run this data kind in this process")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per GPU step")
    args = ap.parse_args()
    if args.kind:
        return worker(args)
    for kind in args.kinds.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--kind", kind, "--streams", str(args.streams), "--reps", str(args.reps)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps({"kind": kind, "failed": rc}), flush=True)
            sys.exit(rc)  # start nothing more on the GPU after a step that failed


if __name__ == "__main__":
    main()
