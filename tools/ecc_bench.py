"""ECC encode / decode / repair timing (kopia_amd.ecc, REED-SOLOMON-CRC32) over the sealed chunks
of a config-2-shaped batch: streams of 4 MiB are split (DYNAMIC-4M-BUZHASH), hashed and sealed
(AES256-GCM-HMAC-SHA256) on the device, and the sealed chunks are encoded, decoded clean, and
decoded with 1 % of them damaged and repaired.  One JSON line per overhead (default 2 and 10 %).
Not a parity test -- tests/test_gpu_ecc.py is.

The driver holds no GPU: every overhead runs in a child process of its own under `timeout`, and
the first child that fails, faults or times out ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12  # bytes/s, MI355X


def worker(args):
    import torch
    from kopia_amd import _lib, batch
    from kopia_amd import ecc as kecc
    from kopia_amd import encryption as ke
    from kopia_amd import hashing as kh
    dev = torch.device("cuda", 0)
    name, ns, L = "DYNAMIC-4M-BUZHASH", args.streams, 4 << 20
    data = torch.empty(ns * L, dtype=torch.uint8, device=dev)
    batch.fill_prng(data, L, ns, L, 0x6B6F706961, 0)
    b = batch.make_device_batch(name, [data.data_ptr() + i * L for i in range(ns)], [L] * ns, dev)
    batch.split_batch_device(name, b)
    offs, lens = kh.chunk_table([i * L for i in range(ns)], batch.read_cuts(b))
    ids = kh.hash_chunks_device(kh.DefaultAlgorithm, data.data_ptr(), offs, lens, bytes(range(32)), dev).contiguous()
    enc = ke.Encryptor(ke.Aes256Gcm, bytes(range(32)))
    so, stotal = ke.sealed_layout(lens, ke.Aes256Gcm)
    sealed = torch.empty(stotal, dtype=torch.uint8, device=dev)
    st = enc.encrypt_chunks_device(data.data_ptr(), offs, lens, ids, 16, sealed, so, dev)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    del data
    slens = np.asarray(lens, np.int64) + enc.Overhead()

    a = kecc.CreateEncryptor(kecc.DefaultAlgorithm, args.overhead)
    eo, esizes, etotal = a.stored_layout(slens)
    stored = torch.empty(etotal, dtype=torch.uint8, device=dev)
    po, ptotal = a.plain_layout(esizes)
    back = torch.empty(ptotal, dtype=torch.uint8, device=dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    enc_ms = timed(lambda: a.encrypt_chunks_device(sealed.data_ptr(), so, slens, stored, eo, dev))
    dec_ms = timed(lambda: a.decrypt_chunks_device(stored.data_ptr(), eo, esizes, back, po, dev))
    dec = a.decrypt_chunks_device(stored.data_ptr(), eo, esizes, back, po, dev)
    torch.cuda.synchronize()
    assert not dec.status.cpu().numpy().any(), "clean decode reported damage"
    assert dec.out_lens.cpu().tolist() == slens.tolist()
    pick = [0, len(slens) // 2, len(slens) - 1]
    for i in pick:
        assert torch.equal(back[int(po[i]):int(po[i]) + int(slens[i])], sealed[int(so[i]):int(so[i]) + int(slens[i])])

    # 1 % of the chunks lose one data shard each (a byte of its payload flipped), in varying blocks
    n = len(slens)
    hit = list(range(0, n, 100)) or [0]
    rec = 4 + a.MaxShardSize
    for k, i in enumerate(hit):
        blocks = -(-(int(slens[i]) + 4) // (a.DataShards * a.MaxShardSize))
        par = a.ParityShards * rec * blocks
        shard = (k * 37) % max(1, (int(esizes[i]) - par) // rec)
        stored[int(eo[i]) + par + shard * rec + 4 + 1] ^= 0x55
    back.zero_()
    dec = a.decrypt_chunks_device(stored.data_ptr(), eo, esizes, back, po, dev)
    torch.cuda.synchronize()
    nd = int((dec.status.cpu().numpy() == _lib.KCDC_ECC_DAMAGED).sum())
    t0 = time.perf_counter()
    dec.repair()
    rep_ms = (time.perf_counter() - t0) * 1e3
    assert not dec.status.cpu().numpy().any(), "repair left failed chunks"
    for i in hit[:3] + hit[-1:]:
        assert torch.equal(back[int(po[i]):int(po[i]) + int(slens[i])], sealed[int(so[i]):int(so[i]) + int(slens[i])])

    nbytes, sbytes = int(slens.sum()), int(esizes.sum())
    gib = nbytes / (1 << 30)
    print(json.dumps({
        "overhead_percent": args.overhead, "data_shards": a.DataShards, "parity_shards": a.ParityShards,
        "shard_size": a.MaxShardSize, "chunks": n, "bytes": nbytes, "stored_bytes": sbytes,
        "encode_ms": round(enc_ms, 3), "encode_gib_s": round(gib / enc_ms * 1e3, 1),
        "encode_hbm_frac": round((nbytes + sbytes) / (enc_ms * 1e-3) / HBM_PEAK, 3),
        "decode_ms": round(dec_ms, 3), "decode_gib_s": round(gib / dec_ms * 1e3, 1),
        "decode_hbm_frac": round((nbytes + sbytes) / (dec_ms * 1e-3) / HBM_PEAK, 3),
        "damaged_chunks": nd, "repair_ms": round(rep_ms, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512, help="4 MiB streams (config 2 has 4096)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--overheads", default="2,10")
    ap.add_argument("--overhead", type=int, default=0, help="(worker) run this overhead in this process")
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds per GPU step")
    args = ap.parse_args()
    if args.overhead:
        return worker(args)
    for o in [int(x) for x in args.overheads.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--overhead", str(o), "--streams", str(args.streams), "--reps", str(args.reps)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps({"overhead_percent": o, "failed": rc}), flush=True)
            sys.exit(rc)  # start nothing more on the GPU after a step that failed


if __name__ == "__main__":
    main()
