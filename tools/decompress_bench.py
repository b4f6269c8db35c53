"""S2 decompression throughput on the device (kcdc_decompress_chunks_device), in decoded GiB/s,
with every decoded byte compared with the original on the device, and pyarrow's Snappy decode on
one host thread in the same run, for scale.  Inputs:
  mixed     random / zero / periodic / word-salad stretches, compressed on the device (s2-default)
  periodic  the reference benchmark's 1..10 pattern and zeros (compressor_test.go:92-93), likewise
  random    uniform PRNG bytes, likewise (every segment is a stored literal)
  blocks1m  the mixed data as streams of 1 MiB Snappy blocks from the tests' block builder
            (tests/test_s2_vectors.py: snappy_framed), the block size of s2.NewWriter
Each input is timed --reps times (--iters calls each); the spread between the repetitions is the
noise a variant has to beat.  Usage: python tools/decompress_bench.py [--mib 1024] [--iters 5] [--reps 5]
Logs: profiles/decompress/."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kopia_amd import _lib  # noqa: E402
from kopia_amd import compression as kc  # noqa: E402
import test_s2_vectors as sv  # noqa: E402

NAME = "s2-default"


def chunk_lengths(nbytes, chunk, seed):
    rng = np.random.default_rng(seed)
    lens, pos = [], 0
    while pos < nbytes:  # ~4 MiB contents (DYNAMIC-4M's range)
        n = min(int(rng.integers(chunk // 2, 2 * chunk)), nbytes - pos)
        lens.append(n)
        pos += n
    return lens


def device_streams(d, lens, dev):
    """Compress contents of the device bytes d on the device; (buffer, offsets, lengths)."""
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    oo, total = kc.compressed_layout(lens)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    ol, _ = kc.Compressor(NAME).compress_chunks_device(d.data_ptr(), offs, lens, out, oo, dev)
    torch.cuda.synchronize()
    return out, oo, ol.cpu().numpy()


def time_decode(comp, c_offs, c_lens, caps, want, iters, reps, dev):
    n = len(caps)
    o_offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.int64)
    out = torch.zeros(int(np.sum(caps)), dtype=torch.uint8, device=dev)
    t = [torch.as_tensor(np.asarray(x, np.int64)).to(dev) for x in (c_offs, c_lens, o_offs, caps)]
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    wb = int(_lib.lib().kcdc_decompress_workspace_size(int(np.sum(c_lens)), int(np.sum(caps)), n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)

    def once():
        _lib.check(_lib.lib().kcdc_decompress_chunks_device(
            NAME.encode(), comp.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), n, out.data_ptr(), t[2].data_ptr(),
            t[3].data_ptr(), ol.data_ptr(), status.data_ptr(), work.data_ptr(), wb, st.cuda_stream))

    once()
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any(), "a content failed to decode"
    assert ol.cpu().numpy().tolist() == list(caps)
    assert torch.equal(out, want), "decoded bytes differ from the original"
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(iters):
            once()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    total = args.mib << 20
    base_n = min(total, 64 << 20)
    res = {"name": NAME, "library": _lib.lib().kcdc_version().decode(), "device_time_excludes_h2d": True}
    for kind in ["mixed", "periodic", "random", "blocks1m"]:
        if args.only and kind != args.only:
            continue
        if kind == "random":
            base = np.random.default_rng(7).integers(0, 256, base_n, dtype=np.uint8)
        elif kind == "periodic":
            base = np.tile(np.arange(1, 11, dtype=np.uint8), base_n // 10 + 1)[:base_n].copy()
            base[base_n // 2:] = 0
        else:
            base = np.frombuffer(sv.mixed(base_n, 9), np.uint8).copy()
        reps = max(1, total // base_n)
        if kind == "blocks1m":  # host-built streams of one base, uploaded once and repeated
            lens1 = chunk_lengths(base_n, 4 << 20, 1)
            pos, blobs = 0, []
            for n in lens1:
                blobs.append(sv.content(sv.snappy_framed(base[pos:pos + n].tobytes(), 1 << 20, sv.IDENT_S2), NAME))
                pos += n
            one = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(dev)
            comp = one.repeat(reps)
            bl = np.array([len(b) for b in blobs], np.int64)
            c_lens = np.tile(bl, reps)
            c_offs = np.concatenate(([0], np.cumsum(c_lens)[:-1])).astype(np.int64)
            lens = lens1 * reps
            d = torch.from_numpy(base).to(dev).repeat(reps)
        else:
            d = torch.from_numpy(base).to(dev).repeat(reps)
            lens = chunk_lengths(d.numel(), 4 << 20, 1)
            comp, c_offs, c_lens = device_streams(d, lens, dev)
        nbytes = d.numel()
        ms = time_decode(comp, c_offs, c_lens, lens, d, args.iters, args.reps, dev)
        rate = [nbytes / m / 1e6 / 1.073741824 for m in ms]
        # one host thread of Google's Snappy over the same kind of blocks, for scale
        import pyarrow as pa
        codec = pa.Codec("snappy")
        sample = base[:16 << 20].tobytes()
        parts = [codec.compress(sample[i:i + (1 << 16)], asbytes=True) for i in range(0, len(sample), 1 << 16)]
        sizes = [min(1 << 16, len(sample) - i) for i in range(0, len(sample), 1 << 16)]
        t0 = time.perf_counter()
        for p, n in zip(parts, sizes):
            codec.decompress(p, decompressed_size=n)
        cpu_s = time.perf_counter() - t0
        res[kind] = {
            "decoded_bytes": nbytes, "contents": len(lens), "compressed_ratio": round(float(np.sum(c_lens)) / nbytes, 4),
            "ms": [round(m, 3) for m in ms],
            "GiB_s_min_median_max": [round(x, 1) for x in (min(rate), float(np.median(rate)), max(rate))],
            "pyarrow_snappy_decode_1thread_GiB_s": round(len(sample) / cpu_s / (1 << 30), 2),
        }
        print(json.dumps({kind: res[kind]}), flush=True)
        del d, comp
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
