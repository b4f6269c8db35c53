"""zstd decoding throughput on the device (kcdc_zstd_decode_chunks_device), in decoded GiB/s, with
every decoded byte compared with the original on the device, and libzstd's ZSTD_decompress on the
host (one thread, and --threads of them) over the same frames in the same run.
  writers  own      the library's frames (kcdc_compress_chunks_device, name zstd)
           libzstd  libzstd level 3, with and without the content checksum
  inputs   mixed     random / zero / periodic / word-salad stretches
           periodic  the reference benchmark's 1..10 pattern and zeros (compressor_test.go:92-93)
           random    uniform PRNG bytes (raw blocks)
  shapes   4m   contents of 4 MiB: 256 of them in 1 GiB, fewer than the 4,096 persistent execute
                waves, so the row shows the rate of one executing wave (the entropy pass still has
                8,192 blocks to spread)
           64k  contents of 64 KiB: 16,384 in 1 GiB, both grids are full
A --base-mib stretch of each input is compressed once and repeated to --mib.  Each row is timed
--reps times after a warm-up call (device events around --iters calls; by default as many calls as
fill a quarter of a second); the spread between the repetitions, and between two runs of this
program, is the noise a variant has to beat.  The kZstdBatch = 1 variant
(make variants VARIANTS="batch1:-DKCDC_ZSTD_BATCH=1") is timed by running this program with KCDC_LIB
(and KCDC_ALLOW_VARIANT_LIB=1), alternating with the product library in one session; the header
line names the library file.
Usage: python tools/zstd_decode_bench.py [--mib 1024] [--iters 0] [--reps 5]   Logs: profiles/zstd_decode/."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kopia_amd import _lib  # noqa: E402
from kopia_amd import compression as kc  # noqa: E402
import test_s2_vectors as sv  # noqa: E402
import zstd_vectors as zv  # noqa: E402  (libzstd through ctypes)

SHAPES = {"4m": 4 << 20, "64k": 64 << 10}


def base_bytes(kind, n):
    if kind == "random":
        return np.random.default_rng(7).integers(0, 256, n, dtype=np.uint8)
    if kind == "periodic":
        base = np.tile(np.arange(1, 11, dtype=np.uint8), n // 10 + 1)[:n].copy()
        base[n // 2:] = 0
        return base
    return np.frombuffer(sv.mixed(n, 9), np.uint8).copy()


def own_streams(name, d, lens, dev):
    """Contents of the device bytes d compressed on the device: (blobs as host bytes)."""
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    oo, total = kc.compressed_layout(lens)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    ol, _ = kc.Compressor(name).compress_chunks_device(d.data_ptr(), offs, lens, out, oo, dev)
    torch.cuda.synchronize()
    host, ol = out.cpu().numpy(), ol.cpu().numpy()
    return [host[o:o + n].tobytes() for o, n in zip(oo, ol)]


def libzstd_streams(name, base, lens, threads, checksum):
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)

    def one(k):
        return zv.content(name, zv.zstd_frame(base[offs[k]:offs[k] + lens[k]].tobytes(), level=3, checksum=checksum))

    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(len(lens))))


def host_rate(blobs, lens, nbytes, threads):
    """ZSTD_decompress of every frame (ctypes releases the GIL), decoded GiB/s on `threads` threads."""
    import ctypes as C
    streams = [(C.create_string_buffer(b[4:], len(b) - 4), len(b) - 4, C.create_string_buffer(max(n, 1)), n) for b, n in zip(blobs, lens)]

    def one(s):
        assert zv.Z.ZSTD_decompress(s[2], s[3], s[0], s[1]) == s[3]

    best = 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        if threads == 1:
            for s in streams:
                one(s)
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(one, streams))
        best = max(best, nbytes / (time.perf_counter() - t0) / (1 << 30))
    return best


def time_decode(name, blobs, lens, want, repeat, iters, reps, dev):
    """The base's streams uploaded once and repeated `repeat` times; ms per call, `reps` of them."""
    one = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(dev)
    comp = one.repeat(repeat)
    c_lens = np.tile(np.array([len(b) for b in blobs], np.int64), repeat)
    c_offs = np.concatenate(([0], np.cumsum(c_lens)[:-1])).astype(np.int64)
    caps = np.tile(np.asarray(lens, np.int64), repeat)
    o_offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.int64)
    n = len(caps)
    out = torch.zeros(int(caps.sum()), dtype=torch.uint8, device=dev)
    t = [torch.as_tensor(x).to(dev) for x in (c_offs, c_lens, o_offs, caps)]
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    wb = int(_lib.lib().kcdc_zstd_decode_workspace_size(int(c_lens.sum()), int(caps.sum()), n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)

    def once():
        _lib.check(_lib.lib().kcdc_zstd_decode_chunks_device(
            name.encode(), comp.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), n, out.data_ptr(), t[2].data_ptr(),
            t[3].data_ptr(), ol.data_ptr(), status.data_ptr(), work.data_ptr(), wb, st.cuda_stream))

    t0 = time.perf_counter()
    once()  # the warm-up, and the check of every byte
    torch.cuda.synchronize()
    if iters <= 0:  # enough calls for a timed window of about a quarter of a second
        iters = max(1, min(400, int(0.25 / max(time.perf_counter() - t0, 1e-4))))
    assert not status.cpu().numpy().any(), "a content failed to decode"
    assert ol.cpu().numpy().tolist() == caps.tolist()
    assert torch.equal(out, want.repeat(repeat)), "decoded bytes differ from the original"
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(iters):
            once()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms, n, float(c_lens.sum()), iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--base-mib", type=int, default=64)
    ap.add_argument("--iters", type=int, default=0, help="calls per repetition; 0: as many as fill a quarter of a second")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--only", default="", help="comma-separated inputs")
    args = ap.parse_args()
    assert _lib.lib().kcdc_device_count() >= 1, "no gfx950 device: " + _lib.last_error()
    dev = torch.device("cuda:0")
    total, base_n = args.mib << 20, min(args.mib, args.base_mib) << 20
    repeat = max(1, total // base_n)
    rows = [("zstd", w, k, s) for k in ("mixed", "periodic", "random") for w in ("own", "libzstd", "libzstd-checksum")
            for s in SHAPES]
    print(json.dumps({"library": _lib.lib().kcdc_version().decode(), "library_file": os.path.basename(_lib.LIB_PATH),
                      "decoded_MiB": args.mib, "base_MiB": base_n >> 20, "host_threads": args.threads,
                      "device_time_excludes_h2d": True, "batch": os.environ.get("KCDC_LIB", "product")}), flush=True)
    for name, writer, kind, shape in rows:
        if args.only and kind not in args.only.split(","):
            continue
        base = base_bytes(kind, base_n)
        lens = [SHAPES[shape]] * (base_n // SHAPES[shape])
        d = torch.from_numpy(base).to(dev)
        blobs = (own_streams(name, d, lens, dev) if writer == "own" else
                 libzstd_streams(name, base, lens, args.threads, writer.endswith("checksum")))
        ms, n, comp_bytes, iters = time_decode(name, blobs, lens, d, repeat, args.iters, args.reps, dev)
        nbytes = base_n * repeat
        rate = [nbytes / m / 1e6 / 1.073741824 for m in ms]
        waves = min(n, 4096)
        row = {"name": name, "writer": writer, "input": kind, "shape": shape, "contents": n, "decoded_bytes": nbytes,
               "compressed_ratio": round(comp_bytes / nbytes, 4), "calls_per_rep": iters, "ms": [round(m, 3) for m in ms],
               "GiB_s_min_median_max": [round(x, 2) for x in (min(rate), float(np.median(rate)), max(rate))],
               "MiB_s_per_wave_median": round(float(np.median(rate)) * 1024 / waves, 2) if n <= 4096 else None,
               "host_libzstd_1thread_GiB_s": round(host_rate(blobs, lens, base_n, 1), 2),
               f"host_libzstd_{args.threads}threads_GiB_s": round(host_rate(blobs, lens, base_n, args.threads), 2)}
        print(json.dumps(row), flush=True)
        del d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
