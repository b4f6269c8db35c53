#!/usr/bin/env python3
"""Which branches of the deflate span plan does the random-mixed test corpus reach?

Compresses the chunks of tests/test_gpu_compress.py::test_ragged_misaligned_chunks[deflate-default]
on the GPU, reads every stream back with tests/deflate_model.py and prints, per regime that
tests/test_gpu_deflate_edges.py plants on purpose, how many spans (or blocks) of the corpus reach
it.  A report, not a check: DESIGN.md 2.7 keeps the table.

    python tools/deflate_census.py [name]
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import deflate_model as dm  # noqa: E402
import test_gpu_compress as tc  # noqa: E402
import test_gpu_deflate_edges as te  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "deflate-default"
    dev = torch.device("cuda:0")
    host, offs, lens = tc.ragged_corpus()
    chunks = [host[o:o + ln].tobytes() for o, ln in zip(offs, lens)]
    blobs = te.compress(name, chunks, dev)  # (a span's plan does not depend on where its chunk lies)
    n = collections.Counter()
    depth = collections.Counter()
    for data, blob in zip(chunks, blobs):
        for s in te.read_back(name, blob, data):
            n["spans"] += 1
            k = s.kinds
            n["span: one stored block"] += k == "S"
            n["span: fixed code"] += "F" in k
            n["span: dynamic code"] += "D" in k
            n["span: coded, stored, coded (header repeated)"] += "DSD" in k or "FSF" in k
            n["span: stored run first"] += len(k) > 1 and k[0] == "S"
            n["span: stored run last (no sync flush)"] += len(k) > 1 and k[-1] == "S"
            per_seg = collections.Counter(p // te.SEG for p, t in te.positions(s) if not isinstance(t, int))
            n["span: a segment of 128 tokens"] += any(v >= 128 for v in per_seg.values())
            for t in s.matches:
                n["token: length 258"] += t[0] == 258
                n["token: length 257"] += t[0] == 257
                n["token: distance 1"] += t[1] == 1
                n["token: distance code 29"] += t[3] == 29
            if not s.dyn:
                continue
            b = s.dyn[0]
            d = [dm.huffman_cost(h)[1] for h in (s.lit_H, s.dist_H, s.cl_H)]
            depth["literal/length depth %d" % d[0]] += 1
            depth["code-length depth %d" % d[2]] += 1
            n["limiter: literal/length tree deeper than 15"] += d[0] > 15
            n["limiter: distance tree deeper than 15"] += d[1] > 15
            n["limiter: code-length tree deeper than 7"] += d[2] > 7
            zr, seam = te.header_runs(b)
            for r in (3, 10, 11, 138, 139):
                n["header: zero run of %d" % r] += r in zr
            n["header: zero run longer than 139"] += any(r > 139 for r in zr)
            vr = te.value_runs(b)
            for r in (4, 7, 8):
                n["header: run of %d equal lengths" % r] += r in vr
            n["header: run across the HLIT/HDIST seam"] += seam
            n["header: HLIT 286"] += b.hlit == 286
            n["header: HLIT < 260"] += b.hlit < 260
            n["header: HLIT 257"] += b.hlit == 257
            n["header: HDIST 30"] += b.hdist == 30
            n["header: HDIST <= 2"] += b.hdist <= 2
            n["header: HCLEN 19"] += b.hclen == 19
            n["header: HCLEN <= 5"] += b.hclen <= 5
            n["header: more than 64 run-length symbols"] += len(b.cl_syms) > 64
            n["header: at most 4 distinct run-length symbols"] += len(set(sy for sy, _ in b.cl_syms)) <= 4
            n["distances: one code used (second one forced)"] += sum(1 for c in s.raw_dist if c) == 1
            n["distances: none used"] += sum(s.raw_dist) == 0
            te.check_span(s)
    print(f"census of test_ragged_misaligned_chunks[{name}]: {len(lens)} chunks")
    for k in sorted(n):
        print(f"  {k:55s} {n[k]}")
    for k in sorted(depth, key=lambda x: (x.split()[0], int(x.split()[-1]))):
        print(f"  {k:55s} {depth[k]}")


if __name__ == "__main__":
    main()
