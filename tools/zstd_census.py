#!/usr/bin/env python3
"""Which branches of the zstd span encoder do the round-trip tests' inputs reach?

Compresses the chunks of tests/test_gpu_compress.py (test_ragged_misaligned_chunks' corpus, the
table-carrier chunks and the adversarial spans) on the GPU, reads every frame back with
tests/zstd_model.py and prints, per regime that tests/test_gpu_zstd_edges.py plants on purpose
(tests/zstd_structure.py regimes()), how many spans of each input reach it.  The invariants are
checked on the way.  A report, not a check: DESIGN.md 2.7 keeps the table.

    python tools/zstd_census.py [name] [largest chunk in bytes]
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import test_gpu_compress as tc  # noqa: E402
import test_gpu_zstd_edges as te  # noqa: E402  (its compress(), as tools/deflate_census.py takes the deflate file's)
import zstd_structure as zs  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "zstd"
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else 150000
    dev = torch.device("cuda:0")
    host, offs, lens = tc.ragged_corpus()
    inputs = {"ragged corpus": [host[o:o + ln].tobytes() for o, ln in zip(offs, lens) if ln <= cap],
              "table carriers": [c.tobytes() for c in tc.table_carrier_chunks()],
              "adversarial spans": [p.tobytes() for p in tc.adversarial_parts()]}
    names = set()
    rows = {}
    for what, chunks in inputs.items():
        n = collections.Counter()
        for k in range(0, len(chunks), 16):
            part = chunks[k:k + 16]
            for data, blob in zip(part, te.compress(name, part, dev)):
                for sp in zs.check(blob[4:], data, te.EFFORT[name]).spans:
                    n["spans"] += 1
                    for r in zs.regimes(sp):
                        n[r] += 1
        rows[what] = n
        names |= set(n)
    print(f"census of {name}: " + ", ".join(f"{w}: {len(c)} chunks, {rows[w]['spans']} spans" for w, c in inputs.items()))
    print("| regime | " + " | ".join(inputs) + " |")
    print("|---|" + "---|" * len(inputs))
    for r in sorted(names - {"spans"}):
        print(f"| {r} | " + " | ".join(str(rows[w][r]) for w in inputs) + " |")


if __name__ == "__main__":
    main()
