"""The many-chunk population shared by tests/test_many_chunks.py (CPU: its structure) and
tests/test_gpu_many_chunks.py (GPU: every per-chunk entry point over it).  No tests here.

Kopia's workload is trees of small files: one call carries thousands of tiny and empty chunks.  The
population is shaped after the code that exists only for such calls:
  - the one-workgroup prefix scans (1024 threads): with n > 1024 a thread owns several entries
    (COUNTS: 1025 gives one thread two; 3071 gives two or three, three 1024-chunk rounds of the ECC
    scan and per = 3 with an idle last thread in the S2 scan);
  - chunk lookup by bisection of a prefix with duplicates: chunks of length 0 own no unit, span or
    block, and they come in runs: the first three, 1022..1026 (across the scan seam at 1024) and the
    last three chunks, plus about 5 % scattered;
  - walks across chunks inside one wave: ordinary chunks are 1..96 bytes, so with a capped grid
    (KCDC_TEST_CHUNK_GRID) every wave crosses dozens of them;
  - non-trivial prefixes: every 257th chunk is 70000 + i % 7 bytes (18 crypt units, 3 compress
    spans, 3 S2 blocks; 9 ECC blocks at options (10, 0), one 130-shard block at (2, 1024)).
Chunks are packed with gaps of 1..3 bytes, so every alignment mod 16 occurs; the bytes are the
mixed data of tests/test_s2_vectors.py (random, zero, periodic and word stretches)."""
import functools

import numpy as np

import test_s2_vectors as sv

COUNTS = (1025, 3071)
SEED = 20  # the population both test files use
SEAM = (1022, 1023, 1024, 1025, 1026)  # empty, across the scan-thread and 1024-round seam
LARGE_EVERY, LARGE_BASE = 257, 70000
SMALL_MAX = 96
GAP = 13  # the least guard between two output slots


def zero_runs(n):
    """The indices that are empty by construction (the scattered ones come on top)."""
    return sorted({0, 1, 2, n - 3, n - 2, n - 1} | {i for i in SEAM if i < n})


def after_seam():
    return max(SEAM) + 1


@functools.lru_cache(maxsize=None)
def population(n, seed):
    """(host bytes uint8, offsets int64, lengths int64) of n chunks; the arrays are read-only."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, SMALL_MAX + 1, n).astype(np.int64)
    lens[rng.random(n) < 0.05] = 0
    runs = set(zero_runs(n))
    for i in range(LARGE_EVERY, n, LARGE_EVERY):
        if i not in runs:
            lens[i] = LARGE_BASE + i % 7
    lens[sorted(runs)] = 0
    for i in sorted(runs):  # every run ends at a chunk with bytes, so a lookup has a whole run to step over
        for j in (i - 1, i + 1):
            if 0 <= j < n and j not in runs and lens[j] == 0:
                lens[j] = 1 + j % SMALL_MAX
    gaps = rng.integers(1, 4, n).astype(np.int64)
    offs = np.cumsum(gaps + np.concatenate(([0], lens[:-1])))
    host = np.frombuffer(sv.mixed(int(offs[-1] + lens[-1]) + 16, seed), np.uint8).copy()
    for a in (host, offs, lens):
        a.setflags(write=False)
    return host, offs, lens


def chunk(pop, i):
    host, offs, lens = pop
    return host[offs[i]:offs[i] + lens[i]].tobytes()


def large_indices(lens):
    return [int(i) for i in np.flatnonzero(np.asarray(lens) >= LARGE_BASE)]


def slots(sizes, align=1):
    """(offsets, total) of output slots of `sizes` bytes with GAP or more guard bytes before, between
    and after them.  align 1: the offsets take every residue mod 16 over a call (the gap grows by one
    after every other slot); align 4: multiples of 4, for the entry points that ask for them."""
    sizes = np.asarray(sizes, np.int64)
    offs = np.zeros(len(sizes), np.int64)
    pos = GAP
    for i, s in enumerate(sizes):
        pos = -(-pos // align) * align
        offs[i] = pos
        pos += int(s) + GAP + (i & 1)
    return offs, pos + GAP


def outside_intact(buf, offs, sizes, fill):
    """Whether every byte of buf outside the slots [offs[i], offs[i] + sizes[i]) still holds `fill`."""
    edge = np.zeros(len(buf) + 1, np.int64)
    np.add.at(edge, np.asarray(offs, np.int64), 1)
    np.add.at(edge, np.asarray(offs, np.int64) + np.asarray(sizes, np.int64), -1)
    inside = np.cumsum(edge[:-1]) > 0
    return bool((np.asarray(buf)[~inside] == fill).all())
