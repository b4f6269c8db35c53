"""CPU model of what the long-stream path (kcdc_split_long_device) sees of its input.

Test infrastructure only (tests/test_long_model.py, tests/test_gpu_long_edges.py): nothing in
the product imports it.

The long path scans every 128 KiB *coordinate* segment of a stream for candidates (positions
whose window hash has its masked bits zero), keeps the first kSegK = 8 of each segment, and
resolves the chunk rule over that list, rescanning where a truncated segment may hide the
candidate it needs (kopia_amd/csrc/kcdc_split_long.h, "long single stream").  Which of those
branches an input reaches depends only on where its candidates lie, so this module computes
exactly that, in numpy, from the hashes' definitions and not from the kernels:

  both hashes XOR-decompose per window slot and the all-zero window hashes to 0, so with the
  64 bytes before the stream taken as zero
      h[p] = XOR_{k=0..63} T_k[d[p-k]]
  buzhash32:    T_k[b] = rotl32(T[b], k)
  rabinkarp64:  T_k[b] = b * x^(8k) mod P

tests/test_long_model.py pins rule(candidates(...)) to the C oracle's cuts, so the
preconditions the GPU tests assert about their inputs (segments with exactly 8 or 9
candidates, cuts on unlisted candidates, ...) can be trusted.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from oracle import rollinghash as rh

WINDOW = rh.WINDOW
SEG = 128 << 10   # dev::kSegBytes
SEG_K = 8         # dev::kSegK
LANE = 2 << 10    # bytes of a segment scanned by one lane
_BLOCK = 1 << 16  # positions hashed per step (keeps the 64 gathers in cache)


@lru_cache(maxsize=None)
def slot_tables(kind: str) -> np.ndarray:
    """T_k[b] for k = 0..63: [64][256], uint32 (buzhash) or uint64 (rabinkarp)."""
    if kind == "buzhash":
        t = rh.buzhash_table().astype(np.uint32)
        return np.stack([t if k % 32 == 0 else (t << np.uint32(k % 32)) | (t >> np.uint32(32 - k % 32))
                         for k in range(WINDOW)])
    assert kind == "rabinkarp", kind
    P, _ = rh.rabin_polynomial()
    out = np.zeros((WINDOW, 256), dtype=np.uint64)
    xk = 1  # x^(8k) mod P
    for k in range(WINDOW):
        out[k] = [rh._gf2_mulmod(xk, b, P) for b in range(256)]
        xk = rh._gf2_mulmod(xk, 1 << 8, P)
    return out


def hashes(kind: str, data) -> np.ndarray:
    """The window hash ending at every position of `data` (the window starts as 64 zeros)."""
    d = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    tabs = slot_tables(kind)
    n = d.size
    pad = np.concatenate([np.zeros(WINDOW - 1, dtype=np.uint8), d])  # pad[i + 63] = d[i]
    h = np.empty(n, dtype=tabs.dtype)
    for a in range(0, n, _BLOCK):
        b = min(a + _BLOCK, n)
        acc = tabs[0][pad[a + WINDOW - 1:b + WINDOW - 1]]
        for k in range(1, WINDOW):
            acc ^= tabs[k][pad[a + WINDOW - 1 - k:b + WINDOW - 1 - k]]
        h[a:b] = acc
    return h


def candidates_of(h: np.ndarray, avg: int) -> np.ndarray:
    """Positions whose hash has the mask's bits zero (avg a power of two: mask = avg - 1)."""
    return np.flatnonzero((h & h.dtype.type(avg - 1)) == 0).astype(np.int64)


def candidates(kind: str, avg: int, data) -> np.ndarray:
    return candidates_of(hashes(kind, data), avg)


def candidates_in(kind: str, avg: int, data: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """Candidates p of `data` with lo <= p < hi, hashing only the bytes their windows cover."""
    lo, hi = max(lo, 0), min(hi, data.size)
    if lo >= hi:
        return np.zeros(0, dtype=np.int64)
    a = max(lo - (WINDOW - 1), 0)  # (a == 0: the zero window before the stream is hashes()' own)
    c = candidates(kind, avg, data[a:hi]) + a
    return c[c >= lo]


def rule(cands, n: int, mn: int, mx: int) -> np.ndarray:
    """Chunk end offsets of an n-byte stream over a sorted candidate list: the first candidate in
    [s + mn - 1, s + mx - 1] ends the chunk starting at s, else the chunk is mx bytes (or the
    rest of the stream) -- the walk of resolve_kernel."""
    c = np.asarray(cands, dtype=np.int64)
    cuts, s = [], 0
    while s < n:
        lo = s + mn - 1
        if lo >= n:
            s = n
        else:
            hi = min(s + mx - 1, n - 1)
            i = int(np.searchsorted(c, lo))
            if i < c.size and c[i] <= hi:
                s = int(c[i]) + 1
            elif s + mx - 1 <= n - 1:
                s += mx
            else:
                s = n
        cuts.append(s)
    return np.asarray(cuts, dtype=np.int64)


def segment_stats(cands, off0: int, n: int | None = None):
    """Per 128 KiB coordinate segment ((p + off0) // SEG) of a stream that starts off0 bytes into
    its 16-byte-aligned base: (candidate counts per segment, the "unlisted" candidates -- rank >= 8
    within their segment, which the scan does not store).  With `n` the counts cover every
    segment of the stream, else the segments up to the last candidate's."""
    c = np.asarray(cands, dtype=np.int64)
    seg = (c + off0) // SEG
    nseg = (n + off0 + SEG - 1) // SEG if n is not None else (int(seg[-1]) + 1 if c.size else 0)
    counts = np.bincount(seg, minlength=nseg).astype(np.int64)
    first = np.searchsorted(seg, seg)  # index of each candidate's segment's first candidate
    unlisted = c[np.arange(c.size) - first >= SEG_K]
    return counts, unlisted
