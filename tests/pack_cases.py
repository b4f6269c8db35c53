"""Inputs shared by tests/test_pack_model.py (CPU: the plan's decisions against the literal loop)
and tests/test_gpu_pack.py (GPU: kcdc_pack_chunks_device over the same shapes).  No tests here.

A Vec is one call seen by the plan: lengths, mask, the lengths of the compressed forms (0: no
compressor ran) and the parameters.  seam_vectors() holds the placement seams: packs that reach
max_pack_size exactly and stop one byte short, a content larger than a pack, 36-byte chunks (64
stored bytes) that fill packs of 4096 and 8192 with exactly 64 and 128 contents, more than 64 packs,
leads 0 and 37, every open_fill shape, the last pack open and closed."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import ecc_model as em
import pack_model as pm

GAP = 13  # the least distance between two source chunks
# the byte-exact case of tests/test_gpu_pack.py
_EXACT = ([0, 1, 2, 3, 4, 5, 15, 16, 17] + list(range(27, 34)) + [63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537,
                                                                  (1 << 17) + 1])
EXACT_LENS = _EXACT + _EXACT[::-1]  # forwards, then backwards: the pack offsets then reach every residue mod 16
EXACT_PACK_SIZES = (4096, 1 << 20)
ECC_OPTS = ((2, 0), (10, 0))


@dataclass
class Vec:
    lengths: list
    max_pack_size: int
    lead: int = 0
    open_fill: int = 0
    keep: list | None = None
    comp_lens: list | None = None
    header_id: int = 0
    ecc: tuple | None = None  # (overhead percent, max shard size)
    max_total: int | None = None
    pack_cap: int | None = None
    packs_cap: int | None = None
    tag: str = ""

    def model(self) -> pm.Result:
        return pm.pack(self.lengths, self.keep, self.comp_lens, self.header_id, self.max_pack_size, self.lead,
                       self.open_fill, ecc_of(self.ecc), self.max_total, self.pack_cap, self.packs_cap)

    def true_total(self) -> int:
        keep = self.keep or [1] * len(self.lengths)
        return sum(int(n) for n, k in zip(self.lengths, keep) if pm.status_of(int(n), bool(k)) == pm.PACKED)


def ecc_of(opt):
    return None if opt is None else em.ReedSolomonCrcECC(*opt)


def sources(lengths, seed=7):
    """(host bytes, offsets) of chunks of these lengths at unaligned source offsets, half text-like."""
    rng = np.random.default_rng(seed)
    offs, pos = [], GAP
    for i, n in enumerate(lengths):
        pos += (5 * i + 1 - pos) % 16  # chunk i starts at residue 5 i + 1 mod 16: every residue within 16 chunks
        offs.append(pos)
        pos += int(n) + GAP
    host = rng.integers(0, 256, pos + GAP, dtype=np.uint8)
    words = np.frombuffer(b"the quick brown fox jumps over the lazy dog and packs its contents densely ", np.uint8)
    for i, (o, n) in enumerate(zip(offs, lengths)):
        if i % 2 == 0 and n:
            host[o:o + n] = np.resize(words, int(n))
    return host, np.array(offs, np.int64)


def seam_vectors() -> list[Vec]:
    out = []
    shapes = [
        ("exact64", [36] * 200, 4096),            # 64 stored bytes each: packs of exactly 64 contents
        ("exact128", [36] * 300, 8192),           # ... and 128
        ("short1", [36] * 63 + [35] + [36] * 5, 4096),   # 4095 after 64 contents: one more goes in
        ("large", [10, 10000, 10, 20000], 4096),  # a content larger than a pack
        ("many", [36] * 200, 100),                # 100 packs
        ("closed", [36] * 128, 4096),             # the last pack closed
        ("open", [36] * 129, 4096),               # the last pack open
    ]
    for tag, lens, mps in shapes:
        for lead in (0, 37):
            for fill in (0, 1, mps - 1, mps - 64):
                out.append(Vec(lens, mps, lead, fill, tag=f"{tag}-lead{lead}-fill{fill}"))
    return out


def mask_vectors() -> list[Vec]:
    lens = [40, 0, 100, 36, 1, 77, 300, 36, 36, 5]
    n = len(lens)
    return [
        Vec([], 4096, tag="empty"),
        Vec(lens, 256, keep=[0] * n, tag="all-skipped"),
        Vec(lens, 256, keep=[0] + [1] * (n - 1), tag="first-skipped"),
        Vec(lens, 256, keep=[1] * (n - 1) + [0], tag="last-skipped"),
        Vec(lens, 256, keep=[i & 1 for i in range(n)], lead=37, tag="alternate-skipped"),
    ]


def refusal_vectors() -> list[Vec]:
    lens = [100, 200, 36, 36, 36, 4000, 1, 0, 50]
    base = Vec(lens, 512, lead=37)
    r = base.model()
    big = Vec([50, pm.SEAL_MAX_LEN + 1, 60, 70], 512, tag="efbig")
    return [
        Vec(lens, 512, lead=37, max_total=sum(lens) - 1, tag="enomem"),
        Vec(lens, 512, lead=37, max_total=sum(lens), tag="total-exact"),
        Vec(lens, 512, lead=37, pack_cap=r.totals[1] - 1, tag="pack-cap-short"),
        Vec(lens, 512, lead=37, pack_cap=r.totals[1], tag="pack-cap-exact"),
        Vec(lens, 512, lead=37, packs_cap=r.totals[0] - 1, tag="packs-cap-short"),
        Vec(lens, 512, lead=37, packs_cap=r.totals[0], tag="packs-cap-exact"),
        big,
    ]


def ecc_lengths(opt) -> list[int]:
    """Chunk lengths whose sealed forms sit on both sides of the ECC's two thresholds and in the
    multi-block range."""
    m = em.ReedSolomonCrcECC(*opt)
    over = pm.SEAL_OVERHEAD + em.LENGTH_SIZE
    a, b = m.threshold_parity_input - over, m.threshold_blocks_input - over
    return [0, 5, a - 1, a, a + 1, b - 1, b, b + 1, 2 * m.threshold_blocks_input + 77]


def ecc_vectors() -> list[Vec]:
    return [Vec(ecc_lengths(o), mps, lead=37, ecc=o, tag=f"ecc{o[0]}-{mps}") for o in ECC_OPTS for mps in (4096, 1 << 20)]


def random_vectors(count=200, seed=2024) -> list[Vec]:
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 300))
        lens = rng.choice([0, 1, 36, 100, 1000, 5000], n).astype(np.int64) + rng.integers(0, 40, n)
        lens[rng.random(n) < 0.1] = 0
        if n and rng.random() < 0.1:
            lens[int(rng.integers(0, n))] = pm.SEAL_MAX_LEN + int(rng.integers(1, 3))
        keep = None if rng.random() < 0.4 else (rng.random(n) < 0.8).astype(int).tolist()
        comp = None
        if rng.random() < 0.5:
            comp = [int(max(5, x * rng.uniform(0.3, 1.2))) for x in lens]
        mps = int(rng.choice([1, 64, 100, 4096, 20000, 1 << 20]))
        lead = int(rng.choice([0, 37, mps, mps + 5]))
        fill = int(rng.choice([0, 1, mps - 1, mps // 2])) if mps > 1 else 0
        ecc = [None, (2, 0), (10, 0), (2, 1024)][int(rng.integers(0, 4))]
        v = Vec(lens.tolist(), mps, lead, fill, keep, comp, 0x1100 if comp else 0, ecc, tag=f"random{k}")
        r = v.model()
        pick = rng.random()
        if pick < 0.1 and v.true_total():
            v.max_total = v.true_total() - 1
        elif pick < 0.2 and r.totals[0]:
            v.packs_cap = r.totals[0] - int(rng.integers(0, 2))
        elif pick < 0.3 and r.totals[1]:
            v.pack_cap = r.totals[1] - int(rng.integers(0, 2))
        out.append(v)
    return out


def all_vectors() -> list[Vec]:
    return seam_vectors() + mask_vectors() + refusal_vectors() + ecc_vectors() + random_vectors()
