"""CPU: the structure of the many-chunk population (tests/many_chunks.py) that
tests/test_gpu_many_chunks.py runs every per-chunk entry point over, pinned so that a later edit
cannot drop an edge, and the oracles' acceptance of every chunk of it."""
import numpy as np
import pytest

import ecc_model as em
import many_chunks as mc
import test_s2_vectors as sv
from oracle import deflate, openssl_aead
from oracle.hashes import kopia_hash

SEED = mc.SEED


@pytest.mark.parametrize("n", mc.COUNTS)
def test_population_structure(n):
    host, offs, lens = mc.population(n, SEED)
    assert len(offs) == len(lens) == n
    # the zero runs: the first three, across the 1024 seam, the last three
    assert mc.zero_runs(n)[:3] == [0, 1, 2] and mc.zero_runs(n)[-3:] == [n - 3, n - 2, n - 1]
    assert {i for i in mc.SEAM if i < n} <= set(mc.zero_runs(n)) and min(mc.SEAM) < 1024 <= max(mc.SEAM)
    assert {1022, 1023, 1024} <= set(mc.zero_runs(n))  # at 1025 chunks the seam run is the call's end too
    assert not lens[mc.zero_runs(n)].any() and lens[-1] == 0
    assert lens[3] > 0 and lens[1021] > 0 and lens[n - 4] > 0  # the runs are bounded by chunks with bytes
    if n > mc.after_seam():
        assert lens[mc.after_seam()] > 0  # the lookups must step over the whole seam run to this chunk
    scattered = int((lens == 0).sum()) - len(mc.zero_runs(n))
    assert 0.03 * n <= scattered <= 0.07 * n, scattered
    # large chunks: every 257th index, several units / spans / blocks each
    large = mc.large_indices(lens)
    assert len(large) >= 2 and large == [i for i in range(257, n, 257)]
    assert all(lens[i] == 70000 + i % 7 for i in large)
    small = np.delete(lens, large)
    assert small.max() == mc.SMALL_MAX and set(small.tolist()) >= set(range(0, 97, 5))
    # packed with gaps of 1..3 bytes, nothing overlaps, every alignment mod 16
    gaps = offs[1:] - (offs[:-1] + lens[:-1])
    assert offs[0] in (1, 2, 3) and set(gaps.tolist()) == {1, 2, 3}
    assert {int(o) % 16 for o, m in zip(offs, lens) if m} == set(range(16))
    assert {int(o) % 16 for o in offs[large]} != {0}
    assert host.size >= offs[-1] + lens[-1] and host.size <= 1_100_000
    # the same call, again: the population is a fixed function of (n, seed)
    again = mc.population.__wrapped__(n, SEED)
    assert all((a == b).all() for a, b in zip(again, (host, offs, lens)))


def test_slots_and_guards():
    for align in (1, 4):
        sizes = [0, 5, 0, 0, 33, 1, 70001, 0]
        offs, total = mc.slots(sizes, align)
        ends = offs + np.asarray(sizes)
        assert offs[0] >= mc.GAP and (offs[1:] - ends[:-1] >= mc.GAP).all() and total - ends[-1] >= mc.GAP
        assert all(o % align == 0 for o in offs)
        buf = np.full(total, 0xAB, np.uint8)
        for o, s in zip(offs, sizes):
            buf[o:o + s] = 7
        assert mc.outside_intact(buf, offs, sizes, 0xAB)
        for at in (0, int(offs[1]) - 1, int(ends[1]), int(offs[3]), total - 1):  # offs[3]: an empty slot owns no byte
            bad = buf.copy()
            bad[at] ^= 1
            assert not mc.outside_intact(bad, offs, sizes, 0xAB), at
    assert len({int(o) % 16 for o in mc.slots([3] * 200)[0]}) == 16


@pytest.mark.parametrize("n", mc.COUNTS)
def test_oracles_accept_every_chunk(n):
    """Every oracle the GPU tests compare with takes every chunk of the population: both OpenSSL
    AEADs, the six content hashes, the ECC model at both option sets (encode, and decode back),
    zlib, libzstd and the S2 oracle behind the reference's framing, and the S2 model over the
    64-byte-block Snappy framing the decompression test feeds the device."""
    assert openssl_aead.available(), "libcrypto.so.3 is the seal oracle of tests/test_gpu_many_chunks.py"
    pop = mc.population(n, SEED)
    lens = pop[2]
    chunks = [mc.chunk(pop, i) for i in range(n)]
    assert [len(c) for c in chunks] == lens.tolist()
    secret, iv, nonce = bytes(range(32)), bytes(range(16)), bytes(range(12))
    for alg in (openssl_aead.AES, openssl_aead.CHACHA):
        s = openssl_aead.Sealer(alg)
        for c in chunks:
            sealed = s.kopia_encrypt(secret, iv, nonce, c)
            assert len(sealed) == len(c) + 28 and sealed[:12] == nonce
    for name in ("BLAKE2B-256-128", "BLAKE2S-128", "HMAC-SHA256", "HMAC-SHA3-224", "BLAKE3-256-128"):
        sizes = {len(kopia_hash(name, secret, c)) for c in chunks}
        assert sizes == {28 if name == "HMAC-SHA3-224" else 16 if name.endswith("128") else 32}, name
    large = set(mc.large_indices(lens))
    for o, ms in ((2, 1024), (10, 0)):
        m = em.ReedSolomonCrcECC(o, ms)
        assert {m.sizes_from_original(int(lens[i])).blocks for i in large} == ({1} if ms else {9})
        for i, c in enumerate(chunks):
            stored = m.encrypt(c)
            assert len(stored) == m.encoded_size(len(c))
            if n == mc.COUNTS[0] or i in large or i % 16 == 0:
                assert m.decrypt(stored) == c, i
    for name in ("deflate-default", "gzip", "s2-default", "zstd"):
        for i in sorted(large) + list(range(0, n, 8)):
            assert deflate.decompress(name, deflate.compress(name, chunks[i])) == chunks[i], (name, i)
    for i in range(1, n, 2):
        blob = sv.content(sv.snappy_framed(chunks[i], block_size=64))
        blocks = -(-len(chunks[i]) // 64)
        assert sv.model_decode(blob, sv.NAME, len(chunks[i]), blocks)[:2] == (0, chunks[i]), i
        if blocks:
            assert sv.model_decode(blob, sv.NAME, len(chunks[i]), blocks - 1)[0] == sv.ENOMEM
