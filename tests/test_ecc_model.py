"""CPU: the numpy model of repo/ecc (tests/ecc_model.py) against the reference's own rows
(tests/golden/ecc_reference.json: stored sizes, computeShards, the 5+5 Reed-Solomon known-answer
vector), and the library's host-side ECC entry points (kcdc_ecc_params / _encoded_size /
_decoded_bound / _matrix) against the model for every overhead and shard size."""
import ctypes as C

import numpy as np
import pytest

import ecc_model as em
from conftest import golden
from kopia_amd import _lib
from kopia_amd import ecc as kecc

REF = golden("ecc_reference.json")
ALG = b"REED-SOLOMON-CRC32"
SHARD_SIZES = (0, 64, 128, 256, 512, 1024)
MATRIX_SHAPES = [(6, 2), (128, 2), (164, 2), (254, 2), (128, 12), (128, 120), (5, 5)]


def edge_lengths(m: em.ReedSolomonCrcECC):
    """The lengths at which Encrypt's geometry changes (the GPU tests encode the same set)."""
    t = m.threshold_parity_input - 4
    block = m.data * m.max_shard_size
    b = block - 4
    return [0, 1, 2, 3, 8, 9, 14, 15, 20, 21, 26, t, t + 1, 10240, b, b + 1, 2 * block - 4, 2 * block - 3, 1 << 20]


def pattern(n: int) -> bytes:
    return (np.arange(n, dtype=np.int64) % 255 + 1).astype(np.uint8).tobytes()  # testPutAndGet


def test_model_reference_sizes():
    for r in REF["sizes"]:
        m = em.ReedSolomonCrcECC(r["overhead_percent"], r["max_shard_size"])
        n = r["original_size"]
        data = pattern(n)
        stored = m.encrypt(data)
        assert len(stored) == n + r["ecc_size"] == m.encoded_size(n)
        assert m.decrypt(stored) == data


def test_model_compute_shards():
    for r in REF["compute_shards"]:
        assert em.compute_shards(r["space_overhead"]) == (r["data"], r["parity"])


def test_model_rs_vector():
    v = REF["rs_vector"]
    data = np.array(v["data"], np.uint8)
    assert em.rs_encode(data, v["parity_shards"]).tolist() == v["parity"]
    got = kecc.matrix(v["data_shards"], v["parity_shards"])
    assert em.gf_matmul(got, data).tolist() == v["parity"]


def test_supported_algorithms():
    assert kecc.SupportedAlgorithms() == ["REED-SOLOMON-CRC32"] == [kecc.AlgorithmReedSolomonWithCrc32]
    assert _lib.lib().kcdc_ecc_default_algorithm().decode() == kecc.DefaultAlgorithm


@pytest.mark.parametrize("ms", SHARD_SIZES)
def test_params_and_sizes_match_model(ms):
    L = _lib.lib()
    for o in range(1, 101):
        m = em.ReedSolomonCrcECC(o, ms)
        info = _lib.EccInfo()
        assert L.kcdc_ecc_params(ALG, o, ms, C.byref(info)) == 0
        got = (info.data_shards, info.parity_shards, info.max_shard_size, info.threshold_parity_input,
               info.threshold_parity_output, info.threshold_blocks_input, info.threshold_blocks_output)
        assert got == m.info(), (o, ms)
        for n in edge_lengths(m):
            size = L.kcdc_ecc_encoded_size(ALG, o, ms, n)
            assert size == m.encrypt_length(n) == m.encoded_size(n), (o, ms, n)
            # AssertSizeAlwaysGrow's second half (ecc_rs_crc_test.go:36-42), at the edges
            assert m.sizes_from_stored(size) == m.sizes_from_original(n), (o, ms, n)
            bound = L.kcdc_ecc_decoded_bound(ALG, o, ms, size)
            s = m.sizes_from_original(n)
            assert n <= bound <= n + s.data * s.shard_size, (o, ms, n)


@pytest.mark.parametrize("o,ms", [(2, 1024), (10, 1024), (1, 0), (10, 0), (100, 0)])
def test_encoded_size_is_model_output_length(o, ms):
    m = em.ReedSolomonCrcECC(o, ms)
    for n in edge_lengths(m):
        assert _lib.lib().kcdc_ecc_encoded_size(ALG, o, ms, n) == len(m.encrypt(pattern(n))) == m.encrypt_length(n), \
            (o, ms, n)


@pytest.mark.parametrize("d,p", MATRIX_SHAPES)
def test_matrix_matches_model_and_decodes(d, p):
    full = em.matrix(d, p)
    assert (full[:d] == np.eye(d, dtype=np.uint8)).all()
    assert (kecc.matrix(d, p) == full[d:]).all()
    rng = np.random.default_rng(d * 1000 + p)
    data = rng.integers(0, 256, (d, 7), dtype=np.uint8)
    shards = list(data) + list(em.rs_encode(data, p))
    for _ in range(3):
        keep = set(rng.choice(d + p, d, replace=False).tolist())
        got = em.rs_reconstruct_data([s if i in keep else None for i, s in enumerate(shards)], d, p)
        assert (np.stack(got[:d]) == data).all()
    with pytest.raises(ValueError):
        em.rs_reconstruct_data([None] * (p + 1) + shards[p + 1:], d, p)


def test_bad_arguments():
    L = _lib.lib()
    info = _lib.EccInfo()
    assert L.kcdc_ecc_params(b"NOPE", 2, 0, C.byref(info)) == _lib.KCDC_ENOENT
    assert L.kcdc_ecc_encoded_size(b"NOPE", 2, 0, 10) == _lib.KCDC_ENOENT
    assert L.kcdc_ecc_decoded_bound(b"NOPE", 2, 0, 100) == _lib.KCDC_ENOENT
    for o in (0, 101):
        assert L.kcdc_ecc_params(ALG, o, 0, C.byref(info)) == _lib.KCDC_EINVAL
        assert L.kcdc_ecc_encoded_size(ALG, o, 0, 10) == _lib.KCDC_EINVAL
    assert L.kcdc_ecc_params(ALG, 2, -1, C.byref(info)) == _lib.KCDC_EINVAL
    assert L.kcdc_ecc_params(ALG, 2, 0, None) == _lib.KCDC_EINVAL
    assert L.kcdc_ecc_matrix(6, 2, None) == _lib.KCDC_EINVAL
    assert L.kcdc_ecc_matrix(200, 100, np.zeros(20000, np.uint8).ctypes.data) == _lib.KCDC_EINVAL
    assert L.kcdc_ecc_encoded_size(ALG, 2, 0, (1 << 32) - 4) == _lib.KCDC_EFBIG
    assert L.kcdc_ecc_encoded_size(ALG, 2, 0, (1 << 32) - 5) > (1 << 32)
    with pytest.raises(_lib.KcdcError):
        kecc.CreateAlgorithm(kecc.Options(Algorithm="NOPE", OverheadPercent=2))
