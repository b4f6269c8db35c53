"""Plain-numpy restatement of Kopia's repo/ecc REED-SOLOMON-CRC32 (ecc_rs_crc.go, ecc_utils.go)
and of the coding matrix of klauspost/reedsolomon (Backblaze's construction over GF(2^8), polynomial
0x11d): the test oracle for kopia_amd.ecc.  It imports nothing from kopia_amd; its own anchors are
the rows of tests/golden/ecc_reference.json (tests/test_ecc_model.py)."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

LENGTH_SIZE = 4
CRC_SIZE = 4
SMALL_DATA, SMALL_PARITY = 6, 2

# ---------------------------------------------------------------- GF(2^8)
_EXP = np.zeros(512, np.uint8)
_LOG = np.zeros(256, np.int32)
_x = 1
for _i in range(255):
    _EXP[_i] = _x
    _LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
_EXP[255:510] = _EXP[:255]
# MUL[a, b] = a * b
_a = np.arange(256)
MUL = np.where((_a[:, None] == 0) | (_a[None, :] == 0), 0, _EXP[(_LOG[:, None] + _LOG[None, :]) % 255]).astype(np.uint8)


def gf_inv(a: int) -> int:
    assert a != 0
    return int(_EXP[255 - _LOG[a]])


def gf_exp(a: int, n: int) -> int:
    if n == 0:
        return 1
    if a == 0:
        return 0
    return int(_EXP[(int(_LOG[a]) * n) % 255])


def gf_matmul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(m x k) . (k x n) over GF(2^8)."""
    out = np.zeros((a.shape[0], b.shape[1]), np.uint8)
    for k in range(a.shape[1]):
        out ^= MUL[a[:, k][:, None], b[k][None, :]]
    return out


def gf_invert(m: np.ndarray) -> np.ndarray:
    """Gauss-Jordan inverse of a square matrix over GF(2^8)."""
    n = m.shape[0]
    w = np.concatenate([m.astype(np.uint8), np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        piv = c + int(np.nonzero(w[c:, c])[0][0])  # IndexError: singular
        if piv != c:
            w[[c, piv]] = w[[piv, c]]
        w[c] = MUL[gf_inv(int(w[c, c])), w[c]]
        f = w[:, c].copy()
        f[c] = 0
        w ^= MUL[f[:, None], w[c][None, :]]
    return w[:, n:].copy()


@lru_cache(maxsize=None)
def _full_matrix(data: int, parity: int) -> np.ndarray:
    n = data + parity
    v = np.array([[gf_exp(r, c) for c in range(data)] for r in range(n)], np.uint8)
    return gf_matmul(v, gf_invert(v[:data]))


def matrix(data: int, parity: int) -> np.ndarray:
    """The (data + parity) x data coding matrix: V . (V[0:data])^-1, V[r][c] = r^c."""
    return _full_matrix(data, parity)


def rs_encode(data_shards: np.ndarray, parity: int) -> np.ndarray:
    """data_shards: data x S bytes -> parity x S bytes."""
    d = data_shards.shape[0]
    return gf_matmul(matrix(d, parity)[d:], data_shards)


def rs_reconstruct_data(shards: list, data: int, parity: int) -> list:
    """ReconstructData: shards is a list of data + parity arrays or None; fills the missing data
    shards from the first `data` present ones.  Raises ValueError with too few."""
    present = [i for i, s in enumerate(shards) if s is not None]
    if len(present) < data:
        raise ValueError("too few shards given")
    if all(shards[i] is not None for i in range(data)):
        return shards
    use = present[:data]
    dec = gf_invert(matrix(data, parity)[use])
    sub = np.stack([shards[i] for i in use])
    missing = [i for i in range(data) if shards[i] is None]
    rebuilt = gf_matmul(dec[missing], sub)
    out = list(shards)
    for k, i in enumerate(missing):
        out[i] = rebuilt[k]
    return out


# ---------------------------------------------------------------- parameters and sizes
def ceil_int(a: int, b: int) -> int:
    return int(math.ceil(float(a) / float(b)))


def _between(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _apply_percent(val: int, percent: np.float32) -> int:
    return int(math.floor(float(val) * float(percent)))


def compute_shards(space_overhead) -> tuple[int, int]:
    """computeShards (ecc_utils.go:5-20); float32 where the reference has it."""
    so = np.float32(space_overhead)
    data = 128
    parity = _between(_apply_percent(data, so / np.float32(100)), 1, 128)
    if parity == 1:
        parity = 2
        data = _between(_apply_percent(parity, np.float32(100) / so), 128, 254)
    return data, parity


@dataclass(frozen=True)
class Sizes:
    blocks: int
    shard_size: int
    data: int
    parity: int
    store_padding: bool


class ReedSolomonCrcECC:
    """newReedSolomonCrcECC (ecc_rs_crc.go:37-89) and its methods."""

    def __init__(self, overhead_percent: int, max_shard_size: int = 0):
        ms = max_shard_size
        if ms == 0:
            ms = 1024 if overhead_percent == 1 else 512 if overhead_percent == 2 else 256 if overhead_percent == 3 \
                else 128 if overhead_percent <= 6 else 64
        self.max_shard_size = ms
        free = np.float32(overhead_percent) - np.float32(100 * CRC_SIZE) / np.float32(ms)
        free = max(free, np.float32(0.01))
        self.data, self.parity = compute_shards(free)
        self.threshold_parity_input = 2 * CRC_SIZE * (self.data + self.parity)
        self.threshold_parity_output = (SMALL_DATA + SMALL_PARITY) * (
            CRC_SIZE + ceil_int(self.threshold_parity_input, SMALL_DATA))
        self.threshold_blocks_input = self.data * ms
        self.threshold_blocks_output = (self.data + self.parity) * (CRC_SIZE + ms)

    def info(self) -> tuple:
        return (self.data, self.parity, self.max_shard_size, self.threshold_parity_input,
                self.threshold_parity_output, self.threshold_blocks_input, self.threshold_blocks_output)

    def sizes_from_original(self, length: int) -> Sizes:
        length += LENGTH_SIZE
        if length <= self.threshold_parity_input:
            return Sizes(1, ceil_int(length, SMALL_DATA), SMALL_DATA, SMALL_PARITY, True)
        if length <= self.threshold_blocks_input:
            return Sizes(1, ceil_int(length, self.data), self.data, self.parity, True)
        return Sizes(ceil_int(length, self.data * self.max_shard_size), self.max_shard_size, self.data, self.parity,
                     False)

    def sizes_from_stored(self, length: int) -> Sizes:
        if length <= self.threshold_parity_output:
            s = max(ceil_int(length, SMALL_DATA + SMALL_PARITY), 1 + CRC_SIZE) - CRC_SIZE
            return Sizes(1, s, SMALL_DATA, SMALL_PARITY, True)
        if length <= self.threshold_blocks_output:
            s = max(ceil_int(length, self.data + self.parity), 1 + CRC_SIZE) - CRC_SIZE
            return Sizes(1, s, self.data, self.parity, True)
        return Sizes(ceil_int(length, (self.data + self.parity) * (CRC_SIZE + self.max_shard_size)),
                     self.max_shard_size, self.data, self.parity, False)

    def encoded_size(self, length: int) -> int:
        """computeFinalFileSize (ecc_rs_crc_test.go:171-182)."""
        s = self.sizes_from_original(length)
        if s.store_padding:
            return (s.parity + s.data) * (CRC_SIZE + s.shard_size) * s.blocks
        lp = LENGTH_SIZE + length
        return s.parity * (CRC_SIZE + s.shard_size) * s.blocks + lp + ceil_int(lp, s.shard_size) * CRC_SIZE

    # ------------------------------------------------------------ Encrypt / Decrypt
    def encrypt(self, data: bytes) -> bytes:
        s = self.sizes_from_original(len(data))
        S, D, P = s.shard_size, s.data, s.parity
        buf = np.zeros(D * S * s.blocks, np.uint8)
        buf[:4] = np.frombuffer(len(data).to_bytes(4, "big"), np.uint8)
        buf[4:4 + len(data)] = np.frombuffer(data, np.uint8)
        blocks = buf.reshape(s.blocks, D, S)
        out = bytearray()
        for b in range(s.blocks):
            par = rs_encode(blocks[b], P)
            for p in range(P):
                out += zlib.crc32(par[p].tobytes()).to_bytes(4, "big") + par[p].tobytes()
        to_store = len(buf) if s.store_padding else LENGTH_SIZE + len(data)
        pos = 0
        flat = buf.tobytes()
        while pos < to_store:
            left = min(to_store - pos, S)
            shard = flat[pos:pos + S]
            out += zlib.crc32(shard).to_bytes(4, "big") + shard[:left]
            pos += S
        return bytes(out)

    def encrypt_length(self, length: int) -> int:
        """len(encrypt(data)) for len(data) == length: Encrypt's appends replayed without the bytes."""
        s = self.sizes_from_original(length)
        out = s.blocks * s.parity * (CRC_SIZE + s.shard_size)
        to_store = s.data * s.shard_size * s.blocks if s.store_padding else LENGTH_SIZE + length
        full, rest = divmod(to_store, s.shard_size)
        return out + full * (CRC_SIZE + s.shard_size) + ((CRC_SIZE + rest) if rest else 0)

    def decrypt(self, stored: bytes) -> bytes:
        """Decrypt (ecc_rs_crc.go:254-350); raises ValueError where the reference returns an error
        (too few shards), and also for an in-band length the stored data cannot fill, where the
        reference silently returns fewer bytes."""
        s = self.sizes_from_stored(len(stored))
        S, D, P = s.shard_size, s.data, s.parity
        rec = CRC_SIZE + S
        full = bytearray((D + P) * rec * s.blocks)
        full[:len(stored)] = stored
        par_total = P * rec * s.blocks
        ecc, dat = bytes(full[:par_total]), bytes(full[par_total:])
        padding_start = len(stored) - par_total
        out = bytearray()
        original = 0
        dpos = epos = 0
        for b in range(s.blocks):
            shards = []
            for _ in range(D):
                start = dpos
                crc = int.from_bytes(dat[dpos:dpos + 4], "big")
                sh = dat[dpos + 4:dpos + rec]
                dpos += rec
                if start < padding_start and crc != zlib.crc32(sh):
                    shards.append(None)
                else:
                    shards.append(np.frombuffer(sh, np.uint8))
            for _ in range(P):
                crc = int.from_bytes(ecc[epos:epos + 4], "big")
                sh = ecc[epos + 4:epos + rec]
                epos += rec
                shards.append(np.frombuffer(sh, np.uint8) if crc == zlib.crc32(sh) else None)
            shards = rs_reconstruct_data(shards, D, P)
            block = b"".join(shards[i].tobytes() for i in range(D))
            skip = 0
            if b == 0:
                original = int.from_bytes(block[:4], "big")
                skip = 4
            take = min(original - len(out), D * S - skip)
            if take > 0:
                out += block[skip:skip + take]
        if len(out) != original:
            raise ValueError("in-band length exceeds the stored data")
        return bytes(out)
