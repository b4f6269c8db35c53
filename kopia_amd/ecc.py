"""Error correction of chunks on the GPU (C ABI: include/kcdc.h, kcdc_ecc_*), mirroring Kopia's
ecc package for REED-SOLOMON-CRC32 (repo/ecc/ecc.go: SupportedAlgorithms, CreateAlgorithm,
CreateEncryptor; ecc_options.go: Options; ecc_rs_crc.go: ReedSolomonCrcECC).  Many chunks per launch,
in the place of encryptorWrapper (repo/format/encryptor_wrapper.go): encode what the encryptor
sealed, decode (and, for damaged chunks, repair) before it opens.
No CPU fallback for the byte path: the library must be loaded."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

AlgorithmReedSolomonWithCrc32 = "REED-SOLOMON-CRC32"  # ecc_rs_crc.go:16
DefaultAlgorithm = AlgorithmReedSolomonWithCrc32  # ecc_options.go DefaultAlgorithm
Damaged = _lib.KCDC_ECC_DAMAGED


def SupportedAlgorithms() -> list[str]:
    arr = (C.c_char_p * 4)()
    n = _lib.lib().kcdc_ecc_algorithms(arr, 4)
    return [arr[i].decode() for i in range(n)]


@dataclass
class Options:
    """ecc_options.go Options."""
    Algorithm: str = DefaultAlgorithm
    OverheadPercent: int = 0
    MaxShardSize: int = 0  # 0: chosen by OverheadPercent


def matrix(data_shards: int, parity_shards: int) -> np.ndarray:
    """The parity rows of the coding matrix, parity x data."""
    out = np.zeros((parity_shards, data_shards), np.uint8)
    _lib.check(_lib.lib().kcdc_ecc_matrix(data_shards, parity_shards, out.ctypes.data))
    return out


def _layout(sizes):
    sizes = np.asarray(sizes, dtype=np.int64)
    slots = (sizes + 3) & ~3
    offs = np.concatenate(([0], np.cumsum(slots)[:-1])).astype(np.int64) if len(slots) else np.zeros(0, np.int64)
    return offs, max(int(slots.sum()), 4)


class ReedSolomonCrcECC:
    """CreateAlgorithm(opts) for the GPU: the batch forms of Encrypt / Decrypt."""

    def __init__(self, opts: Options):
        self.opts = opts
        self._alg = opts.Algorithm.encode()
        info = _lib.EccInfo()
        _lib.check(_lib.lib().kcdc_ecc_params(self._alg, opts.OverheadPercent, opts.MaxShardSize, C.byref(info)))
        self.DataShards, self.ParityShards = info.data_shards, info.parity_shards
        self.MaxShardSize = info.max_shard_size
        self.ThresholdParityInput, self.ThresholdParityOutput = info.threshold_parity_input, info.threshold_parity_output
        self.ThresholdBlocksInput, self.ThresholdBlocksOutput = info.threshold_blocks_input, info.threshold_blocks_output

    def _p(self):
        return self._alg, self.opts.OverheadPercent, self.opts.MaxShardSize

    def encoded_size(self, length: int) -> int:
        return _lib.check(_lib.lib().kcdc_ecc_encoded_size(*self._p(), int(length)))

    def decoded_bound(self, stored_length: int) -> int:
        return _lib.check(_lib.lib().kcdc_ecc_decoded_bound(*self._p(), int(stored_length)))

    def stored_layout(self, lengths):
        """(offsets, stored sizes, total) of a buffer holding every encoded chunk."""
        sizes = np.array([self.encoded_size(n) for n in lengths], np.int64)
        offs, total = _layout(sizes)
        return offs, sizes, total

    def plain_layout(self, stored_lengths):
        """(offsets, total) of the output slots for decoding chunks of these stored sizes."""
        return _layout([self.decoded_bound(n) for n in stored_lengths])

    def encrypt_chunks_device(self, data_ptr: int, offsets, lengths, d_out, out_offsets, device, stream=None):
        """Encode chunk i = [offsets[i], +lengths[i]) of the device bytes at data_ptr into d_out (a
        device uint8 tensor) at out_offsets[i], encoded_size(lengths[i]) bytes.  Returns the device
        int32 status tensor (asynchronous on `stream`)."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        with torch.cuda.stream(stream):  # temporaries ordered on the kernels' stream
            status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
            if n == 0:
                return status[:0]
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(np.asarray(lengths, dtype=np.int64)).to(device)
            d_oo = torch.as_tensor(np.asarray(out_offsets, dtype=np.int64)).to(device)
        _lib.check(_lib.lib().kcdc_ecc_encode_chunks_device(
            *self._p(), C.c_void_p(data_ptr), d_offs.data_ptr(), d_lens.data_ptr(), n, d_out.data_ptr(),
            d_oo.data_ptr(), status.data_ptr(), C.c_void_p(stream.cuda_stream)))
        status._kcdc_keep = (d_offs, d_lens, d_oo)  # alive until the caller syncs
        return status[:n]

    def decrypt_chunks_device(self, stored_ptr: int, offsets, stored_lengths, d_out, out_offsets, device, stream=None):
        """Check stored chunk i = [offsets[i], +stored_lengths[i]) and copy its data to d_out at
        out_offsets[i] (a slot of decoded_bound bytes).  Returns a Decoded: .status (0,
        KCDC_ECC_DAMAGED, KCDC_EBADMSG, KCDC_EINVAL) and .out_lens device tensors, asynchronous on
        `stream`; .repair() rebuilds the damaged chunks."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        with torch.cuda.stream(stream):
            status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
            out_lens = torch.empty(max(n, 1), dtype=torch.int64, device=device)
            if n == 0:
                return Decoded(self, None, status[:0], out_lens[:0], stream)
            lens = np.asarray(stored_lengths, dtype=np.int64)
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(lens).to(device)
            d_oo = torch.as_tensor(np.asarray(out_offsets, dtype=np.int64)).to(device)
            wb = int(_lib.lib().kcdc_ecc_workspace_size(int(lens.sum()), n))
            work = torch.empty(wb, dtype=torch.uint8, device=device)
        args = (*self._p(), C.c_void_p(stored_ptr), d_offs.data_ptr(), d_lens.data_ptr(), n, d_out.data_ptr(),
                d_oo.data_ptr(), out_lens.data_ptr(), status.data_ptr(), work.data_ptr(), work.numel(),
                C.c_void_p(stream.cuda_stream))
        _lib.check(_lib.lib().kcdc_ecc_decode_chunks_device(*args))
        dec = Decoded(self, args, status[:n], out_lens[:n], stream)
        dec._keep = (d_offs, d_lens, d_oo, work, d_out)
        return dec

    @staticmethod
    def repair(decoded: "Decoded"):
        """The repair step of a decrypt_chunks_device result (Decoded.repair)."""
        return decoded.repair()


class Decoded:
    """What decrypt_chunks_device returns: the statuses and lengths, and the repair step."""

    def __init__(self, ecc, args, status, out_lens, stream):
        self.ecc, self._args, self.status, self.out_lens, self.stream = ecc, args, status, out_lens, stream

    def repair(self):
        """ReconstructData for the chunks left KCDC_ECC_DAMAGED: waits for the stream, rebuilds
        their missing data shards on the device and settles status and out_lens; a chunk past
        repair gets KCDC_EBADMSG and a zeroed slot.  Synchronous; no-op for a clean launch."""
        if self._args is not None:
            _lib.check(_lib.lib().kcdc_ecc_repair_chunks_device(*self._args))
        return self.status


def CreateAlgorithm(opts: Options) -> ReedSolomonCrcECC:
    """ecc.go:37-46."""
    if opts.Algorithm not in SupportedAlgorithms():
        raise _lib.KcdcError(_lib.KCDC_ENOENT, "Unknown ECC algorithm: " + opts.Algorithm)
    return ReedSolomonCrcECC(opts)


def CreateEncryptor(algorithm: str, overhead_percent: int) -> ReedSolomonCrcECC:
    """ecc.go:54-60: Parameters carry the algorithm and the overhead only."""
    return CreateAlgorithm(Options(Algorithm=algorithm, OverheadPercent=overhead_percent))
