"""Packing chunks on the GPU (C ABI: include/kcdc.h, kcdc_pack_*): what Kopia's content manager does
with a new content between the cut and the pack blob, maybeCompressAndEncryptDataForPacking
(repo/content/content_manager_lock_free.go:30-89) and the append of addToPackUnlocked
(repo/content/content_manager.go:257-353), for many chunks per call: compress with the keep-or-drop
rule, seal, wrap with ECC, and place the stored bytes densely in packs that close once they reach
MaxPackSize.  One asynchronous call; the decisions (header IDs, pack offsets, pack boundaries) stay
on the device until the caller reads the entries.
No CPU fallback for the byte path: the library must be loaded."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

PACK_SKIPPED = _lib.KCDC_PACK_SKIPPED
ENTRY_DTYPE = np.dtype([("pack", "<u4"), ("pack_offset", "<u4"), ("packed_length", "<u4"),
                        ("original_length", "<u4"), ("header_id", "<u4"), ("status", "<i4")])  # kcdc_pack_entry
INFO_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("first", "<u4"), ("count", "<u4")])  # kcdc_pack_info


class Packer:
    """The repository's write-path settings (compressor, encryptor, ECC, MaxPackSize) and the batch
    form of "compress, encrypt and append to the pack"."""

    def __init__(self, encryption: str, secret: bytes, max_pack_size: int, compression: str | None = None,
                 ecc: str | None = None, ecc_overhead_percent: int = 0, ecc_max_shard_size: int = 0,
                 pack_lead: int = 0, open_fill: int = 0, max_total_bytes: int = 0):
        self.secret = bytes(secret)
        self.params = _lib.PackParams(
            compression.encode() if compression else None, encryption.encode(), self.secret, len(self.secret),
            ecc.encode() if ecc else None, int(ecc_overhead_percent), int(ecc_max_shard_size), int(max_pack_size),
            int(pack_lead), int(open_fill), int(max_total_bytes))

    def with_total(self, max_total_bytes: int) -> "Packer":
        """The same settings with another bound on the sum of the packed chunks' lengths."""
        p = Packer.__new__(Packer)
        p.secret = self.secret
        p.params = _lib.PackParams()
        C.pointer(p.params)[0] = self.params
        p.params.max_total_bytes = int(max_total_bytes)
        p._parent = self  # owns the name strings the copied pointers refer to
        return p

    def bounds(self, nchunks: int) -> tuple[int, int, int]:
        """(bytes of d_pack, rows of d_packs, bytes of workspace) that no call over nchunks chunks
        of at most max_total_bytes in all exceeds (kcdc_pack_bounds)."""
        pb, mp, wb = C.c_uint64(), C.c_uint32(), C.c_uint64()
        _lib.check(_lib.lib().kcdc_pack_bounds(C.byref(self.params), int(nchunks), C.byref(pb), C.byref(mp),
                                               C.byref(wb)))
        return int(pb.value), int(mp.value), int(wb.value)

    def pack_chunks_raw(self, data_ptr, d_offsets, d_lens, d_keep, n, d_ids, id_len, id_stride, d_nonces, pack_ptr,
                        pack_cap, d_entries, d_packs, packs_cap, d_totals, work_ptr, work_bytes, stream) -> int:
        """kcdc_pack_chunks_device with the caller's own device buffers (pointers as ints, tensors
        for the tables); returns the call's return code unchecked."""
        ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        return _lib.lib().kcdc_pack_chunks_device(
            C.byref(self.params), ptr(data_ptr), ptr(d_offsets), ptr(d_lens), ptr(d_keep), int(n), ptr(d_ids),
            int(id_len), int(id_stride), ptr(d_nonces), ptr(pack_ptr), int(pack_cap), ptr(d_entries), ptr(d_packs),
            int(packs_cap), ptr(d_totals), ptr(work_ptr), int(work_bytes), C.c_void_p(stream.cuda_stream))

    def pack_chunks_device(self, data_ptr: int, offsets, lengths, d_ids, d_nonces, device, keep=None, stream=None,
                           id_len: int = 16, id_stride: int | None = None):
        """Pack chunk i = [offsets[i], +lengths[i]) of the device bytes at data_ptr; d_ids: the
        content IDs (device uint8, id_stride bytes apart), d_nonces: 12 bytes per chunk; keep: an
        optional 0/1 mask, a host array or a device uint8 tensor (ContentSet.claim's, still being
        computed on `stream`).  max_total_bytes is taken from the kept lengths; with a device
        mask the host cannot know them and takes every admissible length, a valid bound.
        Returns device tensors (d_pack uint8, entries int32[n, 6], packs uint8[rows, 24], totals
        int64[2]); read entries and packs with entries_numpy / packs_numpy after synchronising.
        Asynchronous on `stream`."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        lens = np.asarray(lengths, dtype=np.int64)
        on_device = hasattr(keep, "data_ptr")
        if on_device and (keep.dtype != torch.uint8 or keep.dim() != 1 or keep.shape[0] != n
                          or not keep.is_contiguous() or not keep.is_cuda):
            raise ValueError("keep: a contiguous device uint8 tensor of one byte per chunk")
        mask = None if keep is None or on_device else np.asarray(keep, dtype=np.uint8)
        kept = lens if mask is None else lens[mask != 0]
        run = self.with_total(int(kept[kept <= (1 << 30) - 64].sum()))
        pack_bytes, max_packs, wb = run.bounds(n)
        with torch.cuda.stream(stream):
            d_pack = torch.empty(max(pack_bytes, 1), dtype=torch.uint8, device=device)
            entries = torch.empty((max(n, 1), 6), dtype=torch.int32, device=device)
            packs = torch.empty((max(max_packs, 1), 24), dtype=torch.uint8, device=device)
            totals = torch.empty(2, dtype=torch.int64, device=device)
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(lens).to(device)
            d_keep = keep if on_device else None if mask is None else torch.as_tensor(mask).to(device)
            work = torch.empty(wb + 256, dtype=torch.uint8, device=device)
        wp = (work.data_ptr() + 255) & ~255
        _lib.check(run.pack_chunks_raw(data_ptr, d_offs, d_lens, d_keep, n, d_ids, id_len,
                                       id_len if id_stride is None else id_stride, d_nonces, d_pack, pack_bytes,
                                       entries, packs, max_packs, totals, wp, wb, stream))
        totals._kcdc_keep = (d_offs, d_lens, d_keep, work, run)  # alive until the caller syncs
        return d_pack, entries[:n], packs, totals


def entries_numpy(entries) -> np.ndarray:
    """Device entries (int32[n, 6]) as a structured host array (ENTRY_DTYPE); synchronises."""
    return np.ascontiguousarray(entries.cpu().numpy()).view(ENTRY_DTYPE).reshape(-1)


def packs_numpy(packs, count: int) -> np.ndarray:
    """The first `count` device pack rows (uint8[rows, 24]) as a structured host array (INFO_DTYPE)."""
    return np.ascontiguousarray(packs[:count].cpu().numpy()).view(INFO_DTYPE).reshape(-1)
