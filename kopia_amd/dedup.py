"""The dedup decision on the GPU (C ABI: include/kcdc.h, kcdc_dedup_*): WriteContent's lookup between
hashData and addToPackUnlocked (repo/content/content_manager.go:812-842) for many chunks per call.  A
ContentSet holds the content IDs the repository already has in device memory; claim() turns a batch
of digests, read where kcdc_hash_chunks_device left them, into the keep mask that
Packer.pack_chunks_device takes, with the sequential semantics of the reference and no host round
trip.  Calls on one set must be ordered by the caller (one stream, or events).
No CPU fallback: the library must be loaded."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

KNOWN = _lib.KCDC_DEDUP_KNOWN
ENOSPC = _lib.KCDC_ENOSPC


def _prefix(prefix) -> int:
    if isinstance(prefix, (str, bytes)):
        prefix = prefix.encode() if isinstance(prefix, str) else prefix
        if len(prefix) > 1:
            raise ValueError("a content ID prefix is one letter or empty")
        return prefix[0] if prefix else 0
    return int(prefix)


def set_bytes(id_len: int, max_keys: int) -> int:
    """Device memory a set of this shape takes (kcdc_dedup_bytes)."""
    b = _lib.lib().kcdc_dedup_bytes(int(id_len), int(max_keys))
    if b == 0:
        raise _lib.KcdcError(_lib.KCDC_EINVAL, _lib.last_error())
    return int(b)


class ContentSet:
    """Up to max_keys content IDs of id_len hash bytes (plus the one-letter prefix) on one device."""

    def __init__(self, device, id_len: int = 16, max_keys: int = 1 << 20):
        import torch
        self.device = torch.device(device)
        index = self.device.index if self.device.index is not None else 0
        h = _lib.lib().kcdc_dedup_new(index, int(id_len), int(max_keys))
        if not h:
            raise _lib.KcdcError(_lib.KCDC_EINVAL, _lib.last_error())
        self._h = h
        self.id_len, self.max_keys = int(id_len), int(max_keys)

    @classmethod
    def new(cls, device, id_len: int = 16, max_keys: int = 1 << 20) -> "ContentSet":
        return cls(device, id_len, max_keys)

    def close(self) -> None:
        """Free the set's device memory; the caller has waited for the calls on it."""
        if self._h:
            _lib.lib().kcdc_dedup_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _stream(self, stream):
        import torch
        return torch.cuda.current_stream(self.device) if stream is None else stream

    def _ids(self, ids, n, id_stride):
        """(pointer, n, stride) of the IDs: a uint8 tensor [n, >= id_len] whose rows may be further
        apart than they are long (a view of the hash output), or a flat uint8 tensor with n and
        id_stride given (ID i at ids[i * id_stride:], any alignment)."""
        if ids.dim() == 2:
            if ids.shape[1] < self.id_len or (ids.shape[1] > 1 and ids.stride(1) != 1):
                raise ValueError("ids: rows of at least id_len contiguous bytes")
            rows = ids.shape[0] if n is None else int(n)
            return ids.data_ptr(), rows, (ids.stride(0) if id_stride is None else int(id_stride))
        if n is None or id_stride is None:
            raise ValueError("a flat ids tensor needs n and id_stride")
        return ids.data_ptr(), int(n), int(id_stride)

    # ---- calls
    def claim(self, ids, prefix=0, n=None, id_stride=None, stream=None, want_first: bool = True):
        """The WriteContent decision for the IDs in index order.  Returns device tensors (keep
        uint8[n], first int32[n] or None, totals int64[3]): keep[i] = 1 iff ID i is new to the set
        and to the IDs before it; first[i] the lowest index of the call with an equal ID, or
        KNOWN (read it with first_numpy); totals = (0 or ENOSPC, keys newly stored, keys stored).
        Asynchronous on `stream`."""
        import torch
        ptr, n, stride = self._ids(ids, n, id_stride)
        stream = self._stream(stream)
        with torch.cuda.stream(stream):
            keep = torch.empty(n, dtype=torch.uint8, device=self.device)
            first = torch.empty(n, dtype=torch.int32, device=self.device) if want_first else None
            totals = torch.empty(3, dtype=torch.int64, device=self.device)
        _lib.check(self.claim_raw(ptr, stride, n, keep, first, totals, stream, prefix))
        totals._kcdc_keep = (ids,)  # alive until the caller syncs
        return keep, first, totals

    def claim_raw(self, ids_ptr, id_stride, n, d_keep, d_first, d_totals, stream, prefix=0) -> int:
        """kcdc_dedup_claim_device with the caller's own device buffers (pointers as ints, or
        tensors); returns the call's return code unchecked."""
        ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        return _lib.lib().kcdc_dedup_claim_device(self._h, _prefix(prefix), ptr(ids_ptr), int(id_stride), int(n),
                                                  ptr(d_keep), ptr(d_first), ptr(d_totals),
                                                  C.c_void_p(stream.cuda_stream))

    def insert(self, ids, prefix=0, n=None, id_stride=None, stream=None):
        """claim without the per-ID outputs (loading the committed index); returns totals."""
        import torch
        ptr, n, stride = self._ids(ids, n, id_stride)
        stream = self._stream(stream)
        with torch.cuda.stream(stream):
            totals = torch.empty(3, dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().kcdc_dedup_insert_device(self._h, _prefix(prefix), C.c_void_p(ptr), stride, n,
                                                       C.c_void_p(totals.data_ptr()), C.c_void_p(stream.cuda_stream)))
        totals._kcdc_keep = (ids,)
        return totals

    def lookup(self, ids, prefix=0, n=None, id_stride=None, stream=None):
        """known uint8[n]: 1 iff ID i is in the set; the set is unchanged."""
        import torch
        ptr, n, stride = self._ids(ids, n, id_stride)
        stream = self._stream(stream)
        with torch.cuda.stream(stream):
            known = torch.empty(n, dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().kcdc_dedup_lookup_device(self._h, _prefix(prefix), C.c_void_p(ptr), stride, n,
                                                       C.c_void_p(known.data_ptr()), C.c_void_p(stream.cuda_stream)))
        known._kcdc_keep = (ids,)
        return known

    def grow(self, to: "ContentSet", stream=None):
        """Insert every key of this set into `to` (the way to enlarge a full set); returns totals."""
        import torch
        stream = self._stream(stream)
        with torch.cuda.stream(stream):
            totals = torch.empty(3, dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().kcdc_dedup_grow_device(self._h, to._h, C.c_void_p(totals.data_ptr()),
                                                     C.c_void_p(stream.cuda_stream)))
        return totals

    def clear(self, stream=None) -> None:
        _lib.check(_lib.lib().kcdc_dedup_clear_device(self._h, C.c_void_p(self._stream(stream).cuda_stream)))

    def count(self, stream=None) -> int:
        """Keys stored; waits for `stream`."""
        return _lib.check(_lib.lib().kcdc_dedup_count(self._h, C.c_void_p(self._stream(stream).cuda_stream)))


def first_numpy(first) -> np.ndarray:
    """A claim's `first` as host uint32 (KNOWN for IDs the set had); synchronises."""
    return first.cpu().numpy().view(np.uint32)
