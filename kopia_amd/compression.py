"""Content compression of chunks on the GPU (C ABI: include/kcdc.h, kcdc_compress_*),
mirroring Kopia's compression package for the deflate, gzip, pgzip and s2 compressors
(repo/compression/compressor.go: Compressor, HeaderID, ByName; compressor_deflate.go,
compressor_gzip.go, compressor_pgzip.go, compressor_s2.go; compression_ids.go) and the content manager's keep-or-drop rule
(repo/content/content_manager_lock_free.go:42-73: the compressed form is kept only when it is
shorter than the content, else the header ID is NoCompression = 0).  The read path's Decompress
(called by committed_read_manager.go:336) runs on the device for the s2 names
(compressor_s2.go:73-90: decompress_chunks_device) and for the deflate, gzip and pgzip names
(compressor_deflate.go:64-78, compressor_gzip.go:68-85, compressor_pgzip.go: inflate_chunks_device) and
for the zstd names (compressor_zstd.go:73-91: zstd_decode_chunks_device).
No CPU fallback for the byte path: the library must be loaded."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

NoCompression = 0  # repo/content/content_manager.go:37
compressionHeaderSize = 4  # compressor.go:15


def SupportedAlgorithms() -> list[str]:
    arr = (C.c_char_p * 64)()
    n = _lib.lib().kcdc_compression_algorithms(arr, 64)
    return [arr[i].decode() for i in range(n)]


def DecompressibleAlgorithms() -> list[str]:
    """The names whose streams decompress_chunks_device decodes (the s2 compressors)."""
    arr = (C.c_char_p * 64)()
    n = _lib.lib().kcdc_decompression_algorithms(arr, 64)
    return [arr[i].decode() for i in range(n)]


def InflatableAlgorithms() -> list[str]:
    """The names whose streams inflate_chunks_device decodes (deflate-*, gzip*, pgzip*)."""
    arr = (C.c_char_p * 64)()
    n = _lib.lib().kcdc_inflate_algorithms(arr, 64)
    return [arr[i].decode() for i in range(n)]


def ZstdDecodableAlgorithms() -> list[str]:
    """The names whose streams zstd_decode_chunks_device decodes (the four zstd* compressors)."""
    arr = (C.c_char_p * 64)()
    n = _lib.lib().kcdc_zstd_decode_algorithms(arr, 64)
    return [arr[i].decode() for i in range(n)]


def HeaderID(name: str) -> int:
    return _lib.check(_lib.lib().kcdc_compression_header_id(name.encode()))


def compress_bound(length: int) -> int:
    return int(_lib.lib().kcdc_compress_bound(int(length)))


def compressed_layout(lengths):
    """Offsets and total size of an output buffer with room for every chunk's bound."""
    bounds = np.array([compress_bound(int(n)) for n in np.asarray(lengths, dtype=np.int64)], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(bounds)[:-1])).astype(np.int64) if len(bounds) else np.zeros(0, np.int64)
    return offs, max(int(bounds.sum()), 1)


class Compressor:
    """ByName[name] for the GPU: the batch form of Compress (plus the content manager's rule)."""

    def __init__(self, name: str):
        if name not in SupportedAlgorithms():
            raise _lib.KcdcError(_lib.KCDC_ENOENT, f"unknown compression algorithm: {name}")
        self.name = name
        self.header_id = HeaderID(name)

    def HeaderID(self) -> int:
        return self.header_id

    def compress_chunks_device(self, data_ptr: int, offsets, lengths, d_out, out_offsets, device, stream=None):
        """Compress chunk i = [offsets[i], +lengths[i]) of the device bytes at data_ptr into d_out
        (a device uint8 tensor) at out_offsets[i] (room for compress_bound(lengths[i]) bytes).
        Returns device tensors (out_lens int64, header_ids int32): header_ids[i] is this
        compressor's ID when the compressed form is shorter than the chunk, else 0.
        Asynchronous on `stream`."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        lens = np.asarray(lengths, dtype=np.int64)
        # Temporaries are allocated and filled on `stream` itself (the kernels run there), and
        # out_lens / ids need no fill: the frame kernel writes every entry.
        with torch.cuda.stream(stream):
            out_lens = torch.empty(max(n, 1), dtype=torch.int64, device=device)
            ids = torch.empty(max(n, 1), dtype=torch.int32, device=device)
            if n == 0:
                return out_lens[:0], ids[:0]
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(lens).to(device)
            d_oo = torch.as_tensor(np.asarray(out_offsets, dtype=np.int64)).to(device)
            wb = int(_lib.lib().kcdc_compress_workspace_size(int(lens.sum()), n))
            work = torch.empty(max(wb, 1), dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().kcdc_compress_chunks_device(
            self.name.encode(), C.c_void_p(data_ptr), d_offs.data_ptr(), d_lens.data_ptr(), n, d_out.data_ptr(),
            d_oo.data_ptr(), out_lens.data_ptr(), ids.data_ptr(), work.data_ptr(), work.numel(),
            C.c_void_p(stream.cuda_stream)))
        out_lens._kcdc_keep = (d_offs, d_lens, d_oo, work)  # alive until the caller syncs
        return out_lens[:n], ids[:n]

    def decompress_chunks_device(self, comp_ptr: int, offsets, lengths, d_out, out_offsets, out_caps, device,
                                 stream=None, work_bytes: int | None = None):
        """Decompress content i = [offsets[i], +lengths[i]) of the device bytes at comp_ptr (the
        4-byte header ID, then the stream, as compress_chunks_device writes them) into d_out (a
        device uint8 tensor) at out_offsets[i], at most out_caps[i] bytes.
        Returns device tensors (out_lens int64, status int32): status[i] is 0 with out_lens[i] the
        decoded length, or KCDC_EBADMSG (wrong header ID, malformed stream, CRC mismatch),
        KCDC_EOVERFLOW (longer than the cap) or KCDC_ENOMEM (more data chunks than one per 16 KiB
        of cap, plus one) with out_lens[i] = 0.  work_bytes: a workspace larger than
        kcdc_decompress_workspace_size, for contents with more data chunks than that (every content
        gets an equal share of the extra descriptors).  Asynchronous on `stream`."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        lens = np.asarray(lengths, dtype=np.int64)
        caps = np.asarray(out_caps, dtype=np.int64)
        # Temporaries are allocated and filled on `stream` itself (the kernels run there);
        # out_lens / status need no fill: the kernels write every entry.
        with torch.cuda.stream(stream):
            out_lens = torch.empty(max(n, 1), dtype=torch.int64, device=device)
            status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(lens).to(device)
            d_oo = torch.as_tensor(np.asarray(out_offsets, dtype=np.int64)).to(device)
            d_caps = torch.as_tensor(caps).to(device)
            wb = int(_lib.lib().kcdc_decompress_workspace_size(int(lens.sum()), int(caps.sum()), n))
            if work_bytes is not None:
                wb = int(work_bytes)
            work = torch.empty(max(wb, 8), dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().kcdc_decompress_chunks_device(
            self.name.encode(), C.c_void_p(comp_ptr), d_offs.data_ptr(), d_lens.data_ptr(), n, d_out.data_ptr(),
            d_oo.data_ptr(), d_caps.data_ptr(), out_lens.data_ptr(), status.data_ptr(), work.data_ptr(), wb,
            C.c_void_p(stream.cuda_stream)))
        out_lens._kcdc_keep = (d_offs, d_lens, d_oo, d_caps, work)  # alive until the caller syncs
        return out_lens[:n], status[:n]

    def inflate_chunks_device(self, comp_ptr: int, offsets, lengths, d_out, out_offsets, out_caps, device, stream=None):
        """decompress_chunks_device for the deflate-*, gzip* and pgzip* names: content i =
        [offsets[i], +lengths[i]) of the device bytes at comp_ptr (the 4-byte header ID, then a raw
        deflate stream or gzip members, from any writer) into d_out at out_offsets[i], at most
        out_caps[i] bytes.  Returns device tensors (out_lens int64, status int32): status[i] is 0
        with out_lens[i] the decoded length, or KCDC_EBADMSG (wrong header ID, malformed or
        truncated stream or member, CRC-32 or ISIZE mismatch) or KCDC_EOVERFLOW (longer than the
        cap) with out_lens[i] = 0.  Asynchronous on `stream`."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        with torch.cuda.stream(stream):
            out_lens = torch.empty(max(n, 1), dtype=torch.int64, device=device)
            status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(np.asarray(lengths, dtype=np.int64)).to(device)
            d_oo = torch.as_tensor(np.asarray(out_offsets, dtype=np.int64)).to(device)
            d_caps = torch.as_tensor(np.asarray(out_caps, dtype=np.int64)).to(device)
            wb = int(_lib.lib().kcdc_inflate_workspace_size(n))
            work = torch.empty(max(wb, 8), dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().kcdc_inflate_chunks_device(
            self.name.encode(), C.c_void_p(comp_ptr), d_offs.data_ptr(), d_lens.data_ptr(), n, d_out.data_ptr(),
            d_oo.data_ptr(), d_caps.data_ptr(), out_lens.data_ptr(), status.data_ptr(), work.data_ptr(), wb,
            C.c_void_p(stream.cuda_stream)))
        out_lens._kcdc_keep = (d_offs, d_lens, d_oo, d_caps, work)  # alive until the caller syncs
        return out_lens[:n], status[:n]

    def zstd_decode_chunks_device(self, comp_ptr: int, offsets, lengths, d_out, out_offsets, out_caps, device,
                                  stream=None, work_bytes: int | None = None):
        """decompress_chunks_device for the zstd* names (zstd.NewReader behind compressor_zstd.go:73-91):
        content i = [offsets[i], +lengths[i]) of the device bytes at comp_ptr (the 4-byte header ID,
        then RFC 8878 frames from any writer) into d_out at out_offsets[i], at most out_caps[i] bytes.
        Returns device tensors (out_lens int64, status int32): status[i] is 0 with out_lens[i] the
        decoded length, or KCDC_EBADMSG (wrong header ID, malformed or truncated frame, content-size
        or checksum mismatch), KCDC_EOVERFLOW (longer than the cap) or KCDC_ENOMEM (more blocks and
        frames than 4 + cap / 1 KiB descriptors) with out_lens[i] = 0.  work_bytes: a workspace larger
        than kcdc_zstd_decode_workspace_size, for contents with more blocks than that (every content
        gets an equal share of the extra descriptors); without it, zstd-fastest takes the room that
        this library's own zstd-fastest frames need.  Asynchronous on `stream`."""
        import torch
        n = len(offsets)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        lens = np.asarray(lengths, dtype=np.int64)
        caps = np.asarray(out_caps, dtype=np.int64)
        with torch.cuda.stream(stream):
            out_lens = torch.empty(max(n, 1), dtype=torch.int64, device=device)
            status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
            d_offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).to(device)
            d_lens = torch.as_tensor(lens).to(device)
            d_oo = torch.as_tensor(np.asarray(out_offsets, dtype=np.int64)).to(device)
            d_caps = torch.as_tensor(caps).to(device)
            wb = int(_lib.lib().kcdc_zstd_decode_workspace_size(int(lens.sum()), int(caps.sum()), n))
            if self.name == "zstd-fastest" and n:
                # this library's own zstd-fastest frames hold a block per 512 bytes, two per KiB: beyond the
                # rule's 4 + cap / 1 KiB, cap / 1 KiB + 2 more descriptors for every content (an equal share each)
                wb += 32 * n * (int(caps.max()) // 1024 + 2)
            if work_bytes is not None:
                wb = int(work_bytes)
            work = torch.empty(max(wb, 8), dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().kcdc_zstd_decode_chunks_device(
            self.name.encode(), C.c_void_p(comp_ptr), d_offs.data_ptr(), d_lens.data_ptr(), n, d_out.data_ptr(),
            d_oo.data_ptr(), d_caps.data_ptr(), out_lens.data_ptr(), status.data_ptr(), work.data_ptr(), wb,
            C.c_void_p(stream.cuda_stream)))
        out_lens._kcdc_keep = (d_offs, d_lens, d_oo, d_caps, work)  # alive until the caller syncs
        return out_lens[:n], status[:n]
