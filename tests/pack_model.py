"""The literal loop of addToPackUnlocked (repo/content/content_manager.go:257-353) over a batch of
contents, with the stored size of a content from its sealed length (+28) and tests/ecc_model.py:
the test oracle for kcdc_pack_chunks_device and for tools/pack_plan_host.cpp.  It imports nothing
from kopia_amd and holds no scan and no bisection; no tests here.

    info.PackOffset = pp.currentPackData.Length()
    append(compressedAndEncrypted)
    info.PackedLength = pp.currentPackData.Length() - info.PackOffset
    if pp.currentPackData.Length() >= mp.MaxPackSize: write the pack; the next content opens a new one

A new pack's length starts at `lead` (the format bytes and the preamble the host writes); pack 0 of a
call may continue an open pack of length `open_fill`."""
from __future__ import annotations

from dataclasses import dataclass

SEAL_OVERHEAD = 28
SEAL_MAX_LEN = (1 << 30) - 64  # kcdc_encrypt_chunks_device: a longer chunk is KCDC_EFBIG
PACK_ALIGN = 256
PACKED, SKIPPED, EFBIG, ENOMEM, EOVERFLOW = 0, 1, -27, -12, -75


@dataclass
class Result:
    entries: list  # (pack, pack_offset, packed_length, original_length, header_id, status) per chunk
    packs: list    # (start, length, first, count) per pack
    totals: tuple  # (packs, bytes of d_pack used)
    stored_total: int  # stored bytes of the packed contents (for the bounds checks)


def stored_size(plain_len: int, ecc) -> int:
    """Bytes of pack for a content of plain_len bytes (compressed or original); ecc: an
    ecc_model.ReedSolomonCrcECC or None."""
    sealed = plain_len + SEAL_OVERHEAD
    return ecc.encoded_size(sealed) if ecc is not None else sealed


def status_of(length: int, keep: bool) -> int:
    return SKIPPED if not keep else EFBIG if length > SEAL_MAX_LEN else PACKED


def pack(lengths, keep, comp_lens, header_id, max_pack_size, lead=0, open_fill=0, ecc=None, max_total=None,
         pack_cap=None, packs_cap=None) -> Result:
    """comp_lens[i]: the length of chunk i's compressed form with its 4 header bytes, or 0 when no
    compressor ran; it is kept iff it is shorter than the chunk."""
    n = len(lengths)
    keep = [True] * n if keep is None else [bool(k) for k in keep]
    comp_lens = [0] * n if comp_lens is None else comp_lens
    status = [status_of(int(lengths[i]), keep[i]) for i in range(n)]
    refused = lambda code: Result([(0, 0, 0, int(lengths[i]) & 0xFFFFFFFF, 0, code) for i in range(n)], [], (0, 0), 0)
    if max_total is not None and sum(int(lengths[i]) for i in range(n) if status[i] == PACKED) > max_total:
        return refused(ENOMEM)

    entries, packs = [], []
    cur = None  # the pending pack: [length, first, count]
    first_pack = True
    stored_total = 0
    for i in range(n):
        if status[i] != PACKED:
            entries.append((0, 0, 0, int(lengths[i]) & 0xFFFFFFFF, 0, status[i]))
            continue
        kept = comp_lens[i] != 0 and comp_lens[i] < lengths[i]
        stored = stored_size(int(comp_lens[i] if kept else lengths[i]), ecc)
        stored_total += stored
        if cur is None:  # getOrCreatePendingPackInfoLocked
            cur = [open_fill if first_pack and open_fill else lead, i, 0]
            first_pack = False
        pack_offset = cur[0]
        cur[0] += stored
        cur[2] += 1
        entries.append((len(packs), pack_offset, stored, int(lengths[i]), header_id if kept else 0, PACKED))
        if cur[0] >= max_pack_size:  # shouldWrite
            packs.append(tuple(cur))
            cur = None
    if cur is not None:
        packs.append(tuple(cur))

    rows, start, end = [], 0, 0
    for length, first, count in packs:
        rows.append((start, length, first, count))
        end = start + length
        start = -(-end // PACK_ALIGN) * PACK_ALIGN
    if (packs_cap is not None and len(rows) > packs_cap) or (pack_cap is not None and end > pack_cap):
        return refused(EOVERFLOW)
    return Result(entries, rows, (len(rows), end), stored_total)
