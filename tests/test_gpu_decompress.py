"""GPU: S2 decompression of many contents per call (kcdc_decompress_chunks_device), the read path's
Decompress (compressor_s2.go:73-90 behind committed_read_manager.go:336).

The device's own streams must come back byte for byte; other writers' streams (the oracle's 64 KiB
blocks, Google's Snappy blocks in Snappy framing, uncompressed / skippable / padding / identifier
chunks) and hand-built blocks with every element form at its seams (tests/test_s2_vectors.py: the
builder and the model decoder that defines the expected bytes) must decode to the model's bytes;
every corrupt content must get its status and a zero length without disturbing its neighbours or a
byte outside its slot (0xAB guards around every slot).  Every hand-built vector goes through the
sanitizer-built host program (tools/s2_decode_host.cpp) before it is sent to the device."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import test_s2_vectors as sv
from kopia_amd import _lib
from kopia_amd import compression as kc
from oracle import deflate

pytestmark = pytest.mark.gpu
GUARD = 0xAB
S2 = list(deflate.S2_NAMES)


@pytest.fixture(scope="module")
def checked():
    """The CPU run of every vector, under the host sanitizers, before any of them is uploaded."""
    res = sv.run_host_program()
    for v in sv.valid_vectors():
        assert res[v.id] == (0, len(v.expected), True), v.id
    for v in sv.corrupt_vectors():
        assert res[v.id] == (v.status, 0, True), v.id
    return res


def _decompress(name, blobs, caps, dev, work_bytes=None):
    """Decode `blobs` in one call: contents packed at odd offsets, output slots at odd offsets with
    a guard before and after each.  Returns (output bytes, slot offsets, lengths, statuses) after
    checking every byte outside the slots.  work_bytes: a workspace above the minimum size."""
    import torch
    comp, offs = bytearray(), []
    for i, b in enumerate(blobs):  # content i starts at an odd offset: 1, 3, 5, 7 mod 8 in turn
        comp += bytes(1 + (2 * i - len(comp)) % 8)
        offs.append(len(comp))
        comp += b
    comp += bytes(8)
    out_offs, total = [], 0
    for i, c in enumerate(caps):  # slots at 3, 1, 7, 5 mod 8 in turn, 32 guard bytes or more between them
        total += 32 + (3 - 2 * i - total) % 8
        out_offs.append(total)
        total += c
    total += 64
    d_comp = torch.from_numpy(np.frombuffer(bytes(comp), np.uint8).copy()).to(dev)
    d_out = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    lens, st = kc.Compressor(name).decompress_chunks_device(d_comp.data_ptr(), offs, [len(b) for b in blobs], d_out,
                                                            out_offs, caps, dev, work_bytes=work_bytes)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    outside = np.ones(total, bool)
    for o, c in zip(out_offs, caps):
        outside[o:o + c] = False
    assert (out[outside] == GUARD).all(), "a byte outside the output slots was written"
    assert all(o % 2 for o in offs) and all(o % 2 for o in out_offs)
    return out, out_offs, lens.cpu().numpy(), st.cpu().numpy()


def _expect(vectors, out, out_offs, lens, st):
    for i, v in enumerate(vectors):
        assert st[i] == v.status, (v.id, st[i])
        assert lens[i] == len(v.expected), (v.id, lens[i])
        got = out[out_offs[i]:out_offs[i] + lens[i]].tobytes()
        if got != v.expected:
            first = next(k for k in range(len(got)) if got[k] != v.expected[k])
            raise AssertionError(f"{v.id}: first wrong byte at {first} of {len(got)}")


@pytest.mark.parametrize("name", S2)
def test_own_streams_round_trip(name, gpu):
    """Compress on the device, decompress on the device: lengths around the 512-byte segments and
    the 32 KiB spans, an empty content and a multi-span one, mixed data, odd offsets both ways."""
    import torch
    sizes = [0, 1, 511, 512, 513, 32767, 32768, 32769, 65537, (1 << 20) + 3]
    host = np.frombuffer(sv.mixed(sum(sizes) + 64, 31), np.uint8)
    offs = [int(x) for x in np.cumsum([3] + sizes[:-1])]
    d = torch.from_numpy(host.copy()).to(gpu)
    oo, total = kc.compressed_layout(sizes)
    comp = torch.zeros(total + 16, dtype=torch.uint8, device=gpu)
    clens, ids = kc.Compressor(name).compress_chunks_device(d.data_ptr(), offs, sizes, comp, oo, gpu)
    torch.cuda.synchronize()
    clens = clens.cpu().numpy()
    comp_host = comp.cpu().numpy()
    blobs = [comp_host[o:o + n].tobytes() for o, n in zip(oo, clens)]
    out, out_offs, lens, st = _decompress(name, blobs, sizes, gpu)
    assert not st.any(), st
    assert lens.tolist() == sizes
    for i, (o, n) in enumerate(zip(offs, sizes)):
        assert out[out_offs[i]:out_offs[i] + n].tobytes() == host[o:o + n].tobytes(), (name, n)


def test_other_writers_and_element_seams(gpu, checked):
    """Every valid vector of tests/test_s2_vectors.py in one call per header ID: the oracle's
    writer, Snappy framing, the other chunk types, every literal length form, copy-1 / copy-2 /
    copy-4 at their extremes, overlapping copies either side of the wave width, all repeat classes,
    blocks of 32768 and 32769 bytes, 1 MiB and 4 MiB blocks (the CRC combined from pieces)."""
    for name in sorted({v.name for v in sv.valid_vectors()}):
        vs = [v for v in sv.valid_vectors() if v.name == name]
        out, out_offs, lens, st = _decompress(name, [v.blob for v in vs], [v.cap for v in vs], gpu)
        _expect(vs, out, out_offs, lens, st)
    ids = {v.id for v in sv.valid_vectors()}
    assert {"block-32768", "block-32769", "block-4MiB", "snappy-framed-200000", "mixed-chunk-types"} <= ids


def test_corrupt_contents_among_good_ones(gpu, checked):
    """Each corrupt content between good neighbours in one call, with a workspace of the minimum
    size: its status, a zero length, exact neighbours, guards intact."""
    good = [v for v in sv.valid_vectors() if v.name == sv.NAME and len(v.blob) < 70000]
    bad = sv.corrupt_vectors()
    assert len(bad) >= 17
    vs = []
    for i, b in enumerate(bad):
        vs += [good[i % len(good)], b]
    vs.append(good[-1])
    out, out_offs, lens, st = _decompress(sv.NAME, [v.blob for v in vs], [v.cap for v in vs], gpu)
    _expect(vs, out, out_offs, lens, st)
    seen = {v.status for v in bad}
    assert seen == {sv.EBADMSG, sv.EOVERFLOW, sv.ENOMEM}


@pytest.fixture
def chunk_grid(request):
    """At most this many workgroups (waves) in the persistent block decode (KCDC_TEST_CHUNK_GRID)."""
    L = _lib.lib()
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, request.param) == 0
    yield request.param
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, 0) == 0


@pytest.mark.parametrize("chunk_grid", (1, 3), indirect=True)
def test_one_wave_decodes_every_vector(chunk_grid, gpu, checked):
    """One wave (or three) takes every block ticket of a call, in block order with one: every valid
    vector of at most 70,000 decoded bytes, per header ID, a corrupt one after each good one while
    they last (a workspace of the minimum size, as the corrupt vectors' statuses assume).  The wave
    that has just refused a block decodes the next content's block with the input window and repeat
    offset it still holds: every content exact, guards intact."""
    seen, took_part = set(), 0
    for name in sorted({v.name for v in sv.valid_vectors()}):
        good = [v for v in sv.valid_vectors() if v.name == name and len(v.expected) <= 70000]
        bad = [v for v in sv.corrupt_vectors() if v.name == name]
        if not good:
            assert not bad
            continue
        assert len(good) > len(bad)
        vs = []
        for i, g in enumerate(good):
            vs += [g] + bad[i:i + 1]
        assert {v.id for v in bad} <= {v.id for v in vs}
        out, out_offs, lens, st = _decompress(name, [v.blob for v in vs], [v.cap for v in vs], gpu)
        _expect(vs, out, out_offs, lens, st)
        seen |= {v.status for v in bad}
        took_part += len(good)
    assert took_part >= 55
    assert seen == {sv.EBADMSG, sv.EOVERFLOW, sv.ENOMEM}


def test_larger_workspace_gives_more_descriptors(gpu, checked):
    """The descriptor room comes from work_bytes: the 1000-chunk stream that a minimum workspace
    refuses decodes when the caller passes room for its chunks."""
    import torch
    v = next(x for x in sv.corrupt_vectors() if x.status == sv.ENOMEM)
    L = _lib.lib()
    d_comp = torch.from_numpy(np.frombuffer(v.blob, np.uint8).copy()).to(gpu)
    d_out = torch.full((v.cap + 8,), GUARD, dtype=torch.uint8, device=gpu)
    meta = torch.tensor([0, len(v.blob), 0, v.cap], dtype=torch.int64, device=gpu)
    lens = torch.zeros(1, dtype=torch.int64, device=gpu)
    st = torch.zeros(1, dtype=torch.int32, device=gpu)
    wb = int(L.kcdc_decompress_workspace_size(len(v.blob), v.cap, 1)) + 1000 * 32
    work = torch.empty(wb, dtype=torch.uint8, device=gpu)
    p = meta.data_ptr()
    _lib.check(L.kcdc_decompress_chunks_device(sv.NAME.encode(), d_comp.data_ptr(), p, p + 8, 1, d_out.data_ptr(), p + 16,
                                               p + 24, lens.data_ptr(), st.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    assert st.item() == 0 and lens.item() == 1000
    out = d_out.cpu().numpy()
    assert out[:1000].tobytes() == bytes(k & 255 for k in range(1000)) and (out[1000:] == GUARD).all()


def test_read_path(gpu):
    """compress (s2-default) -> seal -> open -> decompress what was kept compressed -> hash: the
    bytes and the content IDs of the originals."""
    import torch

    from kopia_amd import encryption as ke
    from kopia_amd import hashing as kh
    parts = [sv.mixed(70001, 41), sv.rand(40000, 42), sv.mixed(33000, 43), sv.rand(100, 44), sv.mixed(5, 45)]
    sizes = [len(p) for p in parts]
    host = b"".join(parts)
    offs = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    d = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).to(gpu)
    key = bytes(range(32))
    ids = kh.hash_chunks_device(kh.DefaultAlgorithm, d.data_ptr(), offs, sizes, key, gpu).contiguous()
    comp = kc.Compressor("s2-default")
    oo, total = kc.compressed_layout(sizes)
    packed = torch.zeros(len(host) + total, dtype=torch.uint8, device=gpu)  # the originals, then the streams
    packed[:len(host)] = d
    clens, kept = comp.compress_chunks_device(d.data_ptr(), offs, sizes, packed[len(host):], oo, gpu)
    torch.cuda.synchronize()
    clens, kept = clens.cpu().numpy(), kept.cpu().numpy()
    assert kept[0] and kept[2] and not kept[1]  # random data is stored as it is
    # what the content manager stores: the stream where it was kept, else the content
    p_offs = [len(host) + int(oo[i]) if kept[i] else offs[i] for i in range(len(sizes))]
    p_lens = [int(clens[i]) if kept[i] else sizes[i] for i in range(len(sizes))]
    enc = ke.Encryptor(ke.ChaCha20Poly1305, bytes(range(50, 82)))
    so, stotal = ke.sealed_layout(p_lens)
    sealed = torch.zeros(stotal, dtype=torch.uint8, device=gpu)
    st = enc.encrypt_chunks_device(packed.data_ptr(), p_offs, p_lens, ids, ids.stride(0), sealed, so, gpu)
    ke.raise_on_status(st)
    # the read path
    s_lens = [n + enc.Overhead() for n in p_lens]
    po, ptotal = ke.plain_layout(s_lens)
    opened = torch.zeros(ptotal, dtype=torch.uint8, device=gpu)
    ke.raise_on_status(enc.decrypt_chunks_device(sealed.data_ptr(), so, s_lens, ids, ids.stride(0), opened, po, gpu))
    pick = [i for i in range(len(sizes)) if kept[i]]
    r_offs = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    restored = torch.zeros(len(host), dtype=torch.uint8, device=gpu)
    lens, st = comp.decompress_chunks_device(opened.data_ptr(), [int(po[i]) for i in pick], [p_lens[i] for i in pick],
                                             restored, [r_offs[i] for i in pick], [sizes[i] for i in pick], gpu)
    for i in range(len(sizes)):
        if not kept[i]:
            restored[r_offs[i]:r_offs[i] + sizes[i]] = opened[int(po[i]):int(po[i]) + sizes[i]]
    ids2 = kh.hash_chunks_device(kh.DefaultAlgorithm, restored.data_ptr(), r_offs, sizes, key, gpu)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and lens.cpu().numpy().tolist() == [sizes[i] for i in pick]
    assert restored.cpu().numpy().tobytes() == host
    assert torch.equal(ids2.cpu(), ids.cpu())
    want = hashlib.blake2b(parts[0], key=key, digest_size=32).digest()[:16]
    assert ids2[0].cpu().numpy().tobytes() == want


def test_argument_errors(gpu):
    import torch
    L = _lib.lib()
    with pytest.raises(_lib.KcdcError) as e:
        kc.Compressor("no-such-compressor")
    assert e.value.code == _lib.KCDC_ENOENT
    t = torch.zeros(64, dtype=torch.uint8, device=gpu)
    p = C.c_void_p(t.data_ptr())
    args = (p, p, p, 1, p, p, p, p, p, p, 64, None)
    assert L.kcdc_decompress_chunks_device(b"no-such-compressor", *args) == _lib.KCDC_ENOENT
    assert L.kcdc_decompress_chunks_device(b"deflate-default", *args) == _lib.KCDC_EINVAL
    assert "deflate-default" in _lib.last_error()
    with pytest.raises(_lib.KcdcError) as e:
        kc.Compressor("deflate-default").decompress_chunks_device(t.data_ptr(), [0], [8], t, [0], [8], gpu)
    assert e.value.code == _lib.KCDC_EINVAL
    # nothing to do: no launch, nothing written
    assert L.kcdc_decompress_chunks_device(b"s2-default", *args[:3], 0, *args[4:]) == 0
    lens, st = kc.Compressor("s2-default").decompress_chunks_device(t.data_ptr(), [], [], t, [], [], gpu)
    torch.cuda.synchronize()
    assert lens.numel() == 0 and st.numel() == 0 and not t.cpu().numpy().any()
    # a workspace below the fixed fields is an argument error, not a launch
    assert L.kcdc_decompress_chunks_device(b"s2-default", *args[:10], 8, None) == _lib.KCDC_EINVAL
