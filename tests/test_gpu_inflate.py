"""GPU: inflate of many contents per call (kcdc_inflate_chunks_device), the read path's Decompress
for the deflate-*, gzip* and pgzip* names (compressor_deflate.go:64-78, compressor_gzip.go:68-85,
compressor_pgzip.go behind committed_read_manager.go:336).

The device's own streams must come back byte for byte; a foreign writer's streams (zlib: every
block type, level, strategy and flush mode) and hand-built streams at the decoder's seams
(tests/inflate_vectors.py; zlib defines the expected bytes) must decode to zlib's bytes; every
corrupt content must get its status and a zero length without disturbing its neighbours or a byte
outside its slot (0xAB guards around every slot).  Every vector goes through the sanitizer-built
host program (tools/inflate_host.cpp) before it is sent to the device."""
import ctypes as C

import numpy as np
import pytest

import inflate_vectors as iv
from kopia_amd import _lib
from kopia_amd import compression as kc

pytestmark = pytest.mark.gpu
GUARD = 0xAB


@pytest.fixture(scope="module")
def checked():
    """The CPU run of every vector, under the host sanitizers, before any of them is uploaded."""
    res = iv.run_host_program()
    for v in iv.valid_vectors():
        assert res[v.id] == (0, len(v.expected), True), v.id
    for v in iv.corrupt_vectors():
        assert res[v.id] == (v.status, 0, True), v.id
    return res


def _inflate(name, blobs, caps, dev):
    """Decode `blobs` in one call: contents packed at odd offsets, output slots at odd offsets with
    a guard before and after each.  Returns (output bytes, slot offsets, lengths, statuses) after
    checking every byte outside the slots."""
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
    lens, st = kc.Compressor(name).inflate_chunks_device(d_comp.data_ptr(), offs, [len(b) for b in blobs], d_out,
                                                         out_offs, caps, dev)
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


@pytest.mark.parametrize("name", iv.NINE)
def test_own_streams_round_trip(name, gpu):
    """Compress on the device, inflate on the device: lengths around the 512-byte segments and the
    32 KiB spans, an empty content and a multi-span one, mixed data, odd offsets both ways: stored,
    fixed and dynamic spans and, for gzip and pgzip, the device's own CRC-32."""
    import torch
    sizes = [0, 1, 511, 512, 513, 32767, 32768, 32769, 65537, (1 << 20) + 3]
    host = np.frombuffer(iv.mixed(sum(sizes) + 64, 31), np.uint8)
    offs = [int(x) for x in np.cumsum([3] + sizes[:-1])]
    d = torch.from_numpy(host.copy()).to(gpu)
    oo, total = kc.compressed_layout(sizes)
    comp = torch.zeros(total + 16, dtype=torch.uint8, device=gpu)
    clens, ids = kc.Compressor(name).compress_chunks_device(d.data_ptr(), offs, sizes, comp, oo, gpu)
    torch.cuda.synchronize()
    clens = clens.cpu().numpy()
    comp_host = comp.cpu().numpy()
    blobs = [comp_host[o:o + n].tobytes() for o, n in zip(oo, clens)]
    out, out_offs, lens, st = _inflate(name, blobs, sizes, gpu)
    assert not st.any(), st
    assert lens.tolist() == sizes
    for i, (o, n) in enumerate(zip(offs, sizes)):
        assert out[out_offs[i]:out_offs[i] + n].tobytes() == host[o:o + n].tobytes(), (name, n)


def test_foreign_and_built_vectors(gpu, checked):
    """Every valid vector of tests/inflate_vectors.py, one call per name."""
    names = sorted({v.name for v in iv.valid_vectors()})
    assert names == sorted(iv.FAMILIES)
    for name in names:
        vs = [v for v in iv.valid_vectors() if v.name == name]
        out, out_offs, lens, st = _inflate(name, [v.blob for v in vs], [v.cap for v in vs], gpu)
        _expect(vs, out, out_offs, lens, st)


def test_corrupt_contents_among_good_ones(gpu, checked):
    """Each corrupt content between good neighbours in one call per name: its status, a zero
    length, exact neighbours, guards intact."""
    seen = set()
    for name in iv.FAMILIES:
        good = [v for v in iv.valid_vectors() if v.name == name and len(v.blob) < 70000]
        bad = [v for v in iv.corrupt_vectors() if v.name == name]
        assert good and bad
        vs = []
        for i, b in enumerate(bad):
            vs += [good[i % len(good)], b]
        vs.append(good[-1])
        out, out_offs, lens, st = _inflate(name, [v.blob for v in vs], [v.cap for v in vs], gpu)
        _expect(vs, out, out_offs, lens, st)
        seen |= {v.status for v in bad}
    assert seen == {iv.EBADMSG, iv.EOVERFLOW}
    assert len(iv.corrupt_vectors()) >= 45


def test_more_contents_than_waves(gpu):
    """5,000 contents of 300 bytes (the persistent grid holds 4,096 waves), a zlib stream each in a
    gzip member, 50 of them corrupted at known indices: the last ticket, the status of every
    content and the CRC kernel's strides."""
    rng = np.random.default_rng(5)
    n, size = 5000, 300
    data = iv.mixed(n * size, 77)
    bad = {int(k): j % 3 for j, k in enumerate(sorted(rng.choice(n, 50, replace=False)))}
    bad[n - 1] = 0  # the last ticket is one of them
    parts, blobs = [], []
    for i in range(n):
        part = data[i * size:(i + 1) * size]
        m = bytearray(iv.gzip_member(iv.zlib_stream(iv.RAW, part), part))
        if bad.get(i) == 0:
            m[-6] ^= 0x40  # the stored CRC-32
        elif bad.get(i) == 1:
            m[-4] ^= 1  # ISIZE
        elif bad.get(i) == 2:
            m = m[:len(m) // 2]  # truncated
        parts.append(part)
        blobs.append(iv.content(iv.GZ, bytes(m)))
        if i in bad:
            assert not iv.zlib_decode(iv.GZ, blobs[-1])[1]
    out, out_offs, lens, st = _inflate(iv.GZ, blobs, [size] * n, gpu)
    want_st = np.array([iv.EBADMSG if i in bad else 0 for i in range(n)])
    assert (st == want_st).all(), np.flatnonzero(st != want_st)[:10]
    assert (lens == np.where(want_st == 0, size, 0)).all()
    for i in range(n):
        if i not in bad:
            assert out[out_offs[i]:out_offs[i] + size].tobytes() == parts[i], i


@pytest.fixture
def chunk_grid(request):
    """At most this many workgroups (waves) in the persistent decode kernel (KCDC_TEST_CHUNK_GRID)."""
    L = _lib.lib()
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, request.param) == 0
    yield request.param
    assert L.kcdc_test_set(_lib.TEST_CHUNK_GRID, 0) == 0


@pytest.mark.parametrize("chunk_grid", (1, 3), indirect=True)
def test_one_wave_decodes_every_vector(chunk_grid, gpu, checked):
    """One wave (or three) takes every ticket of a call, in content order with one: every valid
    vector of at most 70,000 decoded bytes, a corrupt one after each good one while they last.  So the
    wave that has just refused a content, or finished a stored, fixed or dynamic block, decodes the
    next content of another block type with whatever LDS tables, bit window and status it still
    holds: every content exact, guards intact."""
    seen, took_part = set(), 0
    for name in iv.FAMILIES:
        good = [v for v in iv.valid_vectors() if v.name == name and len(v.expected) <= 70000]
        bad = [v for v in iv.corrupt_vectors() if v.name == name]
        assert len(good) > len(bad) > 0
        vs = []
        for i, g in enumerate(good):
            vs += [g] + bad[i:i + 1]
        assert {v.id for v in bad} <= {v.id for v in vs}
        out, out_offs, lens, st = _inflate(name, [v.blob for v in vs], [v.cap for v in vs], gpu)
        _expect(vs, out, out_offs, lens, st)
        seen |= {v.status for v in bad}
        took_part += len(good)
    assert took_part >= 150
    assert seen == {iv.EBADMSG, iv.EOVERFLOW}


def test_argument_errors(gpu):
    import torch
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.uint8, device=gpu)
    p = C.c_void_p(t.data_ptr())
    args = (p, p, p, 1, p, p, p, p, p, p, 1024, None)
    assert L.kcdc_inflate_chunks_device(b"no-such-compressor", *args) == _lib.KCDC_ENOENT
    assert L.kcdc_inflate_chunks_device(b"s2-default", *args) == _lib.KCDC_EINVAL
    assert "s2-default" in _lib.last_error()
    assert L.kcdc_inflate_chunks_device(b"zstd", *args) == _lib.KCDC_EINVAL
    with pytest.raises(_lib.KcdcError) as e:
        kc.Compressor("s2-default").inflate_chunks_device(t.data_ptr(), [0], [8], t, [0], [8], gpu)
    assert e.value.code == _lib.KCDC_EINVAL
    assert L.kcdc_inflate_chunks_device(b"gzip", None, *args[1:]) == _lib.KCDC_EINVAL  # a null argument
    # nothing to do: no launch, nothing written
    assert L.kcdc_inflate_chunks_device(b"deflate-default", *args[:3], 0, *args[4:]) == 0
    lens, st = kc.Compressor("gzip").inflate_chunks_device(t.data_ptr(), [], [], t, [], [], gpu)
    torch.cuda.synchronize()
    assert lens.numel() == 0 and st.numel() == 0 and not t.cpu().numpy().any()
    # a workspace below kcdc_inflate_workspace_size is an argument error, not a launch
    need = int(L.kcdc_inflate_workspace_size(1))
    assert L.kcdc_inflate_chunks_device(b"deflate-default", *args[:10], need - 1, None) == _lib.KCDC_EINVAL
    torch.cuda.synchronize()
    assert not t.cpu().numpy().any()
