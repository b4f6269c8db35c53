"""CPU: the structure of the far-offset population (tests/far_layout.py) that
tests/test_gpu_far_offsets.py runs every per-chunk entry point over, pinned so that a later edit
cannot drop a line, a chunk kind, a slot role or a guard; and the Python layout helpers' int64
arithmetic for totals above 2^32."""
import numpy as np
import pytest

import far_layout as fl
from kopia_amd import compression as kc
from kopia_amd import ecc as kecc
from kopia_amd import encryption as ke

G4 = 1 << 32
ALIGNED = 0x7F12 * G4                 # A = 0: dropped
MIDDLE = 0x7F12 * G4 + 0x45600000     # 2 MiB-aligned, A = 0xBAA00000: kept
AT_2G = 0x7F12 * G4 + (1 << 31)       # A = 2^31: dropped
BELOW_4G = 0x7F12 * G4 + (1 << 20)    # A = 2^32 - 1 MiB: dropped
LOW_A = 0x7F12 * G4 + G4 - (9 << 20)  # A = 9 MiB: kept, its window overlaps the near twin's region
BASES = [ALIGNED, MIDDLE, AT_2G, BELOW_4G, LOW_A]


def test_lines_and_the_dropped_address_line():
    fixed = [("2^31", 1 << 31), ("2^32", G4)]
    assert fl.lines(ALIGNED) == (fixed, "A = 0x0 lies within 4 MiB of the buffer's start")
    assert fl.lines(MIDDLE) == (fixed + [("A", 0xBAA00000)], None)
    assert fl.lines(AT_2G) == (fixed, "A = 0x80000000 lies within 4 MiB of 2^31")
    assert fl.lines(BELOW_4G) == (fixed, "A = 0xfff00000 lies within 4 MiB of 2^32")
    assert fl.lines(LOW_A) == (fixed + [("A", 9 << 20)], None)
    assert fl.lines(MIDDLE + (3 << 20) + 16)[1] is None  # 3 MiB lower: still 4 MiB and more from every line
    assert fl.lines(ALIGNED + G4 - (3 << 30) + (1 << 20), size=3 << 30)[1].endswith("the buffer's end")
    for base in BASES:  # whenever A is kept, base + A is where the address crosses a multiple of 2^32
        named, why = fl.lines(base)
        if why is None:
            assert (base + named[2][1]) % G4 == 0 and 0 < named[2][1] < fl.SIZE
    assert fl.SIZE == (4 << 30) + (8 << 20)
    with pytest.raises(ValueError):
        fl.layout(MIDDLE + 8)


@pytest.mark.parametrize("base", BASES)
def test_source_chunks(base):
    lay = fl.layout(base)
    assert lay.n == fl.PER_LINE * len(lay.xs) and len(lay.xs) == (2 if lay.dropped else 3)
    assert lay.offs.dtype == lay.lens.dtype == np.int64
    lens_by_line = []
    for k, x in enumerate(lay.xs):
        c = {kind: (int(lay.offs[k * fl.PER_LINE + j]), int(lay.lens[k * fl.PER_LINE + j])) for j, kind in enumerate(fl.KINDS)}
        assert sum(c["ends"]) == x and c["ends"][1] > 1000
        assert c["starts"][0] == x and c["starts"][1] > 1000
        assert c["before5"] == (x - 1, 5) and c["after33"] == (x + 1, 33) and c["empty"] == (x, 0)
        assert c["unit_ends"] == (x - 4096, 4096) and c["unit_starts"] == (x, 4096)
        o, n = c["mid"]
        assert n == 70001 and abs(o + n // 2 - x) < 100
        o, n = c["long"]
        assert n == (1 << 20) + 13 and o < x - (1 << 19) + 100 and o + n > x + (1 << 19) - 100
        ws, wl = lay.windows()[k]
        assert ws % 65536 == 0 and ws <= x - fl.HALF and x + fl.HALF <= ws + wl <= lay.size and ws >= 0
        assert (lay.offs[lay.line_of == k] >= ws).all() and ((lay.offs + lay.lens)[lay.line_of == k] <= ws + wl).all()
        lens_by_line.append(c["ends"][1])
    assert len(set(lens_by_line)) == len(lens_by_line)
    assert len({int(o) % 16 for o, n in zip(lay.offs, lay.lens) if n}) >= 8
    assert lay.long_indices() == [i for i in range(lay.n) if lay.lens[i] > (1 << 20)]
    wins = sorted(lay.windows())
    assert all(a[0] + a[1] <= b[0] for a, b in zip(wins, wins[1:])), "the windows of two lines overlap"
    # a shorter straddler keeps every line and every kind
    short = fl.layout(base, long_len=300_000)
    assert (short.lens[short.long_indices()] == 300_000).all() and short.xs == lay.xs
    assert all(o < x < o + 300_000 for o, x in zip(short.offs[short.long_indices()], short.xs))


def _sizes(lay, grow):
    return np.array([grow(int(n)) for n in lay.lens], np.int64)


GROW = {"same": lambda n: n, "sealed": lambda n: (n + 28 + 3) & ~3, "bound": lambda n: 24 + n + 5 * ((n + 511) // 512),
        "ecc": lambda n: n + n // 8 + 700}


@pytest.mark.parametrize("grow", sorted(GROW))
@pytest.mark.parametrize("base", BASES)
def test_slots_roles_guards_and_twin(base, grow):
    lay = fl.layout(base)
    sizes = _sizes(lay, GROW[grow])
    align = 4 if grow in ("sealed", "bound") else 1
    seen = set()
    for variant in range(3):
        offs = lay.slots(sizes, align, variant)
        assert offs.dtype == np.int64 and (offs % align == 0).all()
        order = np.argsort(offs, kind="stable")
        ends = offs + sizes
        filled = [i for i in order if sizes[i]]
        for a, b in zip(filled, filled[1:]):
            assert offs[b] - ends[a] >= fl.GUARD, (variant, a, b)
        for k, x in enumerate(lay.xs):
            i = lay.long_indices()[k]
            role = lay.role(k, variant)
            seen.add((k, role))
            w = -(-int(sizes[i]) // align) * align
            if role == "straddles":
                assert offs[i] < x < ends[i] and min(x - offs[i], ends[i] - x) > sizes[i] // 3
            elif role == "ends":
                assert offs[i] + w == x
            else:
                assert offs[i] == x
            ws, wl = lay.windows()[k]
            mine = lay.line_of == k
            assert (offs[mine] >= ws + fl.GUARD).all() and (ends[mine] <= ws + wl - fl.GUARD).all()
        if align == 1:
            assert len({int(o) % 16 for o in offs}) >= 8
        # the twin: below 32 MiB, low 16 bits kept, the same distances inside a line, still disjoint
        near = lay.near(offs)
        assert ((near & 0xFFFF) == (offs & 0xFFFF)).all() and (near >= 0).all() and (near + sizes <= fl.NEAR_END).all()
        for k in range(len(lay.xs)):
            mine = lay.line_of == k
            assert (np.diff(near[mine]) == np.diff(offs[mine])).all()
        assert sum(len(rel) for rel, _ in fl.split_by_window(lay.windows(True), near, sizes)) == lay.n
        # aliases: every slot at or above 2^32 has its low-32-bit position listed, and it lies in no slot
        al = lay.aliases(offs, sizes)
        low = {i: pos for i, which, pos in al if which == "mod 2^32"}
        above = [i for i in range(lay.n) if sizes[i] and offs[i] >= G4]
        assert above and set(above) <= set(low)
        for i in above:
            assert not any(offs[j] < low[i] + sizes[i] and low[i] < ends[j] for j in filled), i
        assert all(0 <= pos and pos + sizes[i] <= lay.size and pos != offs[i] for i, _, pos in al)
        assert {which for _, which, _ in al} == {"- 2^32", "- 2^31", "mod 2^32"}
    assert seen == {(k, r) for k in range(len(lay.xs)) for r in fl.ROLES}
    assert lay.near(lay.offs).max() < fl.NEAR_END
    with pytest.raises(ValueError):
        lay.near([lay.xs[0] + fl.HALF + (1 << 20)])


def test_slots_for_other_populations():
    """Slots for contents that are not the source population (sealed or compressed chunks placed as
    the input of an open or a decode): lines_of says where, the largest of a line takes the role."""
    lay = fl.layout(MIDDLE)
    sizes = [100, 70000, 0, 5000, 1 << 20, 33, 900_000, 64]
    lines_of = [0, 0, 0, 1, 1, 1, 2, 2]
    for variant in range(3):
        offs = lay.slots(sizes, 1, variant, lines_of)
        for k, i in enumerate((1, 4, 6)):
            x, role = lay.xs[k], lay.role(k, variant)
            assert {"straddles": offs[i] < x < offs[i] + sizes[i], "ends": offs[i] + sizes[i] == x, "starts": offs[i] == x}[role]
        spans = sorted((int(o), int(o) + s) for o, s in zip(offs, sizes) if s)
        assert all(b[0] - a[1] >= fl.GUARD for a, b in zip(spans, spans[1:]))
    with pytest.raises(ValueError):
        lay.slots([3 << 20, 3 << 20], 1, 0, [0, 0])


def test_window_bookkeeping():
    lay = fl.layout(LOW_A)
    sizes = _sizes(lay, GROW["same"])
    offs = lay.slots(sizes, 1, 1)
    wins = lay.windows()
    host = [np.full(wl, 0xAB, np.uint8) for _, wl in wins]
    for o, s in zip(offs, sizes):
        k = next(k for k, (ws, wl) in enumerate(wins) if ws <= o < ws + wl)
        host[k][o - wins[k][0]:o - wins[k][0] + s] = 7
    assert fl.outside_intact(host, wins, offs, sizes, 0xAB)
    i = lay.long_indices()[1]
    assert fl.take(host, wins, int(offs[i]), 9) == b"\x07" * 9 and fl.take(host, wins, int(offs[i]) - 3, 3) == b"\xab" * 3
    for at in (int(offs[i]) - 1, int(offs[i] + sizes[i]), wins[2][0], wins[0][0] + wins[0][1] - 1):
        k = next(k for k, (ws, wl) in enumerate(wins) if ws <= at < ws + wl)
        host[k][at - wins[k][0]] ^= 1
        assert not fl.outside_intact(host, wins, offs, sizes, 0xAB), at
        host[k][at - wins[k][0]] ^= 1
    # the rest of the buffer, in pieces of at most 256 MiB: with the windows it is every byte, once
    for near in (False, True):
        w = lay.windows(near)
        pieces = fl.complement(w, lay.size)
        assert all(0 < b - a <= 256 << 20 for a, b in pieces)
        both = sorted(pieces + [(s, s + n) for s, n in w])
        assert both[0][0] == 0 and both[-1][1] == lay.size and all(a[1] == b[0] for a, b in zip(both, both[1:]))
        assert all(a % 8 == 0 and b % 8 == 0 for a, b in pieces)


def test_layout_helpers_do_not_wrap():
    """The product's own layout helpers over chunks that add up past 2^32: int64 offsets, exact totals."""
    lens = np.full(9, 1 << 29, np.int64) + np.arange(9)  # 4.5 GiB in all
    offs, total = kc.compressed_layout(lens)
    bounds = [kc.compress_bound(int(n)) for n in lens]
    assert offs.dtype == np.int64 and total == sum(bounds) > G4 and offs.tolist() == np.cumsum([0] + bounds[:-1]).tolist()
    for name in (ke.ChaCha20Poly1305, ke.Aes256Gcm):
        offs, total = ke.sealed_layout(lens, name)
        slots = [(int(n) + 28 + 3) & ~3 for n in lens]
        assert offs.dtype == np.int64 and total == sum(slots) > G4 and offs.tolist() == np.cumsum([0] + slots[:-1]).tolist()
        offs, total = ke.plain_layout(lens + 28, name)
        slots = [(int(n) + 3) & ~3 for n in lens]
        assert offs.dtype == np.int64 and total == sum(slots) > G4 and offs.tolist() == np.cumsum([0] + slots[:-1]).tolist()
    offs, total = kecc._layout(lens)
    slots = [(int(n) + 3) & ~3 for n in lens]
    assert offs.dtype == np.int64 and total == sum(slots) > G4 and offs.tolist() == np.cumsum([0] + slots[:-1]).tolist()
    a = kecc.CreateAlgorithm(kecc.Options(OverheadPercent=2, MaxShardSize=1024))
    offs, sizes, total = a.stored_layout(lens)
    assert offs.dtype == sizes.dtype == np.int64 and (sizes > lens).all() and offs[-1] > G4
    assert total == int(((sizes + 3) & ~3).sum()) and offs.tolist() == np.cumsum([0] + ((sizes + 3) & ~3).tolist()[:-1]).tolist()
    po, ptotal = a.plain_layout(sizes)
    assert po.dtype == np.int64 and ptotal > G4 and po[-1] > G4


PAIRS = {"kept-kept": (MIDDLE, LOW_A), "kept-dropped": (MIDDLE, ALIGNED), "dropped-kept": (ALIGNED, MIDDLE),
         "dropped-dropped": (AT_2G, BELOW_4G)}


def _disjoint(lay, offs, sizes):
    spans = sorted((int(o), int(o) + int(s)) for o, s in zip(offs, sizes) if s)
    assert all(b[0] - a[1] >= fl.GUARD for a, b in zip(spans, spans[1:]))
    assert sum(len(rel) for rel, _ in fl.split_by_window(lay.windows(), offs, sizes)) == len(offs)
    near = lay.near(offs)
    assert ((near & 0xFFFF) == (np.asarray(offs) & 0xFFFF)).all() and (near + sizes <= fl.NEAR_END).all()


@pytest.mark.parametrize("grow", sorted(GROW))
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_slot_tables_of_the_gpu_tests(pair, grow):
    """The tables tests/test_gpu_far_offsets.py builds, for a source and an output buffer that keep or
    drop the address line independently: output slots of the source chunks (two long slots share a
    window where the output buffer has fewer lines), the inputs of open / decode placed in the source
    buffer with three further contents, their output slots, and the chunk that is forged, corrupted
    or damaged, one in every variant."""
    ls, lo = fl.layout(PAIRS[pair][0]), fl.layout(PAIRS[pair][1])
    assert (ls.dropped is None, lo.dropped is None) == tuple(w == "kept" for w in pair.split("-"))
    align = 4 if grow in ("sealed", "bound") else 1
    sizes = _sizes(ls, GROW[grow])
    out_lines = fl.out_lines(ls, lo)
    assert len(out_lines) == ls.n and set(out_lines.tolist()) == set(range(min(len(ls.xs), len(lo.xs))))
    extra = np.array([65600, 3000, 70000], np.int64)  # the decode tests' foreign contents
    in_lines = np.concatenate((ls.line_of, np.arange(3) % len(ls.xs)))
    struck_lines, roles = [], set()
    for v in range(3):
        oo = lo.slots(sizes, align, v, out_lines)
        _disjoint(lo, oo, sizes)
        for k, x in enumerate(lo.xs):  # the largest slot of every output line has the line's role
            mine = np.flatnonzero(out_lines == k)
            if len(mine) == 0:
                continue
            i = int(mine[np.argmax(sizes[mine])])
            w = -(-int(sizes[i]) // align) * align
            role = lo.role(k, v)
            roles.add((k, role))
            assert {"straddles": oo[i] < x < oo[i] + sizes[i], "ends": oo[i] + w == x, "starts": oo[i] == x}[role]
        soffs = ls.slots(np.concatenate((sizes, extra)), 1, v, in_lines)
        _disjoint(ls, soffs, np.concatenate((sizes, extra)))
        po = lo.slots(np.concatenate((sizes, extra)), align, (v + 1) % 3, in_lines % len(lo.xs))
        _disjoint(lo, po, np.concatenate((sizes, extra)))
        k, hit, straddles = ls.struck(v)
        assert hit == ls.long_indices()[k] and sizes[hit] == sizes.max()
        x = ls.xs[k]
        if straddles:
            assert soffs[hit] < x < soffs[hit] + sizes[hit]
        else:
            assert len(ls.xs) == 2 and v == 1 and k == 0 and soffs[hit] + sizes[hit] == x
        struck_lines.append(k)
        far = max(range(len(ls.xs)), key=lambda j: abs(ls.xs[j] - x))  # test_ecc's chunk past repair
        assert far != k and abs(int(soffs[hit]) - int(soffs[far * fl.PER_LINE + fl.MID_AT])) >= (1 << 30) - (4 << 20)
    assert set(struck_lines) == set(range(len(ls.xs)))  # every source line's long chunk is struck once or more
    present = sorted(set(out_lines.tolist()))
    assert roles == {(k, r) for k in present for r in fl.ROLES}
