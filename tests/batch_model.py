"""CPU model of what the batch kernels (split_batch_pipe_kernel, split_batch_rk_kernel) see of
their input, and planted inputs that put candidates on the seams of that geometry.

Test infrastructure only (tests/test_batch_model.py, tests/test_gpu_batch_edges.py, and the
background of tests/test_gpu_long_edges.py): nothing in the product imports it.

Three parts, all numpy on top of tests/long_model.py (slot tables, hashes, candidates, rule):

  seeds       64-byte windows without a zero byte whose window hash has its masked bits zero and
              is itself non-zero -- "natural" candidates, in which every one of the 64 bytes
              matters (but for Rabin-Karp's slots 3..6, whose bytes never reach the masked bits:
              tests/test_batch_model.py): a kernel that warms a lane on the wrong bytes, or on none, no longer sees
              them, whereas a window of 64 zero bytes hashes to 0 whatever is missing.  They are
              constructed: 61 random non-zero bytes, the last three solved over all 255^3 values
              with the XOR slot tables (h = base ^ T2[a] ^ T1[b] ^ T0[c]).
  background  counter-PRNG bytes scrubbed of zero bytes and of every candidate of either hash at
              BG_AVG; candidates at a larger power-of-two average are a subset of those at a
              smaller one, so it is candidate-free at every average from BG_AVG up.
  plant()     a stream = a prefix of the background with seed windows (or zero runs) copied in;
              it asserts from the model that the stream's candidates are exactly the planted ones.

  geometry    a restatement -- not an import -- of how the kernels tile a chunk's test region
              (kopia_amd/csrc/kcdc_split_queue.h, _feed.h, _visit.h, _buz.h, _rk.h):
                pregion: lo = s + min - 1 + off0, hi = min(s + max - 1, n - 1) + off0
                  in coordinates (off0 = the stream pointer's misalignment, 0..15);
                pstream_region: the region's tile 0 starts at lo & ~127;
                tile_geom, buzhash: a tile at ct is 64 lanes of
                  L = min(roundup128(ceil((hi - ct + 1) / 64)), lane_cap) bytes, scanned in 128-byte
                  steps; a step that begins past hi is skipped (split_batch_pipe_kernel, `cl <= hi_rel`);
                rk_geom, Rabin-Karp: L rounded up to 256 and capped at 2 * lane_cap
                  (kRkLaneMul); chain A scans a lane's first half, chain B its
                  second (rk_dma_warm); checks are per 64 bytes, the last 64 bytes
                  of B are the drain step (rk_walk);
                the next tile starts at ct + 64 * L (visit_tile; split_batch_rk_kernel);
                a help task is one owner tile [ct, min(ct + T - 1, hi)] (help_find)
                  scanned in sub-tiles with lanes of half the cap (both batch kernels), its
                  lower clip the task's own ct (pregion).
              tests/test_gpu_batch_edges.py checks the lane cap assumed here against the
              library's batch_plan (kcdc_test_batch_plan) before it trusts a layout.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

import long_model as lm
from oracle import coracle

WINDOW = lm.WINDOW
KINDS = ["buzhash", "rabinkarp"]
SEED = 0x6B6F706961
WAVE = 64              # dev::kWave: lanes of a tile
SEED_AVG = 4 << 20     # the seeds are candidates at every power-of-two average up to this one
BG_AVG = 64 << 10      # the background holds no candidate at any average from here up
BG_LEN = 4 << 20       # (the longest planted batch stream: DYNAMIC-4M min size + a few 256 KiB tiles)
BG_SID = 4243


# ------------------------------------------------------------------ seed windows
def _solve_tail(tabs: np.ndarray, base, avg: int):
    """All (a, b, c) in 1..255 with (base ^ T2[a] ^ T1[b] ^ T0[c]) & (avg - 1) == 0 and the hash
    non-zero (at most one c per (a, b) is reported)."""
    dt = tabs.dtype.type
    mask = dt(avg - 1)
    t2, t1, t0 = tabs[2][1:], tabs[1][1:], tabs[0][1:]
    x = dt(base) ^ t2[:, None] ^ t1[None, :]              # [255][255]
    order = np.argsort(t0 & mask, kind="stable")
    srt = (t0 & mask)[order]
    xm = (x & mask).ravel()
    i = np.minimum(np.searchsorted(srt, xm), srt.size - 1)
    out = []
    for flat in np.flatnonzero(srt[i] == xm):
        a, b, c = flat // 255, flat % 255, int(order[i[flat]])
        if x[a, b] ^ t0[c]:
            out.append((int(a) + 1, int(b) + 1, c + 1))
    return out


def seed_windows(kind: str, avg: int, count: int, rng) -> list:
    """`count` 64-byte windows (uint8 arrays) without a zero byte whose window hash -- the hash of
    the stream position at which the window ends -- has the bits of avg - 1 zero and is non-zero."""
    tabs = lm.slot_tables(kind)
    out = []
    while len(out) < count:
        head = rng.integers(1, 256, WINDOW - 3).astype(np.uint8)
        base = tabs.dtype.type(0)
        for i, b in enumerate(head):  # byte i of the window sits in slot 63 - i when the window ends
            base ^= tabs[WINDOW - 1 - i][b]
        for a, b, c in _solve_tail(tabs, base, avg)[:2]:  # (two per head: the heads stay varied)
            out.append(np.concatenate([head, np.asarray([a, b, c], dtype=np.uint8)]))
    return out[:count]


def window_hash(kind: str, w: np.ndarray) -> int:
    assert w.size == WINDOW
    return int(lm.hashes(kind, w)[WINDOW - 1])


@lru_cache(maxsize=None)
def seeds(kind: str) -> tuple:
    """The session's seed windows of `kind`, made at SEED_AVG (so candidates at every smaller
    power-of-two average too)."""
    ws = seed_windows(kind, SEED_AVG, 24, np.random.default_rng(SEED + len(kind)))
    for w in ws:
        w.setflags(write=False)
    return tuple(ws)


# ------------------------------------------------------------------ background
def scrubbed(sid: int, n: int, avg: int) -> np.ndarray:
    """n counter-PRNG bytes (stream `sid`) without zero bytes and without one candidate of either
    hash at average `avg`: zeros become 1, then every candidate's byte has bit 0 flipped (3 where
    that would make a zero) until none is left.  Flipping byte p changes the windows ending at
    p .. p + 63 only, so after the one full pass per hash the re-checks are local."""
    d = coracle.gen_stream(SEED, sid, n)
    d[d == 0] = 1
    todo = np.unique(np.concatenate([lm.candidates(kind, avg, d) for kind in KINDS]))
    for _ in range(8):
        if todo.size == 0:
            break
        d[todo] ^= 1
        d[todo[d[todo] == 0]] = 3
        todo = np.unique(np.concatenate([lm.candidates_in(kind, avg, d, int(p), int(p) + WINDOW)
                                         for kind in KINDS for p in todo] + [np.zeros(0, dtype=np.int64)]))
    assert todo.size == 0, "scrub did not converge"
    assert d.all()
    d.setflags(write=False)
    return d


@lru_cache(maxsize=1)
def background() -> np.ndarray:
    return scrubbed(BG_SID, BG_LEN, BG_AVG)


# ------------------------------------------------------------------ planting
def plant(kind: str, avg: int, n: int, items, bg: np.ndarray | None = None):
    """The first n background bytes with `items` planted:
         ("w", p)      a seed window of `kind` copied so that it ends at p: one natural candidate;
         ("z", p, k)   bytes p - 63 .. p + k - 1 zeroed: the k consecutive candidates p .. p + k - 1
                       (for "many candidates in a row" only: a zero window hides missing bytes).
    Returns (bytes, sorted planted candidates).  Asserts from the model that the stream's
    candidates of `kind` at `avg` are exactly the planted ones: the background has none, and a
    plant changes only the windows ending within 63 bytes past it -- those, and the windows that
    straddle the plant's first byte, are hashed here.  Where a copied window makes a stray
    candidate among them, the next seed is taken."""
    bg = background() if bg is None else bg
    assert avg >= BG_AVG and (avg & (avg - 1)) == 0 and avg <= SEED_AVG and n <= bg.size
    d = bg[:n].copy()
    pool = seeds(kind)
    spans, planted = [], []
    for it in sorted(items, key=lambda it: it[1]):
        p, k = (it[1], 1) if it[0] == "w" else (it[1], it[2])
        a, b = p - (WINDOW - 1), p + k - 1
        assert a >= 0 and b < n, (it, n)
        assert not spans or a > spans[-1][1], f"plants overlap at {p}"
        spans.append((a, b))
        want = list(range(p, p + k))
        # what the bytes written before this plant leave in the range this plant can change
        lo, hi = a, min(b + WINDOW, n)
        if it[0] == "z":
            d[a:b + 1] = 0
            found = lm.candidates_in(kind, avg, d, lo, hi).tolist()
            assert found == [c for c in planted if c >= lo] + want, (it, found)
        else:
            for t in range(len(pool)):
                d[a:b + 1] = pool[(p + t) % len(pool)]
                found = lm.candidates_in(kind, avg, d, lo, hi).tolist()
                if found == [c for c in planted if c >= lo] + want:
                    break
            else:
                raise AssertionError(f"no seed window plants cleanly at {p}")
        planted += want
    d.setflags(write=False)
    return d, np.asarray(planted, dtype=np.int64)


# ------------------------------------------------------------------ geometry
def unit(kind: str) -> int:
    """Bytes a lane's length is rounded up to (tile_geom: 128; rk_geom: 256)."""
    return 128 if kind == "buzhash" else 256


def own_lane(kind: str, lane_cap: int) -> int:
    """Lane bytes of a full own tile; lane_cap is BatchArgs::lane_cap (the plan's)."""
    return lane_cap if kind == "buzhash" else 2 * lane_cap


def help_lane(kind: str, lane_cap: int) -> int:
    """Lane bytes of a help task's full sub-tile."""
    if kind == "buzhash":
        return lane_cap >> 1 if lane_cap >= 512 else lane_cap
    return lane_cap


def region(avg: int, s: int, n: int, off0: int):
    """(lo, hi) of the chunk starting at s, in coordinates; None when the chunk has no test region."""
    mn, mx = avg // 2, 2 * avg
    if s + mn - 1 >= n:
        return None
    return s + mn - 1 + off0, min(s + mx - 1, n - 1) + off0


def tiles_between(kind: str, lane: int, ct: int, hi: int) -> list:
    """[(ct, L)] of the tiles that cover [ct, hi] with lanes of at most `lane` bytes."""
    u, out = unit(kind), []
    while ct <= hi:
        per = -(-(hi - ct + 1) // WAVE)
        L = min(-(-per // u) * u, lane)
        out.append((ct, L))
        ct += WAVE * L
    return out


def tiles(kind: str, lane_cap: int, avg: int, s: int, n: int, off0: int) -> list:
    """[(ct, L)] of the own tiles of the region of the chunk starting at s."""
    lo, hi = region(avg, s, n, off0)
    return tiles_between(kind, own_lane(kind, lane_cap), lo & ~127, hi)


def help_subtiles(kind: str, lane_cap: int, avg: int, s: int, n: int, off0: int, tile: int) -> list:
    """[(ct, L)] of the sub-tiles in which a help task scans own tile `tile` (>= 1) of the region."""
    _, hi = region(avg, s, n, off0)
    ct, _ = tiles(kind, lane_cap, avg, s, n, off0)[tile]
    T = WAVE * own_lane(kind, lane_cap)
    return tiles_between(kind, help_lane(kind, lane_cap), ct, min(ct + T - 1, hi))


def locate(kind: str, lane_cap: int, avg: int, s: int, n: int, off0: int, p: int):
    """Where the own tiles of the region of the chunk starting at s hold stream position p:
    (tile index, lane, offset in the lane, the tile's L, whether it is the region's last tile).
    p may lie in tile 0's head below lo, or in the last tile's overshoot past hi."""
    ts = tiles(kind, lane_cap, avg, s, n, off0)
    c = p + off0
    assert ts[0][0] <= c < ts[-1][0] + WAVE * ts[-1][1], (p, ts[0], ts[-1])
    k = max(i for i, (ct, _) in enumerate(ts) if ct <= c)
    ct, L = ts[k]
    return k, (c - ct) // L, (c - ct) % L, L, k == len(ts) - 1


def position(kind: str, lane_cap: int, avg: int, s: int, n: int, off0: int, tile: int, lane: int, off: int) -> int:
    """The inverse of locate(): the stream position at (tile, lane, offset in the lane)."""
    ct, L = tiles(kind, lane_cap, avg, s, n, off0)[tile]
    assert 0 <= lane < WAVE and 0 <= off < L
    return ct + lane * L + off - off0


def step_of(kind: str, off: int, L: int):
    """The scan step that tests offset `off` of an L-byte lane: buzhash (step, byte in step) with
    128-byte steps; Rabin-Karp (chain 0/1, 64-byte check of the chain, byte in the check)."""
    if kind == "buzhash":
        return off // 128, off % 128
    chain, rel = (0, off) if off < L // 2 else (1, off - L // 2)
    return chain, rel // 64, rel % 64


# ------------------------------------------------------------------ layouts
# A case is one short planted stream: (label, n, off0, items).  The sweeps plant one natural
# candidate per stream at anchor + delta; every stream of a layout gets another misalignment, all
# of 0..15 within a sweep.  Only the first chunk (s = 0) carries the anchor; what follows it is
# whatever the rule makes of the rest, and is compared like everything else.
class Case(NamedTuple):
    label: str
    n: int
    off0: int
    items: tuple


FULL = list(range(-129, 130))
THIN = sorted(set(range(-65, 66)) | {d * g for d in (127, 128, 129) for g in (-1, 1)})


def ragged_rems(kind: str) -> list:
    """Bytes left of the region at the start of its ragged last tile (sweep c)."""
    u = unit(kind)
    return [1, u - 1, u, u + 1, WAVE * u, WAVE * u + 1]


def full_tiles(kind: str, lane_cap: int, avg: int) -> int:
    """Full own tiles of a whole region (max - min bytes, plus tile 0's head: a ragged tile follows)."""
    return (2 * avg - avg // 2) // (WAVE * own_lane(kind, lane_cap))


def far_tile(kind: str, lane_cap: int, avg: int) -> int:
    """k of the far tile boundary k|k+1: 4 where the region has 6 full tiles, else the last
    boundary it has (regions of 3 full tiles and a ragged one end at 2|3)."""
    return min(4, full_tiles(kind, lane_cap, avg) - 1)


def _off0(i: int, salt: int) -> int:
    return (7 * i + salt) % 16


def sweep(kind: str, lane_cap: int, avg: int, anchor: str, deltas, extras: bool = True) -> list:
    """The cases of one anchor:
         lo          the region's first position; delta < 0 lies in tile 0's head (or before it)
                     and must be ignored -- every other stream has a second plant further on, the
                     others end at the stream's end;
         hi          s + max - 1 with the stream going on; delta > 0 must be ignored (forced cut,
                     the plant then lies in the next chunk's first min bytes);
         end:R       hi = n - 1 with R bytes of the region left at the start of its last tile; the
                     plant at n - 1 - delta, delta >= 0;
         tile:K      the boundary of own tiles K | K + 1;
         lane:K:L    the boundary of lanes L | L + 1 of tile K;
         mid:K:L     the middle of lane L of tile K (Rabin-Karp: chain A | chain B);
         half:K      the middle of tile K: the first lane of a help task's second sub-tile."""
    mn, mx = avg // 2, 2 * avg
    T = WAVE * own_lane(kind, lane_cap)
    g = (kind, lane_cap, avg)
    key, *arg = anchor.split(":")
    arg = [int(a) for a in arg]
    out = []
    for i, dl in enumerate(deltas):
        off0 = _off0(i, len(anchor) + sum(arg))
        label = f"{anchor} delta {dl:+d} off0 {off0}"
        if key == "lo":
            n = mn + 2 * T + 13
            items = [("w", mn - 1 + dl)]
            if i % 2 == 0:
                items.append(("w", mn - 1 + T + 300 + 64 * (i % 5)))
        elif key == "hi":
            n = mx + mn + T + 7
            items = [("w", mx - 1 + dl)]
        elif key == "end":
            if dl < 0:
                continue
            ct0 = (mn - 1 + off0) & ~127
            n = ct0 + T + arg[0] - off0
            items = [("w", n - 1 - dl)]
            ts = tiles(*g, 0, n, off0)
            assert len(ts) == 2 and ts[1][0] == ct0 + T and n - 1 + off0 - ts[1][0] + 1 == arg[0], (label, ts)
        elif key == "tile":
            n = mn + (arg[0] + 2) * T + 5
            items = [("w", position(*g, 0, n, off0, arg[0] + 1, 0, 0) + dl)]
        elif key in ("lane", "mid", "half"):
            k = arg[0]
            n = mn + (k + 2) * T
            L = tiles(*g, 0, n, off0)[k][1]
            assert L == own_lane(kind, lane_cap), label
            lane, off = (arg[1] + 1, 0) if key == "lane" else (arg[1], L // 2) if key == "mid" else (WAVE // 2, 0)
            items = [("w", position(*g, 0, n, off0, k, lane, off) + dl)]
        else:
            raise ValueError(anchor)
        out.append(Case(label, n, off0, tuple(items)))
    # The clips at lo and hi act within one step, and where in its step lo or hi lies is the
    # misalignment's doing ((min - 1 + off0) % 128: the step's last byte at off0 = 0, its first at
    # 1): the deltas next to the clip get every such placement, not just their own stream's.
    if key in ("lo", "hi") and extras:
        at = (mn if key == "lo" else mx) - 1
        n = mn + 2 * T + 13 if key == "lo" else mx + mn + T + 7
        for dl in (-2, -1, 0, 1, 2):
            for off0 in (0, 1, 2, 15):
                out.append(Case(f"{anchor} delta {dl:+d} off0 {off0}", n, off0, (("w", at + dl),)))
    return out


def anchors(kind: str, lane_cap: int, avg: int) -> list:
    """Every sweep anchor of a geometry (the issue's a-g)."""
    far = far_tile(kind, lane_cap, avg)
    out = ["lo", "hi"] + [f"end:{r}" for r in ragged_rems(kind)]
    out += sorted({f"tile:{k}" for k in (0, 1, far)})
    out += [f"lane:1:{l}" for l in (0, 31, 62)]
    if kind == "rabinkarp":
        out += [f"mid:1:{l}" for l in (0, 31, 63)]
    out += [f"half:{k}" for k in ((2, 3) if far >= 4 else (1, 2))]
    return out


def kept_alive(kind: str, lane_cap: int, avg: int, off0: int = 3) -> Case:
    """A stream predicted to end that a candidate keeps alive (visit_resolve's `else if (live)`):
    the forced cut would leave less than min, the candidate's cut leaves more.  The candidate must
    lie in the region's last tile: well inside it where one tile holds the whole region (lanes of
    4 KiB at 128K), else in the ragged last tile's few bytes."""
    mn, mx = avg // 2, 2 * avg
    g = (kind, lane_cap, avg)
    n = mx + mn - 1
    p = mx - 2 - 200 if locate(*g, 0, n, off0, mx - 2 - 200)[4] else mx - 2
    assert locate(*g, 0, n, off0, p)[4] and p + mn < n and expected([], n, avg).tolist() == [mx, n]
    return Case("corner kept alive", n, off0, (("w", p),))


def corners(kind: str, lane_cap: int, avg: int) -> list:
    """The named corners, placed with position() and checked with locate()."""
    mn, mx = avg // 2, 2 * avg
    Lo = own_lane(kind, lane_cap)
    T = WAVE * Lo
    g = (kind, lane_cap, avg)
    n, off0 = mn + 4 * T, 3
    pos = lambda tile, lane, off: position(*g, 0, n, off0, tile, lane, off)
    where = lambda p: locate(*g, 0, n, off0, p)[:3]
    out = []

    def add(label, items, n_=n, off0_=off0):
        out.append(Case(f"corner {label}", n_, off0_, tuple(items)))

    # two candidates in one tile: the earlier position late in a lower lane, the later position in
    # the first step of a higher lane -- the lower lane wins
    a, b = pos(1, 5, 2 * 128 + 17), pos(1, 9, 40)
    assert a < b and where(a) == (1, 5, 273) and where(b) == (1, 9, 40)
    assert step_of(kind, 273, Lo)[-2] > step_of(kind, 40, Lo)[-2]
    add("lower lane, higher step", [("w", a), ("w", b)])
    # two in one lane in different steps; the first wins
    a, b = pos(1, 7, 30), pos(1, 7, 2 * 128 + 5)
    assert where(a)[:2] == where(b)[:2] == (1, 7) and step_of(kind, 30, Lo) < step_of(kind, 261, Lo)
    add("one lane, two steps", [("w", a), ("w", b)])
    if kind == "buzhash":  # two in one 128-byte step (natural windows lie >= 64 bytes apart)
        a, b = pos(1, 7, 128 + 1), pos(1, 7, 128 + 70)
        assert step_of(kind, 129, Lo)[0] == step_of(kind, 198, Lo)[0] == 1
        add("one step", [("w", a), ("w", b)])
    else:
        # chain B of lane l before chain A of lane l + 1; both halves of one lane (A first)
        a, b = pos(1, 20, Lo // 2 + 64 + 9), pos(1, 21, 64 + 3)
        assert step_of(kind, Lo // 2 + 73, Lo)[0] == 1 and step_of(kind, 67, Lo)[0] == 0 and a < b
        add("chain B of lane l, chain A of lane l + 1", [("w", a), ("w", b)])
        a, b = pos(1, 20, 3 * 64 + 9), pos(1, 20, Lo // 2 + 11)
        assert step_of(kind, 201, Lo)[0] == 0 and step_of(kind, Lo // 2 + 11, Lo)[0] == 1 and a < b
        add("both chains of one lane", [("w", a), ("w", b)])
        a, b = pos(1, 20, Lo // 2 - 1), pos(1, 20, Lo // 2 + 64)  # A's last byte, B's second check
        add("chain A's last byte, then chain B", [("w", a), ("w", b)])
    # lo - 1 and lo in one step (consecutive candidates: a zero run), and naturally lo - 64 and lo
    lo = mn - 1
    assert (lo + off0) % 128 >= 1
    add("lo - 1 and lo", [("z", lo - 1, 2)])
    assert (lo + 0) % 128 >= 64
    add("lo - 64 and lo", [("w", lo - 64), ("w", lo)], off0_=0)
    add("lo - 64 alone, then the tile's last lane", [("w", lo - 64), ("w", pos(0, 63, 77))])
    # hi and hi + 1, the stream going on (the cut is max either way; the next chunk must not see hi + 1)
    add("hi and hi + 1", [("z", mx - 1, 2)], n_=mx + mn + T)
    out.append(kept_alive(kind, lane_cap, avg, off0))
    # zero runs of 63 + 300 bytes: straddling lo (the cut is at lo) and a tile boundary
    add("zero run over lo", [("z", lo - 150, 300)])
    add("zero run over a tile boundary", [("z", pos(2, 0, 0) - 150, 300)])
    # the stream's last 64 bytes a window ending at n - 2: the cuts end n - 1, n
    n3 = mn + T + 77
    add("window ending at n - 2", [("w", n3 - 2)], n_=n3)
    return out


def backlog_cases(kind: str, lane_cap: int, avg: int, quantum_tiles: int) -> list:
    """Streams for launches with more streams than waves: plants around the tile boundaries next to
    where a visit's quantum ends (q - 2 | q - 1, q - 1 | q, q | q + 1 where the region has them), so a
    resumed wave's first tile starts on or next to a candidate.  Every stream is long enough to
    stay alive after its plant: no yielded stream ends as a tombstone."""
    mn = avg // 2
    T = WAVE * own_lane(kind, lane_cap)
    g = (kind, lane_cap, avg)
    out = []
    for k in (quantum_tiles - 2, quantum_tiles - 1, quantum_tiles):
        for i, dl in enumerate([-64, -1, 0, 1, 63, 64, 127, 128]):
            off0 = _off0(i, k)
            n = mn + (k + 2) * T + mn + T
            ts = tiles(*g, 0, n, off0)
            if len(ts) < k + 2:
                continue  # the region ends before this boundary
            out.append(Case(f"visit tile:{k} delta {dl:+d} off0 {off0}", n, off0,
                            (("w", ts[k + 1][0] - off0 + dl),)))
    return out


def build(kind: str, avg: int, cases) -> list:
    """[(bytes, planted candidates)] of the cases."""
    return [plant(kind, avg, c.n, c.items) for c in cases]


def expected(planted, n: int, avg: int) -> np.ndarray:
    """The cuts of a planted stream by the chunk rule over its planted candidates."""
    return lm.rule(planted, n, avg // 2, 2 * avg)


def few_stream_cases(kind: str, lane_cap: int, avg: int) -> list:
    """A dozen or so streams for a launch whose plan depends on there being few of them: the
    anchors lo, tile 0|1 and 1|2, lane 31|32 and a ragged end, a few deltas each."""
    u = unit(kind)
    out = []
    for anchor, ds in [("lo", [-1, 0, 1]), ("tile:0", [-1, 0, 1, 64]), ("tile:1", [-1, 0]),
                       ("lane:1:31", [-1, 0, 63]), (f"end:{u + 1}", [0, 1, u])]:
        out += sweep(kind, lane_cap, avg, anchor, ds, extras=False)
    return out
