"""The far-offset population shared by tests/test_far_layout.py (CPU: its structure) and
tests/test_gpu_far_offsets.py (GPU: every per-chunk entry point over it).  No tests here, no torch.

The chunk kernels take chunks as 64-bit offsets into one device buffer, and under those sit 32-bit
positions on purpose.  A product batch is 16 GiB resident, so almost every chunk lies beyond offset
2^32; here a few chunks sit on the lines where a narrow offset goes wrong, in a buffer of
4 GiB + 8 MiB of which only a window around every line is ever filled or read back:
  - "2^31": a signed 32-bit offset breaks;
  - "2^32": an unsigned one wraps;
  - "A" = (-base) mod 2^32: the absolute device address base + offset crosses a multiple of 2^32, which
    a pointer add in the low word without a carry gets wrong (dropped, with a reason, where it lies
    within MARGIN of 0, of the buffer's end or of another line).
At every line X the KINDS of chunk below; the free lengths differ by line, so that the starts take
many residues mod 16 and no two lines hold chunks of the same bytes.  Source chunks overlap: they are
only read.  Output slots (Layout.slots) are disjoint, GUARD or more canary bytes apart, and the long
chunk's slot straddles its line, ends at it or starts at it by the call's variant: over variants
0, 1, 2 every line gets every role.  The near twin (Layout.near) is every offset moved down below
32 MiB with its low 16 bits kept: the same call there must give the same bytes."""
from dataclasses import dataclass

import numpy as np

SIZE = (4 << 30) + (8 << 20)
MARGIN = 4 << 20       # A is dropped within this of 0, the end or another line
HALF = 2 << 20         # a window reaches this far below and above its line
WINDOW = 2 * HALF + (1 << 16)
NEAR_STRIDE = 8 << 20  # the twin's windows: line k at k * NEAR_STRIDE
NEAR_END = 32 << 20
GUARD = 64
LONG = (1 << 20) + 13
KINDS = ("ends", "starts", "before5", "after33", "empty", "unit_ends", "unit_starts", "mid", "long")
PER_LINE = len(KINDS)
LONG_AT = KINDS.index("long")
MID_AT = KINDS.index("mid")
ROLES = ("straddles", "ends", "starts")


def lines(base, size=SIZE):
    """([(name, X)], why A was dropped or None) for a buffer of `size` bytes at device address `base`."""
    a = (-int(base)) % (1 << 32)
    fixed = [("2^31", 1 << 31), ("2^32", 1 << 32)]
    for what, at in (("the buffer's start", 0), ("the buffer's end", size)) + tuple(fixed):
        if abs(a - at) < MARGIN:
            return fixed, f"A = {a:#x} lies within 4 MiB of {what}"
    return fixed + [("A", a)], None


def line_chunks(x, k, long_len=LONG):
    """(offsets, lengths) of the chunks at line x, the k-th line of its buffer."""
    table = [
        (x - (3001 + 2 * k), 3001 + 2 * k),        # ends exactly at x
        (x, 2053 + 2 * k),                         # starts exactly at x
        (x - 1, 5),
        (x + 1, 33),
        (x, 0),
        (x - 4096, 4096),                          # a crypt unit that ends at x
        (x, 4096),                                 # and one that starts there
        (x - (35003 + 3 * k), 70001),              # two 32 KiB compression spans, several ECC blocks at (10, 0)
        (x - (long_len // 2 + 7 + 5 * k), long_len),
    ]
    return [o for o, _ in table], [n for _, n in table]


@dataclass
class Layout:
    base: int
    size: int
    names: tuple
    xs: tuple
    dropped: object   # None, or why A is not among the lines
    offs: np.ndarray  # int64: the source chunks, PER_LINE per line, line after line
    lens: np.ndarray
    line_of: np.ndarray

    @property
    def n(self):
        return len(self.offs)

    def long_indices(self):
        return [k * PER_LINE + LONG_AT for k in range(len(self.xs))]

    def windows(self, near=False):
        """[(start, length)] of the window of every line (starts are multiples of 64 KiB)."""
        if near:
            return [(k * NEAR_STRIDE, WINDOW) for k in range(len(self.xs))]
        return [((x - HALF) & ~0xFFFF, WINDOW) for x in self.xs]

    def near(self, offs):
        """The twin of far offsets: window k moved to k * NEAR_STRIDE, low 16 bits kept."""
        offs = np.asarray(offs, np.int64)
        out = np.full(offs.shape, -1, np.int64)
        for k, (ws, wl) in enumerate(self.windows()):
            inside = (offs >= ws) & (offs < ws + wl)
            out[inside] = offs[inside] - ws + k * NEAR_STRIDE
        if (out < 0).any():
            raise ValueError("an offset outside every window has no twin")
        return out

    def slots(self, sizes, align=1, variant=0, lines_of=None):
        """Offsets of disjoint slots of `sizes` bytes, one per chunk, in this buffer's windows.
        lines_of[i]: the line whose window holds slot i (default: chunk i's line modulo this buffer's
        line count).  In every line the largest slot (the first of them) takes the role
        ROLES[(line + variant) % 3] at the line; the others, largest first, are packed below or
        above it, each on the side with more room left in the window (so two long slots that share
        a window, as when this buffer has fewer lines than the source, lie on opposite sides),
        GUARD + j bytes apart (so that, at align 1, offsets take many residues), at multiples of
        `align`."""
        sizes = np.asarray(sizes, np.int64)
        if lines_of is None:
            lines_of = self.line_of[:len(sizes)] % len(self.xs)
        lines_of = np.asarray(lines_of)
        offs = np.zeros(len(sizes), np.int64)
        for k, x in enumerate(self.xs):
            if x % align:
                raise ValueError(f"line {self.names[k]} is no multiple of {align}")
            members = [int(i) for i in np.flatnonzero(lines_of == k)]
            if not members:
                continue
            anchor = max(members, key=lambda i: int(sizes[i]))
            w = -(-int(sizes[anchor]) // align) * align
            role = ROLES[(k + variant) % 3]
            at = {"straddles": (x - w // 2) & ~(align - 1), "ends": x - w, "starts": x}[role]
            offs[anchor] = at
            low, high = at, at + w
            ws, wl = self.windows()[k]
            rest = sorted((m for m in members if m != anchor), key=lambda i: -int(sizes[i]))
            for j, i in enumerate(rest):
                s = int(sizes[i])
                if low - ws >= ws + wl - high:
                    low = (low - GUARD - j - s) & ~(align - 1)
                    offs[i] = low
                else:
                    offs[i] = -(-(high + GUARD + j) // align) * align
                    high = int(offs[i]) + s
            if low < ws + GUARD or high > ws + wl - GUARD:
                raise ValueError(f"the slots at line {self.names[k]} do not fit its window")
        return offs

    def role(self, k, variant):
        return ROLES[(k + variant) % 3]

    def struck(self, variant):
        """(line, index of its long chunk, whether its slot straddles the line): the chunk a call of
        this variant forges, corrupts or damages.  The line whose long slot straddles it; a buffer
        of two lines has none in variant 1, and then the first line's long chunk, whose slot ends at
        the line."""
        for k in range(len(self.xs)):
            if self.role(k, variant) == "straddles":
                return k, self.long_indices()[k], True
        return 0, self.long_indices()[0], False

    def aliases(self, offs, sizes):
        """[(slot, which, position)]: where a store to slot i would land inside this buffer had its
        offset lost 2^32 or 2^31, or kept only its low 32 bits.  The low-32-bit alias of a slot at or
        above 2^32 lies in no slot of the call (tests/test_far_layout.py), so the canary check of the
        GPU tests sees such a store; a "- 2^31" alias may fall into the slot of the line 2 GiB below,
        and there it is that slot's comparison with the oracle that sees it.  The GPU tests check
        every byte outside the slots, these positions among them, and do not single them out."""
        out = []
        for i, (o, s) in enumerate(zip(np.asarray(offs, np.int64).tolist(), np.asarray(sizes, np.int64).tolist())):
            if s == 0:
                continue
            for which, pos in (("- 2^32", o - (1 << 32)), ("- 2^31", o - (1 << 31)), ("mod 2^32", o % (1 << 32))):
                if pos != o and 0 <= pos and pos + s <= self.size:
                    out.append((i, which, pos))
        return out


def out_lines(src, out):
    """The line of the output buffer that holds the slot of every source chunk: its own line where
    the output buffer has it, else (the address line dropped there) folded onto the offset lines."""
    return src.line_of % len(out.xs)


def layout(base, size=SIZE, long_len=LONG):
    """The population of a buffer of `size` bytes at device address `base` (a multiple of 16)."""
    if base % 16:
        raise ValueError("the buffer's address must be a multiple of 16")
    named, dropped = lines(base, size)
    offs, lens, line_of = [], [], []
    for k, (_, x) in enumerate(named):
        o, n = line_chunks(x, k, long_len)
        offs += o
        lens += n
        line_of += [k] * PER_LINE
    return Layout(int(base), int(size), tuple(n for n, _ in named), tuple(x for _, x in named), dropped,
                  np.array(offs, np.int64), np.array(lens, np.int64), np.array(line_of, np.int64))


def split_by_window(windows, offs, sizes):
    """For every window, the (relative offsets, sizes) of the slots that lie in it; raises if a slot with
    bytes lies in none."""
    offs, sizes = np.asarray(offs, np.int64), np.asarray(sizes, np.int64)
    owner = np.full(len(offs), -1)
    out = []
    for k, (ws, wl) in enumerate(windows):
        inside = (offs >= ws) & (offs + sizes <= ws + wl)
        owner[inside] = k
        out.append((offs[inside] - ws, sizes[inside]))
    if (owner[sizes > 0] < 0).any():
        raise ValueError("a slot outside every window")
    return out


def outside_intact(host_windows, windows, offs, sizes, fill):
    """Whether every byte of the windows' host copies outside the slots still holds `fill`."""
    for buf, (rel, sz) in zip(host_windows, split_by_window(windows, offs, sizes)):
        edge = np.zeros(len(buf) + 1, np.int64)
        np.add.at(edge, rel, 1)
        np.add.at(edge, rel + sz, -1)
        if not (np.asarray(buf)[np.cumsum(edge[:-1]) <= 0] == fill).all():
            return False
    return True


def take(host_windows, windows, off, n):
    """Bytes [off, off + n) of the buffer, from the windows' host copies."""
    for buf, (ws, wl) in zip(host_windows, windows):
        if ws <= off and off + n <= ws + wl:
            return buf[off - ws:off - ws + n].tobytes()
    raise ValueError(f"[{off:#x}, +{n}) lies in no window")


def complement(windows, size, piece=256 << 20):
    """[(start, end)] covering [0, size) less the windows, in pieces of at most `piece` bytes."""
    out, pos = [], 0
    for ws, wl in sorted(windows) + [(size, 0)]:
        while pos < ws:
            end = min(ws, (pos // piece + 1) * piece)
            out.append((pos, end))
            pos = end
        pos = max(pos, ws + wl)
    return out
