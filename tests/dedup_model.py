"""The dedup decision as the literal loop: WriteContent's lookup between hashData and
addToPackUnlocked (repo/content/content_manager.go:812-842) over a Python dict fed in index order.
A content whose ID is tracked is deduplicated; any other is added and tracked from then on.  The
device calls of include/kcdc.h ("content dedup") must answer exactly as this does."""
import numpy as np

KNOWN = 0xFFFFFFFF  # KCDC_DEDUP_KNOWN
ENOSPC = -28


def id_list(ids, id_len=None):
    """Rows of a uint8 array [n, id_len] as bytes objects."""
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    if ids.shape[0] == 0:
        return []
    return ids.view(np.dtype((np.void, ids.shape[1]))).ravel().tolist()


class Model:
    def __init__(self, max_keys: int):
        self.max_keys = max_keys
        self.tracked = {}  # (prefix, id bytes) -> (call number, index in that call)
        self.calls = 0

    def __len__(self):
        return len(self.tracked)

    def claim(self, ids, prefix: int = 0):
        """(keep, first, (status, new, stored)) for the IDs one after another."""
        ids = id_list(ids)
        self.calls += 1
        if len(self.tracked) + len(ids) > self.max_keys:  # the conservative rule, for the whole call
            return [0] * len(ids), [KNOWN] * len(ids), (ENOSPC, 0, len(self.tracked))
        keep, first = [], []
        before = len(self.tracked)
        for i, one in enumerate(ids):
            key = (prefix, one)
            if key in self.tracked:
                call, index = self.tracked[key]
                keep.append(0)
                first.append(index if call == self.calls else KNOWN)
            else:
                self.tracked[key] = (self.calls, i)
                keep.append(1)
                first.append(i)
        return keep, first, (0, len(self.tracked) - before, len(self.tracked))

    def insert(self, ids, prefix: int = 0):
        return self.claim(ids, prefix)[2]

    def lookup(self, ids, prefix: int = 0):
        return [1 if (prefix, one) in self.tracked else 0 for one in id_list(ids)]

    def clear(self):
        self.tracked.clear()

    def grow(self, max_keys: int):
        """(the larger model, totals): every key of this one inserted into an empty set."""
        to = Model(max_keys)
        if len(self.tracked) > max_keys:
            return to, (ENOSPC, 0, 0)
        to.tracked = {k: (0, 0) for k in self.tracked}
        return to, (0, len(to.tracked), len(to.tracked))


def run(vec):
    """The expected result of every call of a dedup_cases.Vec, in the form the host program's
    output and the GPU runner's are brought to."""
    m = Model(vec.max_keys)
    out = []
    for c in vec.calls:
        if c.op == "claim":
            keep, first, t = m.claim(c.ids, c.prefix)
            out.append(("t", *t, keep, first))
        elif c.op == "insert":
            out.append(("t", *m.insert(c.ids, c.prefix)))
        elif c.op == "lookup":
            out.append(("l", m.lookup(c.ids, c.prefix)))
        elif c.op == "clear":
            m.clear()
            out.append(("c",))
        elif c.op == "grow":
            m, t = m.grow(c.max_keys)
            out.append(("t", *t))
        else:
            raise ValueError(c.op)
    return out
