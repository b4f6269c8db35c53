"""Inputs shared by tests/test_dedup_model.py (CPU, through build/dedup_host) and
tests/test_gpu_dedup.py: sequences of calls on one content-ID set.  Everything is seeded."""
from dataclasses import dataclass, field

import numpy as np

from dedup_model import id_list


@dataclass
class Call:
    op: str  # claim, insert, lookup, clear, grow
    ids: np.ndarray = None  # uint8 [n, id_len]
    prefix: int = 0
    stride: int = 0  # 0: id_len
    offset: int = 0  # byte offset of ID 0 in its buffer
    max_keys: int = 0  # grow


@dataclass
class Vec:
    tag: str
    id_len: int
    max_keys: int
    calls: list = field(default_factory=list)


def slot_count(max_keys):
    """Slots of a set: the power of two from 16 up that holds two per key."""
    s = 16
    while s < 2 * max_keys:
        s *= 2
    return s


def buffer_of(call, id_len):
    """The bytes a call's IDs lie in: `offset` filler bytes, then the IDs `stride` apart with filler
    between them, and not one byte after the last ID."""
    n = len(call.ids)
    stride = call.stride or id_len
    rng = np.random.default_rng(n + stride)
    rows = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    rows[:, :id_len] = call.ids
    body = rows.ravel()[:(n - 1) * stride + id_len] if n else rows.ravel()
    return np.concatenate([rng.integers(0, 256, call.offset, dtype=np.uint8), body])


def rand_ids(rng, n, id_len):
    return rng.integers(0, 256, (n, id_len), dtype=np.uint8)


def with_repeats(rng, distinct, n):
    """n rows: every row of `distinct` at least once, the rest repeats, in shuffled positions."""
    pick = np.concatenate([np.arange(len(distinct)), rng.integers(0, len(distinct), n - len(distinct))])
    rng.shuffle(pick)
    return distinct[pick]


def size_vectors():
    """Case 1: n = 0, 1, 63, 64, 65 at every id_len, stride and byte offset; each claim repeats a few
    of the IDs before it and of its own."""
    vecs = []
    for id_len in (16, 28, 32):
        for stride in (id_len, id_len + 7):
            for offset in (0, 1, 3):
                rng = np.random.default_rng(id_len * 100 + stride * 10 + offset)
                v = Vec(f"sizes-len{id_len}-stride{stride}-off{offset}", id_len, 400)
                old = rand_ids(rng, 5, id_len)
                v.calls.append(Call("insert", old, stride=stride, offset=offset))
                for n in (0, 1, 63, 64, 65):
                    ids = rand_ids(rng, n, id_len)
                    if n >= 63:
                        ids[7], ids[n - 1], ids[40] = old[n % 5], ids[3], ids[3]
                    v.calls.append(Call("claim", ids, stride=stride, offset=offset))
                    v.calls.append(Call("lookup", np.concatenate([ids, rand_ids(rng, 3, id_len)]), stride=stride,
                                        offset=offset))
                vecs.append(v)
    return vecs


def copies_vectors():
    """Case 2: 64 and 200 copies of one ID: a whole wave and more race for one slot."""
    vecs = []
    for n in (64, 200):
        one = rand_ids(np.random.default_rng(n), 1, 16)
        vecs.append(Vec(f"copies{n}", 16, 256, [Call("claim", np.repeat(one, n, axis=0))]))
    return vecs


def shuffled_ids(seed=3, n=4096, distinct=512, id_len=16):
    rng = np.random.default_rng(seed)
    return with_repeats(rng, rand_ids(rng, distinct, id_len), n)


def shuffled_vector():
    """Case 3: 4,096 IDs with 512 distinct values in shuffled positions."""
    return Vec("shuffled", 16, 4096, [Call("claim", shuffled_ids())])


def repeat_vector():
    """Case 4: a second claim with half the IDs old, a third identical one."""
    rng = np.random.default_rng(4)
    a = rand_ids(rng, 300, 28)
    b = np.concatenate([a[rng.permutation(300)[:150]], rand_ids(rng, 150, 28)])
    rng.shuffle(b)
    return Vec("repeat", 28, 1000, [Call("claim", a), Call("claim", b), Call("claim", b)])


def twins_vector(id_len=32):
    """Case 5: near twins, all distinct: equal in bytes 0-7, 0-15 and 0-(id_len - 2), differing only
    later; IDs that differ only in prefix; the same ID with the same prefix, which is equal."""
    rng = np.random.default_rng(5)
    base = rand_ids(rng, 1, id_len)[0]
    rows = [base.copy()]
    for keep in (8, 16, id_len - 1):
        for k in range(1, 4):
            t = base.copy()
            t[keep:] = rand_ids(rng, 1, id_len)[0][keep:]
            t[id_len - 1] = (int(base[id_len - 1]) + k + keep) % 256  # differs in the last byte for sure
            rows.append(t)
    ids = np.stack(rows)
    assert len({r.tobytes() for r in ids}) == len(ids)
    both = np.concatenate([ids, ids])
    return Vec(f"twins-len{id_len}", id_len, 100, [
        Call("claim", both, prefix=ord("k")), Call("claim", ids, prefix=0), Call("claim", ids, prefix=ord("x")),
        Call("claim", ids, prefix=ord("k")), Call("lookup", ids, prefix=ord("m")), Call("grow", max_keys=200),
        Call("lookup", ids, prefix=ord("x")), Call("lookup", ids, prefix=ord("m")), Call("claim", both, prefix=0)])


def one_home_ids(home, id_len=16, max_keys=512, count=300, back=3, prefix=0, seed=6):
    """Case 6: `count` distinct IDs whose home slot is the table's `back`-th last, by brute force over
    home(id) (kcdc_test_dedup_home); returns (ids, slot)."""
    rng = np.random.default_rng(seed)
    target, got = slot_count(max_keys) - back, []
    while len(got) < count:
        block = rand_ids(rng, 65536, id_len)
        for i, one in enumerate(id_list(block)):
            if home(id_len, max_keys, prefix, one) == target:
                got.append(block[i])
                if len(got) == count:
                    break
    return np.stack(got), target


def one_home_vector(home):
    ids, _ = one_home_ids(home)
    return Vec("one-home", 16, 512, [Call("claim", ids), Call("lookup", ids), Call("claim", ids[::-1][:200].copy())])


def full_vector():
    """Case 7: a fill to exactly max_keys, a refused claim, a grow that makes room."""
    rng = np.random.default_rng(7)
    ids = rand_ids(rng, 1001, 16)
    return Vec("full", 16, 1000, [
        Call("claim", ids[:600]), Call("insert", ids[600:1000]), Call("claim", ids[1000:]), Call("lookup", ids[:1000]),
        Call("claim", ids[:2]), Call("insert", ids[:1]), Call("lookup", ids[999:]),
        Call("grow", max_keys=4000), Call("claim", ids[1000:]), Call("lookup", ids)])


def lookup_vector():
    """Case 8: a lookup changes nothing: the claim after it answers as if it had not happened."""
    rng = np.random.default_rng(8)
    a, b = rand_ids(rng, 200, 16), rand_ids(rng, 200, 16)
    mixed = np.concatenate([a[:100], b])
    return Vec("lookup", 16, 1000, [Call("claim", a), Call("lookup", mixed), Call("lookup", mixed), Call("claim", mixed)])


def clear_vector():
    """Case 9: clear, then reuse."""
    rng = np.random.default_rng(9)
    a = rand_ids(rng, 500, 16)
    return Vec("clear", 16, 1000, [Call("claim", a), Call("clear"), Call("lookup", a), Call("claim", a[100:]),
                                  Call("claim", a)])


def small_vectors(home):
    return (size_vectors() + copies_vectors() +
            [shuffled_vector(), repeat_vector(), twins_vector(32), twins_vector(28), one_home_vector(home), full_vector(),
             lookup_vector(), clear_vector()])


def mixed_ids(seed, n, dup_percent, id_len=16):
    """n random IDs of which about dup_percent repeat an earlier one."""
    rng = np.random.default_rng(seed)
    distinct = rand_ids(rng, n - n * dup_percent // 100, id_len)
    return with_repeats(rng, distinct, n)
