"""The CPU candidate model (tests/long_model.py) against the C oracle: on the 5,000,000-byte KAT
input, the chunk rule walked over the model's candidates gives the oracle's cuts for both hashes
at five averages.  What tests/test_gpu_long_edges.py asserts about its inputs rests on this."""
import numpy as np
import pytest

import long_model as lm
from oracle import coracle

AVERAGES = [4096, 8192, 16384, 32768, 65536]


@pytest.fixture(scope="module", params=["buzhash", "rabinkarp"])
def kat_hashes(request, kat_data):
    data = np.frombuffer(kat_data, dtype=np.uint8)
    return request.param, data, lm.hashes(request.param, data)


@pytest.mark.parametrize("avg", AVERAGES)
def test_model_rule_matches_oracle(kat_hashes, avg):
    kind, data, h = kat_hashes
    cands = lm.candidates_of(h, avg)
    assert cands.size > data.size // avg // 2  # (about n / avg of them)
    got = lm.rule(cands, data.size, avg // 2, 2 * avg)
    np.testing.assert_array_equal(got, coracle.split_stream_kind(kind, avg, data))


@pytest.mark.parametrize("kind", ["buzhash", "rabinkarp"])
def test_model_hash_is_the_rolling_hash(kind):
    """hashes() against the byte-at-a-time rolling hash of oracle/rollinghash.py, from the zero
    window on; a slice is hashed like the whole (candidates_in)."""
    from oracle import rollinghash as rh
    data = coracle.gen_stream(7, 3, 700)
    data[200:300] = 0
    roll = rh.Buzhash32() if kind == "buzhash" else rh.RabinKarp64()
    want = []
    for b in data:
        roll.roll(int(b))
        want.append(roll.sum32() if kind == "buzhash" else roll.sum64())
    h = lm.hashes(kind, data)
    assert [int(v) for v in h] == want
    assert not h[263:300].any() and h[262] and h[300]  # a run of 63 + k zeros: k zero hashes
    for lo, hi in [(0, 700), (0, 10), (63, 64), (250, 320), (699, 700)]:
        np.testing.assert_array_equal(lm.candidates_in(kind, 4, data, lo, hi),
                                      [p for p in range(lo, hi) if want[p] & 3 == 0])


def test_segment_stats():
    c = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, lm.SEG - 6, lm.SEG - 5, lm.SEG, 3 * lm.SEG + 9])
    counts, unlisted = lm.segment_stats(c, 0, n=5 * lm.SEG - 1)
    assert counts.tolist() == [11, 1, 0, 1, 0]
    assert unlisted.tolist() == [8, lm.SEG - 6, lm.SEG - 5]
    counts, unlisted = lm.segment_stats(c, 5)  # coordinates shift by 5: SEG - 5 opens segment 1
    assert counts.tolist() == [10, 2, 0, 1]
    assert unlisted.tolist() == [8, lm.SEG - 6]
    assert lm.segment_stats([], 3)[0].size == 0


def test_rule_forced_cuts_and_tail():
    assert lm.rule([], 10, 4, 8).tolist() == [8, 10]          # tail shorter than min
    assert lm.rule([], 11, 4, 8).tolist() == [8, 11]          # lo == n
    assert lm.rule([], 12, 4, 8).tolist() == [8, 12]          # lo == n - 1, no candidate
    assert lm.rule([10], 12, 4, 8).tolist() == [8, 12]        # a candidate below lo does not cut
    assert lm.rule([10, 11], 13, 4, 8).tolist() == [8, 12, 13]
    assert lm.rule([2, 3, 11], 30, 4, 8).tolist() == [4, 12, 20, 28, 30]
