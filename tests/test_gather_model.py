"""tests/gather_model.py's two statements of the gather contract held to each other, and the two facts that make the device's
form exact: a reference's count never grows from round to round, and a chosen reference is never chosen again."""
import math
import struct

import numpy as np
import pytest

import gather_model as GM


def bits(x):
    return struct.pack("<d", float(x))


def same_rows(a, b):
    assert len(a) == len(b), (a, b)
    for x, y in zip(a, b):
        for f in GM.INTS:
            assert x[f] == y[f], (f, x, y)
        for f in GM.DOUBLES:
            assert bits(x[f]) == bits(y[f]) or (math.isnan(x[f]) and math.isnan(y[f])), (f, x, y)


def random_library(seed):
    """a small hash universe: intersections, ties and subsets everywhere"""
    rng = np.random.default_rng(seed)
    pool = np.arange(1, int(rng.integers(4, 40)), dtype=np.uint64) * 5

    def sk(max_size):
        n = int(rng.integers(0, min(max_size, len(pool)) + 1))
        hs = np.sort(rng.choice(pool, size=n, replace=False))
        return GM.Sk(hs, rng.integers(1, 1000, n))

    refs = [sk(12) for _ in range(int(rng.integers(0, 12)))]
    return sk(len(pool)), refs


def test_by_hand_greedy_order_is_not_the_order_by_common():
    # A contains B, C is apart from A: by `common` the order is A, B, C; the rounds are A, then C -- B has nothing left
    q = GM.Sk(range(1, 11), range(10, 110, 10))
    a, b, c = GM.Sk([1, 2, 3, 4, 5, 6]), GM.Sk([1, 2, 3, 4, 5]), GM.Sk([7, 8, 9, 99])
    for fn in (GM.gather_sets, GM.gather_mask):
        rows = fn(q, [b, a, c])
        assert [(r["reference"], r["overlap"], r["common"], r["remaining"]) for r in rows] == [(1, 6, 6, 4), (2, 3, 3, 1)]
        assert [r["abund"] for r in rows] == [10 + 20 + 30 + 40 + 50 + 60, 70 + 80 + 90]
        assert rows[1]["f_match"] == 3 / 4 and rows[1]["f_unique_to_query"] == 0.3 and rows[0]["average_abund"] == 35.0
        assert rows[0]["f_unique_weighted"] == 210 / 550
    # with a hash of its own, B comes back last, with what the others left it
    b2 = GM.Sk([1, 2, 3, 4, 5, 10])
    rows = GM.gather_sets(q, [b2, a, c])
    assert [(r["reference"], r["overlap"], r["common"]) for r in rows] == [(0, 6, 6), (2, 3, 3), (1, 1, 6)]  # a tie at 6: the lower index
    same_rows(rows, GM.gather_mask(q, [b2, a, c]))


def test_stops():
    q = GM.Sk([1, 2, 3, 4, 5, 6])
    refs = [GM.Sk([1, 2, 3]), GM.Sk([4, 5]), GM.Sk([6]), GM.Sk([])]
    for fn in (GM.gather_sets, GM.gather_mask):
        assert [r["reference"] for r in fn(q, refs)] == [0, 1, 2]
        assert [r["reference"] for r in fn(q, refs, 0)] == [0, 1, 2]  # below 1 is 1: the empty reference explains nothing
        assert [r["reference"] for r in fn(q, refs, -5)] == [0, 1, 2]
        assert [r["reference"] for r in fn(q, refs, 2)] == [0, 1]
        assert [r["reference"] for r in fn(q, refs, 4)] == []
        assert [r["reference"] for r in fn(q, refs, 1, 1)] == [0]
        assert [r["reference"] for r in fn(q, refs, 1, 2)] == [0, 1]
        assert [r["reference"] for r in fn(q, refs, 1, 9)] == [0, 1, 2]
        assert fn(GM.Sk([]), refs) == [] and fn(q, []) == [] and fn(GM.Sk([77]), refs) == []


def test_doubles_are_ieee():
    assert math.isnan(GM.ieee_div(0, 0)) and GM.ieee_div(3, 0) == math.inf and GM.ieee_div(1, 3) == 1 / 3
    rows = GM.gather_sets(GM.Sk([1, 2], [0, 0]), [GM.Sk([1, 2])])  # (counts no sketcher emits: the division is not guarded)
    assert rows[0]["average_abund"] == 0.0 and math.isnan(rows[0]["f_unique_weighted"])
    big = GM.gather_sets(GM.Sk([1, 2, 3], [0xffffffff] * 3), [GM.Sk([1, 2, 3])])
    assert big[0]["abund"] == 3 * 0xffffffff > 1 << 32


@pytest.mark.parametrize("block", range(8))
def test_two_statements_agree(block):
    seen = {"rows": 0, "ties": 0, "dropped": 0}
    for seed in range(block * 60, block * 60 + 60):
        q, refs = random_library(seed)
        for min_overlap in (0, 1, 3, 50):
            for max_rounds in (0, 1, 2):
                trace = []
                a = GM.gather_sets(q, refs, min_overlap, max_rounds, trace=trace)
                same_rows(a, GM.gather_mask(q, refs, min_overlap, max_rounds))
                seen["rows"] += len(a)
                seen["ties"] += any(sorted(c)[-1] == sorted(c)[-2] > 0 for c in trace if len(c) > 1)
                seen["dropped"] += bool(trace) and sum(c >= max(1, min_overlap) for c in trace[0]) > len(a) and max_rounds == 0
    assert all(v > 20 for v in seen.values()), seen


def test_counts_never_grow_and_no_reference_twice():
    for seed in range(300):
        q, refs = random_library(seed)
        for min_overlap in (1, 3):
            trace = []
            rows = GM.gather_sets(q, refs, min_overlap, trace=trace)
            for before, after in zip(trace, trace[1:]):
                assert all(y <= x for x, y in zip(before, after)), seed
            chosen = [r["reference"] for r in rows]
            assert len(set(chosen)) == len(chosen), seed
            for t, r in enumerate(rows):  # a chosen reference has c = 0 afterwards
                assert all(c[r["reference"]] == 0 for c in trace[t + 1:]), seed
            if trace:
                candidates = sum(c >= min_overlap for c in trace[0])
                assert len(rows) <= candidates, seed
                # a reference that starts below min_overlap never wins; one that falls below it never comes back
                assert all(trace[0][w] >= min_overlap for w in chosen), seed
            assert [r["round"] for r in rows] == list(range(len(rows)))
            if rows:
                assert rows[-1]["remaining"] == rows[0]["query_len"] - sum(r["overlap"] for r in rows)
                assert sum(r["abund"] for r in rows) <= sum(q.counts)
