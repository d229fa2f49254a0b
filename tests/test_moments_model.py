"""tests/moments_model.py's two statements of compare_counts held to each other: the loop as written (python.rs:496-559) against
the integers stated on sets and the central sums stated in Fractions."""
import math
from fractions import Fraction

import numpy as np

import moments_model as MM


def random_sketch(rng, universe, n, counts=MM.COUNTS):
    hs = sorted(int(x) for x in rng.choice(universe, size=min(n, universe), replace=False))
    return [(h, int(rng.choice(counts))) for h in hs]


def test_integers_equal_the_walk():
    rng = np.random.default_rng(7)
    seen = {"empty_ref": 0, "empty_query": 0, "disjoint": 0, "ref_stops_early": 0, "query_stops_early": 0}
    for _ in range(600):
        universe = int(rng.choice([6, 20, 60]))
        ref = random_sketch(rng, universe, int(rng.integers(0, 12)))
        query = random_sketch(rng, universe, int(rng.integers(0, 12)))
        got = MM.walk_sums(ref, query)
        assert got[:5] == MM.integers(ref, query), (ref, query)
        seen["empty_ref"] += not ref
        seen["empty_query"] += not query
        seen["disjoint"] += bool(ref) and bool(query) and got[0] == 0
        seen["ref_stops_early"] += got[1] < len(ref)
        seen["query_stops_early"] += got[2] < len(query)
    assert all(v >= 10 for v in seen.values()), seen


def test_by_hand():
    ref = [(1, 5), (3, 7), (4, 1), (9, 2), (12, 1)]
    query = [(0, 1), (3, 2), (4, 4), (9, 6), (10, 1)]
    common, ref_pos, query_pos, ref_count, query_count, var, skew, kurt = MM.compare_counts(ref, query)
    # shared: 3, 4, 9; the query runs out at 10 < 12 with the reference at index 4
    assert (common, ref_pos, query_pos, ref_count, query_count) == (3, 4, 5, 10, 12) == MM.integers(ref, query)
    # the query's shared counts 2, 4, 6: mean 4, population variance 8 / 3, symmetric, kurtosis of three equidistant points 1.5
    assert math.isclose(var, 8 / 3, rel_tol=1e-15) and abs(skew) < 1e-15 and math.isclose(kurt + 3.0, 1.5, rel_tol=1e-14)
    assert MM.central_sums(ref, query) == (3, Fraction(4), Fraction(8), Fraction(0), Fraction(32))


def test_nan_cases_are_the_contract():
    one = [(5, 3)]
    for ref, query in (([], []), ([], one), (one, []), (one, one), ([(1, 1)], [(2, 1)]),
                       ([(1, 9), (2, 9), (3, 9)], [(1, 4), (2, 4), (3, 4)])):
        t = MM.compare_counts(ref, query)
        assert t[:5] == MM.integers(ref, query)
        common = t[0]
        var, skew, kurt = t[5:]
        assert math.isnan(skew) and math.isnan(kurt), (ref, query, t)
        assert math.isnan(var) if common == 0 else var == 0.0
    assert MM.same(MM.compare_counts([], []), (0, 0, 0, 0, 0, float("nan"), -float("nan"), float("nan")))
    assert not MM.same((1, 0, 0, 0, 0, 0.0, 0.0, 0.0), (1, 0, 0, 0, 0, -0.0, 0.0, 0.0))  # bit patterns, not ==


def test_the_recurrence_computes_the_central_sums():
    """small counts: every intermediate is far from overflow, so the doubles are close to the exact sums (the loop is not exact;
    a relative 1e-9 of the sum's scale is far above its rounding and far below any mistake in a coefficient)"""
    rng = np.random.default_rng(11)
    checked = 0
    for _ in range(200):
        ref = random_sketch(rng, 80, int(rng.integers(2, 60)), counts=(1, 2, 3, 7, 50))
        query = random_sketch(rng, 80, int(rng.integers(2, 60)), counts=(1, 2, 3, 7, 50))
        exact = MM.central_sums(ref, query)
        if exact is None or exact[0] < 2 or exact[2] == 0:
            continue
        n, mean, s2, s3, s4 = exact
        common, _, _, _, query_count, m2, m3, m4 = MM.walk_sums(ref, query)
        assert common == n and Fraction(query_count, common) == mean
        scale = float(s2) ** 0.5
        assert abs(float(m2) - float(s2)) <= 1e-9 * scale ** 2
        assert abs(float(m3) - float(s3)) <= 1e-9 * scale ** 3 * n
        assert abs(float(m4) - float(s4)) <= 1e-9 * scale ** 4 * n
        var, skew, kurt = MM.finish(common, m2, m3, m4)
        assert math.isclose(var, float(s2 / n), rel_tol=1e-9)
        assert math.isclose(kurt + 3.0, float(n * s4 / (s2 * s2)), rel_tol=1e-8)
        assert abs(skew - float(s3) * n ** 0.5 / float(s2) ** 1.5) <= 1e-8
        checked += 1
    assert checked >= 100


def test_order_matters_to_the_doubles_only():
    """the same shared multiset in another hash order: the integers stay, the doubles may move -- which is why the device has to
    visit the shared hashes in hash order"""
    big = 2 ** 32 - 1
    ref = [(h, 1) for h in range(1, 9)]
    q1 = [(h, c) for h, c in zip(range(1, 9), (1, big, 2, 3, big, 1, 2, 3))]
    q2 = [(h, c) for h, c in zip(range(1, 9), (big, big, 3, 3, 2, 2, 1, 1))]
    a, b = MM.compare_counts(ref, q1), MM.compare_counts(ref, q2)
    assert a[:5] == b[:5] == MM.integers(ref, q1)
    assert not MM.same(a, b)


def test_rows_order_and_threshold():
    refs = [[(1, 1), (2, 2)], [], [(2, 5), (3, 1), (4, 1)], [(9, 1)]]
    queries = [[(2, 3), (3, 4)], [(1, 1), (2, 1), (3, 1), (4, 1)]]
    all_rows = MM.rows(refs, queries)
    assert [(q, r) for q, r, _ in all_rows] == [(q, r) for q in range(2) for r in range(4)]
    assert [t[0] for _, _, t in all_rows] == [1, 0, 2, 0, 2, 0, 3, 0]
    assert [(q, r) for q, r, _ in MM.rows(refs, queries, 2)] == [(0, 2), (1, 0), (1, 2)]
    assert [(q, r) for q, r, _ in MM.rows(refs, queries, 3)] == [(1, 2)]
    assert MM.rows(refs, queries, 4) == []
