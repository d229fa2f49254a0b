"""tests/index_dist_model.py -- the path finch_index_dist takes -- held to tests/dist_model.py's literal loop: for each
reference, for each query, the merge walk one hash at a time, the distance, the test.  And the soundness of the device's
pre-filter: no pair that the exact test keeps has a jaccard below jmin."""
import math
import struct

import numpy as np
import pytest

import dist_model as M
import index_dist_model as IDM

U64_MAX = (1 << 64) - 1
BELOW_ONE = math.nextafter(1.0, 0.0)
TINY = 5e-324


def bits(x):
    return struct.pack("<d", float(x))


def literal(queries, refs, old_mode, max_distance, equal):
    out = []
    for r in range(len(refs)):
        for q in range(len(queries)):
            if equal(q, r):
                continue
            d = M.distance(queries[q], refs[r], old_mode, walk=True, pinned=True)
            if d["mash_distance"] <= max_distance:
                out.append((q, r, d))
    return out


def same_rows(a, b):
    assert [(q, r) for q, r, _ in a] == [(q, r) for q, r, _ in b]
    for (_, _, x), (q, r, y) in zip(a, b):
        for f in ("containment", "jaccard", "mash_distance"):
            assert bits(x[f]) == bits(y[f]), (q, r, f, x, y)
        assert (x["common_hashes"], x["total_hashes"]) == (y["common_hashes"], y["total_hashes"]), (q, r)


def scaled_m(scale):
    return U64_MAX // int(1.0 / scale)


def sketches(seed, n, empties):
    """Mash and Scaled sketches of three scales and a NaN scale over a pool of 60 hashes that straddle the scales' max hashes,
    k of 11, 21 and 31, and `empties` empty sketches of both variants"""
    rng = np.random.default_rng(seed)
    lo, hi = scaled_m(0.001), scaled_m(0.01)
    pool = np.unique(np.concatenate([rng.integers(0, lo, 20, dtype=np.uint64), rng.integers(lo, hi, 20, dtype=np.uint64),
                                     rng.integers(hi, U64_MAX, 20, dtype=np.uint64), np.array([lo - 1, lo, hi - 1, hi], np.uint64)]))
    kinds = [("mash", 0.0, U64_MAX), ("scaled", 0.001, lo), ("scaled", 0.01, hi), ("scaled", 0.5, scaled_m(0.5)), ("scaled", math.nan, U64_MAX)]
    out = []
    for s in range(n):
        kind, scale, below = kinds[s % len(kinds)]
        own = pool[pool < np.uint64(below)]
        hs = own[rng.random(len(own)) < (0.9 if s % 3 == 0 else 0.5)]
        out.append(M.Sk(hs, kind, scale, (11, 21, 31)[s % 3]))
    for e in range(empties):
        out.append(M.Sk(np.zeros(0, np.uint64), *(("mash", 0.0), ("scaled", 0.01), ("scaled", math.nan))[e % 3], 21))
    return out


def distances_of(queries, refs, old_mode):
    return sorted({d["mash_distance"] for _, _, d in literal(queries, refs, old_mode, BELOW_ONE, lambda q, r: False)})


def bounds_for(queries, refs, old_mode):
    ds = [d for d in distances_of(queries, refs, old_mode) if 0.0 < d]
    mid = ds[len(ds) // 2]
    return [mid, math.nextafter(mid, 0.0), 0.0, -0.0, TINY, 0.1, BELOW_ONE, -1.0, math.nan]


@pytest.mark.parametrize("old_mode", [False, True])
def test_the_path_gives_the_literal_loop_rows(old_mode):
    refs = sketches(1, 12, 0 if old_mode else 3)
    queries = sketches(2, 9, 0 if old_mode else 3) + [refs[0], refs[4]]
    equal = lambda q, r: (q, r) in ((9 if old_mode else 12, 0),)  # noqa: E731  (one pair is skipped)
    for d in bounds_for(queries, refs, old_mode):
        rows, touched, copied, from_device = IDM.dist(queries, refs, old_mode, d, equal)
        same_rows(rows, literal(queries, refs, old_mode, d, equal))
        assert from_device <= copied <= touched
        if d == d and d >= 0:
            assert touched == sum(1 for q in queries for r in refs if len(np.intersect1d(q.hashes, r.hashes)))
    # the mid distance is kept at its own value and dropped just below it
    mid = bounds_for(queries, refs, old_mode)[0]
    at = {(q, r) for q, r, d in IDM.dist(queries, refs, old_mode, mid, equal)[0] if d["mash_distance"] == mid}
    below = {(q, r) for q, r, d in IDM.dist(queries, refs, old_mode, math.nextafter(mid, 0.0), equal)[0] if d["mash_distance"] == mid}
    assert at and not below


@pytest.mark.parametrize("old_mode", [False, True])
def test_pairwise_is_the_library_against_itself(old_mode):
    refs = sketches(3, 11, 0 if old_mode else 2)
    # a sketch is equal to itself unless its scale is NaN (f64 ==)
    equal = lambda q, r: q == r and not (refs[q].kind == "scaled" and refs[q].scale != refs[q].scale)  # noqa: E731
    for d in (0.0, 0.05, BELOW_ONE):
        rows, *_ = IDM.dist(None, refs, old_mode, d, equal)
        same_rows(rows, literal(refs, refs, old_mode, d, equal))
        nan_self = [(q, r) for q, r, _ in rows if q == r]
        assert nan_self and all(refs[q].scale != refs[q].scale for q, _ in nan_self)


def test_empty_sides_new_mode():
    """both sides empty; one side empty and the other Mash; the scale step finding nothing, and something, below M"""
    hi = scaled_m(0.01)
    refs = [M.Sk(np.zeros(0, np.uint64), "mash"), M.Sk(np.zeros(0, np.uint64), "scaled", 0.01), M.Sk(np.array([5, 9], np.uint64), "mash"),
            M.Sk(np.array([hi, hi + 7], np.uint64), "scaled", 0.01), M.Sk(np.array([hi - 1, hi], np.uint64), "scaled", 0.01),
            M.Sk(np.array([3], np.uint64), "scaled", math.nan)]
    queries = refs + [M.Sk(np.zeros(0, np.uint64), "scaled", 0.5, 31), M.Sk(np.zeros(0, np.uint64), "scaled", math.nan, 11)]
    none = lambda q, r: False  # noqa: E731
    for d in (0.0, -0.0, 0.3, BELOW_ONE):
        rows, touched, copied, from_device = IDM.dist(queries, refs, False, d, none)
        same_rows(rows, literal(queries, refs, False, d, none))
        host_made = [(q, r) for q, r, x in rows if x["total_hashes"] == 0]
        assert len(rows) - len(host_made) == from_device
        # (empty scaled 0.01, [hi, hi + 7] scaled 0.01): nothing below M, kept; (empty scaled 0.01, [hi - 1, hi]): one below M, dropped
        assert (1, 3) in host_made and (3, 1) in host_made and (1, 4) not in [(q, r) for q, r, _ in rows]
        assert (0, 2) in host_made and (2, 0) in host_made and (0, 0) in host_made and (7, 5) in host_made


def test_empty_sides_old_mode():
    empty, full = M.Sk(np.zeros(0, np.uint64)), M.Sk(np.array([1, 2, 3], np.uint64))
    none = lambda q, r: False  # noqa: E731
    # every pair whose reference is empty is kept: 0 / 0 ends in distance 0
    for queries, refs in (([full, full], [empty, full, empty]), ([empty, full], [empty, empty])):
        rows, *_ = IDM.dist(queries, refs, True, 0.0, none)
        same_rows(rows, literal(queries, refs, True, 0.0, none))
        assert sum(1 for _, r, d in rows if len(refs[r].hashes) == 0) == len(queries) * sum(1 for r in refs if len(r.hashes) == 0)
        assert all(d["jaccard"] != d["jaccard"] and d["mash_distance"] == 0.0 for _, r, d in rows if len(refs[r].hashes) == 0)
    with pytest.raises(M.ReferencePanics):
        IDM.dist([empty], [full], True, 0.5, none)
    with pytest.raises(M.ReferencePanics):
        literal([empty], [full], True, 0.5, none)


def test_a_bound_that_keeps_nothing():
    refs = sketches(4, 5, 1)
    for d in (math.nan, -1.0, -TINY, -math.inf):
        assert IDM.dist(None, refs, False, d, lambda q, r: False) == ([], 0, 0, 0)


# ----------------------------------------------------------------------------------------------------------------------
# the pre-filter: jaccard >= jmin(k, D) for every pair with mash_distance <= D.  k of every kind a sketch can have, D from 0
# and 1e-12 up to the largest double below 1, totals up to 2^32 - 2 (the most a pair can have), and c within 2 of the boundary
# c* = ceil(total x / (2 - x)) in real numbers -- the only place where the margin is tested; away from it the two tests agree
# by monotony.
# ----------------------------------------------------------------------------------------------------------------------

KS = (1, 4, 11, 21, 31, 32, 51, 64)
DISTANCES = [0.0, -0.0, TINY, 1e-12, 1e-9, 1e-6] + [float(x) for x in np.geomspace(1e-5, 0.999, 72)] + \
            [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -30, BELOW_ONE]
TOTALS = sorted({1, 2, 3, 5, 7, 63, 64, 65, 999, 1000, 1001, 3000, 10000, 2 ** 16, 2 ** 20 + 1, 2 ** 24 - 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3,
                 2 ** 32 - 2} | {int(x) for x in np.geomspace(1, 2 ** 32 - 2, 360)})


def test_pre_filter_is_sound():
    cases = kept_near = 0
    for k in KS:
        for d in DISTANCES:
            bound = IDM.jmin(k, d)
            x = math.exp(-k * max(d, 0.0))
            star = x / (2.0 - x)
            assert bound <= star
            for total in TOTALS:
                c0 = math.ceil(star * total)
                for c in range(max(c0 - 2, 0), min(c0 + 2, total) + 1):
                    cases += 1
                    jac = c / total  # (both below 2^53: Python's division is the IEEE division of the two doubles)
                    if M.mash_distance(jac, k) <= d:
                        kept_near += 1
                        assert jac >= bound, (k, d, total, c)
                    # old mode's form of the same pair: c common of |R| = (total + c) / 2 where that is whole
                    if (total + c) % 2 == 0:
                        assert c / (c + 2 * ((total + c) // 2 - c)) == jac
    assert cases > 1_000_000 and kept_near > cases // 4


def test_pre_filter_drops_something():
    """the bound is no formality: at k = 21 and D = 0.01 a pair that shares 1 of 100 hashes is dropped on the device"""
    assert IDM.device_jaccard(False, 1, 50, 51) < IDM.jmin(21, 0.01) < IDM.device_jaccard(False, 90, 95, 95)
    assert IDM.jmin(21, BELOW_ONE) > 0.0 and IDM.jmin(0, 0.5) == IDM.MARGIN and IDM.jmin(64, 0.0) == IDM.MARGIN
