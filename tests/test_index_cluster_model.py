"""The soundness of finch_index_cluster's three bands, swept the way tests/test_index_dist_model.py sweeps
finch_index_dist's pre-filter: the same k, the same bounds, the same totals, c within 2 of either boundary.  A pair the device
unites by itself (jaccard >= jhi, or jaccard 1) must be one the host's exact test keeps; a pair the device drops (jaccard <
jlo) must be one it drops.  At the default margin 2^-20 and at the tests' 0.25.  And tests/index_cluster_model.py's path through
the index against its own literal loop."""
import math

import numpy as np
import pytest

import dist_model as M
import index_cluster_model as ICM
from test_index_dist_model import BELOW_ONE, DISTANCES, KS, TOTALS, sketches


@pytest.mark.parametrize("m", [2.0 ** -20, 0.25])
def test_bands_are_sound(m):
    cases = sure = dropped = 0
    for k in KS:
        for d in DISTANCES:
            lo, hi = ICM.jlo(k, d), ICM.jhi(k, d, m)
            x = math.exp(-k * max(d, 0.0))
            star = x / (2.0 - x)
            assert lo <= star and lo < hi and (hi > star or star == 0.0)
            for total in TOTALS:
                near = set()
                for edge in (star, min(hi, 2.0)):  # c* of either boundary, in real numbers
                    c0 = math.ceil(edge * total)
                    near.update(range(max(c0 - 2, 0), min(c0 + 2, total) + 1))
                for c in sorted(near):
                    cases += 1
                    jac = c / total  # (both below 2^53: Python's division is the IEEE division of the two doubles)
                    keeps = M.mash_distance(jac, k) <= d
                    if jac >= hi or jac == 1.0:
                        sure += 1
                        assert keeps, (k, d, total, c)
                    elif jac < lo:
                        dropped += 1
                        assert not keeps, (k, d, total, c)
    assert cases > 1_000_000 and sure > cases // 10 and dropped > cases // 10


def test_jaccard_one_is_kept_at_every_k_and_bound():
    """the device's second rule: c == total is distance exactly 0, which every bound >= 0 keeps -- k = 0 included, where the
    distance is min(1, max(0, 0 / 0))"""
    for k in (0,) + KS + (745, 2 ** 32 - 1):
        assert ICM.mash_distance(1.0, k) == 0.0
        for d in DISTANCES:
            if d >= 0.0:
                assert ICM.mash_distance(1.0, k) <= d
    assert ICM.mash_distance(0.5, 0) == 1.0 and ICM.mash_distance(0.0, 0) == 1.0


def test_the_upper_bound_where_it_is_no_number():
    # D = 0: x = 1 and jhi = 1 + m, above every jaccard: only the second rule unites; x underflowed: +inf
    assert ICM.jhi(21, 0.0) == 1.0 + 2.0 ** -20 and ICM.jhi(21, -0.0) == ICM.jhi(21, 0.0)
    assert ICM.jhi(800, BELOW_ONE) == math.inf and ICM.jlo(800, BELOW_ONE) == 0.0
    assert ICM.jhi(745, BELOW_ONE) == math.inf  # (a subnormal x / (2 - x): no margin holds there)
    assert 0.0 < ICM.jlo(64, BELOW_ONE) < ICM.jhi(64, BELOW_ONE) < 1e-20


def test_the_bands_decide_something():
    """at k = 21 and D = 0.1 a near copy is united on the device and a pair that shares 1 hash of 100 is dropped there"""
    assert 1 / 100 < ICM.jlo(21, 0.1) < ICM.jhi(21, 0.1) < 90 / 100
    assert ICM.jhi(21, 0.1, 0.25) > ICM.jhi(21, 0.1) and ICM.jlo(21, 0.1) == ICM.jlo(21, 0.1)


@pytest.mark.parametrize("old_mode", [False, True])
def test_the_path_gives_the_literal_loop_edges(old_mode):
    """united + kept_host + the pairs with an empty side that pass = the literal loop's edges, at both margins"""
    lib = sketches(5, 14, 0 if old_mode else 3)
    for d in (0.0, 0.01, 0.1, 0.4, BELOW_ONE):
        pairs = ICM.passing(lib, old_mode, d)
        shares = lambda q, r: len(np.intersect1d(lib[q].hashes, lib[r].hashes)) > 0  # noqa: E731
        through_index = sum(1 for q, r in pairs if shares(q, r))
        for m in (2.0 ** -20, 0.25):
            b = ICM.bands(lib, old_mode, d, m)
            assert b["united"] + b["kept_host"] == through_index, (d, m, b)
            assert b["copied"] + b["united"] <= b["touched"]
        if not old_mode:  # the closed form of (i, j) as tests/index_model.py has it
            table = ICM.IM.postings(lib)
            for q in range(len(lib)):
                for r, c in ICM.IM.shared(table, lib[q]).items():
                    assert ICM.IM.closed_counts(lib[q], lib[r], c) == M.walk_counts(lib[q].hashes, lib[r].hashes, M.min_scale(lib[q], lib[r]))
        labels, edges = ICM.cluster(lib, old_mode, d)
        assert edges == len(pairs) and all(labels[v] <= v and labels[labels[v]] == labels[v] for v in range(len(lib)))
    for d in (math.nan, -1.0):
        assert ICM.cluster(lib, old_mode, d) == (list(range(len(lib))), 0)


def test_labels_of():
    assert ICM.labels_of(6, [(5, 4), (4, 3), (1, 0), (3, 1)]) == [0, 0, 2, 0, 0, 0]
    assert ICM.labels_of(3, []) == [0, 1, 2]
