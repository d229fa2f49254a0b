"""The distance model (tests/dist_model.py) against the reference's own expected values, its vectorized counts against its
literal walks, and the library's host path (finch_raw_distance, finch_distance) against the model: the same counts and
every double the same bits, over the scales where the scale step changes (1 / scale not an integer, no step, saturation,
NaN) and the clamps of mash_distance.  No device needed."""
import math
import struct

import mpmath
import numpy as np
import pytest

import dist_model as M
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

U64_MAX = M.U64_MAX
NAN = float("nan")
ORDINARY = [0.001, 0.01, 0.3, 1.0]
NO_STEP = [0.0, -0.5]
SATURATING = [1e-20, 5e-324]  # M = 1: 1 / scale is >= 2^64, or inf
SCALES = ORDINARY + NO_STEP + SATURATING + [NAN]
PANICS = [2.0, 1.5, 1e300, math.inf]  # 1 / scale as u64 is 0: the reference divides by zero


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def bits(x):
    return struct.pack("<d", float(x))


def same_double(a, b):
    """the same bits; any NaN matches any NaN (the sign of a 0 / 0 NaN is the hardware's, and serde_json writes null)"""
    return (a != a and b != b) or bits(a) == bits(b)


def same_distance(got, want, what=""):
    for f in ("containment", "jaccard", "mash_distance"):
        assert same_double(got[f], want[f]), (what, f, got, want)
    assert int(got["common_hashes"]) == want["common_hashes"] and int(got["total_hashes"]) == want["total_hashes"], (what, got, want)


def boundary_hashes():
    """0, u64::MAX, and M - 1, M, M + 1 of every scale with a step"""
    hs = {0, 1, 2, U64_MAX - 1, U64_MAX}
    for s in ORDINARY + SATURATING:
        m = M.max_hash(s)
        hs.update(x for x in (m - 1, m, m + 1) if 0 <= x <= U64_MAX)
    return sorted(hs)


# ----------------------------------------------------------------------------------------------------------------------
# the model itself
# ----------------------------------------------------------------------------------------------------------------------

def test_max_hash_and_cast():
    assert M.max_hash(0.001) == U64_MAX // 1000 and M.max_hash(1.0) == U64_MAX
    assert M.max_hash(0.3) == U64_MAX // 3  # 1 / 0.3 = 3.33.. truncates
    assert M.max_hash(1e-18) == 18  # the reference's own note (distance.rs test_raw_distance_scaled)
    assert M.max_hash(1e-20) == 1 and M.max_hash(5e-324) == 1  # the cast saturates at u64::MAX
    assert [M.as_u64(x) for x in (NAN, -3.5, -0.0, 0.99, 2.7, 2.0 ** 64, math.inf)] == [0, 0, 0, 0, 2, U64_MAX, U64_MAX]
    assert M.as_u64(2.0 ** 64 - 2048) == 2 ** 64 - 2048
    for s in PANICS:
        with pytest.raises(M.ReferencePanics):
            M.max_hash(s)
        assert M.max_hash(s, pinned=True) == U64_MAX


def test_f64_min_ignores_nan():
    assert M.f64_min(NAN, 0.5) == 0.5 and M.f64_min(0.5, NAN) == 0.5 and math.isnan(M.f64_min(NAN, NAN))
    assert M.f64_min(0.3, 0.001) == 0.001 and M.f64_max(NAN, 0.0) == 0.0 and M.f64_max(-1.0, NAN) == -1.0


def test_reference_expected_values():
    # distance.rs test_raw_distance and test_raw_distance_scaled (1e-18 gives a max hash of 18): the values only
    cases = [
        ([0, 1, 2], [1, 2], 0., (2. / 2., 2. / 3., 2, 3)),
        ([0, 2], [1, 2], 0., (1. / 2., 1. / 3., 1, 3)),
        ([0, 1], [2, 3], 0., (0. / 2., 0. / 2., 0, 2)),
        ([], [], 0., (0., 1., 0, 0)),
        ([], [5], 0., (0., 1., 0, 0)),
        ([10, 15, 20], [15, 20], 1e-18, (2. / 2., 2. / 3., 2, 3)),
        ([5, 10, 15], [5, 10], 1e-18, (2. / 2., 2. / 3., 2, 3)),
        ([5, 10, 15, 20], [5, 10], 1e-18, (2. / 2., 2. / 3., 2, 3)),
        ([5, 10], [5, 10, 15, 20], 1e-18, (2. / 3., 2. / 3., 2, 3)),
    ]
    for q, r, s, want in cases:
        assert M.raw_distance(q, r, s) == want, (q, r, s)
        assert M.raw_from_counts(*M.counts(q, r, M.max_hash(s) if s > 0 else None)) == want
        assert H.raw_distance(q, r, s) == want
    # test_distance_scaled: two equal Scaled sketches of three hashes
    a = M.Sk([11, 22, 33], "scaled", 0.001, 3)
    d = M.distance(a, a, walk=True)
    assert (d["jaccard"], d["containment"], d["common_hashes"]) == (1.0, 1.0, 3)
    # test_raw_distance_commutes (without a scale; its random u64 lists almost never share a hash, so containment, which
    # is |Q n R| / j, is compared there only by chance: here jaccard and the two counts)
    rng = np.random.default_rng(1)
    for _ in range(300):
        q = sorted(set(rng.integers(0, 50, rng.integers(0, 20)).tolist()))
        r = sorted(set(rng.integers(0, 50, rng.integers(0, 20)).tolist()))
        assert M.raw_distance(q, r, 0.)[1:] == M.raw_distance(r, q, 0.)[1:]


def test_old_distance_as_written():
    # the clamp: the query cursor never passes its last hash, so a reference hash equal to it still counts
    assert M.old_walk_counts([5], [1, 5, 9]) == (1, 3)
    assert M.old_walk_counts([1, 2, 3], []) == (0, 0)
    c = M.old_distance([], [])
    assert math.isnan(c[0]) and math.isnan(c[1]) and c[2:] == (0, 0)
    with pytest.raises(M.ReferencePanics):
        M.old_walk_counts([], [1])
    with pytest.raises(M.ReferencePanics):
        M.old_counts([], [1])


N_RANDOM, N_BOUNDARY = 14000, 6000


def pair_sets():
    """(query, ref) pairs of strictly ascending hash lists: random, adversarial, and the boundary hashes"""
    rng = np.random.default_rng(2024)
    pairs = []
    for _ in range(N_RANDOM):  # random: a small universe for overlaps, then the full range
        hi = [8, 64, 1000, U64_MAX][rng.integers(0, 4)]
        q = np.unique(rng.integers(0, hi, rng.integers(0, 40), dtype=np.uint64, endpoint=True))
        r = np.unique(rng.integers(0, hi, rng.integers(0, 40), dtype=np.uint64, endpoint=True))
        pairs.append((q.tolist(), r.tolist()))
    bnd = boundary_hashes()
    for _ in range(N_BOUNDARY):  # subsets of the boundary hashes, with a few random ones between them
        q = sorted(set(x for x in bnd if rng.random() < 0.4) | set(rng.integers(0, U64_MAX, rng.integers(0, 4), dtype=np.uint64).tolist()))
        r = sorted(set(x for x in bnd if rng.random() < 0.4) | set(rng.integers(0, U64_MAX, rng.integers(0, 4), dtype=np.uint64).tolist()))
        pairs.append((q, r))
    shapes = [[], [0], [U64_MAX], [7], list(range(10, 20)), list(range(100, 110)), list(range(10, 30, 2)), list(range(11, 31, 2)),
              list(range(5, 25)), [0, U64_MAX], bnd, bnd[::2], bnd[1::2], bnd[:5], bnd[-5:]]
    for a in shapes:  # empty, single, disjoint, interleaved, identical, one inside the other; both ways round
        for b in shapes:
            pairs.append((a, b))
    return pairs


def test_vectorized_counts_equal_the_walks():
    pairs = pair_sets()
    steps = [s for s in SCALES if s > 0]
    assert len(pairs) >= 20000
    for n, (q, r) in enumerate(pairs):
        for s in (steps[n % len(steps)], 0.0):  # one scale with a step per pair, and no step
            m = M.max_hash(s) if s > 0 else None
            assert M.walk_counts(q, r, s) == M.counts(q, r, m), (q, r, s)
        if q or not r:
            assert M.old_walk_counts(q, r) == M.old_counts(q, r), (q, r)
    bnd = boundary_hashes()
    for s in steps:  # every step scale on every boundary-made pair
        for q, r in pairs[N_RANDOM:N_RANDOM + N_BOUNDARY:7]:
            assert M.walk_counts(q, r, s) == M.counts(q, r, M.max_hash(s))
        assert M.walk_counts(bnd, bnd[::3], s) == M.counts(bnd, bnd[::3], M.max_hash(s))


# ----------------------------------------------------------------------------------------------------------------------
# the library's host path against the model
# ----------------------------------------------------------------------------------------------------------------------

def test_finch_raw_distance_equals_the_model():
    pairs = pair_sets()[::3]
    for n, (q, r) in enumerate(pairs):
        for s in (SCALES[n % len(SCALES)], 0.0):
            want = M.raw_distance(q, r, s)
            got = H.raw_distance(q, r, s)
            assert same_double(got[0], want[0]) and same_double(got[1], want[1]) and got[2:] == want[2:], (q, r, s, got, want)


def test_finch_raw_distance_where_the_reference_panics():
    # The reference divides by zero here (1 / scale as u64 is 0).  The library's documented choice, M = u64::MAX, is
    # pinned: it is not a reference result.
    bnd = boundary_hashes()
    for s in PANICS:
        with pytest.raises(M.ReferencePanics):
            M.raw_distance(bnd[:4], bnd, s)
        for q, r in [(bnd[:4], bnd), (bnd, bnd[1::2]), ([1, U64_MAX], [2]), ([], [U64_MAX])]:
            assert H.raw_distance(q, r, s) == M.raw_distance(q, r, s, pinned=True)


def mk(name, hashes, params):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
    km = np.zeros((len(hs), params.kmer_length), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, params, H.FilterParams(False))


def sketch_set(scales, seed, per_scale=3, n_mash=4):
    """Scaled sketches at each scale (hashes clustered around every M, and the extremes) and Mash sketches; k mixed.
    -> (Sketches, [M.Sk])"""
    rng = np.random.default_rng(seed)
    bnd = np.array(boundary_hashes(), np.uint64)
    near = np.unique(np.concatenate([bnd] + [np.array([max(0, M.max_hash(s) - d) for d in range(1, 40, 3)], np.uint64)
                                             for s in ORDINARY + SATURATING]))
    pool = np.unique(np.concatenate([near, rng.integers(0, U64_MAX, 400, dtype=np.uint64)]))
    kinds = [("scaled", s) for s in scales for _ in range(per_scale)] + [("mash", None)] * n_mash
    out, model = None, []
    for n, (kind, s) in enumerate(kinds):
        size = int(rng.choice([0, 1, 3, 20, 120, 300])) if n > 1 else 60
        hs = np.sort(rng.choice(pool, min(size, len(pool)), replace=False))
        k = int(rng.choice([21, 15, 31]))
        p = SketchParams.scaled(len(hs), k, s) if kind == "scaled" else SketchParams.mash(kmer_length=k, no_strict=True)
        one = mk("%s%d" % (kind, n), hs, p)
        if out is None:
            out = one
        else:
            out.append(one)
        model.append(M.Sk(hs, kind, s if kind == "scaled" else 0.0, k))
    return out, model


def test_finch_distance_equals_the_model():
    sk, model = sketch_set(SCALES, 7)
    n = len(model)
    nan_q = 0
    for r in range(n):
        for q in range(n):
            want = M.distance(model[q], model[r], walk=True)
            same_distance(H.distance(sk, q, sk, r), want, (q, r, model[q].kind, model[q].scale, model[r].scale))
            nan_q += model[q].scale != model[q].scale and model[r].kind == "scaled"
            if model[q].hashes.size or not model[r].hashes.size:
                same_distance(H.distance(sk, q, sk, r, old_mode=True), M.distance(model[q], model[r], old_mode=True, walk=True))
            else:
                with pytest.raises(FinchError):
                    H.distance(sk, q, sk, r, old_mode=True)
    assert nan_q > 0


@pytest.mark.parametrize("side", ["query", "reference", "both"])
def test_nan_scale(side):
    """distance.rs takes f64::min of the two scales, which ignores a NaN: the other sketch's scale is used"""
    m = M.max_hash(0.5)
    qh, rh = [1, 5, m - 2, m - 1, m + 3], [1, 2, 3]
    qs = NAN if side in ("query", "both") else 0.5
    rs = NAN if side in ("reference", "both") else 0.5
    sk = mk("q", qh, SketchParams.scaled(len(qh), 21, qs))
    sk.append(mk("r", rh, SketchParams.scaled(len(rh), 21, rs)))
    want = M.distance(M.Sk(qh, "scaled", qs), M.Sk(rh, "scaled", rs), walk=True)
    # one NaN: the walk goes on to M(0.5) in the query (1, 5, M-2, M-1); both NaN: no scale step
    assert (want["total_hashes"], want["jaccard"]) == ((6, 1 / 6) if side != "both" else (3, 1 / 3))
    same_distance(H.distance(sk, 0, sk, 1), want)
    # and the other way round: the reference's hashes go on to M
    want = M.distance(M.Sk(rh, "scaled", rs), M.Sk(qh, "scaled", qs), walk=True)
    assert want["total_hashes"] == (6 if side != "both" else 3)
    same_distance(H.distance(sk, 1, sk, 0), want)


def test_finch_distance_where_the_reference_panics():
    # both Scaled with a min_scale that makes the reference divide by zero: the library's M = u64::MAX (pinned, see
    # test_finch_raw_distance_where_the_reference_panics)
    bnd = boundary_hashes()
    for s in PANICS:
        a = M.Sk(bnd[::2], "scaled", s, 21)
        b = M.Sk(bnd[:3], "scaled", max(s, 3.0), 17)
        sk = mk("a", a.hashes, SketchParams.scaled(len(a.hashes), 21, a.scale))
        sk.append(mk("b", b.hashes, SketchParams.scaled(len(b.hashes), 17, b.scale)))
        with pytest.raises(M.ReferencePanics):
            M.distance(a, b, walk=True)
        same_distance(H.distance(sk, 0, sk, 1), M.distance(a, b, walk=True, pinned=True))
        same_distance(H.distance(sk, 1, sk, 0), M.distance(b, a, walk=True, pinned=True))


# ----------------------------------------------------------------------------------------------------------------------
# mash_distance
# ----------------------------------------------------------------------------------------------------------------------

def mp_log(jaccard):
    """ln(x) at 50 digits for the x = 2j / (1 + j) that the double arithmetic forms"""
    x = (2.0 * jaccard) / (1.0 + jaccard)
    with mpmath.workdps(50):
        return mpmath.log(mpmath.mpf(x))


def close_to_mpmath(got, jaccard, k):
    """mash_distance = -ln(x) / k with the logarithm within 1 ulp and the division rounded once (to within half an ulp):
    |got - exact| <= ulp(ln x) / k + ulp(got) / 2.  Values of 1 or more clamp to 1."""
    with mpmath.workdps(50):
        ln = mp_log(jaccard)
        exact = -ln / k
        if exact >= 1:
            return got == 1.0
        bound = mpmath.mpf(math.ulp(float(ln))) / k + mpmath.mpf(math.ulp(got)) / 2
        return abs(mpmath.mpf(got) - exact) <= bound


def jaccards():
    rng = np.random.default_rng(5)
    js = [c / t for t in (1, 2, 3, 7, 10, 999, 1000, 1001, 4096, 10 ** 6) for c in range(1, t + 1, max(1, t // 97))]
    return js + rng.random(3000).tolist() + (10.0 ** -rng.uniform(1, 300, 300)).tolist() + (1 - 10.0 ** -rng.uniform(1, 15, 300)).tolist()


def test_log_within_one_ulp():
    for j in jaccards():
        x = (2.0 * j) / (1.0 + j)
        with mpmath.workdps(50):
            assert abs(mpmath.mpf(math.log(x)) - mp_log(j)) <= mpmath.mpf(math.ulp(math.log(x))), j


def test_mash_distance_against_mpmath():
    for n, j in enumerate(jaccards()):
        k = int(n % 32) + 1
        got = M.mash_distance(j, k)
        assert close_to_mpmath(got, j, k), (j, k, got)


def test_library_mash_distance_against_mpmath():
    sk, model = sketch_set(ORDINARY + [0.0], 9, per_scale=2, n_mash=6)
    seen = 0
    for r in range(len(model)):
        for q in range(len(model)):
            d = H.distance(sk, q, sk, r)
            if 0 < d["jaccard"] < 1:
                assert close_to_mpmath(d["mash_distance"], d["jaccard"], model[q].k), d
                seen += 1
    assert seen > 50


def test_mash_distance_clamps():
    bnd = boundary_hashes()
    sk = mk("a", bnd[:6], SketchParams.mash(kmer_length=21, no_strict=True))
    sk.append(mk("b", bnd[:6], SketchParams.mash(kmer_length=21, no_strict=True)))
    sk.append(mk("c", [3, 4], SketchParams.mash(kmer_length=21, no_strict=True)))
    sk.append(mk("e", [], SketchParams.mash(kmer_length=21, no_strict=True)))
    # jaccard 1: ln(1) = 0, -1.0 * 0 / k = -0.0; the library's clamp gives +0.0 (Rust leaves that sign to f64::max)
    d = H.distance(sk, 0, sk, 1)
    assert d["jaccard"] == 1.0 and bits(d["mash_distance"]) == bits(0.0)
    assert bits(M.mash_distance(1.0, 21)) == bits(0.0)
    # jaccard 0: ln(0) = -inf, the distance inf, clamped to 1
    d = H.distance(sk, 0, sk, 2)
    assert d["jaccard"] == 0.0 and d["mash_distance"] == 1.0 and M.mash_distance(0.0, 21) == 1.0
    # a tiny jaccard clamps to 1 as well
    assert M.mash_distance(1e-300, 1) == 1.0
    # old mode, empty against empty: 0 / 0, containment and jaccard NaN, the NaN distance clamped to 0 by f64::max
    d = H.distance(sk, 3, sk, 3, old_mode=True)
    want = M.distance(M.Sk([]), M.Sk([]), old_mode=True, walk=True)
    assert math.isnan(d["containment"]) and math.isnan(want["containment"]) and math.isnan(d["jaccard"])
    assert bits(d["mash_distance"]) == bits(0.0) == bits(want["mash_distance"])
    same_distance(d, want)
