"""finch_search on the GPU (include/finch_host.h) against tests/search_model.py and against finch_distance run
pair by pair: the same rows in the same order, every double the same bytes; and best_match / filter_to_matches against the
model's statement of python.rs:202-234."""
import math
import struct
from functools import lru_cache

import numpy as np
import pytest

import dist_model as M
import finch_rs_amd as F
import search_model as SM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
DOUBLES = ("containment", "jaccard", "mash_distance")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def bits(x):
    return struct.pack("<d", float(x))


def mk(name, hashes, params=None):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
    p = params or SketchParams.mash(no_strict=True)
    km = np.zeros((len(hs), p.kmer_length), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, p, H.FilterParams(False))


def collect(parts):
    out = parts[0]
    for p in parts[1:]:
        out.append(p)
    return out


def model_sketches(sk):
    L = H.lib()
    out = []
    for i in range(len(sk)):
        hs = np.zeros(L.finch_sketch_n_hashes(sk._p, i), np.uint64)
        assert L.finch_sketch_copy(sk._p, i, hs.ctypes.data, None, None, None) == 0
        p = sk.params_of(i)
        out.append(M.Sk(hs, p.kind, p.scale if p.kind == "scaled" else 0.0, p.kmer_length))
    return out


class Case:
    """a set of queries and a library, with finch_distance's row of every pair (computed once) and the model's sketches"""

    def __init__(self, qs, rs):
        self.qs, self.rs = qs, rs
        self.mq, self.mr = model_sketches(qs), model_sketches(rs)
        self.pair = [[H.distance(qs, q, rs, r) for r in range(len(rs))] for q in range(len(qs))]

    def lib_rows(self, minc, top_n):
        """the contract from finch_distance's doubles: per query [(r, dict)]"""
        out = []
        for q in range(len(self.qs)):
            keep = [(r, d) for r, d in enumerate(self.pair[q]) if d["containment"] >= minc]
            keep.sort(key=lambda x: (-x[1]["containment"], x[0]))
            out.append(keep[:top_n] if top_n > 0 else keep)
        return out

    def check(self, got, minc=0.0, top_n=0):
        """got = H.search's (offsets, rows): equal to finch_distance's rows and to the model's, byte for byte"""
        offsets, rows = got
        want_lib, want_model = self.lib_rows(minc, top_n), SM.search(self.mq, self.mr, minc, top_n)
        assert offsets.tolist() == SM.offsets(want_model) == SM.offsets(want_lib)
        assert rows["query"].tolist() == [q for q, ws in enumerate(want_model) for _ in ws]
        for want in (want_lib, want_model):
            flat = [(r, d) for ws in want for r, d in ws]
            assert rows["reference"].tolist() == [r for r, _ in flat]
            for row, (_, d) in zip(rows, flat):
                for f in DOUBLES:
                    assert bits(row[f]) == bits(d[f]), (f, row, d)
                assert int(row["common_hashes"]) == d["common_hashes"] and int(row["total_hashes"]) == d["total_hashes"], (row, d)
        return rows


def with_options(fn, slice_=None, chunk=None):
    try:
        F.set_option("dist_slice", slice_)
        F.set_option("dist_chunk_pairs", chunk)
        return fn()
    finally:
        F.set_option("dist_slice", None)
        F.set_option("dist_chunk_pairs", None)


# ----------------------------------------------------------------------------------------------------------------------
# by hand
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def hand_case():
    rs = collect([mk("lib0", [1, 2, 3, 4]), mk("empty", []), mk("lib2", [1, 2, 3, 4]), mk("lib3", [10, 20, 30]), mk("lib4", [0, 2, 6, 8])])
    qs = collect([mk("lib0", [1, 2, 3, 4]),  # the library's first sketch, field for field: it matches itself
                  mk("apart", [5, 7, 9]),    # shares no hash with any reference: every containment 0
                  mk("none", [])])           # an empty query
    return Case(qs, rs)


@pytest.mark.parametrize("top_n", [0, 1, 2, 5, 100])
def test_by_hand(top_n):
    case = hand_case()
    rows = case.check(H.search(case.qs, case.rs, 0.0, top_n), 0.0, top_n)
    n = min(top_n, 5) if top_n else 5
    assert len(rows) == 3 * n
    q0 = rows[rows["query"] == 0]
    assert q0["reference"].tolist() == [0, 2, 4, 1, 3][:n]  # 4/4, 4/4 (the lower index first), 1/2 (0 and 2 are within the query), then the zeros by index
    assert q0["containment"].tolist() == [1.0, 1.0, 0.5, 0.0, 0.0][:n]
    for q in (1, 2):
        assert rows[rows["query"] == q]["reference"].tolist() == [0, 1, 2, 3, 4][:n]
        assert not rows[rows["query"] == q]["containment"].any()


def test_by_hand_best_match_and_filter():
    case = hand_case()
    assert [H.best_match(case.rs, case.qs, q) for q in range(3)] == [0, 0, 0]
    assert [SM.best_match(case.mr, case.mq[q]) for q in range(3)] == [0, 0, 0]
    assert H.best_match(case.rs, H.select(case.rs, [4]), 0) == 4
    names = lambda sk: [H.lib().finch_sketch_name(sk._p, i).decode() for i in range(len(sk))]  # noqa: E731
    assert names(H.filter_to_matches(case.rs, case.qs, 0, 0.5)) == ["lib0", "lib2", "lib4"]  # library order, not rank order
    assert names(H.filter_to_matches(case.rs, case.qs, 0, 0.75)) == ["lib0", "lib2"]
    assert names(H.filter_to_matches(case.rs, case.qs, 1, 0.0)) == names(case.rs)
    assert names(H.filter_to_matches(case.rs, case.qs, 1, 1e-300)) == []
    with pytest.raises(FinchError):
        H.best_match(H.select(case.rs, []), case.qs, 0)


# ----------------------------------------------------------------------------------------------------------------------
# a threshold that is a containment
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def threshold_case():
    qs = collect([mk("q", [1, 50])])
    rs = collect([mk("third", [1, 2, 3]),  # c = 1, j = 3
                  mk("whole", [1, 50]),    # c = j = 2
                  mk("zero", [7])])        # c = 0, j = 1
    return Case(qs, rs)


@pytest.mark.parametrize("top_n", [0, 3, 65])
def test_threshold_on_a_value(top_n):
    case = threshold_case()
    assert [d["containment"] for d in case.pair[0]] == [1 / 3, 1.0, 0.0] and [d["common_hashes"] for d in case.pair[0]] == [1, 2, 0]
    kept = [(1 / 3, [1, 0]), (math.nextafter(1 / 3, 1), [1]), (math.nextafter(1 / 3, 0), [1, 0]), (1.0, [1]),
            (math.nextafter(1.0, 2), []), (math.nan, []), (-math.inf, [1, 0, 2]), (0.0, [1, 0, 2]), (-0.0, [1, 0, 2]),
            (5e-324, [1, 0]), (math.inf, [])]
    for minc, refs in kept:
        rows = case.check(H.search(case.qs, case.rs, minc, top_n), minc, top_n)
        assert rows["reference"].tolist() == refs, minc


# ----------------------------------------------------------------------------------------------------------------------
# random libraries from a small pool: intersections and ties are common
# ----------------------------------------------------------------------------------------------------------------------

def pool_sketch(rng, pool, name, min_size, max_size):
    n = int(rng.integers(min_size, max_size + 1))
    return mk(name, np.sort(rng.choice(pool, size=n, replace=False)))


def pool_case(seed, n_queries, n_refs, pool_size=120, max_size=50, planted=()):
    """sketches of 0..max_size hashes from one pool.  With `planted`, (reference index, query index) pairs, that reference is a
    copy of that query; then every query has 20 hashes, the largest its own and above the pool, so that a reference's j is its
    size, and the other references have 8 hashes or more: none of them is a subset of a query, the copies alone reach 1.0"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, U64_MAX - 1000, pool_size * 2, dtype=np.uint64))[:pool_size]
    if planted:
        qhashes = [np.append(np.sort(rng.choice(pool, size=19, replace=False)), np.uint64(U64_MAX - i)) for i in range(n_queries)]
        qparts = [mk("q%d" % i, hs) for i, hs in enumerate(qhashes)]
    else:
        qparts = [pool_sketch(rng, pool, "q%d" % i, 0, max_size) for i in range(n_queries)]
    rparts = [pool_sketch(rng, pool, "r%d" % i, 8 if planted else 0, max_size) for i in range(n_refs)]
    for r, q in planted:
        rparts[r] = mk("r%d" % r, qhashes[q])
    return Case(collect(qparts), collect(rparts))


@lru_cache(None)
def top_case():
    return pool_case(7, 3, 130)


@pytest.mark.parametrize("top_n", [1, 2, 63, 64, 65, 130, 131])
def test_top_n_is_a_prefix(top_n):
    """1..64 are selected by the device's rounds, 65 and more by its list and the host's cut: one ordered list"""
    case = top_case()
    full = SM.search(case.mq, case.mr, 0.0, 0)
    assert all(len(ws) == 130 for ws in full)
    conts = [d["containment"] for _, d in full[0]]
    assert len(set(conts)) < len(conts) and len(set(conts)) > 10  # ties, and more than ties
    offsets, rows = H.search(case.qs, case.rs, 0.0, top_n)
    case.check((offsets, rows), 0.0, top_n)
    n = min(top_n, 130)
    for q in range(3):
        assert rows["reference"][offsets[q]:offsets[q + 1]].tolist() == [r for r, _ in full[q]][:n]


@lru_cache(None)
def edge_case(n_refs):
    # query 0 is twice in the library, in the first and in the last chunk but one of every split; query 1 once, as the
    # last reference: its winner is in the last chunk
    case = pool_case(100 + n_refs, 5, n_refs, planted=((1, 0), (n_refs - 2, 0), (n_refs - 1, 1)))
    assert [r for r, _ in SM.search(case.mq[:2], case.mr, 1.0, 0)[0]] == [1, n_refs - 2]
    assert SM.best_match(case.mr, case.mq[1]) == n_refs - 1
    return case


@pytest.mark.parametrize("chunks", ["one", "two", "many", "per_reference"])
@pytest.mark.parametrize("n_refs", [63, 64, 65, 129])
def test_block_and_chunk_edges(n_refs, chunks):
    case = edge_case(n_refs)
    chunk = {"one": None, "two": str(5 * ((n_refs + 1) // 2)), "many": "35", "per_reference": "3"}[chunks]
    n_launches = {"one": 1, "two": 2, "many": (n_refs + 6) // 7, "per_reference": n_refs}[chunks]
    for top_n in (1, 3, 0):
        st = {}
        rows = case.check(with_options(lambda: H.search(case.qs, case.rs, 0.0, top_n, stats=st), chunk=chunk), 0.0, top_n)
        assert st["launches"] == n_launches
        if top_n == 3:
            assert rows["reference"][:2].tolist() == [1, n_refs - 2]  # equal containments from different chunks
        if top_n == 1:
            assert rows["reference"][:2].tolist() == [1, n_refs - 1]
    a = with_options(lambda: H.search(case.qs, case.rs, 0.25, 2, devices=(0,)), chunk=chunk)
    b = with_options(lambda: H.search(case.qs, case.rs, 0.25, 2, devices=(0, 0, 0)), chunk=chunk)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    case.check(b, 0.25, 2)


@pytest.mark.parametrize("slice_", ["1", "8"])
def test_slices(slice_):
    case = edge_case(65)  # (its queries have 20 hashes)
    for minc, top_n in ((0.0, 0), (0.0, 4), (0.2, 0)):
        a = H.search(case.qs, case.rs, minc, top_n)
        b = with_options(lambda: H.search(case.qs, case.rs, minc, top_n), slice_=slice_)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        case.check(b, minc, top_n)


def scaled_m(scale):
    return U64_MAX // int(1.0 / scale)


@lru_cache(None)
def scale_case():
    rng = np.random.default_rng(5)
    lo, hi = scaled_m(0.001), scaled_m(0.01)
    base = np.unique(np.concatenate([rng.integers(0, lo, 30, dtype=np.uint64), rng.integers(lo, hi, 30, dtype=np.uint64),
                                     rng.integers(hi, U64_MAX, 30, dtype=np.uint64), np.array([lo - 1, lo, hi - 1, hi], np.uint64)]))

    def part(name, share, params, below=U64_MAX):
        """a Scaled sketch holds hashes below its max hash (`below`)"""
        own = base[base < np.uint64(below)]
        return mk(name, own[rng.random(len(own)) < share], params)

    k = 21
    parts = [part("s001_a", 0.6, SketchParams.scaled(1000, k, 0.001), lo), part("s01_a", 0.6, SketchParams.scaled(1000, k, 0.01), hi),
             part("mash_a", 0.5, None), part("s001_b", 0.4, SketchParams.scaled(1000, k, 0.001), lo + 1),
             part("s01_b", 0.7, SketchParams.scaled(1000, k, 0.01), hi), part("mash_b", 0.3, None),
             mk("s01_empty", [], SketchParams.scaled(1000, k, 0.01)), part("s05", 0.5, SketchParams.scaled(1000, k, 0.5), scaled_m(0.5))]
    sk = collect(parts)
    return Case(sk, sk)


@pytest.mark.parametrize("minc, top_n", [(0.0, 0), (0.0, 3), (0.3, 0), (0.3, 2)])
def test_scale_step(minc, top_n):
    case = scale_case()
    # pairs whose counts the scale step moves: with the reference's scale the smaller one, and with the query's; among them
    # pairs whose j -- the containment's divisor -- moves
    moved = [(q, r) for q in range(len(case.mq)) for r in range(len(case.mr))
             if SM.pair_counts(case.mq[q], case.mr[r]) != M.counts(case.mq[q].hashes, case.mr[r].hashes)]
    assert any(case.mr[r].scale < case.mq[q].scale for q, r in moved) and any(case.mq[q].scale < case.mr[r].scale for q, r in moved)
    assert any(SM.pair_counts(case.mq[q], case.mr[r])[2] != M.counts(case.mq[q].hashes, case.mr[r].hashes)[2] for q, r in moved)
    assert all(case.mq[q].kind == case.mr[r].kind == "scaled" for q, r in moved)
    case.check(H.search(case.qs, case.rs, minc, top_n), minc, top_n)


@lru_cache(None)
def random_case():
    return pool_case(42, 40, 200)


@pytest.mark.parametrize("minc, top_n", [(0.0, 0), (0.0, 5), (0.25, 0), (0.25, 5)])
def test_random(minc, top_n):
    case = random_case()
    case.check(H.search(case.qs, case.rs, minc, top_n), minc, top_n)


def test_random_best_match_and_filter():
    case = random_case()
    L = H.lib()
    for q in range(len(case.qs)):
        assert H.best_match(case.rs, case.qs, q) == SM.best_match(case.mr, case.mq[q]), q
        kept = H.filter_to_matches(case.rs, case.qs, q, 0.25)
        want = SM.filter_to_matches(case.mr, case.mq[q], 0.25)
        assert [L.finch_sketch_name(kept._p, i).decode() for i in range(len(kept))] == ["r%d" % r for r in want], q


def test_the_reduction_happens_on_the_device():
    """conditions on what crossed the link, not measurements: the model says how many pairs pass"""
    case = random_case()
    nq, nr = len(case.qs), len(case.rs)
    st = {}
    with_options(lambda: H.search(case.qs, case.rs, 0.0, 1, stats=st), chunk=str(nq * 64))
    assert st["launches"] == 4 and st["candidates_copied"] <= st["launches"] * nq
    k = sum(len(ws) for ws in SM.search(case.mq, case.mr, 0.5, 0))
    assert 0 < k < nq * nr // 8
    for chunk in (None, str(nq * 64)):
        st = {}
        _, rows = with_options(lambda: H.search(case.qs, case.rs, 0.5, 0, stats=st), chunk=chunk)
        assert len(rows) == k and st["candidates_copied"] == k
    st = {}
    _, rows = H.search(case.qs, case.rs, 0.5, 100, stats=st)  # past the device's rounds: its list, cut on the host
    assert len(rows) <= k and st["candidates_copied"] == k


def test_the_current_device_is_left_alone():
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    case = hand_case()
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    H.search(case.qs, case.rs, 0.0, 1, devices=(F.device_count() - 1,))
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
