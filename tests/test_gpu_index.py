"""finch_index_search on the GPU (include/finch_host.h).  Every case is checked three ways: against
tests/search_model.py; byte for byte -- offsets, indices, rows -- against H.search on the same inputs; and what the device did
against the model's counts: candidates_copied = the pairs that pass, pairs_touched = the pairs that share a hash."""
import ctypes as C
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
TINY = 5e-324
TOP_NS = (0, 1, 3, 100)


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


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


class Case:
    """queries and a library, their model sketches, and search_model.search's untruncated answer per threshold, computed once"""

    def __init__(self, qs, rs):
        self.qs, self.rs = qs, rs
        self.mq, self.mr = model_sketches(qs), model_sketches(rs)
        self._model = {}

    def model(self, minc):
        key = bits(minc)
        if key not in self._model:
            self._model[key] = SM.search(self.mq, self.mr, minc, 0)
        return self._model[key]

    @property
    def shared(self):
        """the pairs with c > 0: those whose containment is above 0"""
        return sum(len(ws) for ws in self.model(TINY))

    def a_containment(self):
        """a containment some pair has, below 1 where there is one"""
        conts = sorted({d["containment"] for ws in self.model(TINY) for _, d in ws})
        return conts[len(conts) // 2] if conts[len(conts) // 2] < 1.0 or len(conts) == 1 else conts[0]

    def check(self, ix, minc, top_n):
        st = {}
        got = ix.search(self.qs, minc, top_n, stats=st)
        assert same_bytes(got, H.search(self.qs, self.rs, minc, top_n)), (minc, top_n)
        offsets, rows = got
        full = self.model(minc)
        want = [ws[:top_n] if top_n > 0 else ws for ws in full]  # (the model's own cut: a prefix of its ordered list)
        assert offsets.tolist() == SM.offsets(want)
        assert rows["query"].tolist() == [q for q, ws in enumerate(want) for _ in ws]
        flat = [(r, d) for ws in want for r, d in ws]
        assert rows["reference"].tolist() == [r for r, _ in flat]
        for row, (_, d) in zip(rows, flat):
            for f in DOUBLES:
                assert bits(row[f]) == bits(d[f]), (f, row, d)
            assert int(row["common_hashes"]) == d["common_hashes"] and int(row["total_hashes"]) == d["total_hashes"], (row, d)
        assert st["candidates_copied"] == sum(len(ws) for ws in full), (minc, top_n)
        assert st["pairs_touched"] == self.shared, (minc, top_n)
        return rows, st

    def check_all(self, ix, top_ns=TOP_NS):
        t = self.a_containment()
        for minc in (TINY, 0.1, t, math.nextafter(t, math.inf), 1.0, math.nan):
            for top_n in top_ns:
                self.check(ix, minc, top_n)


# ----------------------------------------------------------------------------------------------------------------------
# by hand
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def hand_case():
    rs = collect([mk("lib0", [1, 2, 3, 4]), mk("empty", []), mk("lib2", [1, 2, 3, 4]),  # two identical references: they tie
                  mk("lib3", [10, 20, 30]), mk("lib4", [0, 2, 6, 8]), mk("ends", [0, U64_MAX]), mk("top", [U64_MAX]), mk("lib7", [3, 20, 40, 50, 60])])
    qs = collect([mk("lib0", [1, 2, 3, 4]), mk("apart", [5, 7, 9]), mk("none", []), mk("ends", [0, U64_MAX]), mk("zero", [0]),
                  mk("mixed", [2, 20, 41, U64_MAX])])
    return Case(qs, rs)


def test_by_hand():
    case = hand_case()
    with H.LibraryIndex(case.rs) as ix:
        assert ix.stats()["n_refs"] == 8 and ix.stats()["postings"] == 23 and ix.stats()["device_bytes"] > 0
        case.check_all(ix)
        rows, st = case.check(ix, TINY, 0)
        q0 = rows[rows["query"] == 0]
        assert q0["reference"].tolist() == [0, 2, 7, 4]  # 4/4 twice, the lower index first; lib7's 1/1 (3 is its only hash <= 4); 1/2
        assert not len(rows[rows["query"] == 1]) and not len(rows[rows["query"] == 2])
        assert rows[rows["query"] == 3]["reference"].tolist() == [5, 6, 4]
        assert st["pairs_touched"] == 4 + 0 + 0 + 3 + 2 + 7


@lru_cache(None)
def bounds_case():
    """query hashes below every key, above every key, between two keys, on the first and on the last key"""
    rs = collect([mk("r0", [10, 20, 30]), mk("r1", [20, 40]), mk("r2", [40, 50])])
    qs = collect([mk("below", [5]), mk("above", [60]), mk("between", [15, 25, 45]), mk("first", [10]), mk("last", [50]),
                  mk("all", [5, 10, 15, 20, 45, 50, 60])])
    return Case(qs, rs)


def test_the_edges_of_the_bound_searches():
    case = bounds_case()
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix, top_ns=(0, 1))
        offsets, rows = ix.search(case.qs, TINY)
        assert np.diff(offsets.astype(np.int64)).tolist() == [0, 0, 0, 1, 1, 3]


# ----------------------------------------------------------------------------------------------------------------------
# random libraries from a pool: 70 and 130 references (either side of 64), queries of 0, 1, 63, 64, 65 and 1025 hashes (either
# side of a wave's and of the workgroup's 256 hashes per batch)
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def pool_case(n_refs):
    rng = np.random.default_rng(n_refs)
    pool = np.unique(rng.integers(0, U64_MAX, 2200, dtype=np.uint64))[:2000]
    apart = np.uint64(U64_MAX) - np.arange(1, 8, dtype=np.uint64)  # above the pool, in no reference
    qparts = [mk("q%d" % n, np.sort(rng.choice(pool, size=n, replace=False))) for n in (0, 1, 63, 64, 65, 1025)]
    qparts.append(mk("apart", np.sort(apart)))  # shares nothing
    rparts = [mk("r%d" % i, np.sort(rng.choice(pool, size=int(rng.integers(0, 51)), replace=False))) for i in range(n_refs)]
    rparts[5] = mk("r5", [])
    return Case(collect(qparts), collect(rparts))


@pytest.mark.parametrize("n_refs", [70, 130])
def test_random(n_refs):
    case = pool_case(n_refs)
    assert 0 < case.shared < 7 * n_refs
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix)


def test_python_helpers_agree_with_the_dense_ones():
    case = pool_case(130)
    L = H.lib()
    names = lambda sk: [L.finch_sketch_name(sk._p, i).decode() for i in range(len(sk))]  # noqa: E731
    with H.LibraryIndex(case.rs) as ix:
        for q in range(len(case.qs)):
            assert ix.best_match(case.qs, q) == H.best_match(case.rs, case.qs, q) == SM.best_match(case.mr, case.mq[q]), q
            for thr in (0.05, 0.0, -1.0):
                assert names(ix.filter_to_matches(case.qs, q, thr)) == names(H.filter_to_matches(case.rs, case.qs, q, thr)), (q, thr)
        apart = len(case.qs) - 1
        assert not SM.search([case.mq[apart]], case.mr, TINY, 0)[0] and ix.best_match(case.qs, apart) == 0


# ----------------------------------------------------------------------------------------------------------------------
# a hash that every one of 5 000 references holds: one posting run of 5 000, walked by the whole workgroup
# ----------------------------------------------------------------------------------------------------------------------

N_HEAVY = 5000
SHARED_HASH = 1 << 40


def own_hashes(r):
    return [1000 * (r + 1) + t for t in range(3)]  # below SHARED_HASH, three per reference


@lru_cache(None)
def heavy_library():
    return collect([mk("r%d" % r, own_hashes(r) + [SHARED_HASH]) for r in range(N_HEAVY)])


@lru_cache(None)
def heavy_case():
    qs = collect([mk("only_shared", [SHARED_HASH]),
                  mk("shared_and_own", sorted(own_hashes(7) + own_hashes(4242)[:2] + [SHARED_HASH, SHARED_HASH + 5]))])
    return Case(qs, heavy_library())


def test_a_hash_every_reference_holds():
    case = heavy_case()
    with H.LibraryIndex(case.rs) as ix:
        assert ix.stats()["postings"] == 4 * N_HEAVY
        for minc, top_n in ((TINY, 0), (TINY, 3), (0.25, 0), (math.nextafter(0.25, 1), 100), (1.0, 1)):
            rows, st = case.check(ix, minc, top_n)
            assert st["pairs_touched"] == 2 * N_HEAVY
        offsets, rows = ix.search(case.qs, TINY, 2)
        assert rows["reference"].tolist() == [0, 1, 7, 4242] and rows["containment"].tolist() == [0.25, 0.25, 1.0, 0.75]


def test_the_work_is_not_dense():
    """a query that shares hashes with exactly 3 of 5 000 references: 3 pairs are counted, not 5 000"""
    qs = collect([mk("three", sorted(own_hashes(11)[:1] + own_hashes(2500) + own_hashes(4999)[1:]))])
    case = Case(qs, heavy_library())
    with H.LibraryIndex(case.rs) as ix:
        for minc in (TINY, 0.5):
            rows, st = case.check(ix, minc, 0)
            assert st["pairs_touched"] == 3
        assert rows["reference"].tolist() == [2500, 4999] and st["candidates_copied"] == 2


# ----------------------------------------------------------------------------------------------------------------------
# the scale step: Scaled sketches of three scales and of a NaN scale, Mash sketches, on either side
# ----------------------------------------------------------------------------------------------------------------------

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
             mk("s01_empty", [], SketchParams.scaled(1000, k, 0.01)), part("s05", 0.5, SketchParams.scaled(1000, k, 0.5), scaled_m(0.5)),
             part("nan_a", 0.5, SketchParams.scaled(1000, k, math.nan)), part("nan_b", 0.4, SketchParams.scaled(1000, k, math.nan), hi)]
    sk = collect(parts)
    return Case(sk, sk)


def test_scale_step():
    case = scale_case()
    # pairs whose counts the scale step moves: with the reference's scale the smaller one, and with the query's; among them
    # pairs whose j -- the containment's divisor -- moves; and pairs in which one scale is NaN and the other one steps
    moved = [(q, r) for q in range(len(case.mq)) for r in range(len(case.mr))
             if SM.pair_counts(case.mq[q], case.mr[r]) != M.counts(case.mq[q].hashes, case.mr[r].hashes)]
    assert any(case.mr[r].scale < case.mq[q].scale for q, r in moved) and any(case.mq[q].scale < case.mr[r].scale for q, r in moved)
    assert any(SM.pair_counts(case.mq[q], case.mr[r])[2] != M.counts(case.mq[q].hashes, case.mr[r].hashes)[2] for q, r in moved)
    assert any(case.mq[q].scale != case.mq[q].scale for q, r in moved) and any(case.mr[r].scale != case.mr[r].scale for q, r in moved)
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix)


# ----------------------------------------------------------------------------------------------------------------------
# state: the counters are the index's, and every search leaves them zero
# ----------------------------------------------------------------------------------------------------------------------

def test_the_index_is_clean_after_every_search():
    a, b = pool_case(130), pool_case(70)
    with H.LibraryIndex(a.rs) as ix:
        first = ix.search(a.qs, 0.05, 3)
        assert same_bytes(first, ix.search(a.qs, 0.05, 3))
        other = ix.search(b.qs, TINY, 0)  # other queries against the same library touch other pairs
        assert same_bytes(other, H.search(b.qs, a.rs, TINY, 0))
        assert same_bytes(first, ix.search(a.qs, 0.05, 3))
        a.check(ix, TINY, 0)


def test_two_indexes_alive_at_once():
    a, b = pool_case(130), hand_case()
    with H.LibraryIndex(a.rs) as ia, H.LibraryIndex(b.rs) as ib:
        a.check(ia, 0.1, 3)
        b.check(ib, 0.1, 3)
        a.check(ia, TINY, 0)
        b.check(ib, TINY, 0)


def test_search_after_close_raises():
    case = hand_case()
    ix = H.LibraryIndex(case.rs)
    case.check(ix, 0.5, 0)
    ix.close()
    with pytest.raises(FinchError):
        ix.search(case.qs, 0.5)


def test_the_library_may_be_freed():
    """the index is self-contained: built from a collection that is gone by the time it is searched"""
    case = hand_case()
    L = H.lib()
    copy = H.select(case.rs, list(range(len(case.rs))))
    p = C.c_void_p()
    assert L.finch_index_new(copy._p, (C.c_int * 1)(0), 1, C.byref(p)) == 0
    del copy
    try:
        r = C.c_void_p()
        assert L.finch_index_search(p, case.qs._p, TINY, 0, C.byref(r)) == 0
        assert same_bytes(H._search_rows(r, len(case.qs), None), H.search(case.qs, case.rs, TINY, 0))
    finally:
        L.finch_index_free(p)


# ----------------------------------------------------------------------------------------------------------------------
# chunks of queries, device entries
# ----------------------------------------------------------------------------------------------------------------------

def index_with_chunk(refs, chunk, devices=(0,)):
    try:
        F.set_option("index_chunk_queries", chunk)  # (read when the index is built)
        return H.LibraryIndex(refs, devices=devices)
    finally:
        F.set_option("index_chunk_queries", None)


def test_chunks_of_queries():
    case = pool_case(70)
    qs = H.select(case.qs, [2, 3, 4, 5, 1])
    want = H.search(qs, case.rs, 0.02, 3)
    assert len(want[1]) > 5
    for chunk, launches in ((1, 5), (2, 3), (None, 1)):
        with index_with_chunk(case.rs, chunk) as ix:
            st = {}
            assert same_bytes(ix.search(qs, 0.02, 3, stats=st), want), chunk
            assert st["launches"] == launches
    with index_with_chunk(case.rs, 2, devices=(0, 0, 0)) as ix:  # chunks dealt over three entries
        st = {}
        assert same_bytes(ix.search(qs, 0.02, 3, stats=st), want) and st["launches"] == 3
        assert same_bytes(ix.search(qs, 0.02, 3), want)


def test_the_current_device_is_left_alone():
    hip = C.CDLL("libamdhip64.so")
    case = hand_case()
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    ix = H.LibraryIndex(case.rs, devices=(F.device_count() - 1,))
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
    ix.search(case.qs, 0.5, 1)
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
    ix.close()
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
