"""finch_index_compare_counts on the GPU (include/finch_host.h).  Every case is checked three ways: the bytes of
the rows against finch_compare_counts on the same inputs; every row against finch_compare_counts_pair (the reference's loop on
the host) and tests/moments_model.py -- integers equal, doubles equal as bit patterns, two NaNs equal --; and what the device
did against the model's counts: pairs_touched = the pairs that share a hash, pairs_walked = records_copied = the pairs with
common >= min_common.  The inputs are test_gpu_compare_counts.py's recipe, restated: hashes from a universe of 6000 values, so
that matches are dense, counts from moments_model.COUNTS."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
import moments_model as MM
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

pytestmark = pytest.mark.gpu

UNIVERSE = 6000
QUERY_LENGTHS = (0, 1, 63, 64, 65, 1000, 4097)   # lane-step edges; 4097: walked along the reference against every reference
REF_LENGTHS = (0, 1, 63, 64, 65, 200)
N_RANDOM_REFS = 130
LONG_REFS = (300, 300, 1500, 1500)               # the 1000-long query is walked along itself against the last two
FIELDS = ("common", "ref_pos", "query_pos", "ref_count", "query_count", "var", "skew", "kurt")
# the planted references
R_PREFIX, R_FULL_BALLOT, R_STEP_EDGE, R_EQUAL_COUNTS, R_ONE_HASH, R_EQUAL_LENGTH = 20, 21, 22, 23, 24, 25


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def mk(name, entries):
    kc = np.zeros(len(entries), KC_DTYPE)
    kc["hash"] = np.asarray([h for h, _ in entries], np.uint64)
    kc["count"] = np.asarray([c for _, c in entries], np.uint32)
    km = np.zeros((len(entries), 21), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, SketchParams.mash(), H.FilterParams(False))


def collect(sketches, prefix):
    out = mk("%s0" % prefix, sketches[0])
    for i, s in enumerate(sketches[1:], 1):
        out.append(mk("%s%d" % (prefix, i), s))
    return out


def lattice(u):
    return int(u) * 977 + 5  # (spread out; still a few thousand distinct values)


def off_lattice(u):
    return int(u) * 977 + 6  # a hash no random sketch holds


def random_sketch(rng, n, lo=0, hi=UNIVERSE):
    us = np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False))
    return [(lattice(u), int(c)) for u, c in zip(us, rng.choice(MM.COUNTS, size=n))]


class Case:
    """queries and a library with, for every pair, the model's tuple, and for every pair that shares a hash
    finch_compare_counts_pair's (computed once); the dense call's rows per threshold (computed once each)"""

    def __init__(self, queries, refs):
        self.mq, self.mr = queries, refs
        self.qs, self.rs = collect(queries, "q"), collect(refs, "r")
        self.model = {(q, r): MM.compare_counts(ref, query) for q, query in enumerate(queries) for r, ref in enumerate(refs)}
        self.host = {key: H.compare_counts_pair(self.rs, key[1], self.qs, key[0]) for key, t in self.model.items() if t[0] >= 1}
        for key, t in self.host.items():
            assert MM.same(t, self.model[key]), (key, t, self.model[key])
        self._dense = {}

    def dense(self, min_common):
        if min_common not in self._dense:
            self._dense[min_common] = H.compare_counts(self.rs, self.qs, min_common)
        return self._dense[min_common]

    def pairs_with(self, at_least):
        return sum(1 for t in self.model.values() if t[0] >= at_least)

    def check(self, ix, min_common):
        st = {}
        rows = ix.compare_counts(self.qs, min_common, stats=st)
        assert rows.dtype == H.COUNTS_DTYPE and rows.tobytes() == self.dense(min_common).tobytes(), min_common
        want = [key for key in sorted(self.model) if self.model[key][0] >= min_common]  # by query, then by reference
        assert list(zip(rows["query"].tolist(), rows["reference"].tolist())) == want
        for row, key in zip(rows, want):
            got = tuple(row[f] for f in FIELDS)
            assert MM.same(got, self.host[key]), (key, got, self.host[key])
            assert MM.same(got, self.model[key]), (key, got, self.model[key])
        assert st["pairs_touched"] == self.pairs_with(1), st
        assert st["pairs_walked"] == st["records_copied"] == len(want), st
        return rows, st


@lru_cache(None)
def edge_case():
    rng = np.random.default_rng(2025)
    queries = [random_sketch(rng, n) for n in QUERY_LENGTHS]
    lengths = list(REF_LENGTHS) * 2 + [int(x) for x in rng.integers(0, 201, N_RANDOM_REFS - 2 * len(REF_LENGTHS))] + list(LONG_REFS)
    refs = [random_sketch(rng, n) for n in lengths]
    q1000, q64 = queries[5], queries[3]
    refs[R_PREFIX] = q1000[:200]                                                        # the recurrence runs long
    refs[R_FULL_BALLOT] = [(h, MM.COUNTS[(i * 7) % 4]) for i, (h, _) in enumerate(q1000[-64:])]  # every lane of one step matches
    # 65 entries, walked along the reference: the only matches are entry 63 (last lane of step 0) and entry 64 (first of step 1)
    refs[R_STEP_EDGE] = [(off_lattice(u), 3) for u in range(63)] + [(q1000[-2][0], 1), (q1000[-1][0], 2)]
    refs[R_EQUAL_COUNTS] = [(h, MM.COUNTS[i % 4]) for i, (h, c) in enumerate(x for x in q1000 if x[1] == 2)][:30]  # NaNs
    refs[R_ONE_HASH] = [(off_lattice(u), 1) for u in range(10)] + [(q1000[-1][0], 7)]
    mine = {h for h, _ in q64}
    others = [lattice(u) for u in range(UNIVERSE) if lattice(u) not in mine][100:132]
    refs[R_EQUAL_LENGTH] = sorted([(h, 2) for h, _ in q64[:32]] + [(h, 3) for h in others])  # 64 entries against the 64-long query
    return Case(queries, refs)


def index_with_chunk(refs, chunk, devices=(0,)):
    try:
        F.set_option("index_chunk_queries", chunk)  # (read when the index is built)
        return H.LibraryIndex(refs, devices=devices)
    finally:
        F.set_option("index_chunk_queries", None)


def exact_threshold(case):
    commons = sorted(t[0] for t in case.model.values() if t[0] > 1)
    exact = commons[len(commons) // 2]  # a value some pairs reach exactly
    assert any(t[0] == exact for t in case.model.values()) and any(1 <= t[0] < exact for t in case.model.values())
    return exact


def test_the_planted_pairs_are_what_they_are_meant_to_be():
    case = edge_case()
    assert [len(q) for q in case.mq] == list(QUERY_LENGTHS) and len(case.mr) == N_RANDOM_REFS + len(LONG_REFS)
    assert case.model[(5, R_PREFIX)][0] == 200 and case.model[(5, R_FULL_BALLOT)][0] == 64 == len(case.mr[R_FULL_BALLOT])
    assert case.model[(5, R_STEP_EDGE)][0] == 2 and len(case.mr[R_STEP_EDGE]) == 65
    equal = case.model[(5, R_EQUAL_COUNTS)]
    assert equal[0] == 30 and equal[5] == 0.0 and np.isnan(equal[6]) and np.isnan(equal[7])
    assert case.model[(5, R_ONE_HASH)][0] == 1 and np.isnan(case.model[(5, R_ONE_HASH)][6])
    assert len(case.mr[R_EQUAL_LENGTH]) == len(case.mq[3]) == 64 and case.model[(3, R_EQUAL_LENGTH)][0] == 32
    # both sides get walked: a touched pair with the shorter query and one with the shorter reference
    shared = [key for key, t in case.model.items() if t[0] >= 1]
    assert any(len(case.mq[q]) < len(case.mr[r]) for q, r in shared) and any(len(case.mq[q]) > len(case.mr[r]) for q, r in shared)
    assert any(t[0] >= 1 for (q, r), t in case.model.items() if q == 5 and len(case.mr[r]) == 1500)


@pytest.mark.parametrize("which", ["one", "exact", "above_exact", "two_to_the_40"])
def test_edges_and_thresholds(which):
    case = edge_case()
    exact = exact_threshold(case)
    min_common = dict(one=1, exact=exact, above_exact=exact + 1, two_to_the_40=2 ** 40)[which]
    with H.LibraryIndex(case.rs) as ix:
        rows, st = case.check(ix, min_common)
    if which == "one":
        assert len(rows) == case.pairs_with(1) > 100 and st["launches"] == 3
        assert not (rows["query"] == 0).any()  # the empty query has no row
    if which == "exact":
        assert (rows["common"] == exact).any()
    if which == "above_exact":
        assert len(rows) and not (rows["common"] == exact).any()
    if which == "two_to_the_40":
        assert len(rows) == 0 and st["pairs_touched"] > 0 and st["launches"] == 2  # (as the dense call clamps it; nothing is walked)


def test_the_counters_are_clean_after_every_call():
    case = edge_case()
    other = H.select(case.qs, [5, 2, 6])
    with H.LibraryIndex(case.rs) as ix:
        first = ix.compare_counts(case.qs, 1)
        between = ix.compare_counts(other, 3)
        third = ix.compare_counts(case.qs, 1)
        offsets, found = ix.search(case.qs, 0.1)
    assert len(first) and first.tobytes() == third.tobytes() == case.dense(1).tobytes()
    assert len(between) and between.tobytes() == H.compare_counts(case.rs, other, 3).tobytes()
    want_offsets, want = H.search(case.qs, case.rs, 0.1)
    assert len(want) and offsets.tobytes() == want_offsets.tobytes() and found.tobytes() == want.tobytes()


@pytest.mark.parametrize("devices", [(0,), (0, 0, 0)], ids=["one_entry", "three_entries"])
@pytest.mark.parametrize("chunk", [1, 2])
def test_chunks_and_device_entries(chunk, devices):
    case = edge_case()
    with index_with_chunk(case.rs, chunk, devices) as ix:
        rows, st = case.check(ix, 1)
        # a chunk launches the count; the selection if a pair was touched; the walk if a pair passed
        groups = [range(q, min(q + chunk, len(case.mq))) for q in range(0, len(case.mq), chunk)]
        touched = [sum(1 for q in g for r in range(len(case.mr)) if case.model[(q, r)][0] >= 1) for g in groups]
        assert st["launches"] == sum(3 if t else 1 for t in touched)
        case.check(ix, exact_threshold(case))


@lru_cache(None)
def sparse_case():
    rng = np.random.default_rng(7)
    per_pool = UNIVERSE // 10
    refs = [random_sketch(rng, 40, (r % 10) * per_pool, (r % 10 + 1) * per_pool) for r in range(300)]
    queries = [random_sketch(rng, 150, 2 * per_pool, 3 * per_pool), random_sketch(rng, 150, 7 * per_pool, 8 * per_pool),
               random_sketch(rng, 150, UNIVERSE, UNIVERSE + per_pool)]  # the last one from no pool
    return Case(queries, refs)


def test_a_sparse_library_touches_few_pairs():
    case = sparse_case()
    with H.LibraryIndex(case.rs) as ix:
        rows, st = case.check(ix, 1)
        assert 0 < st["pairs_touched"] <= 2 * 30 and st["pairs_touched"] * 10 <= len(case.mq) * len(case.mr)
        assert set(rows["query"].tolist()) == {0, 1}  # the query from no pool has no row
        assert set((rows["reference"] % 10).tolist()) == {2, 7}
        case.check(ix, 12)


@lru_cache(None)
def long_run_case():
    rng = np.random.default_rng(99)
    everyone = (lattice(UNIVERSE + 1), 2)  # above every other hash
    refs = [random_sketch(rng, 5) + [(everyone[0], int(rng.choice(MM.COUNTS)))] for _ in range(300)]
    queries = [random_sketch(rng, 50) + [everyone]]
    return Case(queries, refs)


def test_a_hash_that_every_reference_holds():
    case = long_run_case()
    with H.LibraryIndex(case.rs) as ix:
        rows, st = case.check(ix, 1)
        assert len(rows) == 300 == st["pairs_touched"] and (rows["common"] >= 1).all()
        more, st = case.check(ix, 2)
        assert 0 < len(more) < 300 and (more["common"] >= 2).all() and st["pairs_touched"] == 300


def test_counts_must_be_attached_and_may_be_replaced():
    case = edge_case()
    L = H.lib()
    with H.LibraryIndex(case.rs) as ix:
        p = C.c_void_p()
        assert L.finch_index_compare_counts(ix._handle(), case.qs._p, 1, C.byref(p)) == _lib.FH_ERR_STATE
        assert "finch_index_attach_counts" in (L.finch_last_error() or b"").decode() and not p.value
        nbytes = ix.attach_counts()
        assert nbytes == 4 * sum(len(r) for r in case.mr) and ix.stats()["postings"] * 4 == nbytes
        case.check(ix, 1)
        # the same hashes with other counts: after the attachment the rows are the dense call's on that library
        changed = collect([[(h, MM.COUNTS[(i + c) % 4]) for i, (h, c) in enumerate(ref)] for ref in case.mr], "r")
        ix.refs = changed
        assert ix.attach_counts() == nbytes
        rows = ix.compare_counts(case.qs, 1)
        assert rows.tobytes() == H.compare_counts(changed, case.qs, 1).tobytes()
        assert rows.tobytes() != case.dense(1).tobytes() and (rows["common"] == case.dense(1)["common"]).all()
        with pytest.raises(FinchError):
            ix.compare_counts(case.qs, 0)
        # as many sketches and hashes, two sketches' lengths exchanged: refused by name, and what is attached stays
        order = list(range(len(case.mr)))
        order[R_PREFIX], order[R_FULL_BALLOT] = R_FULL_BALLOT, R_PREFIX
        ix.refs = H.select(changed, order)
        with pytest.raises(FinchError) as ei:
            ix.attach_counts()
        assert "refs sketch %d (r%d) has 64 hashes" % (R_PREFIX, R_FULL_BALLOT) in str(ei.value) and "one of 200" in str(ei.value)
        assert ix.compare_counts(case.qs, 1).tobytes() == rows.tobytes()
