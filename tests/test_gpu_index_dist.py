"""finch_index_dist on the GPU (include/finch_host.h).  Every case is checked three ways: the bytes of the rows
and of the JSON text against finch_dist on the same inputs; against tests/index_dist_model.py; and what the device did against
the model's counts: pairs_touched = the pairs that share a hash, rows from the device <= pairs_copied <= pairs_touched."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
import index_dist_cases as X
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError
from index_dist_cases import Spec

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
BELOW_ONE = math.nextafter(1.0, 0.0)
TINY = 5e-324
SHARED_HASH = 1 << 40


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


class Case:
    """a library and queries (None: pairwise), and the model's answer per (mode, bound), computed once"""

    def __init__(self, rspecs, qspecs=None):
        self.rspecs, self.qspecs = rspecs, qspecs
        self.rs = X.build(rspecs)
        self.qs = X.build(qspecs) if qspecs is not None else None
        self._model = {}

    def model(self, old_mode, d):
        key = (old_mode, X.bits(d))
        if key not in self._model:
            self._model[key] = X.model_dist(self.qspecs, self.rspecs, old_mode, d)
        return self._model[key]

    def a_distance(self, old_mode):
        """a distance some pair has exactly, strictly between 0 and 1"""
        ds = sorted({x["mash_distance"] for _, _, x in self.model(old_mode, BELOW_ONE)[0] if 0.0 < x["mash_distance"] < 1.0})
        return ds[len(ds) // 2]

    def check(self, ix, old_mode, d):
        st = {}
        rows = ix.dist(self.qs, d, old_mode, stats=st)
        dense_q = self.qs if self.qs is not None else self.rs
        assert rows.tobytes() == H.dist(dense_q, self.rs, d, old_mode).tobytes(), (old_mode, d)
        assert ix.dist_json(self.qs, d, old_mode) == H.dist_json(dense_q, self.rs, d, old_mode), (old_mode, d)
        want, touched, copied, from_device = self.model(old_mode, d)
        X.rows_equal_model(rows, want)
        assert st["pairs_touched"] == touched, (old_mode, d)
        assert from_device <= st["pairs_copied"] <= st["pairs_touched"], (old_mode, d, st)
        qspecs = self.qspecs if self.qspecs is not None else self.rspecs
        both = sum(1 for row in rows if len(qspecs[row["query"]].hashes) and len(self.rspecs[row["reference"]].hashes))
        assert both == from_device
        return rows, st

    def check_all(self, ix, old_mode):
        t = self.a_distance(old_mode)
        at, _ = self.check(ix, old_mode, t)
        below, _ = self.check(ix, old_mode, math.nextafter(t, 0.0))
        assert (at["mash_distance"] == t).any() and not (below["mash_distance"] == t).any()  # `<=`: kept at t, not below it
        for d in (0.0, -0.0, TINY, BELOW_ONE):
            self.check(ix, old_mode, d)
        zero, _ = self.check(ix, old_mode, -0.0)
        assert len(zero) == sum(1 for _, _, x in self.model(old_mode, 0.0)[0]) and not zero["mash_distance"].any()


def index_with_chunk(refs, chunk, devices=(0,)):
    try:
        F.set_option("index_chunk_queries", chunk)  # (read when the index is built)
        return H.LibraryIndex(refs, devices=devices)
    finally:
        F.set_option("index_chunk_queries", None)


# ----------------------------------------------------------------------------------------------------------------------
# Mash and Scaled sketches of three scales and a NaN scale, k of 11, 21 and 31, empty sketches, and the self-skip's cases:
# equal name and content (skipped), equal name and other content, equal content and other name (both kept); a NaN-scaled sketch
# is not equal to itself, so pairwise keeps its row beside itself
# ----------------------------------------------------------------------------------------------------------------------

def scaled_m(scale):
    return U64_MAX // int(1.0 / scale)


def mixed_specs(empties):
    rng = np.random.default_rng(11)
    lo, hi = scaled_m(0.001), scaled_m(0.01)
    pool = np.unique(np.concatenate([rng.integers(0, lo, 30, dtype=np.uint64), rng.integers(lo, hi, 30, dtype=np.uint64),
                                     rng.integers(hi, U64_MAX, 30, dtype=np.uint64), np.array([lo - 1, lo, hi - 1, hi], np.uint64)]))
    kinds = [("mash", 0.0, U64_MAX), ("scaled", 0.001, lo), ("scaled", 0.01, hi), ("scaled", 0.5, scaled_m(0.5)), ("scaled", math.nan, U64_MAX),
             ("mash", 0.0, U64_MAX), ("scaled", 0.01, hi + 1), ("scaled", math.nan, hi)]
    specs = []
    for s in range(24):
        kind, scale, below = kinds[s % len(kinds)]
        own = pool[pool < np.uint64(below)]
        specs.append(Spec("s%d" % s, own[rng.random(len(own)) < (0.85 if s % 3 == 0 else 0.5)], kind, scale, (11, 21, 31)[s % 3]))
    specs.append(Spec("s0", specs[0].hashes, k=specs[0].k))             # equal name and content: skipped beside s0
    specs.append(Spec("s3", specs[3].hashes[:-1], "scaled", 0.5, specs[3].k))  # equal name, other content: kept
    specs.append(Spec("twin", specs[5].hashes, k=specs[5].k))            # equal content, other name: kept
    if empties:
        specs += [Spec("e_mash", []), Spec("e_s01", [], "scaled", 0.01), Spec("e_nan", [], "scaled", math.nan, 31)]
    return specs


@lru_cache(None)
def mixed_pairwise(empties):
    return Case(mixed_specs(empties))


def test_pairwise_new_mode():
    case = mixed_pairwise(True)
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix, False)
        rows, _ = case.check(ix, False, 0.3)
        pairs = {(int(q), int(r)) for q, r in zip(rows["query"], rows["reference"])}
        assert (0, 0) not in pairs and (24, 0) not in pairs and (0, 24) not in pairs  # equal name and content
        assert (4, 4) in pairs and (29, 29) in pairs  # a NaN scale: not equal to itself (the empty one too)
        assert (5, 26) in pairs and (26, 5) in pairs and (27, 27) not in pairs and (28, 27) in pairs  # (two empty sketches: distance 0)
        assert {int(k) for k in (11, 21, 31)} == {case.rspecs[q].k for q, _ in pairs}


def test_pairwise_old_mode():
    case = mixed_pairwise(False)  # (old mode refuses an empty query beside a non-empty reference)
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix, True)
        case.check(ix, False, 0.2)  # both modes on one index


@lru_cache(None)
def mixed_queries():
    """queries of their own against the library with empty references; in old mode no query is empty"""
    rng = np.random.default_rng(12)
    lib = mixed_specs(True)
    qspecs = [lib[1], lib[4], lib[24], Spec("q_m", np.sort(rng.choice(np.concatenate([s.hashes for s in lib[:6]]), 25, replace=False)), k=31),
              Spec("apart", [7, 8, 9], k=11), lib[9]]
    qspecs[3] = Spec("q_m", np.unique(qspecs[3].hashes), k=31)
    return Case(lib, qspecs), Case(lib, qspecs + [Spec("q_empty", [], "scaled", 0.01)])


@pytest.mark.parametrize("old_mode", [False, True])
def test_queries_against_a_library_with_empty_references(old_mode):
    full, with_empty_query = mixed_queries()
    case = full if old_mode else with_empty_query
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix, old_mode)
        rows, _ = case.check(ix, old_mode, 0.0)
        empty_refs = [r for r, s in enumerate(case.rspecs) if not len(s.hashes)]
        assert set(empty_refs) <= set(rows["reference"].tolist())  # the host's own rows, in their place among the device's


def test_old_mode_refuses_an_empty_query_before_any_launch():
    _, case = mixed_queries()
    with H.LibraryIndex(case.rs) as ix:
        with pytest.raises(FinchError) as ei:
            ix.dist(case.qs, 0.1, True)
        assert "old_distance: empty query sketch" in str(ei.value)
        with pytest.raises(FinchError):
            H.dist(case.qs, case.rs, 0.1, True)
        with pytest.raises(FinchError):
            ix.dist(None, 0.1, True)  # pairwise: the library's own empty sketches
        case.check(ix, False, 0.1)


def test_stats_of_a_dense_result_are_refused():
    L = H.lib()
    a = X.build([Spec("a", [1, 2, 3]), Spec("b", [2, 3])])
    p = C.c_void_p()
    assert L.finch_dist(a._p, a._p, 0, 0.5, (C.c_int * 1)(0), 1, C.byref(p)) == 0
    try:
        nt, nc = C.c_uint64(1234), C.c_uint64(5678)
        assert L.finch_index_dist_stats(p, C.byref(nt), C.byref(nc)) == _lib.FH_ERR_INVALID
        assert (nt.value, nc.value) == (1234, 5678) and "finch_index_dist" in (L.finch_last_error() or b"").decode()
    finally:
        L.finch_dist_free(p)


# ----------------------------------------------------------------------------------------------------------------------
# libraries drawn from a pool: 1, 70 and 300 references (300: more touched pairs per query than the finish kernel's 256
# threads), pools of 40 and 700 values, sketches of 0, 1, 63, 64, 65, 256, 257 and 300 hashes (either side of a wave and of the
# count kernel's 256 hashes per batch), and one hash that every non-empty reference holds
# ----------------------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 256, 257, 300)


def pool_specs(n_refs, pool_size, seed, sizes, small):
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, SHARED_HASH, pool_size + 50, dtype=np.uint64))[:pool_size]
    specs = []
    for i in range(n_refs):
        n = sizes[i] if i < len(sizes) else int(rng.integers(small[0], small[1] + 1))
        hs = np.sort(rng.choice(pool, size=min(n, pool_size), replace=False))
        if len(hs) > 1:
            hs[-1] = SHARED_HASH  # (above the pool: still ascending)
        specs.append(Spec("p%d" % i, hs, k=(21, 31, 11)[i % 3]))
    return specs


@lru_cache(None)
def pool_case(which):
    if which == "one":  # a library of one reference
        return Case(pool_specs(1, 40, 1, (30,), (0, 0)), pool_specs(6, 40, 1, (0, 1, 30, 40), (5, 20)))
    if which == "dense40":  # 70 references over 40 values: nearly every pair shares a hash
        return Case(pool_specs(70, 40, 2, (0, 1, 40), (0, 25)))
    if which == "sizes700":  # the sizes, pairwise
        return Case(pool_specs(14, 700, 3, SIZES, (100, 300)))
    assert which == "wide700"  # 300 references of few hashes, the sizes as queries
    return Case(pool_specs(300, 700, 4, (), (2, 9)), pool_specs(9, 700, 4, SIZES, (5, 5)))


@pytest.mark.parametrize("old_mode", [False, True])
@pytest.mark.parametrize("which", ["one", "dense40", "sizes700", "wide700"])
def test_pools(which, old_mode):
    case = pool_case(which)
    if old_mode:  # (no empty query in old mode)
        rspecs = [s for s in case.rspecs if len(s.hashes)] if case.qspecs is None else case.rspecs
        case = Case(rspecs, None if case.qspecs is None else [s for s in case.qspecs if len(s.hashes)])
    with H.LibraryIndex(case.rs) as ix:
        case.check_all(ix, old_mode)
        if which == "wide700":
            _, st = case.check(ix, old_mode, 0.1)
            assert st["pairs_touched"] >= 7 * 300  # the shared hash: every reference, for every query of more than one hash


# ----------------------------------------------------------------------------------------------------------------------
# the pre-filter is live; chunks of queries and device entries; the counters after a dist
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def single_hash_case():
    """40 references of 20 hashes of their own and one that all share; three near-copies of the first"""
    specs = [Spec("r%d" % r, [1000 * (r + 1) + t for t in range(20)] + [SHARED_HASH]) for r in range(40)]
    specs += [Spec("copy%d" % t, [900 - t] + list(specs[0].hashes[:-1 - t]) + [SHARED_HASH]) for t in range(3)]
    return Case(specs)


def test_the_pre_filter_is_live():
    case = single_hash_case()
    with H.LibraryIndex(case.rs) as ix:
        rows, st = case.check(ix, False, 0.01)
        assert st["pairs_touched"] == 43 * 43 and len(rows) <= st["pairs_copied"] < 43 * 4 < st["pairs_touched"]
        assert len(rows) > 0
        rows, st = case.check(ix, True, 0.01)
        assert st["pairs_copied"] < st["pairs_touched"] == 43 * 43


def test_chunks_of_queries_and_device_entries():
    case = mixed_pairwise(True)
    n = len(case.rspecs)
    want = H.dist(case.rs, case.rs, 0.2)
    assert len(want) > 20
    for chunk, launches in ((1, n), (2, (n + 1) // 2), (5, (n + 4) // 5), (None, 1)):
        for devices in ((0,), (0, 0)):
            with index_with_chunk(case.rs, chunk, devices) as ix:
                st = {}
                assert ix.dist(None, 0.2, stats=st).tobytes() == want.tobytes(), (chunk, devices)
                assert st["launches"] == launches and st["kernel_ms"] > 0
                if chunk == 2:
                    case.check(ix, False, 0.2)
                    case.check(ix, False, 0.0)
    full, _ = mixed_queries()
    with index_with_chunk(full.rs, 5, (0, 0)) as ix:  # queries of their own: 6 in chunks of 5 over two entries, both modes
        full.check(ix, False, 0.2)
        full.check(ix, True, 0.2)


def test_a_dist_leaves_the_counters_clean():
    case, (full, _) = mixed_pairwise(True), mixed_queries()
    with H.LibraryIndex(case.rs) as ix:
        first = ix.search(full.qs, 0.05, 3)
        assert len(first[1]) > 3
        case.check(ix, False, 0.2)  # pairwise: touches pairs the search touched, and others
        again = ix.search(full.qs, 0.05, 3)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        full.check(ix, True, 0.2)
        again = ix.search(full.qs, 0.05, 3)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        assert first[1].tobytes() == H.search(full.qs, case.rs, 0.05, 3)[1].tobytes()
