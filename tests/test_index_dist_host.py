"""finch dist through the index without a device (include/finch_host.h: finch_index_dist, finch_index_dist_stats): the symbols,
the ABI version, everything the call decides before it touches a device, and the all-empty library, whose every row the host
makes itself.  (Two refusals need a device and are in tests/test_gpu_index_dist.py: old mode's refusal of an empty query needs a
non-empty reference, hence an index with postings; finch_index_dist_stats' refusal of a dense result needs finch_dist to make
one.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import index_dist_cases as X
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError
from index_dist_cases import Spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BELOW_ONE = math.nextafter(1.0, 0.0)
TINY = 5e-324


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def last_error(built):
    return (built.finch_last_error() or b"").decode()


def c_index_dist(built, ix, refs, queries, old_mode, d, out="ok"):
    p = C.c_void_p()
    rc = built.finch_index_dist(ix, refs, queries, old_mode, d, C.byref(p) if out == "ok" else None)
    return rc, p, last_error(built)


EMPTY_LIB = [Spec("e0", []), Spec("e1", [], "scaled", 0.01), Spec("e2", [], "scaled", math.nan), Spec("e0", [], k=31)]
HI = (2 ** 64 - 1) // 100  # the max hash of scale 0.01
MIXED = [Spec("e0", []), Spec("m", [5, 9]), Spec("at_m", [HI, HI + 7], "scaled", 0.01), Spec("below_m", [HI - 1, HI], "scaled", 0.01),
         Spec("e1", [], "scaled", 0.01, 11), Spec("nan", [3], "scaled", math.nan, 31), Spec("e2", [], "scaled", math.nan)]


@pytest.fixture()
def empty_index(built):
    lib = X.build(EMPTY_LIB)
    p = C.c_void_p()
    assert built.finch_index_new(lib._p, (C.c_int * 1)(0), 1, C.byref(p)) == _lib.FH_OK, last_error(built)
    yield p, lib
    built.finch_index_free(p)


def test_symbols_exported_declared_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("finch_index_dist", "finch_index_dist_stats"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    assert H._SYMS["finch_index_dist"][1][3:5] == [C.c_int, C.c_double]


def test_abi_version_is_at_least_16(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 16 and _lib.load().fh_abi_version() == want
    assert re.search(r"\b16: .*finch_index_dist", hdr.replace("\n", " "))


def test_null_arguments(built, empty_index):
    ix, lib = empty_index
    for a, r, out in ((None, lib._p, "ok"), (ix, None, "ok"), (ix, lib._p, None)):
        rc, _, msg = c_index_dist(built, a, r, lib._p, 0, 0.1, out=out)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    assert built.finch_index_dist_stats(None, None, None) == _lib.FH_ERR_INVALID


@pytest.mark.parametrize("d", [1.0, math.nextafter(1.0, 2.0), 7.5, math.inf])
def test_a_bound_that_keeps_every_pair_is_refused(built, empty_index, d):
    ix, lib = empty_index
    for q in (lib._p, None):
        rc, _, msg = c_index_dist(built, ix, lib._p, q, 0, d)
        assert rc == _lib.FH_ERR_INVALID and "max_distance" in msg and "use finch_dist" in msg
    with pytest.raises(FinchError):
        H.LibraryIndex(lib).dist(max_distance=d)


def test_refs_that_are_not_the_library_are_refused(built, empty_index):
    ix, lib = empty_index
    fewer = X.build(EMPTY_LIB[:3])
    more_hashes = X.build(EMPTY_LIB[:3] + [Spec("x", [1, 2])])
    for other, text in ((fewer, "refs has 3 sketches and 0 hashes"), (more_hashes, "refs has 4 sketches and 2 hashes")):
        for q in (lib._p, None):
            rc, _, msg = c_index_dist(built, ix, other._p, q, 0, 0.1)
            assert rc == _lib.FH_ERR_INVALID and text in msg and "built from 4 and 0" in msg, msg


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
def test_unsorted_query_refused_by_name(built, empty_index, bad):
    ix, lib = empty_index
    qs = X.build([Spec("g0", [1, 2, 3]), Spec("bad sketch", bad)])
    for old_mode in (0, 1):
        rc, _, msg = c_index_dist(built, ix, lib._p, qs._p, old_mode, 0.5)
        assert rc == _lib.FH_ERR_INVALID
        assert "query sketch 1 (bad sketch)" in msg and "strictly ascending" in msg


@pytest.mark.parametrize("d", [math.nan, -1.0, -TINY, -math.inf])
@pytest.mark.parametrize("old_mode", [False, True])
def test_nan_and_negative_bounds_give_no_rows(built, empty_index, d, old_mode):
    ix, lib = empty_index
    for q in (lib._p, None):
        rc, p, msg = c_index_dist(built, ix, lib._p, q, int(old_mode), d)
        assert rc == _lib.FH_OK and p.value, msg
        try:
            assert built.finch_dist_len(p) == 0
            nt, nc = C.c_uint64(9), C.c_uint64(9)
            assert built.finch_index_dist_stats(p, C.byref(nt), C.byref(nc)) == 0 and (nt.value, nc.value) == (0, 0)
        finally:
            built.finch_dist_free(p)
    with H.LibraryIndex(lib) as pix:
        assert pix.dist_json(max_distance=d, old_mode=old_mode) == "[]"


def check_rows(ix, qspecs, qs, rspecs, rs, old_mode, d):
    """the call against the model, and every row against finch_distance for its pair"""
    st = {}
    rows = ix.dist(qs, d, old_mode, stats=st)
    want, touched, copied, _ = X.model_dist(qspecs, rspecs, old_mode, d)
    X.rows_equal_model(rows, want)
    assert st == dict(kernel_ms=0.0, launches=0, pairs_touched=0, pairs_copied=0) and touched == copied == 0
    for row in rows:
        one = H.distance(rs if qs is None else qs, int(row["query"]), rs, int(row["reference"]), old_mode)
        for f in X.DOUBLES:
            assert X.bits(row[f]) == X.bits(one[f]), (row, one)
        assert (int(row["common_hashes"]), int(row["total_hashes"])) == (one["common_hashes"], one["total_hashes"])
    return rows


@pytest.mark.parametrize("d", [0.0, -0.0, TINY, 0.1, BELOW_ONE])
def test_the_all_empty_library_new_mode(built, d):
    rs, qs = X.build(EMPTY_LIB), X.build(MIXED)
    with H.LibraryIndex(rs) as ix:
        assert ix.stats()["postings"] == 0
        rows = check_rows(ix, MIXED, qs, EMPTY_LIB, rs, False, d)
        kept = {(int(q), int(r)) for q, r in zip(rows["query"], rows["reference"])}
        # an empty query beside every empty reference -- but for ("e0", empty Mash, k 21) beside itself, which is skipped; ("e0",
        # k 31) is another sketch --; a Mash sketch beside all; a Scaled one with nothing below the pair's max hash beside all, one
        # with a hash below it only where the pair has no scale (f64::min ignores a NaN: 0.01 beside NaN is 0.01, NaN beside NaN
        # is no scale)
        assert (0, 0) not in kept and (0, 3) in kept and {(1, r) for r in range(4)} <= kept
        assert {(2, r) for r in range(4)} <= kept and not {(3, 1), (3, 2)} & kept and {(3, 0), (3, 3)} <= kept
        assert {(5, 0), (5, 2), (5, 3)} <= kept and (5, 1) not in kept and (4, 1) in kept and (6, 2) in kept
        assert len(rows) == 7 * 4 - 4 and not rows["mash_distance"].any() and (rows["jaccard"] == 1.0).all()
        assert np.array_equal(rows["reference"], np.sort(rows["reference"], kind="stable"))
        # pairwise: the library beside itself; the empty NaN-scaled sketch is not equal to itself
        prow = check_rows(ix, None, None, EMPTY_LIB, rs, False, d)
        assert len(prow) == 4 * 4 - 3 and (2, 2) in {(int(q), int(r)) for q, r in zip(prow["query"], prow["reference"])}
        assert ix.dist_json(qs, d).count('"query"') == len(rows)


@pytest.mark.parametrize("d", [0.0, 0.1, BELOW_ONE])
def test_the_all_empty_library_old_mode(built, d):
    """old mode: 0 / 0 is NaN and ends in distance 0, for empty and for non-empty queries alike"""
    rs = X.build(EMPTY_LIB)
    with H.LibraryIndex(rs) as ix:
        for qspecs in (MIXED, [s for s in MIXED if len(s.hashes)], [s for s in MIXED if not len(s.hashes)]):
            qs = X.build(qspecs)
            rows = check_rows(ix, qspecs, qs, EMPTY_LIB, rs, True, d)
            skipped = sum(1 for s in qspecs if s.name == "e0" and not len(s.hashes) and s.k == 21)
            assert len(rows) == 4 * len(qspecs) - skipped
            assert np.isnan(rows["jaccard"]).all() and np.isnan(rows["containment"]).all() and not rows["mash_distance"].any()
            assert '"jaccard":null' in ix.dist_json(qs, d, True)


def test_zero_queries_and_zero_references(built):
    rs, qs = X.build(EMPTY_LIB), X.build(MIXED)
    with H.LibraryIndex(rs) as ix:
        assert len(ix.dist(H.select(qs, []), 0.5)) == 0 and ix.dist(H.select(qs, [])).dtype == H.DIST_DTYPE
    with H.LibraryIndex(H.select(rs, [])) as ix:
        assert len(ix.dist(qs, 0.5)) == 0 and len(ix.dist(None, 0.5)) == 0 and ix.dist_json() == "[]"
    with pytest.raises(FinchError):
        ix.dist(qs, 0.5)  # closed
