"""finch_index_gather on the GPU (include/finch_host.h): the gather's rounds over the library index's live
counters.  Every result goes through gather_cases.check_device -- against tests/gather_model.py and against finch_gather_query,
the host's loop: the same rows in the same order, every integer the same, every double the same bytes --, and where it says so
it is finch_gather's (offsets, rows) byte for byte.  The shapes are the smallest at which each piece can go wrong
(tests/index_gather_cases.py)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
import gather_cases as GC
import gather_model as GM
import index_gather_cases as IC
from finch_rs_amd import host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")
    yield
    for ix in _INDEXES.values():
        ix.close()
    _INDEXES.clear()


_INDEXES = {}


def index_of(case, chunk=None, devices=(0,)):
    """the index of the case's library, built once per (case, queries per launch, devices): index_chunk_queries is read when
    the index is built"""
    key = (id(case), chunk, devices)
    if key not in _INDEXES:
        try:
            F.set_option("index_chunk_queries", chunk)
            _INDEXES[key] = H.LibraryIndex(case.rs, devices)
        finally:
            F.set_option("index_chunk_queries", None)
    return _INDEXES[key]


def same_bytes(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# by hand and random
# ----------------------------------------------------------------------------------------------------------------------

SMALL = {"hand": IC.hand_case, "random_70": lambda: IC.random_case(70), "random_130": lambda: IC.random_case(130)}


@pytest.mark.parametrize("max_rounds", IC.MAX_ROUNDS)
@pytest.mark.parametrize("min_overlap", IC.MIN_OVERLAPS)
@pytest.mark.parametrize("name", list(SMALL))
def test_by_hand_and_random(name, min_overlap, max_rounds):
    case = SMALL[name]()
    got = index_of(case).gather(case.qs, min_overlap, max_rounds)
    rows = GC.check_device(case, got, min_overlap, max_rounds)
    same_bytes(got, H.gather(case.qs, case.rs, min_overlap, max_rounds))
    if name == "hand" and min_overlap == 1 and max_rounds in (0, 2, 5):
        assert rows["query"].tolist() == [0, 0, 1, 1, 4, 5, 5]
        assert rows["reference"].tolist() == [1, 2, 4, 5, 7, 0, 2]  # A then C, never B; ties to the lower index
        assert int(rows["abund"][5]) == 2 * 0xffffffff + 0xfffffff0
    if name != "hand" and min_overlap == 1 and max_rounds == 0:
        assert len(rows) > 15 and rows["reference"].max() >= 64
    if min_overlap == 10 ** 6:
        assert len(rows) == 0


def test_min_overlap_below_one_is_one():
    case = IC.hand_case()
    same_bytes(index_of(case).gather(case.qs, 0), index_of(case).gather(case.qs, 1))


# ----------------------------------------------------------------------------------------------------------------------
# the counters between calls: zero, whoever was touched
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_refs", [70, 130])
def test_non_candidates_are_lowered_and_cleaned(n_refs):
    """with min_overlap 3 most touched references are no candidates: they are lowered by the winners all the same, and the
    tail must leave their counters zero -- a search on the same index counts from them"""
    case = IC.random_case(n_refs)
    ix = index_of(case)
    st = {}
    GC.check_device(case, ix.gather(case.qs, 3, stats=st), 3)
    assert 0 < st["candidates"] < st["pairs_touched"]
    same_bytes(ix.search(case.qs, 1e-9), H.search(case.qs, case.rs, 1e-9))


@pytest.mark.parametrize("chunk", [None, 1])
def test_searches_and_gathers_on_one_index_repeat_themselves(chunk):
    """search, gather, search and gather(A), gather(B), gather(A): equal bytes each time; with one query per launch a launch
    triple per query"""
    a, b = IC.random_case(70), IC.hand_case()
    ix = index_of(a, chunk)
    s0 = ix.search(a.qs, 0.05)
    st = {}
    g0 = ix.gather(a.qs, stats=st)
    same_bytes(ix.search(a.qs, 0.05), s0)
    same_bytes(s0, H.search(a.qs, a.rs, 0.05))
    GC.check_device(a, g0)
    assert st["launches"] == 3 * (len(a.mq) if chunk else 1)
    other = ix.gather(b.qs)  # other queries against the same library
    same_bytes(other, H.gather(b.qs, a.rs))
    same_bytes(ix.gather(a.qs), g0)
    same_bytes(ix.gather(b.qs), other)
    same_bytes(ix.search(a.qs, 0.05), s0)


# ----------------------------------------------------------------------------------------------------------------------
# posting runs: a hash every reference holds
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_refs", [300, 1100])
def test_a_hash_every_reference_holds(n_refs):
    """a run of 300 (longer than the count's workgroup) and of 1 100 (longer than the rounds', across two batches of its flat
    deal): the first winner lowers every counter"""
    case = IC.common_hash_case(n_refs)
    ix = index_of(case)
    for min_overlap, max_rounds in ((1, 0), (2, 0), (1, 3)):
        st = {}
        got = ix.gather(case.qs, min_overlap, max_rounds, stats=st)
        rows = GC.check_device(case, got, min_overlap, max_rounds)
        same_bytes(got, H.gather(case.qs, case.rs, min_overlap, max_rounds))
        assert st["pairs_touched"] >= 2 * n_refs  # queries 0 and 2 touch every reference
        if (min_overlap, max_rounds) == (1, 0):
            assert (rows["query"] == 0).sum() > n_refs // 8 and rows["query"].tolist().count(2) == 1
    same_bytes(ix.search(case.qs, 0.3), H.search(case.qs, case.rs, 0.3))  # (every counter is zero again)


def test_a_query_that_is_a_reference_and_two_equal_references():
    case = IC.equal_case()
    got = index_of(case).gather(case.qs)
    rows = GC.check_device(case, got)
    same_bytes(got, H.gather(case.qs, case.rs))
    assert rows["query"].tolist() == [0, 1] and rows["reference"].tolist() == [2, 0]  # the tie goes to the lower index
    assert rows["remaining"].tolist() == [0, 0] and rows["f_match"].tolist() == [1.0, 1.0]


# ----------------------------------------------------------------------------------------------------------------------
# the winner's walk: reference lengths; candidates that earlier winners use up
# ----------------------------------------------------------------------------------------------------------------------

def test_winner_lengths():
    case = IC.winner_length_case()
    st = {}
    got = index_of(case).gather(case.qs, stats=st)
    rows = GC.check_device(case, got)
    same_bytes(got, H.gather(case.qs, case.rs))
    lengths = sorted(n for n in IC.WINNER_LENGTHS if n)
    assert sorted(rows["ref_len"].tolist()) == lengths  # every reference but the empty one wins a round
    assert rows["overlap"].tolist() == sorted(rows["overlap"].tolist(), reverse=True) and int(rows["overlap"][-1]) == 1
    assert st["candidates"] == len(lengths) == st["records_copied"]


def test_a_candidate_used_up_and_one_that_falls_below_the_threshold():
    case = IC.used_up_case()
    ix = index_of(case)
    st = {}
    rows = GC.check_device(case, ix.gather(case.qs, stats=st))
    assert rows["reference"].tolist() == [1, 5, 3] and rows["overlap"].tolist() == [200, 200, 60] and rows["common"].tolist() == [200, 200, 110]
    assert rows["ref_len"].tolist() == [1200, 200, 110]
    assert st["candidates"] == 5 and st["records_copied"] == 3 and st["pairs_touched"] == 5
    # with min_overlap 61 the third round's candidate has fallen below the threshold and is out
    got = ix.gather(case.qs, 61)
    rows = GC.check_device(case, got, 61)
    same_bytes(got, H.gather(case.qs, case.rs, 61))
    assert rows["reference"].tolist() == [1, 5]


# ----------------------------------------------------------------------------------------------------------------------
# query lengths: the word edges of the bitmask, and the whole of it
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_overlap, max_rounds", [(1, 0), (2, 0), (1, 2)])
def test_query_lengths(min_overlap, max_rounds):
    case = IC.length_case()
    got = index_of(case).gather(case.qs, min_overlap, max_rounds)
    rows = GC.check_device(case, got, min_overlap, max_rounds)
    same_bytes(got, H.gather(case.qs, case.rs, min_overlap, max_rounds))
    if (min_overlap, max_rounds) == (1, 0):
        assert set(rows["query"].tolist()) == set(range(1, len(IC.LENGTHS)))
        assert int(rows["remaining"].min()) >= 0 and int(rows["query_len"].max()) == 65537


def test_the_longest_query_fills_the_mask():
    case = IC.longest_case()
    n = 1 << 20
    rows = GC.check_device(case, index_of(case).gather(case.qs))
    assert rows["reference"].tolist() == [2, 1, 0] and rows["overlap"].tolist() == [40, 5, 2] and rows["common"].tolist() == [40, 5, 35]
    assert rows["remaining"].tolist() == [n - 40, n - 45, n - 47]


@pytest.mark.parametrize("order", IC.LONG_ORDERS)
def test_a_long_query_without_candidates_next_to_a_short_one_with(order):
    """the mask is sized for the queries that have candidates: a much longer query of the same launch that has none must leave
    it alone and give no row.  It shares hashes, so its counters are touched, and must be zero afterwards all the same"""
    case = IC.long_without_candidates_case(order)
    ix = index_of(case)
    st = {}
    rows = GC.check_device(case, ix.gather(case.qs, 10, stats=st), 10)
    assert case.long_at not in rows["query"].tolist() and sorted(set(rows["query"].tolist())) == [q for q in range(3) if q != case.long_at]
    assert st["candidates"] == 3 and st["records_copied"] == len(rows) == 2 and st["launches"] == 3  # one chunk of queries
    assert st["pairs_touched"] == 6
    # with min_overlap 1 the long query has candidates -- its counters were left zero -- and the mask is its own
    got = ix.gather(case.qs, 1)
    rows = GC.check_device(case, got, 1)
    assert rows["query"].tolist().count(case.long_at) == 3
    same_bytes(ix.gather(case.qs, 10), H.gather(case.qs, case.rs, 10))


# ----------------------------------------------------------------------------------------------------------------------
# statistics as conditions; devices
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_overlap", [1, 3])
def test_what_was_counted_and_what_crossed_the_link(min_overlap):
    """conditions, not measurements: the model says how many pairs are candidates and how many rows, numpy how many pairs share
    a hash"""
    case = IC.random_case(130)
    st = {}
    rows = GC.check_device(case, index_of(case).gather(case.qs, min_overlap, stats=st), min_overlap)
    k = GM.n_candidates(case.mq, case.mr, min_overlap)
    assert 0 < len(rows) < k < 5 * 130
    assert st["candidates"] == k and st["records_copied"] == len(rows)
    assert st["pairs_touched"] == IC.pairs_sharing_a_hash(case) >= k
    assert st["launches"] == 3 and st["kernel_ms"] > 0


def test_device_entries_give_the_same_rows():
    case = IC.random_case(70)
    sa, sb = {}, {}
    a = index_of(case, 1, (0,)).gather(case.qs, stats=sa)
    b = index_of(case, 1, (0, 0, 0)).gather(case.qs, stats=sb)  # five chunks over three entries, at once
    same_bytes(a, b)
    GC.check_device(case, b)
    assert sa["launches"] == sb["launches"] == 15 and sa["candidates"] == sb["candidates"] and sa["pairs_touched"] == sb["pairs_touched"]


def test_the_current_device_is_left_alone():
    hip = C.CDLL("libamdhip64.so")
    case = IC.hand_case()
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    with H.LibraryIndex(case.rs, (F.device_count() - 1,)) as ix:
        ix.gather(case.qs)
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
