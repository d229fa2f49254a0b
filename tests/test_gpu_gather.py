"""finch_gather on the GPU (include/finch_host.h) against tests/gather_model.py and against finch_gather_query,
the host's loop: the same rows in the same order, every integer the same, every double the same bytes."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
import gather_cases as GC
import gather_model as GM
from finch_rs_amd import host as H

pytestmark = pytest.mark.gpu

OPTIONS = ("dist_slice", "dist_chunk_pairs", "gather_slice", "gather_pos_bytes")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def with_options(fn, **opts):
    assert set(opts) <= set(OPTIONS)
    try:
        for name, value in opts.items():
            F.set_option(name, value)
        return fn()
    finally:
        for name in OPTIONS:
            F.set_option(name, None)


# ----------------------------------------------------------------------------------------------------------------------
# by hand and random
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def hand_case():
    return GC.hand_case()


@lru_cache(None)
def random_case(n_refs):
    """five queries; 70 and 130 references cross the counting kernel's block of 64"""
    return GC.random_case(1000 + n_refs, 5, n_refs, pool_size=150, max_q=120, max_r=10)


@pytest.mark.parametrize("max_rounds", [0, 1, 2, 5])
@pytest.mark.parametrize("min_overlap", [1, 3, 10 ** 6])
def test_by_hand(min_overlap, max_rounds):
    case = hand_case()
    rows = GC.check_device(case, H.gather(case.qs, case.rs, min_overlap, max_rounds), min_overlap, max_rounds)
    if min_overlap == 1 and max_rounds in (0, 2, 5):
        assert rows["query"].tolist() == [0, 0, 1, 1, 4, 5, 5]
        assert rows["reference"].tolist() == [1, 2, 4, 5, 7, 0, 2]  # A then C, never B; ties to the lower index
        assert int(rows["abund"][5]) == 2 * 0xffffffff + 0xfffffff0
    if min_overlap == 10 ** 6:
        assert len(rows) == 0


@pytest.mark.parametrize("max_rounds", [0, 1, 2, 5])
@pytest.mark.parametrize("min_overlap", [1, 3, 10 ** 6])
@pytest.mark.parametrize("n_refs", [70, 130])
def test_random(n_refs, min_overlap, max_rounds):
    case = random_case(n_refs)
    rows = GC.check_device(case, H.gather(case.qs, case.rs, min_overlap, max_rounds), min_overlap, max_rounds)
    if min_overlap == 1 and max_rounds == 0:
        assert len(rows) > 15 and rows["reference"].max() >= 64


def test_min_overlap_below_one_is_one():
    case = hand_case()
    a, b = H.gather(case.qs, case.rs, 0), H.gather(case.qs, case.rs, 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# query lengths: the word edges of the bitmask, and the whole of it
# ----------------------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 1023, 1025, 65537)


@lru_cache(None)
def length_case():
    """one query of every length; the references take the first hash, the last three (the last word's top bits), every third, a
    block in the middle, and hashes no query has"""
    rng = np.random.default_rng(77)
    queries, all_h = [], []
    for n in LENGTHS:
        h = np.unique(rng.integers(0, GC.U64_MAX, n + 50, dtype=np.uint64))[:n]
        assert len(h) == n
        queries.append((h, rng.integers(1, 1 << 30, n)))
        all_h.append(h)
    refs = []
    for h in all_h:
        if len(h):
            refs.append((np.unique(np.concatenate([h[:1], h[-3:]])), None))
            refs.append((h[::3], None))
            refs.append((h[len(h) // 3:len(h) // 3 + 40], None))
    refs.append((np.unique(np.concatenate([a[-2:] for a in all_h if len(a)])), None))  # the last two hashes of every query
    refs.append(([5, 6, 7], None))
    return GC.Case(queries, refs)


@pytest.mark.parametrize("min_overlap, max_rounds", [(1, 0), (2, 0), (1, 2)])
def test_query_lengths(min_overlap, max_rounds):
    case = length_case()
    rows = GC.check_device(case, H.gather(case.qs, case.rs, min_overlap, max_rounds), min_overlap, max_rounds)
    if (min_overlap, max_rounds) == (1, 0):
        assert set(rows["query"].tolist()) == set(range(1, len(LENGTHS)))
        assert int(rows["remaining"].min()) >= 0 and int(rows["query_len"].max()) == 65537


def test_the_longest_query_fills_the_mask():
    """1 048 576 hashes: all of the rounds kernel's 128 KiB of LDS; three small references at its first word, its last word and
    across the middle"""
    n = 1 << 20
    h = np.arange(n, dtype=np.uint64) * 7 + 3
    counts = (np.arange(n, dtype=np.uint64) % 1000 + 1).astype(np.uint32)
    refs = [(np.concatenate([h[:2], h[-33:]]), None), (np.concatenate([[np.uint64(1)], h[31:34], h[n // 2 - 1:n // 2 + 1]]), None),
            (h[-40:], None)]
    case = GC.Case([(h, counts)], refs)
    rows = GC.check_device(case, H.gather(case.qs, case.rs))
    assert rows["reference"].tolist() == [2, 1, 0] and rows["overlap"].tolist() == [40, 5, 2] and rows["common"].tolist() == [40, 5, 35]
    assert rows["remaining"].tolist() == [n - 40, n - 45, n - 47]


@pytest.mark.parametrize("order", ["long_last", "long_first", "long_between"])
def test_a_long_query_without_candidates_next_to_a_short_one_with(order):
    """the rounds kernel's mask is sized for the queries that have candidates: a much longer query of the same chunk that has
    none (it shares hashes, but fewer than min_overlap with any reference) must leave the mask alone and give no row"""
    n = 300_000
    long_h = np.arange(n, dtype=np.uint64) * 11 + 5
    short_h = np.arange(20, dtype=np.uint64) * 11 + 7          # none of them in long_h
    other_h = np.arange(33, dtype=np.uint64) * 11 + 9
    refs = [(np.sort(np.concatenate([short_h[:12], long_h[:3], long_h[-3:]])), None),     # 12 of the short query, 6 of the long one
            (np.sort(np.concatenate([short_h[10:], other_h[:11], long_h[n // 2:n // 2 + 9]])), None),  # 10 / 11 / 9
            (long_h[1000:1009], None)]                                                     # 9 of the long one: below 10
    queries = {"long_last": [(short_h, None), (other_h, None), (long_h, None)],
               "long_first": [(long_h, None), (short_h, None), (other_h, None)],
               "long_between": [(short_h, None), (long_h, None), (other_h, None)]}[order]
    case = GC.Case(queries, refs)
    st = {}
    rows = GC.check_device(case, H.gather(case.qs, case.rs, 10, stats=st), 10)
    long_at = [len(h) for h, _ in queries].index(n)
    assert long_at not in rows["query"].tolist() and sorted(set(rows["query"].tolist())) == [q for q in range(3) if q != long_at]
    assert st["candidates"] == 3 and st["records_copied"] == len(rows) == 2 and st["launches"] == 4  # one chunk of queries
    # with min_overlap 1 the long query has candidates and the mask is its own
    rows = GC.check_device(case, H.gather(case.qs, case.rs, 1), 1)
    assert rows["query"].tolist().count(long_at) == 3


# ----------------------------------------------------------------------------------------------------------------------
# slices of the positions kernel, chunks of the counting pass, the position budget
# ----------------------------------------------------------------------------------------------------------------------

@lru_cache(None)
def slice_case():
    """a 300-hash query; references whose matches sit either side of every slice edge of 7 and 64, and runs across them"""
    rng = np.random.default_rng(3)
    h = np.unique(rng.integers(0, GC.U64_MAX, 400, dtype=np.uint64))[:300]
    edges = sorted(set(i for e in list(range(0, 300, 7)) + list(range(0, 300, 64)) for i in (e - 1, e) if 0 <= i < 300))
    refs = [(h[edges], None), (h[60:70], None), (h[::2], None), (h[1::2][:100], None), (np.sort(np.concatenate([h[250:], h[:5]])), None),
            (h[5:9] + np.uint64(1), None)]
    return GC.Case([(h, rng.integers(1, 100, 300)), (h[100:200], None)], refs)


@pytest.mark.parametrize("slice_", ["1", "7", "64"])
def test_slices(slice_):
    case = slice_case()
    a = H.gather(case.qs, case.rs)
    b = with_options(lambda: H.gather(case.qs, case.rs), gather_slice=slice_, dist_slice=slice_)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    rows = GC.check_device(case, b)
    assert len(rows) >= 6


@pytest.mark.parametrize("chunk", ["5", "35", "325"])
def test_counting_chunks_and_what_crosses_the_link(chunk):
    """conditions on what crossed the link, not measurements: the model says how many pairs are candidates and how many rows"""
    case = random_case(130)
    for min_overlap in (1, 3):
        st = {}
        got = with_options(lambda: H.gather(case.qs, case.rs, min_overlap, stats=st), dist_chunk_pairs=chunk)
        rows = GC.check_device(case, got, min_overlap)
        k = GM.n_candidates(case.mq, case.mr, min_overlap)
        assert 0 < len(rows) < k < 5 * 130
        assert st["candidates"] == k and st["records_copied"] == len(rows)
        n_chunks = -(-130 // max(1, int(chunk) // 5))
        assert st["launches"] == 2 * n_chunks + 2 and st["kernel_ms"] > 0


def test_position_budget():
    case = random_case(70)
    want = H.gather(case.qs, case.rs)
    GC.check_device(case, want)
    need = [4 * sum(len(set(q.hashes) & set(r.hashes)) for r in case.mr) for q in case.mq]
    assert min(need) > 0
    # every query a chunk of its own: the same rows, five launches of each of the two kernels
    st = {}
    got = with_options(lambda: H.gather(case.qs, case.rs, stats=st), gather_pos_bytes=str(max(need)))
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert st["launches"] == 2 + 2 * 5
    # below one query's need: refused, the query named with the bytes it needs; nothing is left behind
    worst = int(np.argmax(need))
    with pytest.raises(F.FinchHipError) as ei:
        with_options(lambda: H.gather(case.qs, case.rs), gather_pos_bytes=str(max(need) - 1))
    assert "query sketch %d (q%d)" % (worst, worst) in str(ei.value) and "%d bytes" % max(need) in str(ei.value)
    again = H.gather(case.qs, case.rs)
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# reference lengths; a candidate that earlier winners use up
# ----------------------------------------------------------------------------------------------------------------------

def test_reference_lengths_and_a_candidate_used_up():
    rng = np.random.default_rng(11)
    h = np.unique(rng.integers(0, GC.U64_MAX // 2, 700, dtype=np.uint64))[:600]
    other = np.unique(rng.integers(GC.U64_MAX // 2, GC.U64_MAX, 1200, dtype=np.uint64))[:1000]
    long_ref = np.sort(np.concatenate([h[:200], other]))  # 1200 hashes: 19 steps of 64 lanes, the matches in the first steps
    refs = [(h[100:180], None),   # inside long_ref's share: a candidate (80 common) that the first winner uses up
            (long_ref, None),
            ([], None),           # a reference of length 0: never a candidate
            (h[150:260], None),   # 110 common; 60 left after long_ref
            (h[190:200], None),   # used up by long_ref as well
            (h[400:], None)]      # 200, ties with long_ref at round 0: the lower index first
    case = GC.Case([(h, rng.integers(1, 50, 600))], refs)
    st = {}
    rows = GC.check_device(case, H.gather(case.qs, case.rs, stats=st))
    assert rows["reference"].tolist() == [1, 5, 3] and rows["overlap"].tolist() == [200, 200, 60] and rows["common"].tolist() == [200, 200, 110]
    assert rows["ref_len"].tolist() == [1200, 200, 110]
    assert st["candidates"] == 5 and st["records_copied"] == 3
    # with min_overlap 61 the third round's candidate has fallen below the threshold and is out
    rows = GC.check_device(case, H.gather(case.qs, case.rs, 61), 61)
    assert rows["reference"].tolist() == [1, 5]


# ----------------------------------------------------------------------------------------------------------------------
# devices
# ----------------------------------------------------------------------------------------------------------------------

def test_device_entries_give_the_same_rows():
    case = random_case(70)
    a = H.gather(case.qs, case.rs, 1, 0, devices=(0,))
    b = H.gather(case.qs, case.rs, 1, 0, devices=(0, 0, 0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    GC.check_device(case, b)


def test_the_current_device_is_left_alone():
    hip = C.CDLL("libamdhip64.so")
    case = hand_case()
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    H.gather(case.qs, case.rs, devices=(F.device_count() - 1,))
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
