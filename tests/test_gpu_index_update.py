"""finch_index_add / finch_index_keep on the GPU (include/finch_host.h).  THE CONTRACT: after any sequence of
adds and keeps the index is indistinguishable from finch_index_new over the resulting list of sketches.  index_update_cases'
checker holds every reading call on the updated index -- search, dist (pairwise too, both modes), gather, compare_counts --
against the dense call on that list (bytes) and against a fresh index over it (bytes and statistics).  Small values of
index_update_tile make many tiles of a small library; no result may depend on it."""
import ctypes as C
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams
from index_update_cases import BELOW_ONE, TINY, TOP, check_index, collect, index_built, queries_for, spec

pytestmark = pytest.mark.gpu

TILES = (1, 3, 64, None)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


@contextmanager
def tile(n):
    try:
        if n is not None:
            F.set_option("index_update_tile", n)
        yield
    finally:
        F.set_option("index_update_tile", None)


def tile_id(n):
    return "tile_default" if n is None else "tile%d" % n


# ---- 1. by hand ----------------------------------------------------------------------------------------------------------

HAND = [spec("r0", [0, 10, 20, TOP]), ("r1_empty", []), spec("r2", [10, 30]), spec("r3_as_r2", [10, 30]), spec("r4", [0, 5]),
        spec("r5", [TOP]), spec("r6", [20, 30, 40, TOP]), spec("r7", [7])]
HAND_MORE = [("a0_empty", []), spec("a1_all_held", [0, 10, 30, TOP]), spec("a2_all_new", [1, 2, 3])]


def test_by_hand():
    assert sum(len(e) for _, e in HAND) == 16
    with H.LibraryIndex(collect(HAND)) as ix:
        st = {}
        ix.add(collect(HAND_MORE), stats=st)
        assert st["kernel_ms"] > 0
        # 16 postings, then 0 + 4 + 3 more; hash 0 is held by r0, r4 and now a1 (reference 9), 2^64 - 1 by r0, r5, r6 and a1
        assert ix.stats()["n_refs"] == 11 and ix.stats()["postings"] == 23
        check_index(ix, HAND + HAND_MORE)
        offsets, rows = ix.search(collect([spec("q", [0, TOP])]), TINY)
        assert sorted(rows["reference"].tolist()) == [0, 4, 5, 6, 9]


# ---- 2. where the new postings fall ---------------------------------------------------------------------------------------

@lru_cache(None)
def placement(which):
    """(old, more) as lists of specs"""
    if which == "below":
        return ([spec("o%d" % i, range(1000 + i, 1100, 7)) for i in range(5)], [spec("n%d" % i, range(i, 100, 9)) for i in range(4)])
    if which == "above":
        return ([spec("o%d" % i, range(i, 100, 9)) for i in range(4)], [spec("n%d" % i, range(1000 + i, 1100, 7)) for i in range(5)])
    if which == "alternating":  # merged, the postings go old, new, old, new, ...
        return ([spec("o%d" % i, range(2 * i, 400, 6)) for i in range(3)], [spec("n%d" % i, range(2 * i + 1, 400, 6)) for i in range(3)])
    if which == "one_old_posting":
        return ([("e", []), spec("o", [50])], [spec("n0", [1, 50, 99]), spec("n1", [50]), spec("n2", [2, 3])])
    if which == "one_new_posting":
        return ([spec("o0", [1, 50, 99]), spec("o1", [50, 60]), spec("o2", [2, 3])], [("e", []), spec("n", [50])])
    assert which == "pool"
    rng = np.random.default_rng(19)
    pool = np.unique(rng.integers(0, 2 ** 64, 2000, dtype=np.uint64, endpoint=False))
    draw = lambda name: spec(name, rng.choice(pool, int(rng.integers(0, 51)), replace=False))
    return [draw("o%d" % i) for i in range(70)], [draw("n%d" % i) for i in range(60)]


@pytest.mark.parametrize("t", TILES, ids=tile_id)
@pytest.mark.parametrize("which", ["below", "above", "alternating", "one_old_posting", "one_new_posting", "pool"])
def test_where_the_new_postings_fall(which, t):
    old, more = placement(which)
    with H.LibraryIndex(collect(old)) as ix:
        with tile(t):
            ix.add(collect(more))
        check_index(ix, old + more)


# ---- 3. a tie longer than any tile ----------------------------------------------------------------------------------------

N_HEAVY, N_HEAVY_MORE, SHARED = 5000, 300, 1 << 40


@lru_cache(None)
def heavy_specs():
    """every reference holds SHARED and three hashes of its own: SHARED's run is as long as the library"""
    return [spec("r%d" % r, [SHARED, 3 * r + 1, 3 * r + 2, (1 << 50) + r]) for r in range(N_HEAVY + N_HEAVY_MORE)]


@pytest.mark.parametrize("t", [64, None], ids=tile_id)
def test_a_tie_longer_than_any_tile(t):
    specs = heavy_specs()
    old, more = specs[:N_HEAVY], specs[N_HEAVY:]
    queries = [spec("only_shared", [SHARED]), spec("shared_and_own", [SHARED, SHARED + 5, 3 * 7 + 1, 3 * 5100 + 2, (1 << 50) + 4242]),
               spec("strangers", [SHARED + 1, SHARED + 2])]
    with H.LibraryIndex(collect(old)) as ix:
        with tile(t):
            ix.add(collect(more))
            check_index(ix, specs, queries, pairwise=False)  # (pairwise: 28 million rows; the small cases have it)
            third = list(range(0, len(specs), 3))
            ix.keep(third)
        assert ix.stats()["postings"] == 4 * len(third)
        check_index(ix, [specs[i] for i in third], queries, pairwise=False)


# ---- 4. sequences ---------------------------------------------------------------------------------------------------------

def test_five_adds_of_one_and_one_add_of_five_agree():
    old, more = placement("pool")
    old, more = old[:20], more[:5]
    with H.LibraryIndex(collect(old)) as one_by_one, H.LibraryIndex(collect(old)) as at_once:
        with tile(3):
            for s in more:
                one_by_one.add(collect([s]))
            at_once.add(collect(more))
        qs = collect(queries_for(old + more))
        assert [x.tobytes() for x in one_by_one.search(qs, TINY)] == [x.tobytes() for x in at_once.search(qs, TINY)]
        check_index(one_by_one, old + more)
        check_index(at_once, old + more)


def test_an_add_a_keep_an_add():
    old, more = placement("pool")
    now = old[:25]
    with H.LibraryIndex(collect(now)) as ix:
        with tile(64):
            ix.add(collect(more[:10]))
            now = now + more[:10]
            check_index(ix, now)
            keep = [i for i in range(len(now)) if i % 4 != 1]
            ix.keep(keep)
            now = [now[i] for i in keep]
            check_index(ix, now)
            ix.add(collect(more[10:17]))
            now = now + more[10:17]
            check_index(ix, now)


# ---- 5. keep --------------------------------------------------------------------------------------------------------------

N_KEEP_LIB = 24
KEEPS = {"drop_first": list(range(1, N_KEEP_LIB)), "drop_last": list(range(N_KEEP_LIB - 1)),
         "drop_middle": [i for i in range(N_KEEP_LIB) if i != 11], "every_other": list(range(0, N_KEEP_LIB, 2)),
         "all_but_one": [13], "none_dropped": list(range(N_KEEP_LIB))}


@pytest.mark.parametrize("t", [1, 64, None], ids=tile_id)
@pytest.mark.parametrize("which", sorted(KEEPS))
def test_keep(which, t):
    lib = placement("pool")[0][:N_KEEP_LIB]
    with H.LibraryIndex(collect(lib)) as ix:
        st = {}
        with tile(t):
            ix.keep(KEEPS[which], stats=st)
        assert st["kernel_ms"] > 0
        check_index(ix, [lib[i] for i in KEEPS[which]])


@pytest.mark.parametrize("t", [1, 64, None], ids=tile_id)
def test_keep_drops_every_hash_and_an_add_brings_them_back(t):
    lib = [spec("a", [1, 2, 3]), ("e0", []), spec("b", [2, 9]), ("e1", []), ("e2", [])]
    qs = collect([spec("q", [2, 3])])
    with H.LibraryIndex(collect(lib)) as ix:
        assert ix.compare_counts(qs, 1)["reference"].tolist() == [0, 2]  # (attaches the counts)
        with tile(t):
            ix.keep([1, 3, 4])
            assert ix.stats() == dict(n_refs=3, postings=0, device_bytes=0, build_kernel_ms=ix.stats()["build_kernel_ms"])
            offsets, rows = ix.search(qs, TINY)
            assert offsets.tolist() == [0, 0] and len(rows) == 0
            check_index(ix, [lib[1], lib[3], lib[4]])
            ix.add(collect([lib[2], lib[0]]))
        assert ix.stats()["postings"] == 5 and ix.stats()["device_bytes"] > 0
        check_index(ix, [lib[1], lib[3], lib[4], lib[2], lib[0]])


# ---- 6. counts ------------------------------------------------------------------------------------------------------------

def c_compare_counts(ix, qs, min_common):
    """finch_index_compare_counts itself, not the wrapper that attaches the counts -> (rc, rows or None)"""
    p = C.c_void_p()
    rc = H.lib().finch_index_compare_counts(ix._handle(), qs._p, min_common, C.byref(p))
    return rc, (H._counts_rows(p, None, from_index=True) if rc == 0 else None)


def test_attached_counts_follow_an_add_and_a_keep():
    old, more = placement("pool")
    old, more = old[:30], more[:12]
    qs = collect(queries_for(old + more))
    with H.LibraryIndex(collect(old)) as ix:
        assert ix.attach_counts() == 4 * sum(len(e) for _, e in old)
        with tile(3):
            ix.add(collect(more))
        now = old + more
        for min_common in (1, 2):
            rc, rows = c_compare_counts(ix, qs, min_common)
            assert rc == 0 and rows.tobytes() == H.compare_counts(collect(now), qs, min_common).tobytes()
        keep = [i for i in range(len(now)) if i % 3]
        with tile(3):
            ix.keep(keep)
        now = [now[i] for i in keep]
        for min_common in (1, 2):
            rc, rows = c_compare_counts(ix, qs, min_common)
            assert rc == 0 and len(rows) and rows.tobytes() == H.compare_counts(collect(now), qs, min_common).tobytes()


@pytest.mark.parametrize("with_hashes_too", [False, True], ids=["one_empty_sketch", "an_empty_sketch_among_others"])
def test_an_add_of_sketches_without_a_hash_to_an_index_with_counts(with_hashes_too):
    """the added sketches bring no counts at all (an empty array, which may be a null pointer): the add goes through as it does
    without attached counts, and the counts stay attached"""
    old, more = placement("pool")
    old = old[:12]
    added = [("empty_a", [])] + ([more[0], ("empty_b", []), more[1]] if with_hashes_too else [])
    with H.LibraryIndex(collect(old)) as ix:
        assert ix.attach_counts() > 0
        ix.add(collect(added))
        now = old + added
        assert ix.stats()["n_refs"] == len(now)
        qs = collect(queries_for(now))
        rc, rows = c_compare_counts(ix, qs, 1)  # (not attached again)
        assert rc == 0 and len(rows) and rows.tobytes() == H.compare_counts(collect(now), qs, 1).tobytes()
        check_index(ix, now)
        ix.add(collect([("empty_c", [])]))  # ... and once more, on the updated index
        check_index(ix, now + [("empty_c", [])])


def test_counts_never_attached_stay_unattached():
    old, more = placement("pool")
    qs = collect(queries_for(old[:10]))
    with H.LibraryIndex(collect(old[:10])) as ix:
        ix.add(collect(more[:3]))
        rc, _ = c_compare_counts(ix, qs, 1)
        assert rc == _lib.FH_ERR_STATE and "finch_index_attach_counts" in (H.lib().finch_last_error() or b"").decode()
        ix.keep([0, 2, 4, 11])
        assert c_compare_counts(ix, qs, 1)[0] == _lib.FH_ERR_STATE
        # attached now, against the updated library
        now = [old[0], old[2], old[4], more[1]]
        assert ix.compare_counts(qs, 1).tobytes() == H.compare_counts(collect(now), qs, 1).tobytes()


def test_an_add_and_a_keep_of_scaled_sketches():
    """the added references bring their scale with them: a pair with an added Scaled reference takes raw_distance's scale step
    (the cursors go on to the first hash >= M), on the device as in the dense call.  (Met by the library fuzz's mutant 4,
    docs/MEASUREMENTS_library_fuzz.md: every other test here adds Mash sketches.)"""
    m = (2 ** 64 - 1) // 2  # M of scale 0.5

    def scaled(name, hashes):
        kc = np.zeros(len(hashes), KC_DTYPE)
        kc["hash"], kc["count"] = np.asarray(sorted(hashes), np.uint64), 1
        return H.sketches_from_arrays(name, 100, 100, kc, np.zeros((len(hashes), 21), np.uint8), SketchParams.scaled(1000, 21, 0.5),
                                      H.FilterParams(False))

    def library(parts):
        out = scaled(*parts[0])
        for part in parts[1:]:
            out.append(scaled(*part))
        return out

    old = [("r0", [10, 20, 30, m - 5, m + 7]), ("r1", [20, 40])]
    more = [("a0", [10, 20, 25, 26, m - 9, m - 3, m + 1]), ("a1", [5, 20]), ("a2", [])]
    qs = library([("q0", [10, 20]), ("q1", [20, 26, m - 3]), ("q2", [m + 1, m + 7])])
    with H.LibraryIndex(library(old)) as ix:
        ix.add(library(more))
        now = library(old + more)
        _, rows = ix.search(qs, TINY)
        a0 = rows[(rows["query"] == 0) & (rows["reference"] == 2)][0]
        # q0 = {10, 20} against a0: both shared, the walk stops at 20 with j = 2, the step takes j to #{r < M} = 6
        assert (int(a0["common_hashes"]), int(a0["total_hashes"]), float(a0["containment"])) == (2, 6, 2 / 6)
        for keep in (None, [0, 2, 3]):
            if keep is not None:
                ix.keep(keep)
                now = H.select(now, keep)
            assert [x.tobytes() for x in ix.search(qs, TINY)] == [x.tobytes() for x in H.search(qs, now, TINY)]
            assert ix.dist(qs, BELOW_ONE).tobytes() == H.dist(qs, now, BELOW_ONE).tobytes()
            assert ix.dist(None, BELOW_ONE).tobytes() == H.dist(now, now, BELOW_ONE).tobytes()
            with H.LibraryIndex(now) as fresh:
                assert [x.tobytes() for x in ix.search(qs, 0.3, 2)] == [x.tobytes() for x in fresh.search(qs, 0.3, 2)]


# ---- 7. chunks and entries ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk, devices", [(2, (0,)), (2, (0, 0, 0)), (None, (0, 0, 0))], ids=["chunk2", "chunk2_three_entries", "three_entries"])
def test_chunks_and_entries(chunk, devices):
    old, more = placement("pool")
    old, more = old[:20], more[:8]
    with index_built(collect(old), devices, chunk) as ix:
        with tile(64):
            ix.add(collect(more))
        # seven queries: four launches of two, dealt over the entries; the checker compares `launches` with a fresh index's
        assert check_index(ix, old + more, devices=devices, chunk=chunk) == 18
        st = {}
        ix.search(collect(queries_for(old + more)), TINY, stats=st)
        assert st["launches"] == (4 if chunk == 2 else 1)
        ix.keep(list(range(3, 25)))
        check_index(ix, (old + more)[3:25], devices=devices, chunk=chunk)


# ---- 8. state -------------------------------------------------------------------------------------------------------------

def test_state_after_updates_and_refusals():
    hip = C.CDLL("libamdhip64.so")
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    old, more = placement("pool")
    old, more = old[:15], more[:6]
    old_refs = collect(old)
    qs = collect(queries_for(old + more))
    with H.LibraryIndex(collect(old), devices=(F.device_count() - 1,)) as ix:
        try:
            F.set_option("index_max_postings", sum(len(e) for _, e in old + more) - 1)
            with pytest.raises(F.FinchHipError):
                ix.add(collect(more))
        finally:
            F.set_option("index_max_postings", None)
        assert len(ix.refs) == len(old)
        check_index(ix, old)  # the refused add left the index answering as before
        ix.add(collect(more))
        assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
        first, again = ix.search(qs, 0.1, 3), ix.search(qs, 0.1, 3)
        assert [x.tobytes() for x in first] == [x.tobytes() for x in again]
        p = C.c_void_p()
        rc = H.lib().finch_index_dist(ix._handle(), old_refs._p, qs._p, 0, 0.5, C.byref(p))
        assert rc == _lib.FH_ERR_INVALID and "refs must be the library of the index" in (H.lib().finch_last_error() or b"").decode()
        with pytest.raises(FinchError):
            ix.keep([len(old) + len(more)])
        ix.keep(list(range(2, len(old) + len(more))))
        assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
        check_index(ix, (old + more)[2:])
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
