"""The gather without a device: finch_gather_query, the host's loop, against tests/gather_model.py; the symbols and the ABI
version; and everything finch_gather decides before it looks for a device.  (The refusal of a sketch of 2^32 - 1 hashes or more
is check_ascending's, shared with finch_dist; a sketch of that size is not built here.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finch_rs_amd as F
import gather_cases as GC
import gather_model as GM
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_gather_query", "finch_gather", "finch_gather_len", "finch_gather_offsets", "finch_gather_copy", "finch_gather_stats",
           "finch_gather_free")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


@pytest.fixture(scope="module")
def hand(built):
    return GC.hand_case()


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    assert "typedef struct finch_gather_result finch_gather_result;" in hdr
    assert H.GATHER_DTYPE.itemsize == 9 * 8 + 5 * 8 and H.GATHER_DTYPE.names == GM.INTS + GM.DOUBLES


def test_abi_version_is_at_least_14_and_the_options_exist(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 14 and _lib.load().fh_abi_version() == want
    names = [n for n, _ in F.option_list()]
    assert "gather_slice" in names and "gather_pos_bytes" in names


# ----------------------------------------------------------------------------------------------------------------------
# finch_gather_query against the model
# ----------------------------------------------------------------------------------------------------------------------

def test_by_hand(hand):
    rows = H.gather_query(hand.rs, hand.qs, 0)
    # by `common` the order would be r1 (A), r0 (B), r2 (C): the rounds are A, then C, and B is never taken
    assert rows["reference"].tolist() == [1, 2] and rows["overlap"].tolist() == [6, 3] and rows["common"].tolist() == [6, 3]
    assert rows["remaining"].tolist() == [4, 1] and rows["abund"].tolist() == [210, 240] and rows["round"].tolist() == [0, 1]
    assert rows["f_match"].tolist() == [1.0, 0.75] and rows["f_unique_weighted"].tolist() == [210 / 550, 240 / 550]
    ties = H.gather_query(hand.rs, hand.qs, 1)  # r4, r5, r6 share four hashes each with it: r4; then r5 and r6 tie at two: r5
    assert ties["reference"].tolist() == [4, 5] and ties["overlap"].tolist() == [4, 2] and ties["common"].tolist() == [4, 4]
    assert len(H.gather_query(hand.rs, hand.qs, 2)) == 0  # an empty query
    assert len(H.gather_query(hand.rs, hand.qs, 3)) == 0  # shares nothing
    same = H.gather_query(hand.rs, hand.qs, 4)             # equal to r7
    assert same["reference"].tolist() == [7] and same["remaining"].tolist() == [0] and same["f_match"].tolist() == [1.0]
    assert same["f_unique_to_query"].tolist() == [1.0] and same["average_abund"].tolist() == [7.0]
    big = H.gather_query(hand.rs, hand.qs, 5)
    assert big["abund"].tolist() == [2 * 0xffffffff + 0xfffffff0, 5 + 0xffffffff] and big["abund"][0] > 1 << 32


@pytest.mark.parametrize("max_rounds", [0, 1, 2])
@pytest.mark.parametrize("min_overlap", [0, 1, 3, 10 ** 6, (1 << 64) - 1])
def test_by_hand_against_the_model(hand, min_overlap, max_rounds):
    GC.check_host(hand, min_overlap, max_rounds)
    n = sum(len(ws) for ws in hand.want(min_overlap, max_rounds))
    assert (n == 0) == (min_overlap > 6)
    if min_overlap <= 1:
        assert [len(ws) for ws in hand.want(min_overlap, max_rounds)] == [min(x, max_rounds or x) for x in (2, 2, 0, 0, 1, 2)]


@pytest.mark.parametrize("seed", range(6))
def test_random_against_the_model(built, seed):
    case = GC.random_case(seed, 6, 12 + 9 * seed, pool_size=30 + 10 * seed)
    total = 0
    for min_overlap in (0, 1, 3, 10 ** 6):
        for max_rounds in (0, 1, 2):
            GC.check_host(case, min_overlap, max_rounds)
            total += sum(len(ws) for ws in case.want(min_overlap, max_rounds))
    assert total > 30
    assert max(len(ws) for ws in case.want(1, 0)) > 2


def test_query_index_and_null_arguments(built, hand):
    n = C.c_uint64(7)
    assert built.finch_gather_query(hand.rs._p, hand.qs._p, len(hand.qs), 1, 0, None, 0, C.byref(n)) == _lib.FH_ERR_INVALID
    assert "query sketch 6 of 6 sketches" in built.finch_last_error().decode()
    for args in ((None, hand.qs._p, 0, 1, 0, None, 0, C.byref(n)), (hand.rs._p, None, 0, 1, 0, None, 0, C.byref(n)),
                 (hand.rs._p, hand.qs._p, 0, 1, 0, None, 0, None), (hand.rs._p, hand.qs._p, 0, 1, 0, None, 3, C.byref(n))):
        assert built.finch_gather_query(*args) == _lib.FH_ERR_INVALID and "null argument" in built.finch_last_error().decode()
    # a short buffer: the first rows, and the number there are
    rows = np.zeros(1, H.GATHER_DTYPE)
    assert built.finch_gather_query(hand.rs._p, hand.qs._p, 0, 1, 0, rows.ctypes.data, 1, C.byref(n)) == 0
    assert n.value == 2 and int(rows["reference"][0]) == 1
    assert built.finch_gather_query(hand.rs._p, hand.qs._p, 0, 1, 0, None, 0, C.byref(n)) == 0 and n.value == 2
    # an empty library
    none = H.select(hand.rs, [])
    assert len(H.gather_query(none, hand.qs, 0)) == 0


# ----------------------------------------------------------------------------------------------------------------------
# what finch_gather decides before any device is touched
# ----------------------------------------------------------------------------------------------------------------------

def c_gather(built, q, r, min_overlap=1, max_rounds=0, devs=(0,), n_devices=None, out="ok"):
    darr = (C.c_int * max(len(devs), 1))(*devs) if devs is not None else None
    p = C.c_void_p()
    rc = built.finch_gather(q, r, min_overlap, max_rounds, darr, len(devs) if n_devices is None else n_devices, C.byref(p) if out == "ok" else None)
    return rc, p, (built.finch_last_error() or b"").decode()


def test_null_arguments_and_too_many_entries(built, hand):
    a = hand.rs
    for args in ((None, a._p), (a._p, None)):
        rc, _, msg = c_gather(built, *args)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_gather(built, a._p, a._p, out=None)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_gather(built, a._p, a._p, devs=None, n_devices=1)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_gather(built, a._p, a._p, devs=[0] * 17)
    assert rc == _lib.FH_ERR_INVALID and "at most 16 device entries (got 17)" in msg
    assert built.finch_gather_len(None) == 0
    assert built.finch_gather_offsets(None, None) == _lib.FH_ERR_INVALID
    assert built.finch_gather_copy(None, None, None, None) == _lib.FH_ERR_INVALID
    assert built.finch_gather_stats(None, None, None, None, None) == _lib.FH_ERR_INVALID
    built.finch_gather_free(None)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9]])
@pytest.mark.parametrize("side", ["query", "reference"])
def test_unsorted_or_duplicate_hashes_refused_by_name(built, bad, side):
    good = GC.collect([GC.mk("g0", [1, 2, 3]), GC.mk("g1", [2, 4])])
    bad_set = GC.collect([GC.mk("g0", [1, 2, 3]), GC.mk("bad sketch", bad)])
    q, r = (bad_set, good) if side == "query" else (good, bad_set)
    rc, _, msg = c_gather(built, q._p, r._p)
    assert rc == _lib.FH_ERR_INVALID
    assert "%s sketch 1 (bad sketch)" % side in msg and "strictly ascending" in msg
    with pytest.raises(FinchError):
        H.gather(q, r)
    with pytest.raises(FinchError) as ei:  # the host's loop refuses the same sketch, by name
        H.gather_query(r, q, 1 if side == "query" else 0)
    assert "%s sketch 1 (bad sketch)" % side in str(ei.value)


def test_a_query_above_the_mask_is_refused_by_name(built):
    limit = 1 << 20
    long_q = GC.collect([GC.mk("short", [1, 2, 3]), GC.mk("too long", np.arange(limit + 1, dtype=np.uint64) * 3)])
    refs = GC.collect([GC.mk("r0", [3, 6, 9])])
    rc, _, msg = c_gather(built, long_q._p, refs._p)
    assert rc == _lib.FH_ERR_UNSUPPORTED
    assert "query sketch 1 (too long)" in msg and "1048577 hashes" in msg and "1048576" in msg
    # the limit is the device's: the host's loop takes the same query
    rows = H.gather_query(refs, long_q, 1)
    assert rows["reference"].tolist() == [0] and rows["overlap"].tolist() == [3] and rows["remaining"].tolist() == [limit - 2]
    # ... and a long reference is no reason to refuse (nothing to do without queries: no device needed)
    none = H.select(long_q, [])
    rc, p, _ = c_gather(built, none._p, long_q._p)
    assert rc == _lib.FH_OK
    built.finch_gather_free(p)


def test_nothing_to_gather_needs_no_device(built, hand):
    a = hand.rs
    none = H.select(a, [])
    for q, r in ((none, a), (a, none), (none, none)):
        rc, p, _ = c_gather(built, q._p, r._p)
        assert rc == _lib.FH_OK and p.value
        try:
            assert built.finch_gather_len(p) == 0
            offs = np.full(len(q) + 1, 77, np.uint64)
            assert built.finch_gather_offsets(p, offs.ctypes.data) == 0 and not offs.any()
            assert built.finch_gather_copy(p, None, None, None) == 0
            ms, nl, nc, nrec = C.c_double(-1), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
            assert built.finch_gather_stats(p, C.byref(ms), C.byref(nl), C.byref(nc), C.byref(nrec)) == 0
            assert (ms.value, nl.value, nc.value, nrec.value) == (0.0, 0, 0, 0)
        finally:
            built.finch_gather_free(p)
        offsets, rows = H.gather(q, r)
        assert offsets.tolist() == [0] * (len(q) + 1) and len(rows) == 0 and rows.dtype == H.GATHER_DTYPE


def test_no_device_is_an_error(built, hand):
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    rc, _, msg = c_gather(built, hand.qs._p, hand.rs._p)
    assert rc == _lib.FH_ERR_NO_DEVICE and "no usable HIP device" in msg
    with pytest.raises(F.FinchHipError) as ei:
        H.gather(hand.qs, hand.rs)
    assert "no usable HIP device" in str(ei.value)
