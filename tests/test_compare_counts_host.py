"""compare_counts without a device: finch_compare_counts_pair (the reference's loop on the host, the judge of the GPU tests)
against tests/moments_model.py bit for bit, the new symbols, options and ABI version, and everything finch_compare_counts
decides before it looks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finch_rs_amd as F
import moments_model as MM
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_compare_counts_pair", "finch_compare_counts", "finch_compare_counts_len", "finch_compare_counts_copy",
           "finch_compare_counts_stats", "finch_compare_counts_free")
BIG = 2 ** 32 - 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def mk(name, entries, k=21):
    """a one-sketch collection from [(hash, count)]"""
    kc = np.zeros(len(entries), KC_DTYPE)
    kc["hash"] = np.asarray([h for h, _ in entries], np.uint64)
    kc["count"] = np.asarray([c for _, c in entries], np.uint32)
    km = np.zeros((len(entries), k), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, SketchParams.mash(kmer_length=k), H.FilterParams(False))


def collect(sketches, prefix="s"):
    out = mk("%s0" % prefix, sketches[0])
    for i, s in enumerate(sketches[1:], 1):
        out.append(mk("%s%d" % (prefix, i), s))
    return out


def check_pair(built, ref, query):
    got = H.compare_counts_pair(mk("r", ref), 0, mk("q", query), 0)
    want = MM.compare_counts(ref, query)
    assert MM.same(got, want), (got, want, ref, query)
    assert got[:5] == MM.integers(ref, query)
    return got


def test_empty_sides_and_one_shared_hash(built):
    some = [(3, 2), (8, 1), (11, BIG)]
    assert check_pair(built, [], [])[:5] == (0, 0, 0, 0, 0)
    assert check_pair(built, [], some)[:5] == (0, 0, 0, 0, 0)
    assert check_pair(built, some, [])[:5] == (0, 0, 0, 0, 0)
    got = check_pair(built, some, [(1, 1), (8, 7), (20, 1)])
    assert got[:5] == (1, 3, 2, 1, 7) and got[5] == 0.0 and np.isnan(got[6]) and np.isnan(got[7])


def test_all_shared_counts_equal(built):
    ref = [(h, c) for h, c in zip(range(10, 30), [1, 2, 3] * 7)]
    for c in (1, 3, BIG):
        got = check_pair(built, ref, [(h, c) for h in range(5, 25)])
        assert got[0] == 15 and got[4] == 15 * c and got[5] == 0.0 and np.isnan(got[6]) and np.isnan(got[7])


def test_counts_from_the_edges_of_u32(built):
    rng = np.random.default_rng(3)
    for _ in range(40):
        n = int(rng.integers(2, 40))
        ref = [(h, int(rng.choice(MM.COUNTS))) for h in range(n)]
        query = [(h, int(rng.choice(MM.COUNTS))) for h in range(n)]
        got = check_pair(built, ref, query)
        assert got[0] == n and got[3] == sum(c for _, c in ref) and got[4] == sum(c for _, c in query)
    # sums that do not fit 32 bits
    got = check_pair(built, [(h, BIG) for h in range(9)], [(h, BIG) for h in range(9)])
    assert got[3] == got[4] == 9 * BIG


def test_disjoint_sketches(built):
    ref, query = [(h, 2) for h in range(0, 40, 2)], [(h, 3) for h in range(1, 41, 2)]
    got = check_pair(built, ref, query)
    assert got[:5] == (0, 20, 19, 0, 0) and all(np.isnan(x) for x in got[5:])  # (the query's 39 is beyond the reference)
    got = check_pair(built, [(h, 1) for h in range(10)], [(h, 1) for h in range(100, 110)])  # the reference runs out first
    assert got[:5] == (0, 10, 0, 0, 0)


def test_a_prefix_stops_the_walk_early(built):
    full = [(h * 3, 1 + h % 3) for h in range(50)]
    pre = full[:17]
    got = check_pair(built, full, pre)
    assert got[:3] == (17, 17, 17)  # the query is the prefix: the reference's walk stops after its 17th hash
    got = check_pair(built, pre, full)
    assert got[:3] == (17, 17, 17)
    got = check_pair(built, full, pre + [(49, 5)])  # one more query hash between two reference hashes (48 < 49 < 51)
    assert got[:3] == (17, 17, 18)


def test_random_dense_pairs(built):
    rng = np.random.default_rng(5)
    shared = 0
    for _ in range(200):
        universe = int(rng.choice([8, 30, 100]))
        ref = [(int(h), int(rng.choice(MM.COUNTS))) for h in sorted(rng.choice(universe, int(rng.integers(0, universe + 1)), replace=False))]
        query = [(int(h), int(rng.choice(MM.COUNTS))) for h in sorted(rng.choice(universe, int(rng.integers(0, universe + 1)), replace=False))]
        shared += check_pair(built, ref, query)[0]
    assert shared > 2000


def test_pair_arguments(built):
    a = collect([[(1, 1)], [(2, 1)]])
    m = H.CCountMoments()
    assert built.finch_compare_counts_pair(None, 0, a._p, 0, C.byref(m)) == _lib.FH_ERR_INVALID
    assert built.finch_compare_counts_pair(a._p, 0, None, 0, C.byref(m)) == _lib.FH_ERR_INVALID
    assert built.finch_compare_counts_pair(a._p, 0, a._p, 0, None) == _lib.FH_ERR_INVALID
    assert built.finch_compare_counts_pair(a._p, 2, a._p, 0, C.byref(m)) == _lib.FH_ERR_INVALID
    assert b"reference sketch 2 of 2" in built.finch_last_error()
    assert built.finch_compare_counts_pair(a._p, 0, a._p, 2, C.byref(m)) == _lib.FH_ERR_INVALID
    assert b"query sketch 2 of 2" in built.finch_last_error()
    with pytest.raises(FinchError):
        H.compare_counts_pair(a, 0, a, 5)


def c_call(built, r, q, min_common=0, devs=(0,), n_devices=None, out="ok"):
    darr = (C.c_int * max(len(devs), 1))(*devs) if devs is not None else None
    p = C.c_void_p()
    rc = built.finch_compare_counts(r, q, min_common, darr, len(devs) if n_devices is None else n_devices, C.byref(p) if out == "ok" else None)
    return rc, p, (built.finch_last_error() or b"").decode()


def test_null_arguments_and_too_many_entries(built):
    a = collect([[(1, 1), (2, 1)]])
    for args in ((None, a._p), (a._p, None)):
        rc, _, msg = c_call(built, *args)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_call(built, a._p, a._p, out=None)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_call(built, a._p, a._p, devs=None, n_devices=1)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_call(built, a._p, a._p, devs=[0] * 17)
    assert rc == _lib.FH_ERR_INVALID and "at most 16 device entries (got 17)" in msg
    assert built.finch_compare_counts_len(None) == 0
    assert built.finch_compare_counts_copy(None, None, None, None) == _lib.FH_ERR_INVALID
    assert built.finch_compare_counts_stats(None, None, None, None) == _lib.FH_ERR_INVALID
    built.finch_compare_counts_free(None)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
@pytest.mark.parametrize("side", ["query", "reference"])
def test_unsorted_or_duplicate_hashes_refused_by_name(built, bad, side):
    good = collect([[(1, 1), (2, 1), (3, 1)], [(2, 1), (4, 1)]], "g")
    bad_set = mk("g0", [(1, 1), (2, 1), (3, 1)])
    bad_set.append(mk("bad sketch", [(h, 1) for h in bad]))
    q, r = (bad_set, good) if side == "query" else (good, bad_set)
    rc, _, msg = c_call(built, r._p, q._p)
    assert rc == _lib.FH_ERR_INVALID
    assert "%s sketch 1 (bad sketch)" % side in msg and "strictly ascending" in msg
    with pytest.raises(FinchError):
        H.compare_counts(r, q)


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    assert "typedef struct finch_compare_counts_result finch_compare_counts_result;" in hdr
    assert "} finch_count_moments;" in hdr
    assert C.sizeof(H.CCountMoments) == 64 and H.COUNTS_DTYPE.itemsize == 72
    assert H._SYMS["finch_compare_counts"][1][2] == C.c_uint64


def test_abi_version_is_at_least_11(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 11 and _lib.load().fh_abi_version() == want


def test_options_listed(built):
    names = [n for n, _ in F.option_list()]
    assert "cmpc_slice" in names and "cmpc_chunk_pairs" in names
    F.set_option("cmpc_slice", 7)
    assert F.get_option("cmpc_slice") == "7"
    F.set_option("cmpc_slice", None)
    assert F.get_option("cmpc_slice") is None


@pytest.mark.parametrize("min_common", [0, 1, 2 ** 40])
def test_nothing_to_compare_needs_no_device(built, min_common):
    a = collect([[(1, 1), (2, 1), (3, 1)], [(2, 1), (3, 1)]])
    none = H.select(a, [])
    for r, q in ((none, a), (a, none), (none, none)):
        rc, p, _ = c_call(built, r._p, q._p, min_common)
        assert rc == _lib.FH_OK and p.value
        try:
            assert built.finch_compare_counts_len(p) == 0
            assert built.finch_compare_counts_copy(p, None, None, None) == 0
            ms, nl, nc = C.c_double(-1), C.c_uint64(9), C.c_uint64(9)
            assert built.finch_compare_counts_stats(p, C.byref(ms), C.byref(nl), C.byref(nc)) == 0
            assert (ms.value, nl.value, nc.value) == (0.0, 0, 0)
        finally:
            built.finch_compare_counts_free(p)
        st = {}
        rows = H.compare_counts(r, q, min_common, stats=st)
        assert len(rows) == 0 and rows.dtype == H.COUNTS_DTYPE and st == {"kernel_ms": 0.0, "launches": 0, "records_copied": 0}


def test_no_device_is_an_error(built):
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    a = collect([[(1, 1), (2, 1), (3, 1)], [(2, 1), (3, 1)]])
    rc, _, msg = c_call(built, a._p, a._p)
    assert rc == _lib.FH_ERR_NO_DEVICE and "no usable HIP device" in msg
    with pytest.raises(F.FinchHipError) as ei:
        H.compare_counts(a, a)
    assert "no usable HIP device" in str(ei.value)
