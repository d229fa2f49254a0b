"""finch_index_gather without a device (include/finch_host.h): the symbols, the ABI version, and everything the call decides
before it looks for a device.  A library without a single hash needs no device, so an index of one is what the refusals are
tried on here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_index_gather", "finch_index_gather_stats")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def mk(name, hashes, k=21):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
    km = np.zeros((len(hs), k), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, SketchParams.mash(kmer_length=k), H.FilterParams(False))


def collect(*sks):
    out = mk(sks[0][0], sks[0][1])
    for name, hs in sks[1:]:
        out.append(mk(name, hs))
    return out


def last_error(built):
    return (built.finch_last_error() or b"").decode()


def c_index_gather(built, ix, q, min_overlap=1, max_rounds=0, out="ok"):
    p = C.c_void_p()
    rc = built.finch_index_gather(ix, q, min_overlap, max_rounds, C.byref(p) if out == "ok" else None)
    return rc, p, last_error(built)


@pytest.fixture()
def hashless_index(built):
    """an index of two empty sketches: built and used without a device"""
    lib = collect(("e0", []), ("e1", []))
    p = C.c_void_p()
    assert built.finch_index_new(lib._p, (C.c_int * 1)(0), 1, C.byref(p)) == _lib.FH_OK and p.value, last_error(built)
    del lib  # (the index is self-contained)
    yield p
    built.finch_index_free(p)


def test_symbols_exported_declared_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int finch_index_gather(const finch_index *ix, const finch_sketches *queries, uint64_t min_overlap, uint64_t max_rounds, "
            "finch_gather_result **out);") in flat
    assert "int finch_index_gather_stats(const finch_gather_result *r, uint64_t *pairs_touched);" in flat
    assert H._SYMS["finch_index_gather"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)])
    assert H._SYMS["finch_index_gather_stats"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    assert callable(H.LibraryIndex.gather)


def test_abi_version_is_at_least_17(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 17 and _lib.load().fh_abi_version() == want
    assert re.search(r"\b17: .*finch_index_gather", hdr.replace("\n", " "))


@pytest.mark.parametrize("min_overlap, max_rounds", [(0, 0), (1, 0), (3, 2), (10 ** 6, 5), ((1 << 64) - 1, (1 << 64) - 1)])
def test_a_library_without_a_hash_needs_no_device(built, hashless_index, min_overlap, max_rounds):
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]), ("c", []))
    for q in (a, H.select(a, [])):
        rc, r, msg = c_index_gather(built, hashless_index, q._p, min_overlap, max_rounds)
        assert rc == _lib.FH_OK and r.value, msg
        try:
            assert built.finch_gather_len(r) == 0
            offs = np.full(len(q) + 1, 77, np.uint64)
            assert built.finch_gather_offsets(r, offs.ctypes.data) == 0 and not offs.any()
            assert built.finch_gather_copy(r, None, None, None) == 0
            kms, nl, nc, nrec, nt = C.c_double(-1), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
            assert built.finch_gather_stats(r, C.byref(kms), C.byref(nl), C.byref(nc), C.byref(nrec)) == 0
            assert built.finch_index_gather_stats(r, C.byref(nt)) == 0
            assert (kms.value, nl.value, nc.value, nrec.value, nt.value) == (0.0, 0, 0, 0, 0)
        finally:
            built.finch_gather_free(r)


def test_null_arguments(built, hashless_index):
    a = collect(("a", [1, 2, 3]))
    for ix, q, out in ((None, a._p, "ok"), (hashless_index, None, "ok"), (hashless_index, a._p, None)):
        rc, _, msg = c_index_gather(built, ix, q, out=out)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    assert built.finch_index_gather_stats(None, None) == _lib.FH_ERR_INVALID


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
def test_unsorted_query_refused_by_name(built, hashless_index, bad):
    qs = collect(("g0", [1, 2, 3]), ("bad sketch", bad))
    rc, _, msg = c_index_gather(built, hashless_index, qs._p)
    assert rc == _lib.FH_ERR_INVALID
    assert "query sketch 1 (bad sketch)" in msg and "strictly ascending" in msg
    with pytest.raises(FinchError):
        H.LibraryIndex(collect(("e", []))).gather(qs)


def test_a_query_above_the_limit_is_refused_as_finch_gather_refuses_it(built, hashless_index):
    n = (1 << 20) + 1
    qs = collect(("fits", np.arange(1 << 20, dtype=np.uint64)), ("too long", np.arange(n, dtype=np.uint64)))
    rc, _, msg = c_index_gather(built, hashless_index, qs._p)
    assert rc == _lib.FH_ERR_UNSUPPORTED
    assert "query sketch 1 (too long)" in msg and "1048577 hashes" in msg and "at most 1048576" in msg
    p = C.c_void_p()
    empty = collect(("e", []))
    assert built.finch_gather(qs._p, empty._p, 1, 0, (C.c_int * 1)(0), 1, C.byref(p)) == _lib.FH_ERR_UNSUPPORTED
    assert last_error(built) == msg  # worded as finch_gather words it
    # the query that fits is served: no device is needed for a library without a hash
    fits = H.select(qs, [0])
    rc, r, msg = c_index_gather(built, hashless_index, fits._p)
    assert rc == _lib.FH_OK, msg
    built.finch_gather_free(r)


def test_gather_stats_of_a_dense_result_are_refused(built):
    a = collect(("a", [1, 2, 3]))
    none = H.select(a, [])
    p = C.c_void_p()
    assert built.finch_gather(none._p, a._p, 1, 0, (C.c_int * 1)(0), 1, C.byref(p)) == 0  # zero queries: no device
    try:
        assert built.finch_gather_len(p) == 0
        nt = C.c_uint64(1234)
        assert built.finch_index_gather_stats(p, C.byref(nt)) == _lib.FH_ERR_INVALID
        assert nt.value == 1234 and "finch_index_gather" in last_error(built)
    finally:
        built.finch_gather_free(p)


def test_python_surface_without_a_device(built):
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    with H.LibraryIndex(collect(("e0", []), ("e1", []))) as ix:
        st = {}
        offsets, rows = ix.gather(a, 1, 0, stats=st)
        assert offsets.tolist() == [0, 0, 0] and len(rows) == 0 and rows.dtype == H.GATHER_DTYPE
        assert st == dict(kernel_ms=0.0, launches=0, candidates=0, records_copied=0, pairs_touched=0)
        offsets, rows = ix.gather(H.select(a, []))
        assert offsets.tolist() == [0] and len(rows) == 0
    with pytest.raises(FinchError):
        ix.gather(a)
