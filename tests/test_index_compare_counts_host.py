"""finch_index_attach_counts, finch_index_compare_counts and finch_index_compare_counts_stats without a device
(include/finch_host.h): the symbols, the ABI version, and everything the calls decide before they look for a
device.  An index of a library without a single hash needs no device, so every refusal and every empty result is tried on one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_index_attach_counts", "finch_index_compare_counts", "finch_index_compare_counts_stats")


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


def c_compare(built, ix, q, min_common, out="ok"):
    p = C.c_void_p()
    rc = built.finch_index_compare_counts(ix, q, min_common, C.byref(p) if out == "ok" else None)
    return rc, p, last_error(built)


@pytest.fixture()
def hashless(built):
    """an index of two empty sketches, and that library: built and used without a device"""
    lib = collect(("e0", []), ("e1", []))
    p = C.c_void_p()
    assert built.finch_index_new(lib._p, (C.c_int * 1)(0), 1, C.byref(p)) == _lib.FH_OK and p.value, last_error(built)
    yield p, lib
    built.finch_index_free(p)


def test_symbols_exported_declared_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    u64p = C.POINTER(C.c_uint64)
    assert H._SYMS["finch_index_attach_counts"] == (C.c_int, [C.c_void_p, C.c_void_p, u64p])
    assert H._SYMS["finch_index_compare_counts"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)])
    assert H._SYMS["finch_index_compare_counts_stats"] == (C.c_int, [C.c_void_p, u64p, u64p])


def test_abi_version_is_at_least_18(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 18 and _lib.load().fh_abi_version() == want
    assert re.search(r"\b18: .*finch_index_attach_counts.*finch_index_compare_counts", hdr.replace("\n", " "))


def test_min_common_zero_is_refused_with_a_pointer_to_the_dense_call(built, hashless):
    ix, _ = hashless
    a = collect(("a", [1, 2, 3]))
    rc, _, msg = c_compare(built, ix, a._p, 0)
    assert rc == _lib.FH_ERR_INVALID and "min_common" in msg and "use finch_compare_counts" in msg
    rc, _, msg = c_compare(built, ix, H.select(a, [])._p, 0)  # before anything else is looked at
    assert rc == _lib.FH_ERR_INVALID and "use finch_compare_counts" in msg


def test_null_arguments(built, hashless):
    ix, lib = hashless
    a = collect(("a", [1, 2, 3]))
    for i, q, out in ((None, a._p, "ok"), (ix, None, "ok"), (ix, a._p, None)):
        rc, _, msg = c_compare(built, i, q, 1, out=out)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    nb = C.c_uint64(77)
    for i, r in ((None, lib._p), (ix, None)):
        assert built.finch_index_attach_counts(i, r, C.byref(nb)) == _lib.FH_ERR_INVALID and "null argument" in last_error(built)
    assert nb.value == 77
    assert built.finch_index_compare_counts_stats(None, None, None) == _lib.FH_ERR_INVALID and "null argument" in last_error(built)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
def test_unsorted_query_refused_by_name(built, hashless, bad):
    qs = collect(("g0", [1, 2, 3]), ("bad sketch", bad))
    rc, _, msg = c_compare(built, hashless[0], qs._p, 1)
    assert rc == _lib.FH_ERR_INVALID
    assert "query sketch 1 (bad sketch)" in msg and "strictly ascending" in msg


@pytest.mark.parametrize("other", [(("e0", []),), (("e0", []), ("e1", []), ("e2", [])), (("e0", []), ("e1", [4, 9]))],
                         ids=["fewer_sketches", "more_sketches", "more_hashes"])
def test_attach_counts_of_another_library_is_refused(built, hashless, other):
    ix, _ = hashless
    lib = collect(*other)
    nb = C.c_uint64(77)
    assert built.finch_index_attach_counts(ix, lib._p, C.byref(nb)) == _lib.FH_ERR_INVALID
    msg = last_error(built)
    assert "refs has %d sketches and %d hashes" % (len(other), sum(len(h) for _, h in other)) in msg
    assert "the index was built from 2 and 0" in msg and "refs must be the library of the index" in msg
    assert nb.value == 77


def test_attach_counts_to_an_index_without_hashes_attaches_nothing(built, hashless):
    ix, lib = hashless
    nb = C.c_uint64(77)
    assert built.finch_index_attach_counts(ix, lib._p, C.byref(nb)) == _lib.FH_OK and nb.value == 0
    assert built.finch_index_attach_counts(ix, lib._p, None) == _lib.FH_OK
    nr, npost, nbytes, ms = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9), C.c_double(-1)
    assert built.finch_index_stats(ix, C.byref(nr), C.byref(npost), C.byref(nbytes), C.byref(ms)) == 0
    assert (nr.value, npost.value, nbytes.value, ms.value) == (2, 0, 0, 0.0)


@pytest.mark.parametrize("min_common", [1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 64 - 1])
def test_an_index_without_hashes_gives_an_empty_result(built, hashless, min_common):
    ix, _ = hashless
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    for q in (a, H.select(a, [])):
        rc, r, msg = c_compare(built, ix, q._p, min_common)  # (no counts attached: nothing to attach them to)
        assert rc == _lib.FH_OK and r.value, msg
        try:
            assert built.finch_compare_counts_len(r) == 0
            assert built.finch_compare_counts_copy(r, None, None, None) == 0
            kms, nl, nc, nt, nw = C.c_double(-1), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
            assert built.finch_compare_counts_stats(r, C.byref(kms), C.byref(nl), C.byref(nc)) == 0
            assert built.finch_index_compare_counts_stats(r, C.byref(nt), C.byref(nw)) == 0
            assert (kms.value, nl.value, nc.value, nt.value, nw.value) == (0.0, 0, 0, 0, 0)
            assert built.finch_index_compare_counts_stats(r, None, None) == 0
        finally:
            built.finch_compare_counts_free(r)


def test_index_stats_of_a_dense_result_are_refused(built):
    a = collect(("a", [1, 2, 3]))
    none = H.select(a, [])
    p = C.c_void_p()
    assert built.finch_compare_counts(a._p, none._p, 1, (C.c_int * 1)(0), 1, C.byref(p)) == 0  # zero queries: no device
    try:
        nt, nw = C.c_uint64(1234), C.c_uint64(5678)
        assert built.finch_index_compare_counts_stats(p, C.byref(nt), C.byref(nw)) == _lib.FH_ERR_INVALID
        assert (nt.value, nw.value) == (1234, 5678) and "finch_index_compare_counts" in last_error(built)
    finally:
        built.finch_compare_counts_free(p)


def test_python_surface_without_a_device(built):
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    hashless = collect(("e0", []), ("e1", []))
    with H.LibraryIndex(hashless) as ix:
        assert ix.attach_counts() == 0
        st = {}
        rows = ix.compare_counts(a, stats=st)
        assert len(rows) == 0 and rows.dtype == H.COUNTS_DTYPE
        assert st == dict(kernel_ms=0.0, launches=0, records_copied=0, pairs_touched=0, pairs_walked=0)
        assert len(ix.compare_counts(a, 2 ** 40)) == 0
        for min_common in (0, -1):
            with pytest.raises(FinchError):
                ix.compare_counts(a, min_common)
        ix.refs = a  # another library than the index's: the attachment is refused
        with pytest.raises(FinchError) as ei:
            ix.attach_counts()
        assert "refs must be the library of the index" in str(ei.value)
    with pytest.raises(FinchError):
        ix.compare_counts(a)
    with pytest.raises(FinchError):
        ix.attach_counts()
