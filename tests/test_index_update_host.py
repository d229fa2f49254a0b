"""finch_index_add / finch_index_keep without a device (include/finch_host.h): the symbols, the ABI version, the
option, every refusal the two calls decide before they look for a device, the whole life of an index of a library without a
hash -- which has no device entries, so that adds and keeps that leave it without one need no device either --, and the merge's
diagonal search, which lives in a header that compiles for the host (tests/hostcore/merge_path_host.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError
from index_update_cases import TINY, collect, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_index_add", "finch_index_keep")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def last_error(built):
    return (built.finch_last_error() or b"").decode()


def c_add(built, ix, more, ms="ok"):
    """more: a Sketches (alive for the call) or None"""
    t = C.c_double(-1.0)
    rc = built.finch_index_add(ix, more._p if more is not None else None, C.byref(t) if ms == "ok" else None)
    return rc, t.value, last_error(built)


def c_keep(built, ix, keep, n=None, ms="ok"):
    arr = (C.c_uint32 * max(len(keep), 1))(*keep) if keep is not None else None
    t = C.c_double(-1.0)
    rc = built.finch_index_keep(ix, arr, len(keep) if n is None else n, C.byref(t) if ms == "ok" else None)
    return rc, t.value, last_error(built)


def c_stats(built, ix):
    nr, npost, nbytes, ms = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9), C.c_double(-1)
    assert built.finch_index_stats(ix, C.byref(nr), C.byref(npost), C.byref(nbytes), C.byref(ms)) == 0
    return nr.value, npost.value, nbytes.value, ms.value


@pytest.fixture()
def hashless(built):
    """an index of three empty sketches: built, updated and searched without a device"""
    lib = collect([("e0", []), ("e1", []), ("e2", [])])
    p = C.c_void_p()
    assert built.finch_index_new(lib._p, None, 0, C.byref(p)) == _lib.FH_OK and p.value, last_error(built)
    yield p
    built.finch_index_free(p)


def test_symbols_exported_declared_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(finch_index \*ix" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    assert H._SYMS["finch_index_keep"][1][2] == C.c_uint32
    assert "OLD + NEW" in hdr  # the header says what an update's peak device memory is


def test_abi_version_is_at_least_19(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 19 and _lib.load().fh_abi_version() == want
    assert re.search(r"\b19: .*finch_index_add and finch_index_keep .*index_update_tile", hdr.replace("\n", " "))


def test_the_option_exists(built):
    assert "index_update_tile" in [n for n, _ in F.option_list()]
    F.set_option("index_update_tile", 3)
    assert F.get_option("index_update_tile") == "3"
    F.set_option("index_update_tile", None)
    assert F.get_option("index_update_tile") is None


def test_null_arguments(built, hashless):
    a = collect([spec("a", [1, 2, 3])])
    for ix, more in ((None, a), (hashless, None)):
        rc, _, msg = c_add(built, ix, more)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_keep(built, None, [0])
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_keep(built, hashless, None, n=2)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    assert c_stats(built, hashless)[:2] == (3, 0)
    # kernel_ms may be NULL; keep may be NULL where n_keep is 0
    assert c_add(built, hashless, collect([("e3", [])]), ms=None)[0] == _lib.FH_OK
    assert c_stats(built, hashless)[:2] == (4, 0)
    assert c_keep(built, hashless, None, n=0, ms=None)[0] == _lib.FH_OK
    assert c_stats(built, hashless)[:2] == (0, 0)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
def test_unsorted_added_sketch_refused_by_name(built, hashless, bad):
    kc_ok = spec("g0", [1, 2, 3])
    more = collect([kc_ok, ("bad sketch", [(h, 2) for h in bad])])
    rc, _, msg = c_add(built, hashless, more)
    assert rc == _lib.FH_ERR_INVALID
    assert "added sketch 1 (bad sketch)" in msg and "strictly ascending" in msg
    assert c_stats(built, hashless) == (3, 0, 0, 0.0)
    with H.LibraryIndex(collect([("e0", [])])) as ix:
        with pytest.raises(FinchError):
            ix.add(more)
        assert len(ix.refs) == 1 and ix.stats()["n_refs"] == 1


@pytest.mark.parametrize("keep, where", [([1, 0], "keep[1] = 0 after 1"), ([0, 2, 1], "keep[2] = 1 after 2"), ([1, 1], "keep[1] = 1 after 1"),
                                         ([0, 0, 1], "keep[1] = 0 after 0"), ([3], "keep[0] = 3"), ([0, 1, 2, 7], "keep[3] = 7"),
                                         ([2 ** 32 - 1], "keep[0] = 4294967295")])
def test_keep_unsorted_repeated_or_out_of_range_refused_with_the_position(built, hashless, keep, where):
    rc, _, msg = c_keep(built, hashless, keep)
    assert rc == _lib.FH_ERR_INVALID and "finch_index_keep" in msg and where in msg, msg
    assert c_stats(built, hashless) == (3, 0, 0, 0.0)
    with H.LibraryIndex(collect([("e0", []), ("e1", []), ("e2", [])])) as ix:
        with pytest.raises(FinchError):
            ix.keep(keep)
        assert len(ix.refs) == 3 and ix.stats()["n_refs"] == 3


def test_an_add_past_index_max_postings_is_refused_before_any_device(built, hashless):
    more = collect([spec("a", [1, 2, 3]), spec("b", [2])])
    try:
        F.set_option("index_max_postings", 3)
        rc, _, msg = c_add(built, hashless, more)
        assert rc == _lib.FH_ERR_UNSUPPORTED and "4 postings" in msg and "at most 3" in msg, msg
        assert c_stats(built, hashless) == (3, 0, 0, 0.0)
        # ... and hash-less sketches still go in under the same bound
        assert c_add(built, hashless, collect([("e3", [])]))[0] == _lib.FH_OK
        assert c_stats(built, hashless)[:2] == (4, 0)
    finally:
        F.set_option("index_max_postings", None)


def test_an_add_that_brings_the_first_hash_needs_a_device(built, hashless):
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    rc, _, msg = c_add(built, hashless, collect([spec("a", [1, 2, 3])]))
    assert rc == _lib.FH_ERR_NO_DEVICE and "no usable HIP device" in msg
    assert c_stats(built, hashless) == (3, 0, 0, 0.0)


def search_shape(built, ix, queries):
    p = C.c_void_p()
    assert built.finch_index_search(ix, queries._p, TINY, 0, C.byref(p)) == _lib.FH_OK, last_error(built)
    try:
        offs = np.full(len(queries) + 1, 77, np.uint64)
        assert built.finch_search_offsets(p, offs.ctypes.data) == 0
        return offs.tolist(), built.finch_search_len(p)
    finally:
        built.finch_search_free(p)


def test_a_hashless_index_grows_and_shrinks_without_a_device(built, hashless):
    qs = collect([spec("q0", [1, 2, 3]), ("q1", [])])
    rc, ms, msg = c_add(built, hashless, collect([("e3", []), ("e4", [])]))
    assert (rc, ms) == (_lib.FH_OK, 0.0), msg
    assert c_stats(built, hashless) == (5, 0, 0, 0.0)
    assert search_shape(built, hashless, qs) == ([0, 0, 0], 0)
    rc, ms, msg = c_add(built, hashless, H.select(qs, []))  # an empty `more`: a no-op that succeeds
    assert (rc, ms) == (_lib.FH_OK, 0.0) and c_stats(built, hashless)[0] == 5
    rc, ms, msg = c_keep(built, hashless, [0, 2, 4])
    assert (rc, ms) == (_lib.FH_OK, 0.0), msg
    assert c_stats(built, hashless) == (3, 0, 0, 0.0)
    assert search_shape(built, hashless, qs) == ([0, 0, 0], 0)
    rc, _, msg = c_keep(built, hashless, [3])  # held against the updated size
    assert rc == _lib.FH_ERR_INVALID and "keep[0] = 3" in msg and "3 references" in msg
    assert c_keep(built, hashless, [])[0] == _lib.FH_OK
    assert c_stats(built, hashless) == (0, 0, 0, 0.0)
    assert search_shape(built, hashless, qs) == ([0, 0, 0], 0)
    rc, _, msg = c_keep(built, hashless, [0])
    assert rc == _lib.FH_ERR_INVALID and "keep[0] = 0" in msg
    assert c_add(built, hashless, collect([("back", [])]))[0] == _lib.FH_OK
    assert c_stats(built, hashless)[:2] == (1, 0)


def test_python_surface_without_a_device(built):
    lib = collect([("e0", []), ("e1", []), ("e2", [])])
    qs = collect([spec("q0", [1, 2, 3])])
    with H.LibraryIndex(lib) as ix:
        st = {}
        ix.add(collect([("e3", []), ("e4", [])]), stats=st)
        assert st == dict(kernel_ms=0.0) and len(ix.refs) == 5 and ix.refs is lib and ix.stats()["n_refs"] == 5
        names = lambda: [H.lib().finch_sketch_name(ix.refs._p, i).decode() for i in range(len(ix.refs))]
        ix.delete(1)
        assert names() == ["e0", "e2", "e3", "e4"] and ix.stats()["n_refs"] == 4
        ix.delete(-1)
        assert names() == ["e0", "e2", "e3"]
        with pytest.raises(FinchError):
            ix.delete(3)
        ix.filter_to_names(["e3", "e0", "nobody"], stats=st)
        assert names() == ["e0", "e3"] and st == dict(kernel_ms=0.0) and ix.stats()["n_refs"] == 2
        offsets, rows = ix.search(qs, 0.5)
        assert offsets.tolist() == [0, 0] and len(rows) == 0
        assert ix.dist(qs, 0.5).dtype == H.DIST_DTYPE  # dist holds its refs against the updated library, which ix.refs is
        with pytest.raises(FinchError):
            ix.add(ix.refs)  # the library itself
        ix.keep([])
        assert len(ix.refs) == 0 and ix.stats() == dict(n_refs=0, postings=0, device_bytes=0, build_kernel_ms=0.0)
    with pytest.raises(FinchError):
        ix.add(qs)
    with pytest.raises(FinchError):
        ix.keep([0])


def test_the_merge_path_cuts_obey_the_rank_formulas(tmp_path):
    exe = str(tmp_path / "merge_path_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "finch_rs_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "hostcore", "merge_path_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.fullmatch(r"ok \d+", r.stdout.strip()) and int(r.stdout.split()[1]) > 10000, r.stdout
