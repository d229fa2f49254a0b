"""The library search without a device: tests/search_model.py against a literal transliteration of the two python.rs loops it
stands for, the six finch_search symbols and the ABI version, and everything finch_search decides before it looks for a device.
(The refusal of a sketch of 2^32 - 1 hashes or more is check_ascending's, shared with finch_dist; a sketch of that size -- 32 GiB
of hashes -- is not built here.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dist_model as M
import finch_rs_amd as F
import search_model as SM
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_search", "finch_search_len", "finch_search_offsets", "finch_search_copy", "finch_search_stats", "finch_search_free")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


# ----------------------------------------------------------------------------------------------------------------------
# the model against the reference's loops as written
# ----------------------------------------------------------------------------------------------------------------------

def rs_best_match(sketches, query):
    """python.rs:202-216, line by line"""
    best_sketch = 0
    max_containment = 0.0
    for ix, sketch in enumerate(sketches):
        dist = M.distance(query, sketch, False, walk=True)
        if dist["containment"] > max_containment:
            max_containment = dist["containment"]
            best_sketch = ix
    sketches[best_sketch]  # (the reference clones sketches[best_sketch]: a panic on an empty library)
    return best_sketch


def rs_filter_to_matches(sketches, query, threshold):
    """python.rs:223-234, line by line; the indices of the sketches kept"""
    filtered = []
    for ix, sketch in enumerate(sketches):
        dist = M.distance(query, sketch, False, walk=True)
        if dist["containment"] >= threshold:
            filtered.append(ix)
    return filtered


def random_sketch(rng, pool, scaled_share):
    n = int(rng.integers(0, 9)) if rng.random() < 0.8 else 0
    hs = sorted(int(x) for x in rng.choice(pool, size=min(n, len(pool)), replace=False))
    if rng.random() < scaled_share:
        return M.Sk(hs, "scaled", float(rng.choice([0.5, 0.25, 0.1])), 21)
    return M.Sk(hs, "mash", 0.0, int(rng.choice([15, 21])))


def random_library(seed):
    rng = np.random.default_rng(seed)
    kind = seed % 4
    if kind == 0:  # a few values: ties everywhere
        pool = np.arange(1, 8, dtype=np.uint64) * 3
    elif kind == 1:  # values either side of the Scaled sketches' max hashes (u64::MAX / 2, / 4, / 10)
        pool = np.array([1, 5, M.U64_MAX // 10 - 1, M.U64_MAX // 10, M.U64_MAX // 4, M.U64_MAX // 4 + 1, M.U64_MAX // 2 - 1,
                         M.U64_MAX // 2, M.U64_MAX // 2 + 7, M.U64_MAX - 1, M.U64_MAX], np.uint64)
    else:
        pool = np.unique(rng.integers(0, 1 << 20, 14, dtype=np.uint64))
    scaled_share = (0.0, 0.9, 0.5, 0.3)[kind]
    refs = [random_sketch(rng, pool, scaled_share) for _ in range(int(rng.integers(0, 9)))]
    if kind == 3:  # a query that shares nothing: every containment 0
        query = M.Sk([int(pool.max()) + 1 + i for i in range(int(rng.integers(0, 4)))], "mash", 0.0, 21)
    else:
        query = random_sketch(rng, pool, scaled_share)
    return refs, query


def test_model_equals_the_reference_loops():
    seen = {"all_zero": 0, "tie_at_top": 0, "empty_ref": 0, "empty_query": 0, "scaled_pair": 0, "empty_library": 0}
    for seed in range(400):
        refs, query = random_library(seed)
        conts = [M.distance(query, r, False, walk=True)["containment"] for r in refs]
        if not refs:
            seen["empty_library"] += 1
            with pytest.raises(IndexError):
                rs_best_match(refs, query)
            with pytest.raises(SM.EmptyLibrary):
                SM.best_match(refs, query)
            assert SM.filter_to_matches(refs, query, 0.0) == rs_filter_to_matches(refs, query, 0.0) == []
            continue
        seen["all_zero"] += max(conts) == 0.0
        seen["tie_at_top"] += max(conts) > 0.0 and conts.count(max(conts)) > 1
        seen["empty_ref"] += any(len(r.hashes) == 0 for r in refs)
        seen["empty_query"] += len(query.hashes) == 0
        seen["scaled_pair"] += query.kind == "scaled" and any(r.kind == "scaled" for r in refs)
        assert SM.best_match(refs, query) == SM.best_match(refs, query, walk=True) == rs_best_match(refs, query), seed
        for thr in sorted(set(conts)) + [0.0, -1.0, 0.5, 1.0, math.nextafter(1.0, 2.0), math.inf, -math.inf, math.nan]:
            assert SM.filter_to_matches(refs, query, thr) == rs_filter_to_matches(refs, query, thr), (seed, thr)
            if conts and thr == max(conts) and thr > 0:
                above = math.nextafter(thr, math.inf)
                assert SM.filter_to_matches(refs, query, above) == rs_filter_to_matches(refs, query, above) == []
    assert all(v >= 10 for v in seen.values()), seen


def test_model_rows_and_order():
    q = M.Sk([1, 2, 3, 50], "mash", 0.0, 21)
    refs = [M.Sk([1, 2, 3]), M.Sk([]), M.Sk([1, 60]), M.Sk([1, 2, 3]), M.Sk([2, 7, 9])]
    found = SM.search([q], refs)[0]
    assert [r for r, _ in found] == [0, 2, 3, 4, 1]  # 3/3, 1/1 (60 is beyond the query), 3/3, 1/3, 0: ties by index
    assert [d["containment"] for _, d in found] == [1.0, 1.0, 1.0, 1 / 3, 0.0]
    for r, d in found:
        assert d == M.distance(q, refs[r], False, walk=True)
    assert [r for r, _ in SM.search([q], refs, 1 / 3, 0)[0]] == [0, 2, 3, 4]
    assert [r for r, _ in SM.search([q], refs, math.nextafter(1 / 3, 1), 0)[0]] == [0, 2, 3]
    assert [r for r, _ in SM.search([q], refs, 0.0, 2)[0]] == [0, 2]
    assert SM.search([q], refs, math.nan)[0] == []
    assert SM.offsets(SM.search([q, q], refs, 0.5)) == [0, 3, 6]


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------------------------------

def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    assert "typedef struct finch_search_result finch_search_result;" in hdr
    assert H._SYMS["finch_search"][1][2:4] == [C.c_double, C.c_uint32]


def test_abi_version_is_at_least_10(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 10 and _lib.load().fh_abi_version() == want


def mk(name, hashes, params=None, k=21):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
    km = np.zeros((len(hs), k), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, params or SketchParams.mash(kmer_length=k), H.FilterParams(False))


def collect(*sks):
    out = mk(sks[0][0], sks[0][1])
    for name, hs in sks[1:]:
        out.append(mk(name, hs))
    return out


def c_search(built, q, r, minc=0.0, top_n=0, devs=(0,), n_devices=None, out="ok"):
    darr = (C.c_int * max(len(devs), 1))(*devs) if devs is not None else None
    p = C.c_void_p()
    rc = built.finch_search(q, r, minc, top_n, darr, len(devs) if n_devices is None else n_devices, C.byref(p) if out == "ok" else None)
    return rc, p, (built.finch_last_error() or b"").decode()


def test_null_arguments_and_too_many_entries(built):
    a = collect(("a", [1, 2, 3]))
    for args in ((None, a._p), (a._p, None)):
        rc, _, msg = c_search(built, *args)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_search(built, a._p, a._p, out=None)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_search(built, a._p, a._p, devs=None, n_devices=1)
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_search(built, a._p, a._p, devs=[0] * 17)
    assert rc == _lib.FH_ERR_INVALID and "at most 16 device entries (got 17)" in msg
    assert built.finch_search_len(None) == 0
    assert built.finch_search_offsets(None, None) == _lib.FH_ERR_INVALID
    assert built.finch_search_copy(None, None, None, None) == _lib.FH_ERR_INVALID
    assert built.finch_search_stats(None, None, None, None) == _lib.FH_ERR_INVALID
    built.finch_search_free(None)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
@pytest.mark.parametrize("side", ["query", "reference"])
def test_unsorted_or_duplicate_hashes_refused_by_name(built, bad, side):
    good = collect(("g0", [1, 2, 3]), ("g1", [2, 4]))
    bad_set = collect(("g0", [1, 2, 3]), ("bad sketch", bad))
    q, r = (bad_set, good) if side == "query" else (good, bad_set)
    rc, _, msg = c_search(built, q._p, r._p)
    assert rc == _lib.FH_ERR_INVALID
    assert "%s sketch 1 (bad sketch)" % side in msg and "strictly ascending" in msg
    with pytest.raises(FinchError):
        H.search(q, r, top_n=1)


@pytest.mark.parametrize("top_n", [0, 1, 100])
def test_nothing_to_search_needs_no_device(built, top_n):
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    none = H.select(a, [])
    for q, r in ((none, a), (a, none), (none, none)):
        rc, p, _ = c_search(built, q._p, r._p, 0.0, top_n)
        assert rc == _lib.FH_OK and p.value
        try:
            assert built.finch_search_len(p) == 0
            offs = np.full(len(q) + 1, 77, np.uint64)
            assert built.finch_search_offsets(p, offs.ctypes.data) == 0 and not offs.any()
            assert built.finch_search_copy(p, None, None, None) == 0
            ms, nl, nc = C.c_double(-1), C.c_uint64(9), C.c_uint64(9)
            assert built.finch_search_stats(p, C.byref(ms), C.byref(nl), C.byref(nc)) == 0
            assert (ms.value, nl.value, nc.value) == (0.0, 0, 0)
        finally:
            built.finch_search_free(p)
        offsets, rows = H.search(q, r, top_n=top_n)
        assert offsets.tolist() == [0] * (len(q) + 1) and len(rows) == 0 and rows.dtype == H.DIST_DTYPE


def test_python_surface_without_a_device(built):
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    none = H.select(a, [])
    with pytest.raises(FinchError):
        H.best_match(none, a, 0)
    kept = H.filter_to_matches(none, a, 1, 0.5)
    assert isinstance(kept, H.Sketches) and len(kept) == 0


def test_no_device_is_an_error(built):
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    rc, _, msg = c_search(built, a._p, a._p)
    assert rc == _lib.FH_ERR_NO_DEVICE and "no usable HIP device" in msg
    for call in (lambda: H.search(a, a), lambda: H.search(a, a, math.nan, 1), lambda: H.best_match(a, a), lambda: H.filter_to_matches(a, a, 0, 0.1)):
        with pytest.raises(F.FinchHipError) as ei:
            call()
        assert "no usable HIP device" in str(ei.value)
