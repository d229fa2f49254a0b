"""finch_compare_counts on the GPU (include/finch_host.h): every row against finch_compare_counts_pair (the
reference's loop on the host) and against tests/moments_model.py -- integers equal, doubles equal as bit patterns, two NaNs
equal -- over the shape edges of the kernel: lane steps, reference blocks, LDS slices, chunks, device entries, thresholds."""
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
import moments_model as MM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams

pytestmark = pytest.mark.gpu

UNIVERSE = 6000                                  # hashes come from a few thousand values: matches are dense
QUERY_LENGTHS = (0, 1, 63, 64, 65, 1000, 4097)   # 4097 crosses a slice at the default cmpc_slice
REF_LENGTHS = (0, 1, 63, 64, 65, 200)            # lane-step edges
N_REFS = 130                                     # two blocks of 64 and two more
FIELDS = ("common", "ref_pos", "query_pos", "ref_count", "query_count", "var", "skew", "kurt")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def mk(name, entries):
    kc = np.zeros(len(entries), KC_DTYPE)
    kc["hash"] = np.asarray([h for h, _ in entries], np.uint64)
    kc["count"] = np.asarray([c for _, c in entries], np.uint32)
    km = np.zeros((len(entries), 21), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, SketchParams.mash(), H.FilterParams(False))


def collect(sketches, prefix):
    out = mk("%s0" % prefix, sketches[0])
    for i, s in enumerate(sketches[1:], 1):
        out.append(mk("%s%d" % (prefix, i), s))
    return out


def random_sketch(rng, n):
    hs = np.sort(rng.choice(UNIVERSE, size=n, replace=False)) * 977 + 5  # (spread out; still a few thousand distinct values)
    return [(int(h), int(c)) for h, c in zip(hs, rng.choice(MM.COUNTS, size=n))]


class Case:
    """queries and a library with, for every pair, the model's tuple and finch_compare_counts_pair's (computed once)"""

    def __init__(self, queries, refs):
        self.mq, self.mr = queries, refs
        self.qs, self.rs = collect(queries, "q"), collect(refs, "r")
        self.model = {(q, r): MM.compare_counts(ref, query) for q, query in enumerate(queries) for r, ref in enumerate(refs)}
        self.host = {(q, r): H.compare_counts_pair(self.rs, r, self.qs, q) for q in range(len(queries)) for r in range(len(refs))}
        for key, t in self.model.items():
            assert MM.same(self.host[key], t), (key, self.host[key], t)

    def check(self, rows, min_common=0, n_refs=None):
        """rows = H.compare_counts' against both judges: the pairs with common >= min_common, query-major, references ascending"""
        n_refs = len(self.mr) if n_refs is None else n_refs
        want = [(q, r) for q in range(len(self.mq)) for r in range(n_refs) if self.model[(q, r)][0] >= min_common]
        assert list(zip(rows["query"].tolist(), rows["reference"].tolist())) == want
        for row, key in zip(rows, want):
            got = tuple(row[f] for f in FIELDS)
            assert MM.same(got, self.host[key]), (key, got, self.host[key])
            assert MM.same(got, self.model[key]), (key, got, self.model[key])
        return want


@lru_cache(None)
def edge_case():
    rng = np.random.default_rng(2024)
    queries = [random_sketch(rng, n) for n in QUERY_LENGTHS]
    lengths = list(REF_LENGTHS) * 2 + [int(x) for x in rng.integers(0, 201, N_REFS - 2 * len(REF_LENGTHS))]
    refs = [random_sketch(rng, n) for n in lengths]
    # pairs that share everything, so that the recurrence runs long: the 1000-long query's first 200 entries, its last 64 with
    # other counts, and the 4097-long query's entries either side of the default slice's edge
    refs[20] = queries[5][:200]
    refs[21] = [(h, MM.COUNTS[(i * 7) % 4]) for i, (h, _) in enumerate(queries[5][-64:])]
    refs[70] = queries[6][4000:4097]
    refs[129] = queries[6][4090:4097]
    return Case(queries, refs)


def with_options(fn, slice_=None, chunk=None):
    try:
        F.set_option("cmpc_slice", slice_)
        F.set_option("cmpc_chunk_pairs", chunk)
        return fn()
    finally:
        F.set_option("cmpc_slice", None)
        F.set_option("cmpc_chunk_pairs", None)


def test_edges_by_default():
    case = edge_case()
    st = {}
    rows = H.compare_counts(case.rs, case.qs, stats=st)
    want = case.check(rows)
    assert len(want) == len(QUERY_LENGTHS) * N_REFS == st["records_copied"] and st["launches"] == 1
    commons = rows["common"].reshape(len(QUERY_LENGTHS), N_REFS)
    assert commons[5, 20] == 200 and commons[5, 21] == 64 and commons[6, 70] == 97 and commons[6, 129] == 7
    assert not commons[0].any() and np.isnan(rows["var"][:N_REFS]).all()  # the empty query
    assert rows.dtype == H.COUNTS_DTYPE


@pytest.mark.parametrize("n_refs", [1, 63, 64, 65])
def test_reference_block_edges(n_refs):
    case = edge_case()
    st = {}
    rows = H.compare_counts(H.select(case.rs, list(range(n_refs))), case.qs, stats=st)
    case.check(rows, 0, n_refs)
    assert st["records_copied"] == len(QUERY_LENGTHS) * n_refs


@pytest.mark.parametrize("slice_", [1, 7, 64, 4096])
def test_slices_carry_the_state(slice_):
    """the same inputs under every slice length: the running state of a pair waits in LDS between the slices"""
    case = edge_case()
    case.check(with_options(lambda: H.compare_counts(case.rs, case.qs, 0), slice_=slice_))


@pytest.mark.parametrize("devices", [(0,), (0, 0, 0)])
def test_chunks_and_device_entries(devices):
    case = edge_case()
    st = {}
    per_chunk = 9  # references per launch: 15 chunks, the last one short
    rows = with_options(lambda: H.compare_counts(case.rs, case.qs, 0, devices=devices, stats=st), chunk=per_chunk * len(QUERY_LENGTHS))
    case.check(rows)
    assert st["launches"] == (N_REFS + per_chunk - 1) // per_chunk and st["records_copied"] == len(QUERY_LENGTHS) * N_REFS


def test_thresholds_and_stats():
    case = edge_case()
    commons = sorted(t[0] for t in case.model.values() if t[0] > 1)
    exact = commons[len(commons) // 2]  # a value some pairs reach exactly
    assert any(t[0] == exact for t in case.model.values()) and any(t[0] < exact for t in case.model.values())
    for min_common in (0, 1, exact, exact + 1, 2 ** 40):
        for chunk in (None, 20 * len(QUERY_LENGTHS)):
            st = {}
            rows = with_options(lambda: H.compare_counts(case.rs, case.qs, min_common, stats=st), chunk=chunk)
            want = case.check(rows, min_common)
            assert st["records_copied"] == len(want) == sum(1 for t in case.model.values() if t[0] >= min_common)
            assert st["launches"] == (1 if chunk is None else (N_REFS + 19) // 20)
            if min_common == 0:
                assert len(want) == len(QUERY_LENGTHS) * N_REFS
            if min_common == 2 ** 40:
                assert len(want) == 0


def test_same_call_twice_same_bytes():
    case = edge_case()
    a = with_options(lambda: H.compare_counts(case.rs, case.qs, 1), chunk=30 * len(QUERY_LENGTHS))
    b = with_options(lambda: H.compare_counts(case.rs, case.qs, 1), chunk=30 * len(QUERY_LENGTHS))
    assert len(a) and a.tobytes() == b.tobytes()


def test_the_current_device_is_left_alone():
    """(tells a call that leaves the device changed only where there is a second GPU: with one, the last device is device 0)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    rs = collect([[(1, 2), (2, 1), (3, 5), (4, 1)], [], [(2, 3), (4, 4), (9, 1)]], "r")
    qs = collect([[(2, 1), (3, 1), (4, 7)], [(5, 1)]], "q")
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    rows = H.compare_counts(rs, qs, devices=(F.device_count() - 1,))
    assert rows["common"].tolist() == [3, 0, 2, 0, 0, 0]
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
