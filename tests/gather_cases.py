"""What tests/test_gather_host.py and tests/test_gpu_gather.py share: sketches built from arrays with their model twins, the
by-hand and random cases of the gather contract (tests/gather_model.py), and the comparison of the library's rows with the
model's -- integers by value, doubles as bit patterns, two NaNs being equal."""
import math
import struct

import numpy as np

import gather_model as GM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams

U64_MAX = (1 << 64) - 1


def mk(name, hashes, counts=None):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, (1 if counts is None else np.asarray(counts, np.uint32)), 0
    p = SketchParams.mash(no_strict=True)
    km = np.zeros((len(hs), p.kmer_length), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, p, H.FilterParams(False))


def collect(parts):
    out = parts[0]
    for p in parts[1:]:
        out.append(p)
    return out


class Case:
    """queries and a library, as the library's sketches (names q<i> / r<j>) and as the model's"""

    def __init__(self, queries, refs):
        """queries, refs: lists of (hashes, counts or None)"""
        self.mq = [GM.Sk(h, c) for h, c in queries]
        self.mr = [GM.Sk(h, c) for h, c in refs]
        self.qs = collect([mk("q%d" % i, h, c) for i, (h, c) in enumerate(queries)])
        self.rs = collect([mk("r%d" % i, h, c) for i, (h, c) in enumerate(refs)])
        self._want = {}

    def want(self, min_overlap=1, max_rounds=0):
        """the model's rows per query (computed once per setting)"""
        key = (min_overlap, max_rounds)
        if key not in self._want:
            self._want[key] = GM.gather(self.mq, self.mr, min_overlap, max_rounds)
        return self._want[key]


def bits(x):
    return struct.pack("<d", float(x))


def same_rows(got, want):
    """got: GATHER_DTYPE rows; want: the model's dicts"""
    assert len(got) == len(want), (len(got), len(want))
    for row, w in zip(got, want):
        for f in GM.INTS:
            assert int(row[f]) == w[f], (f, row, w)
        for f in GM.DOUBLES:
            assert bits(row[f]) == bits(w[f]) or (math.isnan(row[f]) and math.isnan(w[f])), (f, row, w)


def same_as_host(rows, host_rows):
    """two sets of the library's rows: every field bit for bit, two NaNs being equal"""
    assert len(rows) == len(host_rows)
    for f in GM.INTS:
        assert np.array_equal(rows[f], host_rows[f]), f
    for f in GM.DOUBLES:
        a, b = rows[f].view(np.uint64), host_rows[f].view(np.uint64)
        assert np.all((a == b) | (np.isnan(rows[f]) & np.isnan(host_rows[f]))), f


def hand_case():
    """query 0: A contains B, C is apart from A -- the rounds are A, C and B is never taken; query 1: ties on the count, which go
    to the lower index; query 2 is empty; query 3 shares nothing; query 4 equals a reference; query 5's counts make abund pass 2^32"""
    a, b, c = [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5], [7, 8, 9, 99]
    refs = [(b, None), (a, None), (c, None), ([], None), ([20, 21, 22, 23], None), ([22, 23, 24, 25], None), ([20, 21, 24, 25], None),
            ([40, 41, 42], None)]
    queries = [(list(range(1, 11)), list(range(10, 110, 10))),
               ([20, 21, 22, 23, 24, 25], [3, 1, 4, 1, 5, 9]),
               ([], None),
               ([1000, 1001], None),
               ([40, 41, 42], [7, 7, 7]),
               ([1, 2, 3, 7, 8], [0xffffffff, 0xffffffff, 0xfffffff0, 5, 0xffffffff])]
    return Case(queries, refs)


def random_case(seed, n_queries, n_refs, pool_size=60, max_q=50, max_r=25):
    """sketches from one small pool of hashes spread over the u64 range: ties and subsets everywhere"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, U64_MAX, pool_size * 2, dtype=np.uint64))[:pool_size]

    def part(max_size):
        n = int(rng.integers(0, min(max_size, len(pool)) + 1))
        return np.sort(rng.choice(pool, size=n, replace=False)), rng.integers(1, 1 << 20, n)

    return Case([part(max_q) for _ in range(n_queries)], [part(max_r) for _ in range(n_refs)])


def check_host(case, min_overlap=1, max_rounds=0, queries=None):
    """finch_gather_query against the model, for every query (or those named)"""
    want = case.want(min_overlap, max_rounds)
    for q in range(len(case.mq)) if queries is None else queries:
        same_rows(H.gather_query(case.rs, case.qs, q, min_overlap, max_rounds), want[q])


def check_device(case, got, min_overlap=1, max_rounds=0):
    """H.gather's (offsets, rows) against the model and against finch_gather_query"""
    offsets, rows = got
    want = case.want(min_overlap, max_rounds)
    assert offsets.tolist() == GM.offsets(want)
    same_rows(rows, [r for ws in want for r in ws])
    host = [H.gather_query(case.rs, case.qs, q, min_overlap, max_rounds) for q in range(len(case.mq))]
    same_as_host(rows, np.concatenate(host) if host else rows[:0])
    return rows
