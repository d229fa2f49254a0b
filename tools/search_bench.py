#!/usr/bin/env python3
"""finch_search next to the route it replaces -- finch_dist(max_distance = 1.0) and a numpy reduction to the same rows -- on
one GPU, the same inputs, the same process; prints one JSON line.

    python tools/search_bench.py [--refs 10000] [--queries 100] [--top-n 10] [--min-containment 0.0] [--reps 3]

Sketches: synthetic Mash-1000 sketches as tools/dist_bench.py makes them; the queries are the library's first `--queries`
sketches, so each finds itself (the search has no self-skip; finch_dist skips equal sketches, which is why the queries get
names of their own here: then no pair is skipped and the two routes must give the same rows, and this tool asserts that they
do, bit for bit).  Timed per route, alternating, after one warm-up of each: the whole call (wall clock, the rows in numpy
arrays at the end) and the kernels (HIP events); for the search also the candidates that crossed from device to host.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import SketchParams  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402


def renamed(sk, idx, prefix):
    """the sketches idx of sk under names of their own"""
    out = None
    for i in idx:
        s = sk.sketch(i)
        kc, km = s.arrays
        one = H.sketches_from_arrays("%s%d" % (prefix, i), s.seq_length, s.num_valid_kmers, kc, km, SketchParams.mash(), H.FilterParams(False))
        if out is None:
            out = one
        else:
            out.append(one)
    return out


def reduce_dist_rows(rows, n_queries, min_containment, top_n):
    """the search's contract applied to finch_dist's rows: per query containment >= min_containment, ordered by containment
    descending then reference ascending, the first top_n"""
    rows = rows[rows["containment"] >= min_containment]
    order = np.lexsort((rows["reference"], -rows["containment"], rows["query"]))
    rows = rows[order]
    counts = np.bincount(rows["query"], minlength=n_queries)
    starts = np.concatenate([[0], np.cumsum(counts)])
    if top_n > 0:
        rank = np.arange(len(rows)) - starts[rows["query"]]
        rows = rows[rank < top_n]
        counts = np.minimum(counts, top_n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--min-containment", type=float, default=0.0)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    refs = sketches(a.refs, a.groups, a.seed)
    queries = renamed(refs, range(a.queries), "query")

    def search_route():
        st = {}
        t0 = time.perf_counter()
        offsets, rows = H.search(queries, refs, a.min_containment, a.top_n, stats=st)
        return time.perf_counter() - t0, st, offsets, rows

    def dist_route():
        st = {}
        t0 = time.perf_counter()
        rows = H.dist(queries, refs, max_distance=1.0, stats=st)
        t1 = time.perf_counter()
        offsets, kept = reduce_dist_rows(rows, a.queries, a.min_containment, a.top_n)
        t2 = time.perf_counter()
        st["dist_rows"], st["reduce_s"] = len(rows), t2 - t1
        return t2 - t0, st, offsets, kept

    _, _, so, sr = search_route()  # warm-up of each route: code object load, first allocations
    _, _, do, dr = dist_route()
    assert np.array_equal(so, do), "offsets differ"
    assert sr.tobytes() == dr.tobytes(), "rows differ"
    runs = {"search": [], "dist": []}
    for _ in range(a.reps):  # alternating
        for name, fn in (("search", search_route), ("dist", dist_route)):
            wall, st, o, r = fn()
            assert np.array_equal(o, so) and r.tobytes() == sr.tobytes(), "%s: rows differ between runs" % name
            runs[name].append((wall, st))
    out = {"refs": a.refs, "queries": a.queries, "pairs": a.refs * a.queries, "top_n": a.top_n, "min_containment": a.min_containment,
           "rows": int(len(sr)), "rows_equal": True}
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        out[name + "_kernel_s"] = [round(st["kernel_ms"] / 1e3, 6) for _, st in rs]
        out[name + "_launches"] = rs[0][1]["launches"]
    out["search_candidates_copied"] = runs["search"][0][1]["candidates_copied"]
    out["dist_rows_made"] = runs["dist"][0][1]["dist_rows"]
    out["dist_numpy_reduce_s"] = [round(st["reduce_s"], 6) for _, st in runs["dist"]]
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    out["wall_ratio_dist_over_search"] = round(med(out["dist_wall_s"]) / med(out["search_wall_s"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
