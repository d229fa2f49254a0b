#!/usr/bin/env python3
"""finch_index_search next to finch_search on one GPU: the same library, the same queries, the same process; prints one JSON
line.

    python tools/index_bench.py [--refs 10000] [--queries 1000] [--top-n 10] [--min-containment 0.1] [--reps 3]

The library: synthetic Mash-1000 sketches as tools/dist_bench.py makes them (`--groups` pools; a sketch keeps a random share of
its pool's hashes and fills up with hashes of its own).  The queries: a tenth are made from library members the same way -- a
random share of the member's hashes, the rest fresh --, so they share hashes with that member's pool; the others are fresh
throughout and share nothing.  After one warm-up of each route and the check that both give the same bytes, timed alternating:
building the index, the index search, finch_search (the dense route: code this tool's subject does not touch) -- the whole call
(wall clock) and the kernels (HIP events) of each.  Reported besides: the pairs the index search counted, as a share of
queries x references, and the number of searches after which building the index has paid for itself.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402


def make_queries(refs, n, seed):
    rng = np.random.default_rng(seed + 1000)
    size = 1000
    km = np.zeros((size, 21), np.uint8)
    out = None
    for i in range(n):
        if i % 10 == 0:
            member = refs.sketch(int(rng.integers(0, len(refs)))).arrays[0]["hash"]
            kept = member[rng.random(len(member)) < rng.random()]
        else:
            kept = np.zeros(0, np.uint64)
        fresh = rng.integers(0, 1 << 63, size - len(kept) + 50, dtype=np.uint64) * 2 + 1  # (odd: in no pool)
        hs = np.unique(np.concatenate([kept, fresh]))[:size]
        kc = np.zeros(len(hs), KC_DTYPE)
        kc["hash"], kc["count"] = hs, 1
        s = H.sketches_from_arrays("query%d" % i, 1000000, 1000000, kc, km[:len(hs)], SketchParams.mash(), H.FilterParams(False))
        if out is None:
            out = s
        else:
            out.append(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--min-containment", type=float, default=0.1)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    refs = sketches(a.refs, a.groups, a.seed)
    queries = make_queries(refs, a.queries, a.seed)

    def build_route():
        t0 = time.perf_counter()
        ix = H.LibraryIndex(refs)
        return time.perf_counter() - t0, ix

    def index_route(ix):
        st = {}
        t0 = time.perf_counter()
        offsets, rows = ix.search(queries, a.min_containment, a.top_n, stats=st)
        return time.perf_counter() - t0, st, offsets, rows

    def dense_route():
        st = {}
        t0 = time.perf_counter()
        offsets, rows = H.search(queries, refs, a.min_containment, a.top_n, stats=st)
        return time.perf_counter() - t0, st, offsets, rows

    _, ix = build_route()  # warm-up of each route: code object load, first allocations
    _, st, io, ir = index_route(ix)
    _, _, do, dr = dense_route()
    equal = io.tobytes() == do.tobytes() and ir.tobytes() == dr.tobytes()
    out = {"refs": a.refs, "queries": a.queries, "pairs": a.refs * a.queries, "top_n": a.top_n, "min_containment": a.min_containment,
           "rows": int(len(ir)), "results_equal_bytes": equal, "pairs_touched": st["pairs_touched"],
           "touched_share": st["pairs_touched"] / (a.refs * a.queries), "candidates_copied": st["candidates_copied"],
           "index_launches": st["launches"]}
    out.update({"index_" + k: v for k, v in ix.stats().items() if k != "build_kernel_ms"})
    ix.close()
    runs = {"build": [], "index": [], "dense": []}
    for _ in range(a.reps):  # alternating
        wall, ix = build_route()
        runs["build"].append((wall, ix.stats()["build_kernel_ms"]))
        wall, st, o, r = index_route(ix)
        runs["index"].append((wall, st["kernel_ms"]))
        equal = equal and o.tobytes() == do.tobytes() and r.tobytes() == dr.tobytes()
        ix.close()
        wall, st, o, r = dense_route()
        runs["dense"].append((wall, st["kernel_ms"]))
        equal = equal and o.tobytes() == do.tobytes() and r.tobytes() == dr.tobytes()
        out["dense_launches"] = st["launches"]
    out["results_equal_bytes"] = equal
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        out[name + "_kernel_s"] = [round(ms / 1e3, 6) for _, ms in rs]
    gain = med(out["dense_wall_s"]) - med(out["index_wall_s"])
    out["wall_ratio_dense_over_index"] = round(med(out["dense_wall_s"]) / med(out["index_wall_s"]), 3)
    out["kernel_ratio_dense_over_index"] = round(med(out["dense_kernel_s"]) / max(med(out["index_kernel_s"]), 1e-9), 3)
    out["break_even_searches"] = round(med(out["build_wall_s"]) / gain, 3) if gain > 0 else None  # build / (dense - index)
    print(json.dumps(out))
    if not equal:
        sys.exit("the index search and finch_search differ")


if __name__ == "__main__":
    main()
