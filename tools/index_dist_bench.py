#!/usr/bin/env python3
"""finch_index_dist (`finch dist --pairwise -d D` through the library index) next to finch_dist on one GPU: the same library, the
same process; prints one JSON line.

    python tools/index_dist_bench.py [--n 10000] [--max-distance 0.1] [--groups N/200] [--reps 3] [--no-dense]

The library: synthetic Mash-1000 sketches as tools/dist_bench.py makes them (`--groups` pools of 1000 hashes; a sketch keeps a
share f ~ U(0,1)^2 of its pool and fills up with hashes of its own), so only the sketches of one pool share hashes.  The default
is one pool per 200 sketches: 200 n pairs share a hash, and at --max-distance 0.1 fewer than half of them are kept -- below 10^7
rows at n = 100 000, where 50 pools (tools/dist_bench.py's default) would keep some 10^8.  After one warm-up of each route and
the check that both give the same bytes, timed alternating: building the index, the pairwise call through it, and finch_dist
(the dense route: code this tool's subject does not touch) -- the whole call (wall clock) and the kernels (HIP events) of each.
--no-dense leaves the dense route out (at n = 100 000 it would be 10^10 pairs).  kernel_ns_per_query_hash is the index route's
kernels, count and finish together, over the library's hashes: an upper bound of what the count kernel spends per query hash.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--max-distance", type=float, default=0.1)
    ap.add_argument("--groups", type=int, default=0, help="pools (default: n / 200)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--old-mode", action="store_true")
    ap.add_argument("--no-dense", action="store_true")
    a = ap.parse_args()
    groups = a.groups or max(1, a.n // 200)
    t0 = time.perf_counter()
    sk = sketches(a.n, groups, a.seed)
    made_s = time.perf_counter() - t0

    def build_route():
        t0 = time.perf_counter()
        ix = H.LibraryIndex(sk)
        return time.perf_counter() - t0, ix

    def index_route(ix):
        st = {}
        t0 = time.perf_counter()
        rows = ix.dist(None, a.max_distance, a.old_mode, stats=st)
        return time.perf_counter() - t0, st, rows

    def dense_route():
        st = {}
        t0 = time.perf_counter()
        rows = H.dist(sk, sk, a.max_distance, a.old_mode, stats=st)
        return time.perf_counter() - t0, st, rows

    _, ix = build_route()  # warm-up of each route: code object load, first allocations
    _, st, rows = index_route(ix)
    want = rows.tobytes()
    equal = None
    if not a.no_dense:
        equal = dense_route()[2].tobytes() == want
    out = {"n": a.n, "pairs": a.n * a.n, "groups": groups, "max_distance": a.max_distance, "old_mode": a.old_mode, "rows": int(len(rows)),
           "pairs_touched": st["pairs_touched"], "touched_share": st["pairs_touched"] / (a.n * a.n), "pairs_copied": st["pairs_copied"],
           "index_launches": st["launches"], "sketches_made_s": round(made_s, 3)}
    out.update({"index_" + k: v for k, v in ix.stats().items() if k != "build_kernel_ms"})
    ix.close()
    del rows
    runs = {"build": [], "index": []} if a.no_dense else {"build": [], "index": [], "dense": []}
    for _ in range(a.reps):  # alternating
        wall, ix = build_route()
        runs["build"].append((wall, ix.stats()["build_kernel_ms"]))
        wall, st, rows = index_route(ix)
        runs["index"].append((wall, st["kernel_ms"]))
        same = rows.tobytes() == want
        ix.close()
        if not a.no_dense:
            wall, st, rows = dense_route()
            runs["dense"].append((wall, st["kernel_ms"]))
            same = same and rows.tobytes() == want
            out["dense_launches"] = st["launches"]
            equal = equal and same
        elif not same:
            sys.exit("two calls through the index differ")
        del rows
    out["results_equal_bytes"] = equal
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        out[name + "_kernel_s"] = [round(ms / 1e3, 6) for _, ms in rs]
    out["kernel_ns_per_query_hash"] = round(med(out["index_kernel_s"]) * 1e9 / max(1, out["index_postings"]), 3)
    if not a.no_dense:
        index_wall, build_wall = med(out["index_wall_s"]), med(out["build_wall_s"])
        out["wall_ratio_dense_over_index"] = round(med(out["dense_wall_s"]) / index_wall, 3)
        out["wall_ratio_dense_over_build_and_index"] = round(med(out["dense_wall_s"]) / (index_wall + build_wall), 3)
        out["kernel_ratio_dense_over_index"] = round(med(out["dense_kernel_s"]) / max(med(out["index_kernel_s"]), 1e-9), 3)
    print(json.dumps(out))
    if equal is False:
        sys.exit("finch_index_dist and finch_dist differ")


if __name__ == "__main__":
    main()
