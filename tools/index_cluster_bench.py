#!/usr/bin/env python3
"""finch_index_cluster (single-linkage clusters through the library index) next to what a user did before it existed -- the
pairwise finch_index_dist and a union-find over its rows on the host -- on one GPU: the same library, the same index, the same
process; prints one JSON line.

    python tools/index_cluster_bench.py [--n 10000] [--max-distance 0.1] [--groups N/200] [--reps 3] [--margin M]

The library: tools/index_dist_bench.py's (synthetic Mash-1000 sketches, one pool of 1000 hashes per 200 sketches).  After one
warm-up of each route and the check that both give the same labels, timed alternating: LibraryIndex.cluster, and
LibraryIndex.dist followed by the union-find (numpy: the rows' endpoints hooked to their smaller label and the labels
pointer-jumped until nothing moves).  Wall clock of the whole call and the kernels (HIP events) of each; the baseline's wall is
given with and without its union-find.  --margin sets option index_cluster_margin (default: the library's 2^-20).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import finch_rs_amd as F  # noqa: E402
from finch_rs_amd import host as H  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402


def labels_from_rows(n, q, r):
    """the smallest index of every component of the graph whose edges are the rows (q, r)"""
    labels = np.arange(n, dtype=np.int64)
    q, r = np.asarray(q, np.int64), np.asarray(r, np.int64)
    while True:
        low = np.minimum(labels[q], labels[r])
        nxt = labels.copy()
        np.minimum.at(nxt, labels[q], low)  # hook each endpoint's label to the smaller one
        np.minimum.at(nxt, labels[r], low)
        nxt = np.minimum(nxt, nxt[nxt])     # pointer jumping
        while True:
            jump = nxt[nxt]
            if np.array_equal(jump, nxt):
                break
            nxt = jump
        if np.array_equal(nxt, labels):
            return labels.astype(np.uint32)
        labels = nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--max-distance", type=float, default=0.1)
    ap.add_argument("--groups", type=int, default=0, help="pools (default: n / 200)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--old-mode", action="store_true")
    ap.add_argument("--margin", type=float, default=0.0)
    a = ap.parse_args()
    if a.margin:
        F.set_option("index_cluster_margin", repr(a.margin))
    groups = a.groups or max(1, a.n // 200)
    sk = sketches(a.n, groups, a.seed)
    ix = H.LibraryIndex(sk)

    def cluster_route():
        st = {}
        t0 = time.perf_counter()
        labels = ix.cluster(a.max_distance, a.old_mode, stats=st)
        return time.perf_counter() - t0, st, labels

    def dist_route():
        st = {}
        t0 = time.perf_counter()
        rows = ix.dist(None, a.max_distance, a.old_mode, stats=st)
        t1 = time.perf_counter()
        labels = labels_from_rows(len(sk), rows["query"], rows["reference"])
        return time.perf_counter() - t0, t1 - t0, st, labels, len(rows)

    _, st, want = cluster_route()  # warm-up of each route
    _, _, dst, other, n_rows = dist_route()
    equal = bool(np.array_equal(want, other))
    out = {"n": a.n, "pairs": a.n * a.n, "groups": groups, "max_distance": a.max_distance, "old_mode": a.old_mode,
           "margin": a.margin or 2.0 ** -20, "clusters": st["clusters"], "edges": st["edges"], "dist_rows": n_rows,
           "pairs_touched": st["pairs_touched"], "pairs_united": st["pairs_united"], "pairs_copied": st["pairs_copied"],
           "pairs_kept_host": st["pairs_kept_host"], "cluster_launches": st["launches"], "dist_pairs_copied": dst["pairs_copied"],
           "dist_launches": dst["launches"]}
    runs = {"cluster": [], "dist_uf": [], "dist": []}
    for _ in range(a.reps):  # alternating
        wall, st, labels = cluster_route()
        runs["cluster"].append((wall, st["kernel_ms"]))
        equal = equal and bool(np.array_equal(labels, want))
        wall, dist_wall, dst, labels, _ = dist_route()
        runs["dist_uf"].append((wall, dst["kernel_ms"]))
        runs["dist"].append((dist_wall, dst["kernel_ms"]))
        equal = equal and bool(np.array_equal(labels, want))
    ix.close()
    out["labels_equal"] = equal
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        if name != "dist":
            out[name + "_kernel_s"] = [round(ms / 1e3, 6) for _, ms in rs]
    out["wall_ratio_dist_over_cluster"] = round(med(out["dist_wall_s"]) / med(out["cluster_wall_s"]), 3)
    out["wall_ratio_dist_uf_over_cluster"] = round(med(out["dist_uf_wall_s"]) / med(out["cluster_wall_s"]), 3)
    out["kernel_ratio_cluster_over_dist"] = round(med(out["cluster_kernel_s"]) / max(med(out["dist_uf_kernel_s"]), 1e-9), 3)
    print(json.dumps(out))
    if not equal:
        sys.exit("LibraryIndex.cluster and the union-find over LibraryIndex.dist's rows differ")


if __name__ == "__main__":
    main()
