#!/usr/bin/env python3
"""finch_compare_counts on one GPU next to the loop it stands for, finch_compare_counts_pair on one core; writes
profiles/compare_counts_bench.json and prints it as one JSON line.

    python tools/compare_counts_bench.py [--refs 10000] [--queries 100] [--reps 3] [--host-sample 20000]

Shape: a library of `--refs` Mash-1000 sketches with counts, `--queries` queries, run twice:
  * "dissimilar": the queries share little with the library (fresh hashes; a handful of shared ones per pair at most), so a pair
    is all lookups and almost no recurrence;
  * "similar": every query is a near copy of the one genome the whole library is made of near copies of, so every
    pair shares most of its 1000 hashes and the wave-uniform f64 recurrence runs a thousand steps per pair.
Per run: the whole call (wall clock, rows in a numpy array at the end), the kernels (HIP events), the records that crossed the
link, finch_dist's kernel time on the same sketches (the same lookups without the recurrence), and the host loop over a sample of
pairs (the ctypes cost of an empty call taken off), extrapolated to all pairs.  A sample of rows is held against the host loop
bit for bit before anything is timed.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams  # noqa: E402

SIZE = 1000


def make(name, hs, cs):
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"] = hs, cs
    return H.sketches_from_arrays(name, 1000000, 1000000, kc, np.zeros((len(hs), 21), np.uint8), SketchParams.mash(), H.FilterParams(False))


def collection(n, rng, pools, keep, prefix):
    """n sketches of SIZE hashes: a share `keep` of a pool's hashes, the rest fresh; counts ~ a depth per sketch, Poisson"""
    out = None
    for i in range(n):
        pool = pools[i % len(pools)]
        kept = pool[rng.random(len(pool)) < keep]
        fresh = rng.integers(0, 1 << 62, SIZE - min(len(kept), SIZE) + 50, dtype=np.uint64) * 2 + 1
        hs = np.unique(np.concatenate([kept, fresh]))
        hs = np.sort(rng.choice(hs, SIZE, replace=False))
        cs = np.maximum(1, rng.poisson(float(rng.integers(2, 60)), SIZE)).astype(np.uint32)
        s = make("%s%d" % (prefix, i), hs, cs)
        if out is None:
            out = s
        else:
            out.append(s)
    return out


def same_bits(a, b):
    return all((x != x and y != y) or np.float64(x).tobytes() == np.float64(y).tobytes() for x, y in zip(a, b))


def run(name, refs, queries, a, rng):
    L = H.lib()
    nq, nr = len(queries), len(refs)
    rows = H.compare_counts(refs, queries)  # warm-up: code object load, first allocations
    assert len(rows) == nq * nr
    for i in rng.integers(0, len(rows), 200).tolist():  # the judge, before anything is timed
        row = rows[i]
        want = H.compare_counts_pair(refs, int(row["reference"]), queries, int(row["query"]))
        got = tuple(row[f] for f in H.COUNTS_DTYPE.names[2:])
        assert got[:5] == want[:5] and same_bits(got[5:], want[5:]), (i, got, want)
    H.dist(queries, refs)
    walls, kernels, dist_kernels, st = [], [], [], {}
    for _ in range(a.reps):
        st = {}
        t0 = time.perf_counter()
        rows = H.compare_counts(refs, queries, stats=st)
        walls.append(time.perf_counter() - t0)
        kernels.append(st["kernel_ms"] / 1e3)
        ds = {}
        H.dist(queries, refs, stats=ds)
        dist_kernels.append(ds["kernel_ms"] / 1e3)
    # the host loop on one core over a sample of pairs
    qi = rng.integers(0, nq, a.host_sample).tolist()
    ri = rng.integers(0, nr, a.host_sample).tolist()
    m = H.CCountMoments()
    fn, rp, qp = L.finch_compare_counts_pair, refs._p, queries._p
    t0 = time.perf_counter()
    for q, r in zip(qi, ri):
        fn(rp, r, qp, q, C.byref(m))
    t_call = (time.perf_counter() - t0) / a.host_sample
    empty = L.finch_sketch_n_hashes
    t0 = time.perf_counter()
    for q, r in zip(qi, ri):
        empty(rp, r)
    t_empty = (time.perf_counter() - t0) / a.host_sample
    per_pair = max(t_call - t_empty, 1e-9)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    pairs = nq * nr
    return {"run": name, "refs": nr, "queries": nq, "pairs": pairs, "mean_common": round(float(rows["common"].mean()), 2),
            "wall_s": [round(x, 6) for x in walls], "kernel_s": [round(x, 6) for x in kernels],
            "finch_dist_kernel_s": [round(x, 6) for x in dist_kernels], "launches": st["launches"],
            "records_copied": st["records_copied"], "bytes_to_host": st["records_copied"] * 64 + 4 * st["launches"],
            "pairs_per_s_kernel": round(pairs / med(kernels)), "pairs_per_s_wall": round(pairs / med(walls)),
            "host_us_per_pair": round(per_pair * 1e6, 4), "host_ctypes_us_per_call": round(t_empty * 1e6, 4),
            "host_loop_s_extrapolated": round(per_pair * pairs, 3),
            "speedup_wall_vs_host_loop": round(per_pair * pairs / med(walls), 1),
            "kernel_over_finch_dist_kernel": round(med(kernels) / med(dist_kernels), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_counts_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    pool = lambda: np.unique(rng.integers(0, 1 << 62, SIZE * 2, dtype=np.uint64) * 2)[:SIZE]  # noqa: E731
    runs = []
    pools = [pool() for _ in range(50)]
    refs = collection(a.refs, rng, pools, 0.02, "lib")
    runs.append(run("dissimilar", refs, collection(a.queries, rng, pools, 0.02, "query"), a, rng))
    pools = [pool()]  # one genome: every pair shares most of its hashes
    refs = collection(a.refs, rng, pools, 0.98, "lib")
    runs.append(run("similar", refs, collection(a.queries, rng, pools, 0.98, "query"), a, rng))
    out = {"tool": "compare_counts_bench", "sketch_size": SIZE, "reps": a.reps, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
