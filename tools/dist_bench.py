#!/usr/bin/env python3
"""finch_dist (`finch dist --pairwise`) on N synthetic Mash-1000 sketches on one GPU; prints one JSON line.

    python tools/dist_bench.py --n 10000 [--reps 3] [--max-distance 1.0] [--host-sample 20000]

Sketches: `groups` pools of 1000 hashes; a sketch keeps a fraction f ~ U(0,1)^2 of its pool and fills up with fresh hashes, so
Jaccard spans 0..1 inside a group and is 0 across groups.  Timed: the kernels (HIP events, summed over the launches) and the
whole call (wall clock: upload, kernels, host epilogue, rows).  Host baseline: finch_distance -- the reference's loop body --
per pair on one core, over a random sample of pairs, the ctypes call cost of an empty call taken off, extrapolated to all pairs.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams  # noqa: E402


def sketches(n, groups, seed):
    rng = np.random.default_rng(seed)
    size = 1000
    bases = [np.unique(rng.integers(0, 1 << 63, size * 3, dtype=np.uint64) * 2)[:size] for _ in range(groups)]
    out = None
    km = np.zeros((size, 21), np.uint8)
    for i in range(n):
        base = bases[i % groups]
        kept = base[rng.random(size) < rng.random() ** 2]
        fresh = rng.integers(0, 1 << 63, size - len(kept) + 50, dtype=np.uint64) * 2 + 1
        hs = np.unique(np.concatenate([kept, fresh]))[:size]
        kc = np.zeros(size, KC_DTYPE)
        kc["hash"], kc["count"] = hs, 1
        s = H.sketches_from_arrays("s%d" % i, 1000000, 1000000, kc, km, SketchParams.mash(), H.FilterParams(False))
        if out is None:
            out = s
        else:
            out.append(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-distance", type=float, default=1.0)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    L = H.lib()
    sk = sketches(a.n, a.groups, a.seed)
    pairs = a.n * a.n
    lookups = pairs * 1000  # every reference hash is looked up in its query once
    dev = (C.c_int * 1)(0)

    def one():
        out = C.c_void_p()
        t0 = time.perf_counter()
        rc = L.finch_dist(sk._p, sk._p, 0, a.max_distance, dev, 1, C.byref(out))
        t1 = time.perf_counter()
        if rc != 0:
            raise RuntimeError(L.finch_last_error().decode())
        ms, nl = C.c_double(), C.c_uint64()
        L.finch_dist_stats(out, C.byref(ms), C.byref(nl))
        rows = L.finch_dist_len(out)
        t2 = time.perf_counter()
        L.finch_dist_free(out)
        return t1 - t0, ms.value / 1e3, nl.value, rows, time.perf_counter() - t2

    one()  # warm-up: code object load, first allocations
    runs = [one() for _ in range(a.reps)]
    wall = sorted(r[0] for r in runs)[len(runs) // 2]
    kern = sorted(r[1] for r in runs)[len(runs) // 2]

    # host baseline: finch_distance per pair on this core
    rng = np.random.default_rng(a.seed + 1)
    qi = rng.integers(0, a.n, a.host_sample).tolist()
    ri = rng.integers(0, a.n, a.host_sample).tolist()
    d = H.CDistance()
    fn, p = L.finch_distance, sk._p
    t0 = time.perf_counter()
    for q, r in zip(qi, ri):
        fn(p, q, p, r, 0, C.byref(d))
    t_call = (time.perf_counter() - t0) / a.host_sample
    empty = L.finch_sketch_n_hashes
    t0 = time.perf_counter()
    for q, r in zip(qi, ri):
        empty(p, q)
    t_empty = (time.perf_counter() - t0) / a.host_sample
    per_pair = max(t_call - t_empty, 1e-9)
    print(json.dumps({
        "n": a.n, "pairs": pairs, "rows": runs[0][3], "launches": runs[0][2], "max_distance": a.max_distance,
        "kernel_s": round(kern, 6), "wall_s": round(wall, 6), "free_s": round(runs[0][4], 6),
        "pairs_per_s_kernel": round(pairs / kern), "pairs_per_s_wall": round(pairs / wall),
        "lookups_per_s_kernel": round(lookups / kern),
        "host_us_per_pair": round(per_pair * 1e6, 4), "host_ctypes_us_per_call": round(t_empty * 1e6, 4),
        "host_loop_s_extrapolated": round(per_pair * pairs, 2), "speedup_wall_vs_host_loop": round(per_pair * pairs / wall, 1),
    }))


if __name__ == "__main__":
    main()
