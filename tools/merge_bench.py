#!/usr/bin/env python3
"""finch_merge_groups on one GPU next to the loop it stands for, finch_merge_pair folded on one core; writes
profiles/merge_bench.json and prints it as one JSON line.

    python tools/merge_bench.py [--mash-sketches 20000] [--scaled-sketches 2000] [--reps 3] [--host-groups 100]

Two synthetic libraries:
  * "mash": `--mash-sketches` Mash sketches of 1000 hashes in groups of 20 (the strains of a species: every member keeps most of
    its group's pool of hashes), merged with size = 1000;
  * "scaled": `--scaled-sketches` Scaled sketches of about 5000 hashes (scale 0.001) in groups of 10, merged with no size, so the
    accumulator grows with every step.
Per library: the whole call (wall clock), and inside it the upload of the sketches, the kernels (HIP events), the copies back and
the k-mer gather on the host, each summed over the launches; the host fold over a sample of groups, extrapolated to all groups.
A sample of groups is held against the host fold field by field before anything is timed.
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

K = 21


def make(name, hs, cs, params):
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"] = hs, cs
    km = np.full((len(hs), K), 65, np.uint8)
    return H.sketches_from_arrays(name, 1000000, 1000000, kc, km, params, H.FilterParams(False))


def library(n, group, length, keep, params, top, rng):
    """n sketches in groups of `group`: each keeps a share `keep` of its group's pool of `length` hashes below `top`, the rest fresh"""
    out, pool = None, None
    for i in range(n):
        if i % group == 0:
            pool = np.unique(rng.integers(0, top, length, dtype=np.uint64))
        kept = pool[rng.random(len(pool)) < keep]
        fresh = rng.integers(0, top, max(length - len(kept), 0), dtype=np.uint64)
        hs = np.unique(np.concatenate([kept, fresh]))[:length]
        cs = np.maximum(1, rng.poisson(20.0, len(hs))).astype(np.uint32)
        s = make("s%d" % i, hs, cs, params)
        if out is None:
            out = s
        else:
            out.append(s)
    return out


def arrays(sk, i):
    L = H.lib()
    n = L.finch_sketch_n_hashes(sk._p, i)
    hs, cs, es, km = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, K), np.uint8)
    H._check(L.finch_sketch_copy(sk._p, i, hs.ctypes.data, cs.ctypes.data, es.ctypes.data, km.ctypes.data))
    return hs, cs, es, km, L.finch_sketch_seq_length(sk._p, i), L.finch_sketch_name(sk._p, i)


def host_fold(sk, group, size):
    acc = H.select(sk, [group[0]])
    for i in group[1:]:
        acc = H.merge_pair(acc, 0, sk, i, size)
    return acc


def run(name, sk, groups, size, a, rng):
    out = H.merge(sk, groups, size)  # warm-up: code object load, first allocations
    for g in rng.integers(0, len(groups), min(20, len(groups))).tolist():  # the judge, before anything is timed
        got, want = arrays(out, g), arrays(host_fold(sk, groups[g], size), 0)
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4])) and got[4:] == want[4:], (name, g)
    walls, stats = [], []
    for _ in range(a.reps):
        st = {}
        t0 = time.perf_counter()
        out = H.merge(sk, groups, size, stats=st)
        walls.append(time.perf_counter() - t0)
        stats.append(st)
    sample = rng.choice(len(groups), min(a.host_groups, len(groups)), replace=False).tolist()
    t0 = time.perf_counter()
    for g in sample:
        host_fold(sk, groups[g], size)
    per_group = (time.perf_counter() - t0) / len(sample)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    L = H.lib()
    return {"run": name, "sketches": len(sk), "groups": len(groups), "members_per_group": len(groups[0]), "size": size,
            "input_records": int(sum(L.finch_sketch_n_hashes(sk._p, i) for i in range(len(sk)))),
            "result_records": stats[-1]["records_copied"], "launches": stats[-1]["launches"],
            "wall_s": [round(x, 6) for x in walls],
            "upload_s": [round(s["upload_ms"] / 1e3, 6) for s in stats], "kernel_s": [round(s["kernel_ms"] / 1e3, 6) for s in stats],
            "copy_back_s": [round(s["copy_ms"] / 1e3, 6) for s in stats], "gather_s": [round(s["gather_ms"] / 1e3, 6) for s in stats],
            "host_fold_ms_per_group": round(per_group * 1e3, 4), "host_fold_s_extrapolated": round(per_group * len(groups), 4),
            "host_fold_over_wall": round(per_group * len(groups) / med(walls), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mash-sketches", type=int, default=20000)
    ap.add_argument("--scaled-sketches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-groups", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    runs = []
    sk = library(a.mash_sketches, 20, 1000, 0.9, SketchParams.mash(kmer_length=K), 1 << 63, rng)
    runs.append(run("mash", sk, [list(range(g, min(g + 20, len(sk)))) for g in range(0, len(sk), 20)], 1000, a, rng))
    del sk
    scale = 0.001
    sk = library(a.scaled_sketches, 10, 5000, 0.9, SketchParams.scaled(1000, K, scale), (2 ** 64 - 1) // 1000, rng)
    runs.append(run("scaled", sk, [list(range(g, min(g + 10, len(sk)))) for g in range(0, len(sk), 10)], None, a, rng))
    out = {"tool": "merge_bench", "reps": a.reps, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
