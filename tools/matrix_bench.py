#!/usr/bin/env python3
"""finch_minmer_matrix (the count matrix of distance.rs:345-364) on one GPU next to the reference's loop on one core.

    python tools/matrix_bench.py [--shapes 1000x10000x1000,100000x4000x1000,2000000x1000x1000] [--reps 3] [--no-baseline] [--out profiles/matrix_bench.json]

A shape is RxSxN: a reference sketch of R hashes against S sketches of N hashes.  Input: S "genome" sketches of N random
u64 each (counts 1..40); the reference takes a third of its hashes from the genomes' (spread over all of them) and the rest
from nowhere, a metagenome that holds part of every genome.  Per shape: the whole call (wall clock: checks, the reference's
upload, per chunk the sketches up, the kernel, the rows back into pinned memory and from there into the numpy array; best of
--reps after a warm-up call), the kernels' time (HIP events, summed over the launches), the launches, and the bytes that
cross the link each way.  Baseline: tools/matrix_baseline.cpp, the loop restated in C++ on ONE core over the same input
(`calloc` for Array2::zeros), labelled as such; its count of matching cells must equal the matrix's nonzero cells.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams  # noqa: E402


def distinct(rng, n):
    p = np.zeros(0, np.uint64)
    while len(p) < n:
        p = np.unique(np.concatenate([p, rng.integers(0, (1 << 64) - 1, n - len(p), dtype=np.uint64, endpoint=True)]))
    return p


def one_sketch(name, hashes, counts):
    kc = np.zeros(len(hashes), KC_DTYPE)
    kc["hash"], kc["count"] = hashes, counts
    return H.sketches_from_arrays(name, 0, len(hashes), kc, np.zeros((0, 21), np.uint8), SketchParams.mash(no_strict=True),
                                  H.FilterParams(False))


def make(R, S, N, seed):
    rng = np.random.default_rng(seed)
    genomes = [distinct(rng, N) for _ in range(S)]
    every = np.unique(np.concatenate(genomes))
    shared = rng.choice(every, min(R // 3, len(every)), replace=False)
    strangers = rng.choice(np.setdiff1d(distinct(rng, R), every), R - len(shared), replace=False)
    ref = np.sort(np.concatenate([shared, strangers]))
    counts = [rng.integers(1, 41, N, dtype=np.uint32) for _ in range(S)]
    return ref, genomes, counts


def baseline(ref, genomes, counts):
    exe = os.path.join(tempfile.gettempdir(), "matrix_baseline_%d" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "matrix_baseline.cpp")])
    off = np.zeros(len(genomes) + 1, np.uint64)
    off[1:] = np.cumsum([len(g) for g in genomes])
    with tempfile.NamedTemporaryFile(delete=False) as f:
        for a in (np.array([len(ref), len(genomes)], np.uint64), ref, off, np.concatenate(genomes), np.concatenate(counts)):
            f.write(a.tobytes())
    try:
        secs, hits, _ = subprocess.check_output([exe, f.name], text=True).split()
    finally:
        os.unlink(f.name)
        os.unlink(exe)
    return float(secs), int(hits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x10000x1000,100000x4000x1000,2000000x1000x1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_bench.json"))
    a = ap.parse_args()
    lines = []
    for n_shape, shape in enumerate(a.shapes.split(",")):
        R, S, N = (int(x) for x in shape.split("x"))
        ref, genomes, counts = make(R, S, N, 20260000 + n_shape)
        refs = one_sketch("metagenome", ref, np.ones(R, np.uint32))
        sk = one_sketch("g0", genomes[0], counts[0])
        for i in range(1, S):
            sk.append(one_sketch("g%d" % i, genomes[i], counts[i]))
        best = None
        for rep in range(a.reps + 1):  # (the first call warms up: it is not reported)
            stats = {}
            t0 = time.perf_counter()
            m = H.minmer_matrix(refs, 0, sk, stats=stats)
            wall = time.perf_counter() - t0
            if rep and (best is None or wall < best[0]):
                best = (wall, stats["kernel_ms"], stats["launches"])
        wall, ms, launches = best
        cells, hits = S * R, int(np.count_nonzero(m))
        up, down = 8 * R + S * N * 12 + 8 * (S + launches), 4 * cells
        line = {"R": R, "S": S, "hashes_per_sketch": N, "cells": cells, "matching_cells": hits, "whole_call_s": round(wall, 4),
                "kernel_ms": round(ms, 3), "launches": launches, "bytes_to_device": up, "bytes_to_host": down,
                "whole_call_gcells_per_s": round(cells / wall / 1e9, 3), "kernel_gcells_per_s": round(cells / ms / 1e6, 2),
                "kernel_write_GBps": round(down / ms / 1e6, 1), "whole_call_link_GBps": round((up + down) / wall / 1e9, 2)}
        del m
        if not a.no_baseline:
            secs, bhits = baseline(ref, genomes, counts)
            assert bhits == hits, (bhits, hits)
            line["baseline_one_core_cpp"] = {"what": "tools/matrix_baseline.cpp: distance.rs:345-364's loop restated in C++, one core, calloc for the zeros",
                                             "seconds": round(secs, 4), "matching_cells": bhits}
        print(json.dumps(line), flush=True)
        lines.append(line)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/matrix_bench.py", "shapes": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
