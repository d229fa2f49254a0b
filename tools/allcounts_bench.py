#!/usr/bin/env python3
"""The AllCounts sketcher (FH_KIND_ALL_COUNTS) on one GPU over a device-resident synthetic read block; one JSON line per k.

    python tools/allcounts_bench.py [--gbases 10] [--ks 4,8,12,16] [--reps 3] [--baseline-mb 64]

Input: bench.py's configs[3] generator (a 5 Mb genome, 150-base reads with 1 % substitutions and 0.05 % N, one breaker
byte per read), made on the device.  Timed per k: the counting kernel (HIP events around every launch, fh_kernel_time) and
the whole call (wall clock: fh_reset, fh_push_device, fh_finish -- fold, mark, scan, compact, rows to the host -- and
fh_copy_out_records with the k-mer bytes).  Baseline (--baseline-mb > 0): tools/allcounts_baseline.cpp, a plain C++
restatement of counts.rs's loop (normalize + bit_kmers + saturating add) on ONE core over the first MB of the same reads,
labelled as such.
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
from finch_rs_amd import sketch_schemes as S  # noqa: E402
from finch_rs_amd.sketch_schemes import SketchParams  # noqa: E402

SEED, GENOME_LEN, READ_LEN, SUB_PPM, N_PPM = 20250620, 5_000_000, 150, 10_000, 500


def baseline(k, mb):
    exe = os.path.join(tempfile.gettempdir(), "allcounts_baseline_%d" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "allcounts_baseline.cpp")])
    g = S.synth_genome_host(GENOME_LEN, SEED)
    n_reads = int(mb * 1e6) // (READ_LEN + 1)
    reads = S.synth_reads_host(g, 0, n_reads, READ_LEN, SEED, SUB_PPM, N_PPM)
    with tempfile.NamedTemporaryFile(delete=False) as f:
        f.write(reads.tobytes())
    try:
        out = subprocess.check_output([exe, f.name, str(k)], text=True)
    finally:
        os.unlink(f.name)
        os.unlink(exe)
    secs, windows = out.split()
    return float(secs), int(windows), reads.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=10.0)
    ap.add_argument("--ks", default="4,8,12,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-mb", type=float, default=64.0)
    a = ap.parse_args()
    n_reads = int(a.gbases * 1e9) // READ_LEN
    nbytes = n_reads * (READ_LEN + 1)
    dg, dr = S.DeviceBuffer(GENOME_LEN + 64), S.DeviceBuffer(nbytes + 64)
    S.synth_genome_device(dg, GENOME_LEN, SEED)
    S.synth_reads_device(dr, dg, GENOME_LEN, 0, n_reads, READ_LEN, SEED, SUB_PPM, N_PPM)
    for k in [int(x) for x in a.ks.split(",")]:
        sk = SketchParams.all_counts(k).create_sketcher(device=0)
        best = None
        for rep in range(a.reps + 1):  # (the first pass warms up: it is not reported)
            sk.reset()
            sk.set_profiling(True)
            t0 = time.perf_counter()
            sk.push_device(dr.ptr, nbytes)
            n, nvk = sk.finish()
            kc, km, _ = sk.to_arrays()
            wall = time.perf_counter() - t0
            ms, launches, positions = sk.kernel_time()
            if rep and (best is None or wall < best[0]):
                best = (wall, ms, launches, positions, n, nvk)
        wall, ms, launches, positions, n, nvk = best
        line = {"k": k, "gbases": round(nbytes / 1e9, 3), "windows_counted": nvk, "rows": n, "kernel_ms": round(ms, 3),
                "kernel_launches": launches, "kernel_gbases_per_s": round(positions / ms / 1e6, 1),
                "whole_call_s": round(wall, 4), "whole_call_gbases_per_s": round(nbytes / wall / 1e9, 1)}
        if a.baseline_mb > 0:
            secs, windows, nb = baseline(k, a.baseline_mb)
            line["baseline_one_core_cpp"] = {"what": "tools/allcounts_baseline.cpp: counts.rs's loop restated in C++, one core",
                                             "mbytes": round(nb / 1e6, 1), "seconds": round(secs, 4),
                                             "gbases_per_s": round(nb / secs / 1e9, 3)}
        print(json.dumps(line), flush=True)
        sk.close()
    dr.free()
    dg.free()


if __name__ == "__main__":
    main()
