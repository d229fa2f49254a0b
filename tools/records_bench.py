#!/usr/bin/env python3
"""finch_sketch_records over a synthetic multi-FASTA: one sketch per record; one JSON line per workload.

    python tools/records_bench.py [--workload a|b|c|d|e|f|all|long] [--scale 1.0] [--reps 3] [--threads 0] [--k 21] [--n 1000]
                                  [--files-subset 20000] [--skip-files] [--skip-lds0] [--stream] [--out FILE]

Workloads (records of uniform random ACGT from synth_genome_host, 70-column lines, header '>rec_<i> len=<L>', lengths uniform
from the per-record seed; `--scale` multiplies the record counts):
    a  200 000 records of 1 200 - 1 800 bases   (a 16S reference set)
    b   50 000 records of 2 - 8 kb              (plasmids, viral genomes, contigs)
    c    2 000 records of 50 kb                 (all beyond the record sketcher's bound: every record one by one)
    d      500 records of 200 kb                (`long` = c d e f: contigs, plasmids, viral and bacterial genomes; not part of `all`)
    e      200 records of 1 Mb
    f       50 records of 5 Mb
Sketched with SketchParams.mash(n, n, no_strict, k, 0) on one GPU.  Per workload: one warm-up call, then `--reps` timed calls of
    lds    H.sketch_records as it stands (records the door serves in a workgroup's LDS, many per launch)
    lds0   the same call with the option records_lds=0 (every record one by one through its own sketcher)
    stream (with --stream) the same call with the option records_stream=1: records beyond the LDS form's bound streamed through
           a workgroup each (fh_records_new_stream), many per launch; its line also carries the streamed records, the streamed
           kernel's milliseconds and launches, and folds_per_record of the first 64 records through F.RecordSketcher(stream=True)
all alternating; records/s and Gbases/s of the best call, every call's wall time, the record kernel's event-measured
milliseconds and launches, the share of records per route; both modes' sketches are compared field by field.
    files  what a user could do before finch_sketch_records: the first `--files-subset` records written one per file and sketched
           by finch_sketch_files (one warm-up, `--reps` timed calls), reported per record."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import finch_rs_amd as F  # noqa: E402
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd import sketch_schemes as S  # noqa: E402

SEED = 20261020
WORKLOADS = {"a": (200_000, 1200, 1800), "b": (50_000, 2000, 8000), "c": (2_000, 50_000, 50_000), "d": (500, 200_000, 200_000), "e": (200, 1_000_000, 1_000_000),
             "f": (50, 5_000_000, 5_000_000)}
MODE_OPTIONS = {"lds": {}, "lds0": {"records_lds": 0}, "stream": {"records_stream": 1}}


def record_bases(i, lo, hi, genome):
    """the bases of record i: a slice of `genome`, length and offset from the per-record seed"""
    u = S._splitmix64(SEED + 7919 * i)
    L = lo + (u >> 11) % (hi - lo + 1)
    off = (u >> 3) % (len(genome) - L)
    return genome[off:off + L]


def record(i, lo, hi, genome):
    """record i as FASTA text: 70-column lines"""
    b = record_bases(i, lo, hi, genome)
    L = len(b)
    rows = (L + 69) // 70
    a = np.full((rows, 71), ord("\n"), np.uint8)
    gp = np.zeros(rows * 70, np.uint8)
    gp[:L] = b
    a[:, :70] = gp.reshape(rows, 70)
    last = L - (rows - 1) * 70
    return b">rec_%07d len=%d\n" % (i, L) + a.reshape(-1)[:(rows - 1) * 71 + last].tobytes() + b"\n", L


def folds_per_record(n_records, genome, lo, hi, k, n, limit=64):
    """folds the streamed kernel makes per record, over the first `limit` records"""
    rs = F.RecordSketcher(n, k, 0, max_records=limit, stage_bytes=8 << 20, stream=True)
    try:
        res = rs.sketch_many([record_bases(i, lo, hi, genome) for i in range(min(limit, n_records))])
        taken = sum(1 for r in res if r is not None)
        return rs.folds() / taken if taken else None
    finally:
        rs.close()


def same_sketches(x, y, k):
    """every sketch of x equals that of y: name, seq_length, num_valid_kmers, hashes, counts, extra counts, k-mer bytes"""
    L = H.lib()
    if len(x) != len(y):
        return False
    for i in range(len(x)):
        n = L.finch_sketch_n_hashes(x._p, i)
        if n != L.finch_sketch_n_hashes(y._p, i) or L.finch_sketch_name(x._p, i) != L.finch_sketch_name(y._p, i):
            return False
        if (L.finch_sketch_seq_length(x._p, i), L.finch_sketch_num_valid_kmers(x._p, i)) != (L.finch_sketch_seq_length(y._p, i), L.finch_sketch_num_valid_kmers(y._p, i)):
            return False
        cols = []
        for s in (x, y):
            hs, cs, es, km = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, k), np.uint8)
            H._check(L.finch_sketch_copy(s._p, i, hs.ctypes.data, cs.ctypes.data, es.ctypes.data, km.ctypes.data))
            cols.append((hs, cs, es, km))
        if not all(np.array_equal(u, v) for u, v in zip(*cols)):
            return False
    return True


def timed(fn, reps):
    fn()  # warm-up
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append(time.perf_counter() - t0)
    return walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=sorted(WORKLOADS) + ["all", "long"])
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the record counts")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0, help="workers (0: the library's choice)")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--n", type=int, default=1000, help="kmers_to_sketch = final_size")
    ap.add_argument("--files-subset", type=int, default=20000)
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--skip-lds0", action="store_true")
    ap.add_argument("--stream", action="store_true", help="also time the call with records_stream=1")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    params = S.SketchParams.mash(a.n, a.n, True, a.k, 0)
    genome = S.synth_genome_host(64 << 20, SEED)
    for name in ({"all": ["a", "b", "c"], "long": ["c", "d", "e", "f"]}.get(a.workload, [a.workload])):
        count, lo, hi = WORKLOADS[name]
        count = max(1, int(count * a.scale))
        recs = [record(i, lo, hi, genome) for i in range(count)]
        text = b"".join(r for r, _ in recs)
        bases = sum(L for _, L in recs)
        out = {"workload": name, "records": count, "bases": bases, "k": a.k, "n": a.n, "threads": a.threads}
        state = {}

        def call(mode):
            for opt in ("records_lds", "records_stream"):
                F.set_option(opt, MODE_OPTIONS[mode].get(opt))
            st = {}
            state["res_" + mode] = H.sketch_records(text, params, n_threads=a.threads, stats=st)
            state["st_" + mode] = st
            state["ss_" + mode] = H.records_stream_stats()

        modes = ["lds"] + ([] if a.skip_lds0 else ["lds0"]) + (["stream"] if a.stream else [])
        walls = {m: [] for m in modes}
        for m in modes:
            call(m)  # warm-up
        for _ in range(a.reps):
            for m in modes:
                t0 = time.perf_counter()
                call(m)
                walls[m].append(time.perf_counter() - t0)
        for opt in ("records_lds", "records_stream"):
            F.set_option(opt, None)
        for m in modes:
            best, st = min(walls[m]), state["st_" + m]
            out[m] = {"records_per_s": count / best, "gbases_per_s": bases / best / 1e9, "walls_s": walls[m], "kernel_ms": st["kernel_ms"],
                      "launches": st["launches"], "share_in_lds": st["in_lds"] / count, "share_one_by_one": st["one_by_one"] / count}
        if "lds0" in modes:
            out["same_sketches"] = same_sketches(state["res_lds"], state["res_lds0"], a.k)
            out["lds_over_lds0"] = min(walls["lds0"]) / min(walls["lds"])
        if "stream" in modes:
            out["stream"].update(streamed=state["st_stream"]["streamed"], stream_kernel_ms=state["ss_stream"][1], stream_launches=state["ss_stream"][2],
                                 folds_per_record=folds_per_record(count, genome, lo, hi, a.k, a.n))
            out["stream_same_sketches"] = same_sketches(state["res_stream"], state["res_lds"], a.k)
            out["stream_over_lds"] = min(walls["lds"]) / min(walls["stream"])
        state.clear()
        if not a.skip_files:
            n_files = min(a.files_subset, count)
            d = tempfile.mkdtemp(prefix="finch_records_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
            try:
                paths = []
                for i in range(n_files):
                    p = os.path.join(d, "r%07d.fa" % i)
                    with open(p, "wb") as f:
                        f.write(recs[i][0])
                    paths.append(p)
                fw = timed(lambda: H.sketch_files(paths, params, H.FilterParams(False), n_threads=a.threads), a.reps)
                out["files"] = {"files": n_files, "records_per_s": n_files / min(fw), "gbases_per_s": sum(L for _, L in recs[:n_files]) / min(fw) / 1e9, "walls_s": fw}
                if "lds" in out:
                    out["lds_over_files"] = out["lds"]["records_per_s"] / out["files"]["records_per_s"]
            finally:
                shutil.rmtree(d, ignore_errors=True)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
