#!/usr/bin/env python3
"""finch_sketch_files at Mash sizes above 3000 over a directory of genomes, with and without the many-per-launch groups; one JSON line.

    python tools/batch_large_bench.py [--files 1000] [--distinct 250] [--n 10000] [--k 21] [--reps 3] [--threads 16] [--dir DIR]
                                      [--only batch|one] [--want W] [--group-files G] [--out FILE]

Input: bench.py's configs[4] generator (synth_fasta_file: log-uniform 1-10 Mb genomes, 70-column lines); `--distinct` files
are written to a temporary directory and the list of `--files` names cycles over them, so the page cache feeds every pass.
Sketched with SketchParams.mash(n, n, False, k, 0).  Per mode -- option file_batch=0 (every file through a sketcher of its own:
what the library did above 3000 hashes before fh_batch_new_large) and the default -- one warm-up pass, then `--reps` timed
passes, the two modes alternating (one, batch, one, batch, ...) so that what else runs on the machine weighs on both alike:
files/s of the best pass, every pass's wall time and their spread ((max - min) / min), files taken / not taken by the groups, the
sketch kernels' time (HIP events, summed over the workers) and the launches behind it.  Both modes' sketches are compared row for
row.  `--want` / `--group-files` set the options batch_large_want / batch_large_files for an A/B.  With FH_LIB naming an older
build of the library, symbols it does not have are left unbound: such a build is measured the same way (its `batch` mode is
whatever it did for those parameters -- one by one).

The epilogue's time comes from a trace of its own (never in the timed passes):
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/batch_large_bench.py --files 256 --distinct 256 --reps 1 --only batch"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("FH_LIB"):  # an older build of the library: what it does not export cannot be bound, and is not called here
    import ctypes  # noqa: E402

    from finch_rs_amd import _lib  # noqa: E402
    _old = ctypes.CDLL(os.environ["FH_LIB"])
    for _name in [n for n in _lib.SYMBOLS if not hasattr(_old, n)]:
        _lib.SYMBOLS.pop(_name)
import finch_rs_amd as F  # noqa: E402
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd import sketch_schemes as S  # noqa: E402

SEED = 20250620


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--distinct", type=int, default=250)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="workers of finch_sketch_files (0: the library's choice)")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory, removed afterwards)")
    ap.add_argument("--only", choices=["batch", "one"], default=None)
    ap.add_argument("--n", type=int, default=10000, help="kmers_to_sketch = final_size")
    ap.add_argument("--want", default=None, help="option batch_large_want")
    ap.add_argument("--group-files", default=None, help="option batch_large_files")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--k", type=int, default=21, help="kmer_length")
    a = ap.parse_args()
    distinct = min(a.distinct, a.files)
    d = a.dir or tempfile.mkdtemp(prefix="finch_batch_large_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        names = []
        for i in range(distinct):
            p = os.path.join(d, "g%05d.fa" % i)
            if not os.path.exists(p):
                with open(p, "wb") as f:
                    f.write(S.synth_fasta_file(i, SEED))
            names.append(p)
        paths = [names[i % distinct] for i in range(a.files)]
        nbytes = sum(os.path.getsize(names[i % distinct]) for i in range(a.files))
        params, said = S.SketchParams.mash(a.n, a.n, False, a.k, 0), "mash(%d, %d, False, %d, 0)" % (a.n, a.n, a.k)
        opts = {}
        if F.get_option("batch_large_want") is not None or a.want or a.group_files:  # (an older library knows neither option)
            opts = dict(batch_large_want=a.want, batch_large_files=a.group_files)
        out = {"files": a.files, "distinct": distinct, "text_gbytes": round(nbytes / 1e9, 3), "params": said, "threads": a.threads,
               "lib": os.environ.get("FH_LIB") or "built", "options": {k: v for k, v in opts.items() if v}}
        sketches = {}
        modes = [m for m in ("one", "batch") if not a.only or a.only == m]
        for mode in modes:
            F.debug_set(file_batch="0" if mode == "one" else None, **opts)
            H.sketch_files(names, params, H.FilterParams(None), n_threads=a.threads)  # warm-up: handles, page cache
        bests, last = {}, {}
        for rep in range(a.reps):
            for mode in modes:
                F.debug_set(file_batch="0" if mode == "one" else None, **opts)
                t0, n0 = H.debug_file_batch()
                H.debug_kernel_times(1)
                w0 = time.perf_counter()
                last[mode] = H.sketch_files(paths, params, H.FilterParams(None), n_threads=a.threads)
                wall = time.perf_counter() - w0
                ms, launches, positions = H.debug_kernel_times(0)
                t1, n1 = H.debug_file_batch()
                if mode not in bests or wall < bests[mode][0]:
                    bests[mode] = (wall, ms, launches, positions, t1 - t0, n1 - n0)
                out.setdefault(mode + "_walls_s", []).append(round(wall, 4))
        for mode in modes:
            res = last[mode]
            wall, ms, launches, positions, taken, not_taken = bests[mode]
            rows = [len(res.sketch(i).arrays[0]) for i in range(distinct)]
            out[mode] = {"files_per_s": round(a.files / wall, 1), "wall_s": round(wall, 4), "text_gbytes_per_s": round(nbytes / wall / 1e9, 2),
                         "taken": taken, "not_taken": not_taken, "sketch_kernel_ms": round(ms, 2), "sketch_kernel_launches": launches,
                         "sketch_kernel_ms_per_launch": round(ms / launches, 4) if launches else None,
                         "taken_share": round(taken / a.files, 4),
                         "spread": round((max(out[mode + "_walls_s"]) - min(out[mode + "_walls_s"])) / min(out[mode + "_walls_s"]), 4),
                         "rows_min_median_max": [min(rows), sorted(rows)[len(rows) // 2], max(rows)]}
            sketches[mode] = [(res.sketch(i).arrays[0].tobytes(), res.sketch(i).arrays[1].tobytes()) for i in range(distinct)]
        F.debug_set(file_batch=None, **{k: None for k in opts})
        if len(sketches) == 2:
            out["sketches_equal"] = sketches["one"] == sketches["batch"]
            out["speedup"] = round(out["batch"]["files_per_s"] / out["one"]["files_per_s"], 3)
        print(json.dumps(out), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(out) + "\n")
        if len(sketches) == 2 and not out["sketches_equal"]:
            sys.exit(1)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
