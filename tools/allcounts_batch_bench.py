#!/usr/bin/env python3
"""finch_sketch_files with AllCounts parameters (`finch sketch -s none`) over a directory of genomes: the groups of
fh_batch_new_counts against a sketcher per file.

    python tools/allcounts_batch_bench.py [--files 1000] [--distinct 200] [--reps 5] [--threads 16] [--ks 4,7]
                                          [--parent-lib LIB] [--no-trace] [--out-dir profiles]

Input: bench.py's `--workload c5` generator (synth_fasta_file: log-uniform 1-10 Mb genomes, 70-column lines); `--distinct`
files are written to a temporary directory and the list of `--files` names cycles over them, so the page cache feeds every
pass.  Per k: one warm-up pass per mode, then `--reps` rounds, each ONE pass with option file_batch=0 (every file through a
sketcher of its own) and ONE pass with the groups, alternating, on the same library in the same process; every pass's wall
time is kept, files/s is quoted from the median pass, the spread is (max - min) / median.  The two modes' sketches are
compared row for row.

--parent-lib LIB: the file_batch=0 passes once more in a child process on another build of the library (FH_LIB; the parent
commit's, which has no groups for AllCounts whatever the option says): that a sketcher per file costs the same there.

Unless --no-trace: a child run of the groups alone (256 genomes, one timed pass per k) under
`rocprofv3 --kernel-trace --stats`, never part of a timed pass; the rows of the two batch kernels go to
<out-dir>/allcounts_batch_kernel_stats.txt.  The result goes to <out-dir>/allcounts_batch_bench.json and to stdout."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from finch_rs_amd import _lib  # noqa: E402

if os.environ.get("FH_LIB"):  # an older build of the library has no fh_batch_new_counts to bind: it is measured without it
    import ctypes
    if not hasattr(ctypes.CDLL(os.environ["FH_LIB"]), "fh_batch_new_counts"):
        _lib.SYMBOLS.pop("fh_batch_new_counts", None)
import finch_rs_amd as F  # noqa: E402
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd import sketch_schemes as S  # noqa: E402

SEED = 20250620


def write_files(d, distinct):
    names = []
    for i in range(distinct):
        p = os.path.join(d, "g%05d.fa" % i)
        if not os.path.exists(p):
            with open(p, "wb") as f:
                f.write(S.synth_fasta_file(i, SEED))
        names.append(p)
    return names


def one_pass(paths, params, threads, groups):
    F.debug_set(file_batch=None if groups else "0")
    t0, n0 = H.debug_file_batch()
    w0 = time.perf_counter()
    res = H.sketch_files(paths, params, H.FilterParams(None), n_threads=threads)
    wall = time.perf_counter() - w0
    t1, n1 = H.debug_file_batch()
    return wall, t1 - t0, n1 - n0, res


def summary(walls, n_files):
    med = statistics.median(walls)
    return {"walls_s": [round(w, 4) for w in walls], "median_s": round(med, 4), "files_per_s": round(n_files / med, 1),
            "spread": round((max(walls) - min(walls)) / med, 3)}


def measure(a, names, paths, modes):
    out = {}
    for k in a.ks:
        params = S.SketchParams.all_counts(k)
        r = {}
        for m in modes:  # warm-up: handles, page cache
            one_pass(names, params, a.threads, m == "groups")
        walls = {m: [] for m in modes}
        counters = {m: [0, 0] for m in modes}
        last = {}
        for _ in range(a.reps):
            for m in modes:
                wall, taken, not_taken, res = one_pass(paths, params, a.threads, m == "groups")
                walls[m].append(wall)
                counters[m][0] += taken
                counters[m][1] += not_taken
                last[m] = res
        for m in modes:
            r[m] = summary(walls[m], len(paths))
            r[m]["taken"], r[m]["not_taken"] = counters[m]
        if len(modes) == 2:
            same = True
            for i in range(len(names)):
                x, y = last["one"].sketch(i), last["groups"].sketch(i)
                same = same and x.arrays[0].tobytes() == y.arrays[0].tobytes() and x.arrays[1].tobytes() == y.arrays[1].tobytes() and \
                    (x.seq_length, x.num_valid_kmers) == (y.seq_length, y.num_valid_kmers)
            r["sketches_equal"] = same
            r["speedup"] = round(r["groups"]["files_per_s"] / r["one"]["files_per_s"], 3)
        r["rows_of_file_0"] = len(last[modes[-1]].sketch(0).arrays[0])
        out["k%d" % k] = r
    F.debug_set(file_batch=None)
    return out


def child(args, env_extra=None, prefix=()):
    env = dict(os.environ)
    env.update(env_extra or {})
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        return {"failed": p.returncode, "stderr": p.stderr[-2000:]}
    return json.loads(lines[-1])


def kernel_table(trace_dir, dst, cmdline):
    rows, header = [], None
    for fn in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(fn, newline="") as f:
            rd = csv.reader(f)
            header = next(rd)
            rows += [r for r in rd if any("k_ac_batch" in c for c in r)]
    with open(dst, "w") as f:
        f.write("# %s\n# the two kernels of an AllCounts batch over the whole run (per k: a warm-up pass and one timed pass of 256 genomes of\n"
                "# 1-10 Mb, 16 workers); durations in ns\n" % cmdline)
        if header:
            f.write("# columns: " + ", ".join(header) + "\n")
        for r in rows:
            f.write("  ".join(r) + "\n")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--distinct", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--ks", default="4,7")
    ap.add_argument("--dir", default=None, help="where the files are (written if missing; default: a temporary directory, removed afterwards)")
    ap.add_argument("--only", choices=["groups", "one"], default=None, help="one mode, one JSON line, nothing written (the child runs)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    a.ks = [int(x) for x in a.ks.split(",")]
    distinct = min(a.distinct, a.files)
    d = a.dir or tempfile.mkdtemp(prefix="finch_allcounts_batch_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        names = write_files(d, distinct)
        paths = [names[i % distinct] for i in range(a.files)]
        nbytes = sum(os.path.getsize(p) for p in paths)
        if a.only:
            print(json.dumps(measure(a, names, paths, [a.only])), flush=True)
            return
        out = {"files": a.files, "distinct": distinct, "text_gbytes": round(nbytes / 1e9, 3), "threads": a.threads, "reps": a.reps,
               "params": ["all_counts(%d)" % k for k in a.ks],
               "how": "per k: a warm-up pass per mode, then reps rounds of one file_batch=0 pass and one pass with the groups, alternating; "
                      "files/s from the median pass, spread = (max - min) / median"}
        common = ["--files", str(a.files), "--distinct", str(distinct), "--reps", str(a.reps), "--threads", str(a.threads),
                  "--ks", ",".join(map(str, a.ks)), "--dir", d]
        # the children first: this process has not touched the GPU yet
        if a.parent_lib:
            out["parent_library_one_by_one"] = child(common + ["--only", "one"], {"FH_LIB": os.path.abspath(a.parent_lib)})
        if not a.no_trace and shutil.which("rocprofv3"):
            td = tempfile.mkdtemp(prefix="finch_allcounts_trace_")
            try:
                targs = ["--files", "256", "--distinct", str(min(256, distinct)), "--reps", "1", "--threads", str(a.threads),
                         "--ks", ",".join(map(str, a.ks)), "--dir", d, "--only", "groups"]
                prefix = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--"]
                out["trace_run"] = child(targs, None, prefix)
                os.makedirs(a.out_dir, exist_ok=True)
                n = kernel_table(td, os.path.join(a.out_dir, "allcounts_batch_kernel_stats.txt"),
                                 "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/allcounts_batch_bench.py " + " ".join(targs[:-4] + targs[-2:]))
                out["trace_kernel_rows"] = n
            finally:
                shutil.rmtree(td, ignore_errors=True)
        out.update(measure(a, names, paths, ["one", "groups"]))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "allcounts_batch_bench.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out), flush=True)
        if not all(out["k%d" % k].get("sketches_equal") for k in a.ks):
            sys.exit(1)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
