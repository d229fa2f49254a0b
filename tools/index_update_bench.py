#!/usr/bin/env python3
"""finch_index_add / finch_index_keep next to the rebuild they replace, on one GPU: the same library, the same process; prints
one JSON line per configuration and writes the measurement record.

    python tools/index_update_bench.py [--refs 100000] [--adds 1,1000,10000] [--drops 1,0.1,0.5] [--queries 20] [--reps 3]
                                       [--write docs/MEASUREMENTS_index_update.md]

Library: synthetic Mash-1000 sketches as tools/dist_bench.py makes them (`--groups` pools of related sketches), counts
attached.  Per configuration the tool FIRST asserts that a search and a compare_counts on the updated index give the bytes of a
fresh index over the same sketches (queries: tools/index_bench.py's); then, alternating, `--reps` times each:
  * the update -- finch_index_add of `--adds` sketches, or finch_index_keep dropping `--drops` sketches (a number >= 1: that
    many; below 1: that share, evenly spread) --, the whole call (wall clock) and its kernels (HIP events);
  * the rebuild a caller had to make before: finch_index_free + finch_index_new + finch_index_attach_counts over the
    resulting library (wall clock; the build's kernels).
Between two timed adds the index is put back by a keep of the first `--refs` references; between two timed keeps by a rebuild;
neither is timed.  Reported: the medians, and the update kernels' bytes per second -- 24 bytes per posting of the updated index,
12 read and 12 written, over ALL the update's kernels, the added postings' sort included: a lower bound on the merge kernel's
rate -- next to the streaming-read rate of this GPU's HBM as bench.py measures it.  `--write PATH` puts a table of the medians
and the raw lines between the two marker lines of PATH (the file is made if it is not there; what stands outside the markers
stays).
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
from finch_rs_amd import sketch_schemes as S  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402
from tools.index_bench import make_queries  # noqa: E402
from tools.index_gather_bench import fmt_s, med  # noqa: E402

BEGIN, END = "<!-- tools/index_update_bench.py: begin -->", "<!-- tools/index_update_bench.py: end -->"
MIN_CONTAINMENT, MIN_COMMON = 0.05, 20


def c_add(ix, more):
    ms = C.c_double()
    t0 = time.perf_counter()
    H._check(H.lib().finch_index_add(ix._handle(), more._p, C.byref(ms)))
    return time.perf_counter() - t0, ms.value


def c_keep(ix, idx):
    arr = np.ascontiguousarray(idx, np.uint32)
    ms = C.c_double()
    t0 = time.perf_counter()
    H._check(H.lib().finch_index_keep(ix._handle(), arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(arr), C.byref(ms)))
    return time.perf_counter() - t0, ms.value


def rebuild(old, refs):
    """what a caller did before: free, build over the whole library, attach the counts -> (wall, the build's kernels, the index)"""
    t0 = time.perf_counter()
    if old is not None:
        old.close()
    ix = H.LibraryIndex(refs)
    ix.attach_counts()
    return time.perf_counter() - t0, ix.stats()["build_kernel_ms"], ix


def answers(ix, queries):
    """(bytes of a search, bytes of a compare_counts); the counts are attached: the wrapper's flag is set by hand for an index
    that was updated below the wrapper"""
    ix._counts_attached = True
    offsets, rows = ix.search(queries, MIN_CONTAINMENT, 0)
    return offsets.tobytes() + rows.tobytes(), ix.compare_counts(queries, MIN_COMMON).tobytes()


def one_configuration(kind, amount, base, more, queries, a):
    R = len(base)
    if kind == "add":
        part = H.select(more, np.arange(amount))
        result = H.select(base, np.arange(R))
        result.append(part)
        label = "add %d" % amount
    else:
        n_drop = int(amount) if amount >= 1 else int(round(R * amount))
        drop = np.unique(np.linspace(0, R - 1, n_drop).astype(np.int64)) if n_drop > 1 else np.asarray([R // 2])
        keep = np.setdiff1d(np.arange(R), drop)
        result = H.select(base, keep)
        label = "keep, dropping %d" % (R - len(keep))
    _, _, ix = rebuild(None, base)
    _, _, fresh = rebuild(None, result)

    def update():
        return c_add(ix, part) if kind == "add" else c_keep(ix, keep)

    update()  # warm-up, and the check before anything is timed
    equal = answers(ix, queries) == answers(fresh, queries)
    assert equal, "%s: the updated index and a fresh one differ" % label
    n_refs, postings = ix.stats()["n_refs"], ix.stats()["postings"]
    assert (n_refs, postings) == (fresh.stats()["n_refs"], fresh.stats()["postings"])
    runs = {"update": [], "rebuild": []}
    for _ in range(a.reps):  # alternating
        if kind == "add":
            c_keep(ix, np.arange(R))  # back to the library of R (not timed)
        else:
            _, _, ix = rebuild(ix, base)
        runs["update"].append(update())
        wall, kernel_ms, fresh = rebuild(fresh, result)
        runs["rebuild"].append((wall, kernel_ms))
    equal = equal and answers(ix, queries) == answers(fresh, queries)
    assert equal, "%s: the updated index and a fresh one differ" % label
    ix.close()
    fresh.close()
    out = {"what": label, "refs_before": R, "refs_after": n_refs, "postings_after": postings, "results_equal_bytes": equal}
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        out[name + "_kernel_s"] = [round(ms / 1e3, 6) for _, ms in rs]
    out["wall_ratio_rebuild_over_update"] = round(med(out["rebuild_wall_s"]) / med(out["update_wall_s"]), 2)
    out["update_kernels_GBps"] = round(24.0 * postings / max(med(out["update_kernel_s"]), 1e-9) / 1e9, 1)
    return out


def record(results, stream_gbps, argv):
    rows = [("references after", lambda o: str(o["refs_after"])),
            ("postings after", lambda o: str(o["postings_after"])),
            ("update: kernels", lambda o: fmt_s(med(o["update_kernel_s"]))),
            ("update: wall", lambda o: fmt_s(med(o["update_wall_s"]))),
            ("rebuild (free + new + attach): build kernels", lambda o: fmt_s(med(o["rebuild_kernel_s"]))),
            ("rebuild (free + new + attach): wall", lambda o: fmt_s(med(o["rebuild_wall_s"]))),
            ("wall, rebuild / update", lambda o: "%.2f x" % o["wall_ratio_rebuild_over_update"]),
            ("update kernels: 24 B x postings after / kernel time", lambda o: "%.0f GB/s" % o["update_kernels_GBps"]),
            ("search and compare_counts equal a fresh index's bytes", lambda o: "yes" if o["results_equal_bytes"] else "NO")]
    lines = [BEGIN, "", "```", "python tools/index_update_bench.py " + " ".join(argv), "```", "",
             "Medians of %d; the values of every run are in the raw lines below.  Streaming-read rate of this GPU's HBM, measured in the "
             "same process as bench.py measures it: %s." % (len(results[0]["update_wall_s"]), "%.0f GB/s" % stream_gbps if stream_gbps else "not measured"),
             "", "| | " + " | ".join(o["what"] for o in results) + " |", "|---|" + "---|" * len(results)]
    lines += ["| %s | " % name + " | ".join(f(o) for o in results) + " |" for name, f in rows]
    lines += ["", "Raw output, one line per configuration:", "", "```"] + [json.dumps(o) for o in results] + ["```", "", END]
    return "\n".join(lines)


def write(path, block):
    text = open(path).read() if os.path.exists(path) else \
        "# Measurements: the library index grown and shrunk in place (`finch_index_add`, `finch_index_keep`, DESIGN §3.19)\n\n%s\n%s\n" % (BEGIN, END)
    if BEGIN not in text or END not in text:
        sys.exit("%s has no marker lines" % path)
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + block + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--adds", default="1,1000,10000")
    ap.add_argument("--drops", default="1,0.1,0.5")
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    adds = [int(x) for x in a.adds.split(",") if x]
    drops = [float(x) for x in a.drops.split(",") if x]
    base = sketches(a.refs, a.groups, a.seed)
    more = sketches(max(adds + [1]), a.groups, a.seed + 7)
    queries = make_queries(base, a.queries, a.seed)
    try:
        buf = S.DeviceBuffer(1 << 30)
        stream_gbps = S.measure_read_bandwidth(buf, 1 << 30)
        buf.free()
    except Exception:
        stream_gbps = None
    print(json.dumps({"hbm_stream_read_GBps": stream_gbps}), flush=True)
    results = []
    for kind, amount in [("add", n) for n in adds] + [("keep", d) for d in drops]:
        out = one_configuration(kind, amount, base, more, queries, a)
        out["hbm_stream_read_GBps"] = stream_gbps
        print(json.dumps(out), flush=True)
        results.append(out)
        if a.write:  # (after every configuration: a run cut short leaves what it had)
            write(a.write, record(results, stream_gbps, sys.argv[1:]))


if __name__ == "__main__":
    main()
