#!/usr/bin/env python3
"""finch_index_compare_counts next to finch_compare_counts on one GPU: the same library, the same queries, the same process;
prints one JSON line per configuration and writes the measurement record.

    python tools/index_compare_counts_bench.py [--refs 10000,100000] [--queries 100] [--members 20] [--noise 500]
                                               [--min-common 20] [--reps 3] [--write docs/MEASUREMENTS_index_compare_counts.md]

Library: synthetic Mash-1000 sketches as tools/dist_bench.py makes them (`--groups` pools of related sketches).  Queries:
tools/index_gather_bench.py's synthetic "metagenomes", each the union of `--members` library members plus `--noise` hashes of
its own, with random counts: about 20 K hashes.  Per library size the sketches are made once and the index is built once; each
route is warmed up once and the two results are checked to be the same bytes before anything is printed; then, alternating,
`--reps` times each: attaching the counts, finch_index_compare_counts, finch_compare_counts (the dense route: code this tool's
subject does not touch) -- the whole call (wall clock) and the kernels (HIP events) of each.  Reported: the medians, the pairs
the index counted, the pairs the moment kernel walked, the records that crossed the link.  `--write PATH` puts a table of the
medians and the raw lines between the two marker lines of PATH (the file is made if it is not there; what stands outside the
markers stays).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402
from tools.index_gather_bench import fmt_s, make_queries, med  # noqa: E402

BEGIN, END = "<!-- tools/index_compare_counts_bench.py: begin -->", "<!-- tools/index_compare_counts_bench.py: end -->"


def one_configuration(refs, queries, a):
    def attach_route(ix):
        t0 = time.perf_counter()
        nbytes = ix.attach_counts()
        return time.perf_counter() - t0, nbytes

    def index_route(ix):
        st = {}
        t0 = time.perf_counter()
        rows = ix.compare_counts(queries, a.min_common, stats=st)
        return time.perf_counter() - t0, st, rows

    def dense_route():
        st = {}
        t0 = time.perf_counter()
        rows = H.compare_counts(refs, queries, a.min_common, stats=st)
        return time.perf_counter() - t0, st, rows

    t0 = time.perf_counter()
    ix = H.LibraryIndex(refs)
    build_wall = time.perf_counter() - t0
    _, attached = attach_route(ix)  # warm-up of each route: code object load, first allocations
    _, ist, ir = index_route(ix)
    _, dst, dr = dense_route()
    equal = ir.tobytes() == dr.tobytes()
    assert equal, "finch_index_compare_counts and finch_compare_counts differ"
    out = {"refs": len(refs), "queries": len(queries), "pairs": len(refs) * len(queries), "min_common": a.min_common,
           "query_hashes_mean": int(np.mean([len(queries.sketch(q).arrays[0]) for q in range(len(queries))])),
           "rows": int(len(ir)), "pairs_touched": ist["pairs_touched"], "touched_share": ist["pairs_touched"] / (len(refs) * len(queries)),
           "pairs_walked": ist["pairs_walked"], "records_copied": ist["records_copied"], "dense_records_copied": dst["records_copied"],
           "index_launches": ist["launches"], "dense_launches": dst["launches"], "attached_bytes": attached,
           "index_build_wall_s": round(build_wall, 6)}
    out.update({"index_" + k: v for k, v in ix.stats().items()})
    runs = {"attach": [], "index": [], "dense": []}
    for _ in range(a.reps):  # alternating
        wall, _ = attach_route(ix)
        runs["attach"].append((wall, 0.0))
        wall, st, r = index_route(ix)
        runs["index"].append((wall, st["kernel_ms"]))
        equal = equal and r.tobytes() == dr.tobytes()
        wall, st, r = dense_route()
        runs["dense"].append((wall, st["kernel_ms"]))
        equal = equal and r.tobytes() == dr.tobytes()
    ix.close()
    assert equal, "finch_index_compare_counts and finch_compare_counts differ"
    out["results_equal_bytes"] = equal
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        if name != "attach":
            out[name + "_kernel_s"] = [round(ms / 1e3, 6) for _, ms in rs]
    out["wall_ratio_dense_over_index"] = round(med(out["dense_wall_s"]) / med(out["index_wall_s"]), 3)
    out["kernel_ratio_dense_over_index"] = round(med(out["dense_kernel_s"]) / max(med(out["index_kernel_s"]), 1e-9), 3)
    return out


def record(results, argv):
    rows = [("index build: wall (once)", lambda o: fmt_s(o["index_build_wall_s"])),
            ("`finch_index_attach_counts`: wall", lambda o: fmt_s(med(o["attach_wall_s"]))),
            ("attached bytes", lambda o: str(o["attached_bytes"])),
            ("`finch_index_compare_counts`: kernels", lambda o: fmt_s(med(o["index_kernel_s"]))),
            ("`finch_index_compare_counts`: wall", lambda o: fmt_s(med(o["index_wall_s"]))),
            ("`finch_compare_counts`: kernels", lambda o: fmt_s(med(o["dense_kernel_s"]))),
            ("`finch_compare_counts`: wall", lambda o: fmt_s(med(o["dense_wall_s"]))),
            ("launches: index / dense", lambda o: "%d / %d" % (o["index_launches"], o["dense_launches"])),
            ("`pairs_touched`", lambda o: str(o["pairs_touched"])),
            ("`pairs_touched / (Q x R)`", lambda o: "%.4f" % o["touched_share"]),
            ("`pairs_walked`", lambda o: str(o["pairs_walked"])),
            ("records over the link: index / dense", lambda o: "%d / %d" % (o["records_copied"], o["dense_records_copied"])),
            ("rows", lambda o: str(o["rows"])),
            ("the two results are equal bytes", lambda o: "yes" if o["results_equal_bytes"] else "NO"),
            ("kernels, `finch_compare_counts` / `finch_index_compare_counts`", lambda o: "%.2f x" % o["kernel_ratio_dense_over_index"]),
            ("wall, `finch_compare_counts` / `finch_index_compare_counts`", lambda o: "%.2f x" % o["wall_ratio_dense_over_index"])]
    lines = [BEGIN, "", "```", "python tools/index_compare_counts_bench.py " + " ".join(argv), "```", "",
             "Medians of %d; the values of every run are in the raw lines below." % len(results[0]["index_wall_s"]), "",
             "| | " + " | ".join("R = %d, Q = %d" % (o["refs"], o["queries"]) for o in results) + " |",
             "|---|" + "---|" * len(results)]
    lines += ["| %s | " % name + " | ".join(f(o) for o in results) + " |" for name, f in rows]
    lines += ["", "Raw output, one line per configuration:", "", "```"] + [json.dumps(o) for o in results] + ["```", "", END]
    return "\n".join(lines)


def write(path, block):
    text = open(path).read() if os.path.exists(path) else \
        "# Measurements: compare_counts through the library index (`finch_index_compare_counts`, DESIGN §3.18)\n\n%s\n%s\n" % (BEGIN, END)
    if BEGIN not in text or END not in text:
        sys.exit("%s has no marker lines" % path)
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + block + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", default="10000,100000")
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--members", type=int, default=20)
    ap.add_argument("--noise", type=int, default=500)
    ap.add_argument("--min-common", type=int, default=20)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    results = []
    for n_refs in (int(x) for x in a.refs.split(",")):
        refs = sketches(n_refs, a.groups, a.seed)
        ref_hashes = [refs.sketch(i).arrays[0]["hash"].copy() for i in range(n_refs)]
        out = one_configuration(refs, make_queries(ref_hashes, a.queries, a.members, a.noise, a.seed), a)
        print(json.dumps(out), flush=True)
        results.append(out)
        if a.write:  # (after every configuration: a run cut short leaves what it had)
            write(a.write, record(results, sys.argv[1:]))


if __name__ == "__main__":
    main()
