#!/usr/bin/env python3
"""finch_index_gather next to finch_gather on one GPU: the same library, the same queries, the same process; prints one JSON
line per configuration and writes the measurement record.

    python tools/index_gather_bench.py [--refs 10000,100000] [--queries 10,100] [--members 20] [--noise 500] [--min-overlap 1]
                                       [--reps 3] [--write docs/MEASUREMENTS_index_gather.md]

Library: synthetic Mash-1000 sketches as tools/dist_bench.py makes them (`--groups` pools of related sketches: near-duplicates
everywhere).  Queries: tools/gather_bench.py's synthetic "metagenomes", each the union of `--members` library members plus
`--noise` hashes of its own, with random counts: about 20 K hashes.  Per library size the sketches are made once; per
configuration each route is warmed up once, the two results are checked to be the same bytes (offsets and rows), and then,
alternating, `--reps` times each: building the index, finch_index_gather on it, finch_gather (the dense route: code this tool's
subject does not touch) -- the whole call (wall clock) and the kernels (HIP events) of each.  Reported: the medians, the pairs
the index counted, the candidates, the rows.  `--write PATH` puts a table of the medians and the raw lines between the two
marker lines of PATH (the file is made if it is not there; what stands outside the markers stays).
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
from tools.gather_bench import collect, one_sketch  # noqa: E402

BEGIN, END = "<!-- tools/index_gather_bench.py: begin -->", "<!-- tools/index_gather_bench.py: end -->"


def make_queries(ref_hashes, n, members, noise, seed):
    """tools/gather_bench.py's queries"""
    rng = np.random.default_rng(seed + 1)
    parts = []
    for q in range(n):
        picked = rng.choice(len(ref_hashes), size=min(members, len(ref_hashes)), replace=False)
        fresh = rng.integers(0, 1 << 63, noise, dtype=np.uint64)
        h = np.unique(np.concatenate([ref_hashes[m] for m in picked] + [fresh]))
        parts.append(one_sketch("metagenome%d" % q, h, rng.integers(1, 100, len(h))))
    return collect(parts)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def one_configuration(refs, queries, a):
    def build_route():
        t0 = time.perf_counter()
        ix = H.LibraryIndex(refs)
        return time.perf_counter() - t0, ix

    def index_route(ix):
        st = {}
        t0 = time.perf_counter()
        offsets, rows = ix.gather(queries, a.min_overlap, 0, stats=st)
        return time.perf_counter() - t0, st, offsets, rows

    def dense_route():
        st = {}
        t0 = time.perf_counter()
        offsets, rows = H.gather(queries, refs, a.min_overlap, 0, stats=st)
        return time.perf_counter() - t0, st, offsets, rows

    _, ix = build_route()  # warm-up of each route: code object load, first allocations
    _, ist, io, ir = index_route(ix)
    _, dst, do, dr = dense_route()
    equal = io.tobytes() == do.tobytes() and ir.tobytes() == dr.tobytes()
    out = {"refs": len(refs), "queries": len(queries), "pairs": len(refs) * len(queries), "min_overlap": a.min_overlap,
           "query_hashes_mean": int(np.mean([len(queries.sketch(q).arrays[0]) for q in range(len(queries))])),
           "rows": int(len(ir)), "pairs_touched": ist["pairs_touched"], "touched_share": ist["pairs_touched"] / (len(refs) * len(queries)),
           "candidates": ist["candidates"], "dense_candidates": dst["candidates"], "records_copied": ist["records_copied"],
           "index_launches": ist["launches"], "dense_launches": dst["launches"]}
    out.update({"index_" + k: v for k, v in ix.stats().items() if k != "build_kernel_ms"})
    ix.close()
    runs = {"build": [], "index": [], "dense": []}
    for _ in range(a.reps):  # alternating
        wall, ix = build_route()
        runs["build"].append((wall, ix.stats()["build_kernel_ms"]))
        wall, st, o, r = index_route(ix)
        runs["index"].append((wall, st["kernel_ms"]))
        equal = equal and o.tobytes() == do.tobytes() and r.tobytes() == dr.tobytes()
        ix.close()
        wall, st, o, r = dense_route()
        runs["dense"].append((wall, st["kernel_ms"]))
        equal = equal and o.tobytes() == do.tobytes() and r.tobytes() == dr.tobytes()
    out["results_equal_bytes"] = equal
    for name, rs in runs.items():
        out[name + "_wall_s"] = [round(w, 6) for w, _ in rs]
        out[name + "_kernel_s"] = [round(ms / 1e3, 6) for _, ms in rs]
    out["wall_ratio_dense_over_index"] = round(med(out["dense_wall_s"]) / med(out["index_wall_s"]), 3)
    out["kernel_ratio_dense_over_index"] = round(med(out["dense_kernel_s"]) / max(med(out["index_kernel_s"]), 1e-9), 3)
    gain = med(out["dense_wall_s"]) - med(out["index_wall_s"])
    out["break_even_gathers"] = round(med(out["build_wall_s"]) / gain, 3) if gain > 0 else None  # build / (dense - index)
    return out


def fmt_s(s):
    return "%.1f ms" % (s * 1e3) if s < 1 else "%.3f s" % s


def record(results, argv):
    rows = [("index build: kernels", lambda o: fmt_s(med(o["build_kernel_s"]))),
            ("index build: wall", lambda o: fmt_s(med(o["build_wall_s"]))),
            ("`finch_index_gather`: kernels", lambda o: fmt_s(med(o["index_kernel_s"]))),
            ("`finch_index_gather`: wall", lambda o: fmt_s(med(o["index_wall_s"]))),
            ("`finch_gather`: kernels", lambda o: fmt_s(med(o["dense_kernel_s"]))),
            ("`finch_gather`: wall", lambda o: fmt_s(med(o["dense_wall_s"]))),
            ("launches: index / dense", lambda o: "%d / %d" % (o["index_launches"], o["dense_launches"])),
            ("`pairs_touched`", lambda o: str(o["pairs_touched"])),
            ("`pairs_touched / (Q x R)`", lambda o: "%.4f" % o["touched_share"]),
            ("candidates", lambda o: str(o["candidates"])),
            ("rows", lambda o: str(o["rows"])),
            ("the two results are equal bytes", lambda o: "yes" if o["results_equal_bytes"] else "NO"),
            ("kernels, `finch_gather` / `finch_index_gather`", lambda o: "%.2f x" % o["kernel_ratio_dense_over_index"]),
            ("wall, `finch_gather` / `finch_index_gather`", lambda o: "%.2f x" % o["wall_ratio_dense_over_index"])]
    lines = [BEGIN, "", "```", "python tools/index_gather_bench.py " + " ".join(argv), "```", "",
             "Medians of %d; the values of every run are in the raw lines below." % len(results[0]["index_wall_s"]), "",
             "| | " + " | ".join("R = %d, Q = %d" % (o["refs"], o["queries"]) for o in results) + " |",
             "|---|" + "---|" * len(results)]
    lines += ["| %s | " % name + " | ".join(f(o) for o in results) + " |" for name, f in rows]
    lines += ["", "Raw output, one line per configuration:", "", "```"] + [json.dumps(o) for o in results] + ["```", "", END]
    return "\n".join(lines)


def write(path, block):
    text = open(path).read() if os.path.exists(path) else "# Measurements: the gather through the library index (`finch_index_gather`, DESIGN §3.16)\n\n%s\n%s\n" % (BEGIN, END)
    if BEGIN not in text or END not in text:
        sys.exit("%s has no marker lines" % path)
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + block + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", default="10000,100000")
    ap.add_argument("--queries", default="10,100")
    ap.add_argument("--members", type=int, default=20)
    ap.add_argument("--noise", type=int, default=500)
    ap.add_argument("--min-overlap", type=int, default=1)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    results = []
    for n_refs in (int(x) for x in a.refs.split(",")):
        refs = sketches(n_refs, a.groups, a.seed)
        ref_hashes = [refs.sketch(i).arrays[0]["hash"].copy() for i in range(n_refs)]
        for n_queries in (int(x) for x in a.queries.split(",")):
            out = one_configuration(refs, make_queries(ref_hashes, n_queries, a.members, a.noise, a.seed), a)
            print(json.dumps(out), flush=True)
            results.append(out)
            if a.write:  # (after every configuration: a run cut short leaves what it had)
                write(a.write, record(results, sys.argv[1:]))
    if not all(o["results_equal_bytes"] for o in results):
        sys.exit("finch_index_gather and finch_gather differ")


if __name__ == "__main__":
    main()
