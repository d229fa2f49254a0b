#!/usr/bin/env python3
"""finch_gather next to its two baselines on one GPU, the same inputs, the same process; prints one JSON line.

    python tools/gather_bench.py [--refs 10000] [--queries 10] [--members 20] [--noise 500] [--min-overlap 1] [--reps 3]
                                 [--host-queries 1]

Library: synthetic Mash-1000 sketches as tools/dist_bench.py makes them (groups of related sketches: a best-first search is
full of near-duplicates).  Queries: synthetic "metagenomes", each the union of `--members` library members plus `--noise`
hashes of its own, with random counts.  Three routes to the same rows, and this tool asserts that they are the same:

  gather   finch_gather: the loop on the device;
  host     finch_gather_query on one core, the contract's loop as written, for the first `--host-queries` queries (each round
           looks every hash of the library up: seconds per query);
  rounds   the host-driven alternative: per round one finch_search-sized counting pass over the whole library for what is left of
           every query (finch_search with no threshold: every pair's count crosses to the host), the arg-max and the set
           difference in numpy, the remaining queries made into sketches again.  The seconds inside the finch_search calls
           are reported on their own (rounds_search_calls_s): the rest of the route's time is that Python.

Timed after one warm-up of the device routes: the whole call (wall clock, best of --reps) and for the gather the kernels (HIP
events), the launches, the candidates and the records that crossed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams  # noqa: E402
from tools.dist_bench import sketches  # noqa: E402


def one_sketch(name, hashes, counts):
    kc = np.zeros(len(hashes), KC_DTYPE)
    kc["hash"], kc["count"] = hashes, counts
    km = np.zeros((len(hashes), 21), np.uint8)
    return H.sketches_from_arrays(name, 1000000, 1000000, kc, km, SketchParams.mash(), H.FilterParams(False))


def collect(parts):
    out = parts[0]
    for p in parts[1:]:
        out.append(p)
    return out


def rounds_route(qhashes, refs, ref_hashes, min_overlap):
    """one counting pass over the library per round, for every query that has not stopped -> per query [(reference, overlap)], the
    passes, and the seconds spent inside the passes (finch_search) alone: the rest is Python -- the remaining queries made into
    sketches again, the arg-max, the set difference"""
    left = [h.copy() for h in qhashes]
    live = list(range(len(left)))
    out = [[] for _ in left]
    passes, search_s = 0, 0.0
    while live:
        qs = collect([one_sketch("left%d" % q, left[q], 1) for q in live])
        t0 = time.perf_counter()
        _, rows = H.search(qs, refs, 0.0, 0)
        search_s += time.perf_counter() - t0
        passes += 1
        nxt = []
        for at, q in enumerate(live):
            mine = rows[rows["query"] == at]
            common = mine["common_hashes"].astype(np.int64)
            best = np.lexsort((mine["reference"], -common))[0]
            if common[best] < max(1, min_overlap):
                continue
            w = int(mine["reference"][best])
            out[q].append((w, int(common[best])))
            left[q] = np.setdiff1d(left[q], ref_hashes[w], assume_unique=True)
            nxt.append(q)
        live = nxt
    return out, passes, search_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=10)
    ap.add_argument("--members", type=int, default=20)
    ap.add_argument("--noise", type=int, default=500)
    ap.add_argument("--min-overlap", type=int, default=1)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    refs = sketches(a.refs, a.groups, a.seed)
    ref_hashes = [refs.sketch(i).arrays[0]["hash"].copy() for i in range(a.refs)]
    rng = np.random.default_rng(a.seed + 1)
    qhashes, qparts = [], []
    for q in range(a.queries):
        members = rng.choice(a.refs, size=min(a.members, a.refs), replace=False)
        noise = rng.integers(0, 1 << 63, a.noise, dtype=np.uint64)  # (a hash the library has too would only be one more match)
        h = np.unique(np.concatenate([ref_hashes[m] for m in members] + [noise]))
        qhashes.append(h)
        qparts.append(one_sketch("metagenome%d" % q, h, rng.integers(1, 100, len(h))))
    queries = collect(qparts)

    def gather_route():
        st = {}
        t0 = time.perf_counter()
        offsets, rows = H.gather(queries, refs, a.min_overlap, 0, stats=st)
        return time.perf_counter() - t0, st, offsets, rows

    _, _, offsets, rows = gather_route()  # warm-up: code object load, first allocations
    gather_runs = [gather_route() for _ in range(a.reps)]
    for _, _, o, r in gather_runs:
        assert np.array_equal(o, offsets) and r.tobytes() == rows.tobytes(), "gather: rows differ between runs"

    t0 = time.perf_counter()
    host = [H.gather_query(refs, queries, q, a.min_overlap, 0) for q in range(min(a.host_queries, a.queries))]
    host_s = time.perf_counter() - t0
    for q, hr in enumerate(host):
        mine = rows[offsets[q]:offsets[q + 1]]
        assert len(hr) == len(mine) and all(np.array_equal(hr[f].view(np.uint64), mine[f].view(np.uint64)) for f in H.GATHER_DTYPE.names), \
            "finch_gather_query differs for query %d" % q

    rounds_route(qhashes, refs, ref_hashes, a.min_overlap)  # warm-up
    rounds_runs, rounds_search = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        picked, passes, search_s = rounds_route(qhashes, refs, ref_hashes, a.min_overlap)
        rounds_runs.append(time.perf_counter() - t0)
        rounds_search.append(search_s)
    for q, p in enumerate(picked):
        mine = rows[offsets[q]:offsets[q + 1]]
        assert [(int(r), int(c)) for r, c in zip(mine["reference"], mine["overlap"])] == p, "the round-by-round route differs for query %d" % q

    best = min(gather_runs, key=lambda x: x[0])
    out = {"refs": a.refs, "queries": a.queries, "members": a.members, "noise": a.noise, "min_overlap": a.min_overlap,
           "query_hashes": [int(len(h)) for h in qhashes], "rows": int(len(rows)), "rows_per_query": np.diff(offsets).astype(int).tolist(),
           "rows_equal": True,
           "gather_wall_s": [round(w, 6) for w, _, _, _ in gather_runs], "gather_kernel_s": [round(st["kernel_ms"] / 1e3, 6) for _, st, _, _ in gather_runs],
           "gather_launches": best[1]["launches"], "gather_candidates": best[1]["candidates"], "gather_records_copied": best[1]["records_copied"],
           "host_queries": len(host), "host_wall_s": round(host_s, 3), "host_s_per_query": round(host_s / max(1, len(host)), 3),
           "rounds_wall_s": [round(w, 6) for w in rounds_runs], "rounds_search_calls_s": [round(w, 6) for w in rounds_search],
           "rounds_counting_passes": passes}
    g = min(out["gather_wall_s"])
    out["kernel_share_of_gather"] = round(min(out["gather_kernel_s"]) / g, 3)
    out["wall_ratio_host_over_gather"] = round(out["host_s_per_query"] * a.queries / g, 1)
    out["wall_ratio_rounds_over_gather"] = round(min(rounds_runs) / g, 2)
    out["wall_ratio_rounds_search_calls_over_gather"] = round(min(rounds_search) / g, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
