#!/usr/bin/env python3
"""finch_index_screen (containment of a library's references in raw reads) on one GPU, next to the two things it is made of or
replaces -- the existing hashing path (finch_sketch_buffer, Mash 1000, the same k) and the contract on the host
(finch_screen_host on 16 threads, the sample in 16 slices) -- on the same sample; prints one JSON line.

    python tools/index_screen_bench.py [--genomes 4000] [--genome-len 50000] [--gbases 1.0] [--reps 3] [--host-threads 16]

The library: Mash-1000, k = 21 sketches of `genomes` random genomes, made by finch_sketch_records from one multi-FASTA.  The
sample: 150-base reads (FASTA, one line each, either strand) drawn from twenty of the genomes at depths 2, 4, .. 40, plus reads
of unrelated random sequence up to `gbases` in all.  After one warm-up call, `reps` timed calls of LibraryIndex.screen: wall clock
of the call and the figures of finch_screen_stats; then the yardsticks, once each after a warm-up of their own.  The members'
median_mult is printed beside the depth they were drawn at: a k-mer of a genome read at depth D by reads of 150 bases is
expected D * (150 - k + 1) / 150 times.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import SketchParams  # noqa: E402

READ = 150
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def fasta_of_rows(rows, tag):
    """(n, L) bases -> n records of one line each"""
    n, length = rows.shape
    out = np.empty((n, length + 4), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, -1] = ord(">"), tag, ord("\n"), ord("\n")
    out[:, 3:-1] = rows
    return out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=4000)
    ap.add_argument("--genome-len", type=int, default=50000)
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    k = a.k

    genomes = ACGT[rng.integers(0, 4, (a.genomes, a.genome_len), dtype=np.uint8)]
    params = SketchParams.mash(1000, 1000, False, k)
    t0 = time.perf_counter()
    refs = H.sketch_records(fasta_of_rows(genomes, ord("g")), params)
    sketch_s = time.perf_counter() - t0

    members = [int(g) for g in rng.choice(a.genomes, 20, replace=False)]
    depths = [2 * (i + 1) for i in range(20)]
    parts = []
    for g, d in zip(members, depths):
        n = d * a.genome_len // READ
        starts = rng.integers(0, a.genome_len - READ + 1, n)
        reads = genomes[g][starts[:, None] + np.arange(READ)[None, :]]
        flip = rng.random(n) < 0.5
        reads[flip] = COMP[reads[flip][:, ::-1]]
        parts.append(fasta_of_rows(reads, ord("m")))
    member_bases = sum(len(p) for p in parts) * READ // (READ + 4)
    n_noise = max(0, int(a.gbases * 1e9) - member_bases) // READ
    step = 1 << 16  # (many parts: the host yardstick deals them round-robin over its threads)
    for o in range(0, n_noise, step):
        m = min(step, n_noise - o)
        parts.append(fasta_of_rows(ACGT[rng.integers(0, 4, (m, READ), dtype=np.uint8)], ord("n")))
    del genomes
    slices = [b"".join(parts[i::a.host_threads]) for i in range(a.host_threads)]  # (whole records each)
    sample = b"".join(slices)
    del parts

    ix = H.LibraryIndex(refs)

    def one():
        st = {}
        t0 = time.perf_counter()
        rows = ix.screen(sample, stats=st)
        return time.perf_counter() - t0, st, rows

    _, st, want = one()  # warm-up
    walls, kernels, tables = [], [], []
    same = True
    for _ in range(a.reps):
        w, st, rows = one()
        walls.append(w), kernels.append(st["kernel_ms"] / 1e3), tables.append(st["table_ms"])
        same = same and rows.tobytes() == want.tobytes()
    positions = st["positions"]
    gb = positions / 1e9

    ff = H.FilterParams(False)
    H.sketch_stream(sample[:1 << 24], "warm", params, ff)
    t0 = time.perf_counter()
    H.sketch_stream(sample, "sample", params, ff)
    sketch_buffer_s = time.perf_counter() - t0

    def host_slice(s):
        hst = {}
        return H.screen_host(refs, s, k, 0, 1, stats=hst), hst

    with ThreadPoolExecutor(a.host_threads) as ex:
        t0 = time.perf_counter()
        host = list(ex.map(host_slice, slices))
        host_s = time.perf_counter() - t0
    # the slices' rows merged: shared hashes cannot be added up, sum_mult and the figures can
    host_sum = np.zeros(len(refs), np.uint64)
    for rows, _ in host:
        host_sum[rows["reference"]] += rows["sum_mult"]
    dev_sum = np.zeros(len(refs), np.uint64)
    dev_sum[want["reference"]] = want["sum_mult"]
    host_equal = bool(np.array_equal(host_sum, dev_sum)) and sum(h["kmers"] for _, h in host) == st["kmers"]

    by_ref = {int(r["reference"]): r for r in want}
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    out = {"genomes": a.genomes, "genome_len": a.genome_len, "k": k, "library_sketch_s": round(sketch_s, 3),
           "positions": positions, "kmers": st["kmers"], "hits": st["hits"], "hits_per_window": st["hits"] / max(1, st["kmers"]),
           "distinct": st["distinct"], "table_bytes": st["table_bytes"], "table_ms": [round(x, 3) for x in tables],
           "launches": st["launches"], "rows": len(want), "rows_equal_across_calls": same,
           "screen_wall_s": [round(x, 4) for x in walls], "screen_kernel_s": [round(x, 4) for x in kernels],
           "screen_call_gbases_per_s": round(gb / med(walls), 3), "screen_kernel_gbases_per_s": round(gb / med(kernels), 3),
           "sketch_buffer_wall_s": round(sketch_buffer_s, 4), "sketch_buffer_gbases_per_s": round(gb / sketch_buffer_s, 3),
           "host_threads": a.host_threads, "host_wall_s": round(host_s, 3), "host_gbases_per_s": round(gb / host_s, 4),
           "host_sum_mult_equal": host_equal,
           "members": [{"reference": g, "depth": d, "expected_kmer_depth": round(d * (READ - k + 1) / READ, 2),
                        "median_mult": int(by_ref[g]["median_mult"]) if g in by_ref else None,
                        "shared": int(by_ref[g]["shared"]) if g in by_ref else 0} for g, d in zip(members, depths)],
           "rows_not_members": int(sum(1 for r in by_ref if r not in set(members)))}
    ix.close()
    print(json.dumps(out))
    if not (same and host_equal):
        sys.exit("the screen's calls, or the device and the host, disagree")


if __name__ == "__main__":
    main()
