"""finch_dist on the GPU against the reference's loop (cli/src/main.rs:315-333) run pair by pair through finch_distance:
the same rows in the same order, every double the same bits."""
import json
import os
import struct
import tempfile

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
FIELDS = ("containment", "jaccard", "mash_distance", "common_hashes", "total_hashes")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def bits(x):
    return struct.pack("<d", float(x))


def mk(name, hashes, params=None, filters=None, seq_length=100, counts=None):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, 1 if counts is None else counts, 0
    p = params or SketchParams.mash()
    km = np.zeros((len(hs), p.kmer_length), np.uint8)
    return H.sketches_from_arrays(name, seq_length, 100, kc, km, p, filters or H.FilterParams(False))


def collect(parts):
    out = parts[0]
    for p in parts[1:]:
        out.append(p)
    return out


def rust_eq(a, b):
    """Sketch's derived PartialEq (serialization/mod.rs:45) on two Sketch records (Sketches._sketch_loaded)"""
    if (a.name, a.seq_length, a.num_valid_kmers, a.comment) != (b.name, b.seq_length, b.num_valid_kmers, b.comment):
        return False
    fa, fb = a.filter_params, b.filter_params
    if fa.filter_on != fb.filter_on or fa.abun_filter != fb.abun_filter:
        return False
    if not (fa.err_filter == fb.err_filter and fa.strand_filter == fb.strand_filter):  # f64 ==: NaN is not equal to itself
        return False
    pa, pb = a.sketch_params, b.sketch_params
    if pa.kind != pb.kind or pa.kmer_length != pb.kmer_length:
        return False
    if pa.kind == "mash" and (pa.kmers_to_sketch, pa.final_size, pa.no_strict, pa.hash_seed) != \
            (pb.kmers_to_sketch, pb.final_size, pb.no_strict, pb.hash_seed):
        return False
    if pa.kind == "scaled" and not (pa.kmers_to_sketch == pb.kmers_to_sketch and pa.scale == pb.scale and pa.hash_seed == pb.hash_seed):
        return False
    ka, kb = a.arrays, b.arrays
    return np.array_equal(ka[0], kb[0]) and np.array_equal(ka[1], kb[1])


def loop(qs, rs, old_mode=False, pairs=None):
    """the reference's loop, every pair kept (no max_distance yet): list of (q, r, dict)"""
    qsk = [qs._sketch_loaded(i) for i in range(len(qs))]
    rsk = qsk if rs is qs else [rs._sketch_loaded(i) for i in range(len(rs))]
    out = []
    it = pairs if pairs is not None else ((q, r) for r in range(len(rs)) for q in range(len(qs)))
    for q, r in it:
        if qsk[q].name == rsk[r].name and rust_eq(qsk[q], rsk[r]):
            continue
        out.append((q, r, H.distance(qs, q, rs, r, old_mode)))
    return out


def same_rows(rows, want, max_distance):
    want = [w for w in want if w[2]["mash_distance"] <= max_distance]
    assert len(rows) == len(want)
    assert np.array_equal(rows["query"], np.array([w[0] for w in want], np.uint32))
    assert np.array_equal(rows["reference"], np.array([w[1] for w in want], np.uint32))
    for row, (_, _, d) in zip(rows, want):
        for f in ("containment", "jaccard", "mash_distance"):
            assert bits(row[f]) == bits(d[f]), (f, row, d)
        assert int(row["common_hashes"]) == d["common_hashes"] and int(row["total_hashes"]) == d["total_hashes"], (row, d)


def pool_sketches(n, rng, size=1000, groups=12, prefix="s"):
    """Mash-sized sketches drawn from shared pools: within a group the shared fraction runs from 0 to 1"""
    bases = [np.unique(rng.integers(0, 1 << 63, size * 3, dtype=np.uint64) * 2)[:size] for _ in range(groups)]
    out = []
    for i in range(n):
        base = bases[i % groups]
        keep = rng.random() ** 2
        kept = base[rng.random(size) < keep]
        fresh = rng.integers(0, 1 << 63, size - len(kept) + 50, dtype=np.uint64) * 2 + 1  # odd: never in a base
        hs = np.unique(np.concatenate([kept, fresh]))[:size]
        out.append(mk("%s%d" % (prefix, i), hs))
    return collect(out)


@pytest.fixture(scope="module")
def mixed():
    sk = pool_sketches(400, np.random.default_rng(11))
    return sk, loop(sk, sk)


@pytest.mark.parametrize("which", ["1.0", "0.05", "0.0", "pair"])
def test_mixed_overlaps(mixed, which):
    sk, want = mixed
    js = np.array([w[2]["jaccard"] for w in want])
    assert js.min() == 0.0 and js.max() > 0.9
    if which == "pair":  # exactly one pair's distance: the comparison is <=
        mids = sorted(w[2]["mash_distance"] for w in want if 0 < w[2]["mash_distance"] < 1)
        assert len(mids) > 100
        md = mids[len(mids) // 2]
    else:
        md = float(which)
    rows = H.dist(sk, sk, max_distance=md)
    same_rows(rows, want, md)
    if which == "pair":
        assert np.any(rows["mash_distance"] == md)


def scaled_m(scale):
    return U64_MAX // int(1.0 / scale)


def shape_sketches():
    rng = np.random.default_rng(5)
    out = []
    sc = [(0.001, 21), (0.01, 21), (0.001, 15), (0.5, 21)]
    base = np.unique(rng.integers(0, U64_MAX, 5000, dtype=np.uint64))
    for i, (s, k) in enumerate(sc):
        m = scaled_m(s)
        extra = np.array([m - 1, m, m + 1, 0, U64_MAX - 1, U64_MAX], np.uint64)
        hs = np.unique(np.concatenate([base[rng.random(len(base)) < 0.6], extra[: 3 + i]]))
        out.append(mk("scaled%d" % i, hs, SketchParams.scaled(len(hs), k, s)))
    for k in (21, 17):
        hs = np.unique(np.concatenate([base[rng.random(len(base)) < 0.5][:900], np.array([0, scaled_m(0.001), U64_MAX], np.uint64)]))
        out.append(mk("mash_k%d" % k, hs, SketchParams.mash(kmer_length=k, no_strict=True)))
    for n in (0, 0, 1, 63, 64, 65, 129):
        hs = np.unique(base[rng.permutation(len(base))[:n]]) if n else np.zeros(0, np.uint64)
        out.append(mk("len%d_%d" % (n, len(out)), hs, SketchParams.mash(no_strict=True)))
    big = np.unique(np.concatenate([base, rng.integers(0, U64_MAX, 46000, dtype=np.uint64)]))
    out.append(mk("big", big, SketchParams.mash(kmers_to_sketch=len(big), final_size=len(big))))
    out.append(mk("one_max", [U64_MAX], SketchParams.scaled(1, 21, 0.001)))
    out.append(mk("one_zero", [0], SketchParams.scaled(1, 21, 0.01)))
    return collect(out)


@pytest.fixture(scope="module")
def shapes():
    sk = shape_sketches()
    return sk, loop(sk, sk)


@pytest.mark.parametrize("slice_, chunk", [(None, None), ("7", "5"), ("64", None)])
def test_sketch_shapes(shapes, slice_, chunk):
    sk, want = shapes
    assert any(w[2]["total_hashes"] != 0 and w[2]["containment"] not in (0.0, 1.0) for w in want)
    try:
        F.set_option("dist_slice", slice_)
        F.set_option("dist_chunk_pairs", chunk)
        same_rows(H.dist(sk, sk), want, 1.0)
    finally:
        F.set_option("dist_slice", None)
        F.set_option("dist_chunk_pairs", None)


def test_sketch_shapes_old_mode(shapes):
    sk, _ = shapes
    full = [i for i in range(len(sk)) if H.lib().finch_sketch_n_hashes(sk._p, i) > 0]
    qs = H.select(sk, full)
    same_rows(H.dist(qs, sk, old_mode=True), loop(qs, sk, old_mode=True), 1.0)
    # empty against empty is 0 / 0 in old mode
    empties = [i for i in range(len(sk)) if H.lib().finch_sketch_n_hashes(sk._p, i) == 0]
    e = H.select(sk, empties)
    rows = H.dist(e, e, old_mode=True)
    want = loop(e, e, old_mode=True)
    assert len(want) == 2 and np.isnan(want[0][2]["containment"])
    same_rows(rows, want, 1.0)


def test_old_mode_empty_query_error(shapes):
    sk, _ = shapes
    with pytest.raises(F.FinchError) as ref:
        H.distance(sk, 7, sk, 0, old_mode=True)
    with pytest.raises(F.FinchError) as ei:
        H.dist(sk, sk, old_mode=True)
    assert str(ei.value) == str(ref.value)


def test_self_skip():
    rng = np.random.default_rng(3)
    hs = np.unique(rng.integers(0, U64_MAX, 300, dtype=np.uint64))
    nan_f = H.FilterParams(False, (None, None), float("nan"), 0.0)
    parts = [mk("A", hs), mk("A", hs), mk("B", hs), mk("A", hs), mk("D", hs, filters=nan_f), mk("A", hs, seq_length=101)]
    sk = collect(parts)
    sk.set_comment(3, "another comment")
    rows = H.dist(sk, sk)
    got = set(zip(rows["query"].tolist(), rows["reference"].tolist()))
    for a in (0, 1):
        for b in (0, 1):
            assert (a, b) not in got  # identical: skipped both ways, and each against itself
    for a, b in [(0, 2), (2, 0), (0, 3), (3, 0), (4, 4), (0, 4), (0, 5), (5, 0), (3, 3), (2, 2)]:
        assert ((a, b) in got) == (a == b == 4 or a != b), (a, b)
    assert (4, 4) in got and (3, 3) not in got and (2, 2) not in got
    same_rows(rows, loop(sk, sk), 1.0)


def test_end_to_end_files():
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genomes = [rng.integers(0, 4, 30000) for _ in range(6)]
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(240):
            g = genomes[i % 6].copy()
            mut = rng.random(len(g)) < rng.random() * 0.05
            g[mut] = rng.integers(0, 4, int(mut.sum()))
            p = os.path.join(d, "g%03d.fa" % i)
            with open(p, "wb") as f:
                f.write(b">g%d\n" % i + acgt[g].tobytes() + b"\n")
            paths.append(p)
        sk = H.sketch_files(paths, SketchParams.mash(), H.FilterParams(False))
    rows = H.dist_command(sk, pairwise=True)
    same_rows(rows, loop(sk, sk), 1.0)
    text = H.dist_json(sk, sk)
    parsed = json.loads(text, object_pairs_hook=lambda kv: kv)
    assert len(parsed) == len(rows)
    names = [H.lib().finch_sketch_name(sk._p, i).decode() for i in range(len(sk))]
    for row, kv in zip(rows, parsed):
        assert [k for k, _ in kv] == ["containment", "jaccard", "mashDistance", "commonHashes", "totalHashes", "query", "reference"]
        v = dict(kv)
        for f, j in (("containment", "containment"), ("jaccard", "jaccard"), ("mash_distance", "mashDistance")):
            assert bits(v[j]) == bits(row[f])
        assert v["commonHashes"] == row["common_hashes"] and v["totalHashes"] == row["total_hashes"]
        assert v["query"] == names[row["query"]] and v["reference"] == names[row["reference"]]
    # --queries and the default (the first sketch only)
    qrows = H.dist_command(sk, queries={names[3], names[100]}, max_distance=0.02)
    same_rows(qrows, [w for w in loop(sk, sk) if w[0] in (3, 100)], 0.02)
    frows = H.dist_command(sk)
    assert set(frows["query"].tolist()) == {0} and len(frows) == len(sk) - 1


def test_two_entries_on_one_device(mixed):
    sk, want = mixed
    try:
        F.set_option("dist_chunk_pairs", "20000")
        a = H.dist(sk, sk, devices=[0])
        b = H.dist(sk, sk, devices=[0, 0])
        st = {}
        H.dist(sk, sk, devices=[0, 0], stats=st)
        assert st["launches"] == (400 + 49) // 50
    finally:
        F.set_option("dist_chunk_pairs", None)
    assert a.tobytes() == b.tobytes()
    same_rows(b, want, 1.0)


def test_size_3000_pairwise():
    rng = np.random.default_rng(99)
    n = 3000
    sk = pool_sketches(n, rng, groups=40)
    st = {}
    rows = H.dist(sk, sk, stats=st)
    assert st["launches"] >= 2
    assert len(rows) == n * n - n
    r = np.repeat(np.arange(n, dtype=np.uint32), n - 1)
    q = np.tile(np.arange(n, dtype=np.uint32), n)
    q = q[q != np.repeat(np.arange(n, dtype=np.uint32), n)]
    assert np.array_equal(rows["reference"], r) and np.array_equal(rows["query"], q)
    pick = np.sort(rng.choice(len(rows), 50000, replace=False))
    for i in pick:
        row = rows[i]
        d = H.distance(sk, int(row["query"]), sk, int(row["reference"]))
        for f in FIELDS[:3]:
            assert bits(row[f]) == bits(d[f])
        assert int(row["common_hashes"]) == d["common_hashes"] and int(row["total_hashes"]) == d["total_hashes"]
