"""finch_dist on the GPU against the reference's loop (cli/src/main.rs:315-333) run pair by pair through finch_distance,
and against the independent model of distance.rs (tests/dist_model.py): the same rows in the same order, every double the
same bits."""
import json
import math
import os
import struct
import tempfile

import numpy as np
import pytest

import dist_model as M
import finch_rs_amd as F
from dist_model import rust_eq
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


def model_sketches(sk):
    """the sketches as the model sees them: hashes, variant, scale, k"""
    L = H.lib()
    out = []
    for i in range(len(sk)):
        hs = np.zeros(L.finch_sketch_n_hashes(sk._p, i), np.uint64)
        assert L.finch_sketch_copy(sk._p, i, hs.ctypes.data, None, None, None) == 0
        p = sk.params_of(i)
        out.append(M.Sk(hs, p.kind, p.scale if p.kind == "scaled" else 0.0, p.kmer_length))
    return out


def model_loop(qs, rs, old_mode=False, pairs=None, pinned=False):
    """the model's calc_sketch_distances, every pair kept: list of (q, r, dict)"""
    mq = model_sketches(qs)
    mr = mq if rs is qs else model_sketches(rs)
    L = H.lib()
    qn = [L.finch_sketch_name(qs._p, i) for i in range(len(qs))]
    rn = [L.finch_sketch_name(rs._p, i) for i in range(len(rs))]
    equal = lambda q, r: qn[q] == rn[r] and rust_eq(qs._sketch_loaded(q), rs._sketch_loaded(r))  # noqa: E731
    return M.calc_sketch_distances(mq, mr, old_mode, math.inf, equal, pairs, pinned)


def expected(qs, rs, old_mode=False, pairs=None, pinned=False):
    """(finch_distance's rows, the model's rows) of the reference's loop, every pair kept"""
    return loop(qs, rs, old_mode, pairs), model_loop(qs, rs, old_mode, pairs, pinned)


def only(want, keep):
    return tuple([w for w in ws if keep(w)] for ws in want)


def same_double(a, b):
    """the same bits; any NaN matches any NaN (the model's 0 / 0 has Python's sign, the library's the hardware's)"""
    return (a != a and b != b) or bits(a) == bits(b)


def same_rows(rows, want, max_distance):
    """rows = finch_distance's rows (bit for bit) and the model's rows (bit for bit, NaN for NaN), filtered by max_distance"""
    lib_rows, model_rows = want
    for ws, eq in ((lib_rows, lambda a, b: bits(a) == bits(b)), (model_rows, same_double)):
        ws = [w for w in ws if w[2]["mash_distance"] <= max_distance]
        assert len(rows) == len(ws)
        assert np.array_equal(rows["query"], np.array([w[0] for w in ws], np.uint32))
        assert np.array_equal(rows["reference"], np.array([w[1] for w in ws], np.uint32))
        for row, (_, _, d) in zip(rows, ws):
            for f in ("containment", "jaccard", "mash_distance"):
                assert eq(row[f], d[f]), (f, row, d)
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
    return sk, expected(sk, sk)


@pytest.mark.parametrize("which", ["1.0", "0.05", "0.0", "pair"])
def test_mixed_overlaps(mixed, which):
    sk, want = mixed
    js = np.array([w[2]["jaccard"] for w in want[0]])
    assert js.min() == 0.0 and js.max() > 0.9
    if which == "pair":  # exactly one pair's distance: the comparison is <=
        mids = sorted(w[2]["mash_distance"] for w in want[0] if 0 < w[2]["mash_distance"] < 1)
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
    return sk, expected(sk, sk)


@pytest.mark.parametrize("slice_, chunk", [(None, None), ("7", "5"), ("64", None)])
def test_sketch_shapes(shapes, slice_, chunk):
    sk, want = shapes
    assert any(w[2]["total_hashes"] != 0 and w[2]["containment"] not in (0.0, 1.0) for w in want[0])
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
    same_rows(H.dist(qs, sk, old_mode=True), expected(qs, sk, old_mode=True), 1.0)
    # empty against empty is 0 / 0 in old mode
    empties = [i for i in range(len(sk)) if H.lib().finch_sketch_n_hashes(sk._p, i) == 0]
    e = H.select(sk, empties)
    rows = H.dist(e, e, old_mode=True)
    want = expected(e, e, old_mode=True)
    assert len(want[0]) == 2 and np.isnan(want[0][0][2]["containment"]) and np.isnan(want[1][0][2]["containment"])
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
    same_rows(rows, expected(sk, sk), 1.0)


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
    want = expected(sk, sk)
    same_rows(rows, want, 1.0)
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
    same_rows(qrows, only(want, lambda w: w[0] in (3, 100)), 0.02)
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
    ms = model_sketches(sk)
    for i in pick:
        row = rows[i]
        q, r = int(row["query"]), int(row["reference"])
        for d in (H.distance(sk, q, sk, r), M.distance(ms[q], ms[r])):
            for f in FIELDS[:3]:
                assert bits(row[f]) == bits(d[f]), (f, row, d)
            assert int(row["common_hashes"]) == d["common_hashes"] and int(row["total_hashes"]) == d["total_hashes"]


# ----------------------------------------------------------------------------------------------------------------------
# Scaled sketches over many scales: 1 / scale not an integer, no scale step, saturation (M = 1), NaN on either side
# ----------------------------------------------------------------------------------------------------------------------

SCALES = [0.001, 0.01, 0.3, 1.0, 0.0, -0.5, 1e-20, 5e-324, float("nan")]


def scaled_set():
    """about 300 sketches: ~30 Scaled per scale, hashes clustered around every M (and 0, u64::MAX), and some Mash ones;
    k mixed (k comes from the query); two sketches repeated under the same name (one with a NaN scale, never equal)"""
    rng = np.random.default_rng(17)
    centres = sorted({M.max_hash(s) for s in SCALES if s > 0} | {0, U64_MAX})
    pool = [np.array([0, 1, 2, U64_MAX - 1, U64_MAX], np.uint64)]
    for c in centres:
        lo, hi = max(0, c - 3000), min(U64_MAX, c + 3000)
        pool.append(rng.integers(lo, hi, 2000, dtype=np.uint64, endpoint=True))
        pool.append(np.array([x for x in (c - 1, c, c + 1) if 0 <= x <= U64_MAX], np.uint64))
    pool.append(rng.integers(0, U64_MAX, 3000, dtype=np.uint64))
    pool = np.unique(np.concatenate(pool))
    out, n = [], 0
    for s in SCALES:
        for _ in range(30):
            size = [0, 1, 2, 40, 150, 400][rng.integers(0, 6)]
            hs = np.sort(rng.choice(pool, size, replace=False))
            k = [21, 15, 31][rng.integers(0, 3)]
            out.append(mk("sc%d" % n, hs, SketchParams.scaled(max(1, len(hs)), k, s)))
            n += 1
    for _ in range(30):
        hs = np.sort(rng.choice(pool, [0, 5, 200][rng.integers(0, 3)], replace=False))
        out.append(mk("mash%d" % n, hs, SketchParams.mash(kmer_length=[21, 17][rng.integers(0, 2)], no_strict=True)))
        n += 1
    nan_one = next(i for i, s in enumerate(out) if s.params.scale != s.params.scale and H.lib().finch_sketch_n_hashes(s._p, 0) > 1)
    out.append(mk("sc%d" % nan_one, out[nan_one].sketch(0).arrays[0]["hash"], out[nan_one].params))
    out.append(mk("sc1", out[1].sketch(0).arrays[0]["hash"], out[1].params))
    return collect(out)


@pytest.fixture(scope="module")
def scaled():
    sk = scaled_set()
    return sk, expected(sk, sk)


def test_scaled_set_pairwise(scaled):
    sk, want = scaled
    ms = model_sketches(sk)
    n, n_nan = len(sk), sum(s.scale != s.scale for s in ms)
    # every sketch skips itself but those with a NaN scale (f64 ==); "sc1" and its copy are equal both ways, the NaN-scale
    # copy is not equal to its original
    assert n_nan == 31 and len(want[0]) == n * n - (n - n_nan) - 2
    rows = H.dist(sk, sk)
    same_rows(rows, want, 1.0)
    # a NaN query against a Scaled reference with a step takes the reference's M, and that changes counts
    nan_q = [(ms[q].hashes, ms[r].hashes, M.max_hash(ms[r].scale)) for q, r, _ in want[1]
             if ms[q].scale != ms[q].scale and ms[r].kind == "scaled" and ms[r].scale > 0]
    assert sum(M.counts(a, b) != M.counts(a, b, m) for a, b, m in nan_q) > 100


def test_scaled_set_max_distance_on_one_row(scaled):
    sk, want = scaled
    vals = [w[2]["mash_distance"] for w in want[1]]
    once = sorted(v for v, c in zip(*np.unique(vals, return_counts=True)) if c == 1 and 0 < v < 1)
    assert len(once) > 10
    md = float(once[len(once) // 2])
    rows = H.dist(sk, sk, max_distance=md)
    same_rows(rows, want, md)
    assert np.sum(rows["mash_distance"] == md) == 1


def test_scaled_set_old_mode(scaled):
    sk, _ = scaled
    full = [i for i in range(len(sk)) if H.lib().finch_sketch_n_hashes(sk._p, i) > 0]
    qs = H.select(sk, full)
    same_rows(H.dist(qs, sk, old_mode=True), expected(qs, sk, old_mode=True), 1.0)


def test_scales_where_the_reference_panics():
    """scale > 1 or +inf: the reference divides by zero; the library's documented M = u64::MAX, on both paths"""
    rng = np.random.default_rng(8)
    out = []
    for n, s in enumerate([2.0, 1.5, float("inf"), 3.0, 0.5]):
        hs = np.unique(np.concatenate([rng.integers(0, U64_MAX, 50, dtype=np.uint64),
                                       np.array([0, M.max_hash(0.5), U64_MAX - 1, U64_MAX][: 1 + n % 4], np.uint64)]))
        out.append(mk("p%d" % n, hs, SketchParams.scaled(len(hs), 21, s)))
    sk = collect(out)
    same_rows(H.dist(sk, sk), expected(sk, sk, pinned=True), 1.0)


def test_json_zero_distance():
    hs = [3, 9, 27]
    sk = collect([mk("a", hs), mk("b", hs)])
    rows = H.dist(sk, sk)
    assert len(rows) == 2 and all(bits(x) == bits(0.0) for x in rows["mash_distance"])
    assert H.dist_json(sk, sk).count('"mashDistance":0.0,') == 2


# ----------------------------------------------------------------------------------------------------------------------
# LDS slices, grid and chunk edges
# ----------------------------------------------------------------------------------------------------------------------

QUERY_LENGTHS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 20000]


@pytest.fixture(scope="module")
def slice_edges():
    """queries of lengths around powers of two and the slice cap; references of 0..200 hashes, partly from the queries'
    pool; two thirds Scaled at 0.01 with the hashes around its M, so that the scale step's counts cross slices too"""
    rng = np.random.default_rng(23)
    m = M.max_hash(0.01)
    pool = np.unique(np.concatenate([rng.integers(0, 2 * m, 60000, dtype=np.uint64), np.array([m - 1, m, m + 1], np.uint64)]))

    def params(i, n):
        return SketchParams.scaled(max(1, n), [21, 15][i % 2], 0.01) if i % 3 else SketchParams.mash(kmer_length=21, no_strict=True)
    qs = collect([mk("q%d" % i, np.sort(rng.choice(pool, n, replace=False)), params(i, n)) for i, n in enumerate(QUERY_LENGTHS)])
    refs = []
    for n in range(201):
        own = rng.choice(pool, n, replace=False)
        fresh = rng.integers(0, U64_MAX, n // 4, dtype=np.uint64)
        hs = np.unique(np.concatenate([own, fresh]))[:n] if n % 5 else np.sort(own)
        refs.append(mk("r%d" % n, hs, params(n + 1, n)))
    rs = collect(refs)
    return qs, rs, expected(qs, rs)


@pytest.mark.parametrize("slice_", [None, "1", "8192", "100000"])
def test_slice_edges(slice_edges, slice_):
    qs, rs, want = slice_edges
    try:
        F.set_option("dist_slice", slice_)
        same_rows(H.dist(qs, rs), want, 1.0)
    finally:
        F.set_option("dist_slice", None)


@pytest.fixture(scope="module")
def grid_set():
    rng = np.random.default_rng(31)
    return pool_sketches(7, rng, size=300, groups=3, prefix="q"), pool_sketches(257, rng, size=200, groups=3, prefix="r")


@pytest.mark.parametrize("nr", [1, 63, 64, 65, 257])
def test_reference_counts(grid_set, nr):
    qs, refs = grid_set
    rs = H.select(refs, list(range(nr)))
    same_rows(H.dist(qs, rs), expected(qs, rs), 1.0)


def test_one_query_many_references():
    """the default `finch dist` shape: the first sketch against all of them"""
    sk = pool_sketches(5001, np.random.default_rng(37), size=100, groups=8)
    rows = H.dist_command(sk)
    assert len(rows) == 5000
    same_rows(rows, expected(sk, sk, pairs=[(0, r) for r in range(5001)]), 1.0)


def test_many_queries_few_references():
    rng = np.random.default_rng(41)
    qs = pool_sketches(2000, rng, size=60, groups=4, prefix="q")
    rs = pool_sketches(3, rng, size=60, groups=4, prefix="r")
    same_rows(H.dist(qs, rs), expected(qs, rs), 1.0)


@pytest.mark.parametrize("devices, chunk, launches", [([0], "10", 20), ([0, 0, 0], "10", 20), ([0, 0, 0], "80", 10)])
def test_chunks_below_the_query_count(devices, chunk, launches):
    """dist_chunk_pairs < queries: one reference per launch; three entries on one device with 20 or 10 chunks"""
    rng = np.random.default_rng(43)
    qs = pool_sketches(40, rng, size=150, groups=4, prefix="q")
    rs = pool_sketches(20, rng, size=150, groups=4, prefix="r")
    st = {}
    try:
        F.set_option("dist_chunk_pairs", chunk)
        rows = H.dist(qs, rs, devices=devices, stats=st)
    finally:
        F.set_option("dist_chunk_pairs", None)
    assert st["launches"] == launches
    same_rows(rows, expected(qs, rs), 1.0)


def hand_sketches():
    qs = collect([mk("q0", [1, 2, 3, 4]), mk("q1", [5, 7, 9])])
    rs = collect([mk("r0", [1, 2, 3, 4]), mk("r1", []), mk("r2", [0, 2, 7, 8])])
    return qs, rs


def test_the_current_device_is_left_alone():
    """(tells a call that leaves the device changed only where there is a second GPU: with one, the last device is device 0)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    qs, rs = hand_sketches()
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    rows = H.dist(qs, rs, devices=(F.device_count() - 1,))
    assert len(rows) == 6
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before


@pytest.mark.parametrize("devices, chunk, launches", [((0, 0, 0), None, 1), ((0, 0), "2", 3)])
def test_more_device_entries_than_chunks(devices, chunk, launches):
    """2 queries x 3 references: one chunk for three entries; then three chunks of one reference dealt over two entries.  The
    rows are the single entry's, byte for byte"""
    qs, rs = hand_sketches()
    one = H.dist(qs, rs, devices=(0,))
    same_rows(one, expected(qs, rs), 1.0)
    assert list(zip(one["reference"].tolist(), one["query"].tolist())) == [(r, q) for r in range(3) for q in range(2)]
    st = {}
    try:
        F.set_option("dist_chunk_pairs", chunk)
        rows = H.dist(qs, rs, devices=devices, stats=st)
    finally:
        F.set_option("dist_chunk_pairs", None)
    assert st["launches"] == launches
    assert rows.dtype == one.dtype and rows.tobytes() == one.tobytes()
