"""bench.py --dump-outputs without a GPU: the float files hold the sketch exactly (64-bit hashes as two 32-bit halves), and an
output larger than the cap is cut to the same seeded sample of records every time."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _records(n, k, seed):
    rng = np.random.default_rng(seed)
    kc = np.zeros(n, dtype=[("hash", "<u8"), ("count", "<u4"), ("extra_count", "<u4")])
    kc["hash"] = np.sort(rng.integers(0, 2 ** 64, n, dtype=np.uint64, endpoint=False))
    kc["hash"][-1] = 2 ** 64 - 1
    kc["count"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32, endpoint=False)
    kc["extra_count"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32, endpoint=False)
    km = rng.integers(0, 256, (n, k), dtype=np.uint8)
    pos = rng.integers(0, 2 ** 40, n, dtype=np.uint64)
    return kc, km, pos


def test_dump_of_a_sketch_is_exact_and_float(tmp_path):
    bench = _bench()
    kc, km, pos = _records(1000, 21, 1)
    bench.dump_sketch(str(tmp_path), kc, km, pos, 50_000_000_123)
    d = _load(tmp_path)
    assert sorted(d) == ["count", "extra_count", "first_pos", "hash_hi", "hash_lo", "kmer", "total_kmers"]
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    h = (d["hash_hi"].astype(np.uint64) << np.uint64(32)) | d["hash_lo"].astype(np.uint64)
    assert np.array_equal(h, kc["hash"])
    assert np.array_equal(d["count"].astype(np.uint32), kc["count"]) and np.array_equal(d["extra_count"].astype(np.uint32), kc["extra_count"])
    assert np.array_equal(d["kmer"].astype(np.uint8), km) and d["kmer"].dtype == np.float32
    assert np.array_equal(d["first_pos"].astype(np.uint64), pos) and int(d["total_kmers"][0]) == 50_000_000_123


def test_dump_larger_than_the_cap_is_a_fixed_sample(tmp_path):
    bench = _bench()
    n = 700_000  # 700 000 records of k = 31: 133 MB as floats
    kc, km, pos = _records(n, 31, 2)
    per_file = {"file_index": np.arange(1000, dtype=np.int64)}
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"hash": kc["hash"], "count": kc["count"], "kmer": km, "first_pos": pos.astype(np.int64)},
                           per_file)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT + 4096 * len(os.listdir(tmp_path / "a"))  # (+ the .npy headers)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["record_index"].astype(np.int64)
    assert 100_000 < len(idx) < n and np.all(np.diff(idx) > 0)
    h = (a["hash_hi"].astype(np.uint64) << np.uint64(32)) | a["hash_lo"].astype(np.uint64)
    assert np.array_equal(h, kc["hash"][idx]) and np.array_equal(a["kmer"].astype(np.uint8), km[idx])
    assert np.array_equal(a["file_index"], np.arange(1000))  # (the small arrays are written whole)
