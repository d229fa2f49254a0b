"""tests/index_model.py -- the postings, the shared-hash counts and the closed forms for i and j -- against raw_distance's literal
walk (search_model.pair_counts(..., walk=True)) and against search_model.search, on random sketches from small pools: Mash
sketches, Scaled sketches of different scales, a NaN scale, empty sketches.  This pins the reduction the index kernels rely on,
not the library."""
import math

import numpy as np

import dist_model as M
import index_model as IM
import search_model as SM

SCALES = (0.5, 0.25, 0.1, math.nan)


def random_sketch(rng, pool):
    n = int(rng.integers(0, 10)) if rng.random() < 0.85 else 0
    hs = sorted(int(x) for x in rng.choice(pool, size=min(n, len(pool)), replace=False))
    if rng.random() < 0.6:
        scale = float(SCALES[int(rng.integers(0, len(SCALES)))])
        if scale == scale:  # a Scaled sketch holds hashes below its max hash; half of them do here, the rest are as loaded from a file
            if rng.random() < 0.5:
                hs = [h for h in hs if h < M.max_hash(scale)]
        return M.Sk(hs, "scaled", scale, 21)
    return M.Sk(hs, "mash", 0.0, int(rng.choice([15, 21])))


def random_sets(seed):
    rng = np.random.default_rng(seed)
    if seed % 3 == 0:  # values either side of the max hashes (u64::MAX / 2, / 4, / 10)
        pool = np.array([0, 1, 5, M.U64_MAX // 10 - 1, M.U64_MAX // 10, M.U64_MAX // 10 + 1, M.U64_MAX // 4 - 1, M.U64_MAX // 4,
                         M.U64_MAX // 4 + 1, M.U64_MAX // 2 - 1, M.U64_MAX // 2, M.U64_MAX // 2 + 7, M.U64_MAX - 1, M.U64_MAX], np.uint64)
    elif seed % 3 == 1:  # a few values: ties everywhere
        pool = np.arange(1, 12, dtype=np.uint64) * 3
    else:
        pool = np.unique(rng.integers(0, M.U64_MAX, 16, dtype=np.uint64))
    refs = [random_sketch(rng, pool) for _ in range(int(rng.integers(0, 10)))]
    queries = [random_sketch(rng, pool) for _ in range(int(rng.integers(1, 5)))]
    return queries, refs


def test_postings_ascend_and_count_the_shared_hashes():
    refs = [M.Sk([1, 5, 9]), M.Sk([]), M.Sk([5]), M.Sk([1, 5, 7])]
    table = IM.postings(refs)
    assert table == {1: [0, 3], 5: [0, 2, 3], 9: [0], 7: [3]}
    assert IM.shared(table, M.Sk([5, 7, 8])) == {0: 1, 2: 1, 3: 2}
    assert IM.shared(table, M.Sk([])) == {} and IM.shared(table, M.Sk([2, 3])) == {}


def test_closed_forms_equal_the_walk():
    seen = {"scaled_pair": 0, "step_moves_j": 0, "nan_scale": 0, "empty": 0, "scales_differ": 0, "pairs": 0, "shared_nothing": 0}
    for seed in range(300):
        queries, refs = random_sets(seed)
        table = IM.postings(refs)
        for q in queries:
            cnt = IM.shared(table, q)
            for r, ref in enumerate(refs):
                want = SM.pair_counts(q, ref, walk=True)
                seen["empty"] += not len(q.hashes) or not len(ref.hashes)
                if r not in cnt:
                    assert want[0] == 0, (seed, r)  # what the index does not reach has containment 0
                    seen["shared_nothing"] += 1
                    continue
                assert IM.closed_counts(q, ref, cnt[r]) == want, (seed, r)
                seen["pairs"] += 1
                both = q.kind == ref.kind == "scaled"
                seen["scaled_pair"] += both
                seen["nan_scale"] += both and (q.scale != q.scale or ref.scale != ref.scale)
                seen["scales_differ"] += both and q.scale == q.scale and ref.scale == ref.scale and q.scale != ref.scale
                seen["step_moves_j"] += want[2] != M.walk_counts(q.hashes, ref.hashes, 0.0)[2]
    assert all(v >= 20 for v in seen.values()), seen


def test_search_equals_the_dense_model():
    for seed in range(120):
        queries, refs = random_sets(seed)
        conts = sorted({float(SM.containment(c, j)) for q in queries for ref in refs for c, _, j in [SM.pair_counts(q, ref)]} - {0.0})
        thresholds = [5e-324, 0.1, 1.0, math.nan, math.inf] + conts[:2] + [math.nextafter(x, math.inf) for x in conts[:2]]
        n_shared = sum(SM.pair_counts(q, ref)[0] > 0 for q in queries for ref in refs)
        for minc in thresholds:
            for top_n in (0, 1, 3):
                found, touched, passing = IM.search(queries, refs, minc, top_n)
                assert found == SM.search(queries, refs, minc, top_n, walk=True), (seed, minc, top_n)
                assert touched == n_shared
                assert passing == sum(len(ws) for ws in SM.search(queries, refs, minc, 0))
