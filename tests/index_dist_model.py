"""A model of finch dist through the library index (finch_index_dist, include/finch_host.h) in plain Python,
path by path as the library takes it: c only for the pairs the postings reach; (i, j) from bound searches as
tests/index_model.py has them, or old mode's total = |R|; the device's jaccard pre-filter jmin and then the exact test; the
pairs with an empty side, which the host makes itself; the self-skip and the reference-major order.  It does not import
finch_rs_amd; tests/test_index_dist_model.py holds it to tests/dist_model.py's literal loop."""
import math
from bisect import bisect_left

import dist_model as M
import index_model as IM

MARGIN = 1.0 - 2.0 ** -20


def jmin(k: int, max_distance: float) -> float:
    """the device's bound for a query of this k: the jaccard whose distance is max_distance in real numbers, x / (2 - x) with
    x = exp(-k d), lowered by 2^-20 of itself"""
    x = math.exp(-float(k) * max(max_distance, 0.0))
    return x / (2.0 - x) * MARGIN


def device_jaccard(old_mode: bool, c: int, i: int, j: int) -> float:
    """what the finish kernel compares with jmin: distance_from_counts' division (old mode: i = |R|)"""
    if old_mode:
        return M.ratio(c, c + 2 * (i - c))
    total = i - c + j
    return 1.0 if total == 0 else M.ratio(c, total)


def row_from_counts(query: M.Sk, old_mode: bool, c: int, i: int, j: int) -> dict:
    cont, jac, common, total = M.old_from_counts(c, i) if old_mode else M.raw_from_counts(c, i, j)
    return {"containment": cont, "jaccard": jac, "mash_distance": M.mash_distance(jac, query.k), "common_hashes": common,
            "total_hashes": total}


def empty_side_counts(query: M.Sk, ref: M.Sk):
    """(0, i, j) of the walk for a pair with an empty side: only the scale step moves a cursor"""
    i = j = 0
    scale = M.min_scale(query, ref)
    if scale > 0.0:
        m = M.max_hash(scale, pinned=True)
        i, j = bisect_left([int(x) for x in query.hashes], m), bisect_left([int(x) for x in ref.hashes], m)
    return 0, i, j


def dist(queries, refs, old_mode=False, max_distance=0.1, equal=None):
    """(rows, touched, copied, from_device): rows as dist_model.calc_sketch_distances gives them, [(q, r, dict)], for a bound
    below 1; queries=None is pairwise.  touched = the pairs with c > 0, copied = those of them that pass jmin, from_device =
    those of them that are rows"""
    assert not max_distance >= 1.0
    if queries is None:
        queries = refs
    if old_mode and any(len(q.hashes) == 0 for q in queries) and any(len(r.hashes) for r in refs):
        raise M.ReferencePanics("old_distance indexes an empty query sketch")
    if not max_distance >= 0.0 or not queries or not refs:
        return [], 0, 0, 0
    rows = {}

    def keep(q, r, c, i, j):
        if equal is not None and equal(q, r):
            return False
        d = row_from_counts(queries[q], old_mode, c, i, j)
        if d["mash_distance"] <= max_distance:
            assert (r, q) not in rows
            rows[(r, q)] = d
            return True
        return False

    # the host's own pairs: every empty sketch of either side against the other side
    for r, ref in enumerate(refs):
        if len(ref.hashes) == 0:
            for q, query in enumerate(queries):
                keep(q, r, *((0, 0, 0) if old_mode else empty_side_counts(query, ref)))
    if not old_mode:
        for q, query in enumerate(queries):
            if len(query.hashes) == 0:
                for r, ref in enumerate(refs):
                    if len(ref.hashes):
                        keep(q, r, *empty_side_counts(query, ref))
    # the device's: the pairs that share a hash
    table = IM.postings(refs)
    touched = copied = from_device = 0
    for q, query in enumerate(queries):
        bound = jmin(query.k, max_distance)
        for r, c in IM.shared(table, query).items():
            touched += 1
            if old_mode:
                i, j = len(refs[r].hashes), 0
            else:
                _, i, j = IM.closed_counts(query, refs[r], c)
            if device_jaccard(old_mode, c, i, j) >= bound:
                copied += 1
                from_device += keep(q, r, c, i, j)
    return [(q, r, rows[(r, q)]) for r, q in sorted(rows)], touched, copied, from_device
