"""A model of the clustering contract (finch_index_cluster / finch_cluster_host, include/finch_host.h) in plain
Python.  `cluster` is the contract as written: tests/dist_model.py's literal loop over every ordered pair q != r -- no name-based
skip --, the test `mash_distance <= max_distance`, then a union-find whose labels are each component's smallest index.  `bands`
follows the path the library takes through the index -- the pairs that share a hash, the device's jaccard and its two bounds --
and counts what the device unites, drops and sends to the host.  It does not import finch_rs_amd."""
import math
from bisect import bisect_left, bisect_right

import dist_model as M
import index_dist_model as IDM
import index_model as IM

MARGIN_DEFAULT = 2.0 ** -20


def mash_distance(jaccard: float, k: int) -> float:
    """dist_model.mash_distance, and for k = 0 the IEEE division Python refuses: -ln / 0 is NaN for ln = 0 and +inf otherwise,
    f64::max ignores the NaN"""
    if k != 0:
        return M.mash_distance(jaccard, k)
    x = (2.0 * jaccard) / (1.0 + jaccard)
    if x == 1.0:
        return 0.0  # min(1, max(0, NaN))
    return 1.0 if x < 1.0 else 0.0  # min(1, max(0, +inf)); x > 1 never happens for a jaccard in [0, 1]


def jlo(k: int, max_distance: float) -> float:
    """finch_index_dist's jmin, unchanged"""
    return IDM.jmin(k, max_distance)


def jhi(k: int, max_distance: float, m: float = MARGIN_DEFAULT) -> float:
    """x / (2 - x) * (1 + m), x = exp(-k d); +inf where that is no normal positive number"""
    x = math.exp(-float(k) * max(max_distance, 0.0))
    v = x / (2.0 - x) * (1.0 + m)
    return v if v >= 2.0 ** -1022 and v != math.inf else math.inf


def labels_of(n, pairs):
    """the smallest index of each component of the graph on 0 .. n - 1 with these edges"""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    for a, b in pairs:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(v) for v in range(n)]


def passing(sketches, old_mode=False, max_distance=0.1):
    """the ordered pairs (q, r), q != r, that pass: the literal loop"""
    if old_mode and any(len(s.hashes) == 0 for s in sketches) and any(len(s.hashes) for s in sketches):
        raise M.ReferencePanics("old_distance indexes an empty query sketch")
    if not max_distance >= 0.0:
        return []
    out = []
    for r in range(len(sketches)):
        for q in range(len(sketches)):
            if q != r and M.distance(sketches[q], sketches[r], old_mode, walk=True, pinned=True)["mash_distance"] <= max_distance:
                out.append((q, r))
    return out


def cluster(sketches, old_mode=False, max_distance=0.1):
    """(labels, edges): labels[v] = the smallest index of v's component, edges = the ordered pairs q != r that pass"""
    pairs = passing(sketches, old_mode, max_distance)
    return labels_of(len(sketches), pairs), len(pairs)


def bands(sketches, old_mode=False, max_distance=0.1, m=MARGIN_DEFAULT):
    """what the device does with the pairs that share a hash: dict(touched, united, copied, kept_host) as finch_cluster_stats
    counts them (united and kept_host: q != r only; a self pair has jaccard 1 and neither crosses nor counts)"""
    table = IM.postings(sketches)
    ints = [[int(x) for x in s.hashes] for s in sketches]  # (once: index_model.closed_counts converts per pair)
    out = dict(touched=0, united=0, copied=0, kept_host=0)
    for q, query in enumerate(sketches):
        lo, hi = jlo(query.k, max_distance), jhi(query.k, max_distance, m)
        for r, c in IM.shared(table, query).items():
            out["touched"] += 1
            if old_mode:
                i, j = len(sketches[r].hashes), 0
            else:
                Q, R = ints[q], ints[r]  # index_model.closed_counts
                i, j = bisect_right(Q, R[-1]), bisect_right(R, Q[-1])
                scale = M.min_scale(query, sketches[r])
                if scale > 0.0:
                    top = M.max_hash(scale)
                    i, j = max(i, bisect_left(Q, top)), max(j, bisect_left(R, top))
            jac = IDM.device_jaccard(old_mode, c, i, j)
            if jac >= hi or jac == 1.0:
                out["united"] += q != r
            elif jac >= lo:
                out["copied"] += 1
                d = IDM.row_from_counts(query, old_mode, c, i, j)["mash_distance"]
                out["kept_host"] += q != r and d <= max_distance
    return out
