"""A model of the index search (finch_index_search, include/finch_host.h) in plain Python: the library's postings
as a dict hash -> references, the shared-hash count c of the pairs the postings reach, and i and j of raw_distance's walk in
closed form from each side's last hash and the pair's max hash -- the reduction DESIGN.md §3.7 states and the index kernels rely
on.  It does not import finch_rs_amd, and takes from tests/dist_model.py only the choice of a pair's scale and its max hash;
tests/test_index_model.py holds it to the literal walk."""
from bisect import bisect_left, bisect_right
from fractions import Fraction

import dist_model as M
import search_model as SM


def postings(refs):
    """hash -> the references that hold it, ascending (references are visited in order)"""
    table = {}
    for r, ref in enumerate(refs):
        for h in ref.hashes:
            table.setdefault(int(h), []).append(r)
    return table


def shared(table, query: M.Sk):
    """reference -> c = |Q n R| for the references with c > 0: one increment per posting of every query hash"""
    cnt = {}
    for h in query.hashes:
        for r in table.get(int(h), ()):
            cnt[r] = cnt.get(r, 0) + 1
    return cnt


def closed_counts(query: M.Sk, ref: M.Sk, c: int):
    """(c, i, j) of the walk for a pair that shares c > 0 hashes: i0 = #{q <= max R}, j0 = #{r <= max Q}, and where the pair has
    a scale > 0 the step to #{q < M}, #{r < M}"""
    Q, R = [int(x) for x in query.hashes], [int(x) for x in ref.hashes]
    assert c > 0 and Q and R
    i, j = bisect_right(Q, R[-1]), bisect_right(R, Q[-1])
    scale = M.min_scale(query, ref)
    if scale > 0.0:
        m = M.max_hash(scale)
        i, j = max(i, bisect_left(Q, m)), max(j, bisect_left(R, m))
    return c, i, j


def search(queries, refs, min_containment: float, top_n: int = 0):
    """(found, touched, passing): found as search_model.search gives it, for a threshold above 0; touched = the pairs with
    c > 0 (what the device counts), passing = those of them whose containment passes (what crosses to the host)"""
    assert min_containment > 0 or min_containment != min_containment
    table = postings(refs)
    found, touched, passing = [], 0, 0
    for q in queries:
        cands = []
        for r, c in shared(table, q).items():
            touched += 1
            c, i, j = closed_counts(q, refs[r], c)
            cont = Fraction(c, j)
            if SM.passes(cont, min_containment):
                passing += 1
                cands.append((-float(cont), r, SM.row(q, c, i, j)))
        cands.sort(key=lambda x: (x[0], x[1]))
        if top_n > 0:
            cands = cands[:top_n]
        found.append([(r, d) for _, r, d in cands])
    return found, touched, passing
