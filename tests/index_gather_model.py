"""finch_index_gather's form of the gather (include/finch_host.h) in Python: the library's postings sorted by
(hash, reference), one counter per reference raised over the posting runs of the query's hashes, and rounds that take an arg-max
over the candidates' counters and lower, for every hash the winner removes, the counter of every reference in that hash's run.
Nothing is recounted.  tests/test_index_gather_model.py holds it to tests/gather_model.py, the contract.

Why it is exact.  The postings hold every stored hash and both sides ascend strictly, so after the count the counter of r is the
plain count |Q n H_r| = c_r(0).  When round t removes S_t n H_w, each removed hash h is in S_t, and every reference that holds h
has it counted once in its counter: lowering the counters of h's run by one keeps cnt[r] == |S_t n H_r| for every touched r,
candidate or not.  The winner's counter is 0 afterwards; a position is removed at most once, so all rounds together lower no more
postings than the count raised; integer additions commute, so the order in which they land decides nothing."""
from bisect import bisect_left, bisect_right

import gather_model as GM


class Index:
    """the postings of a library: keys ascending, equal keys in ascending reference order; per reference its length"""

    def __init__(self, refs):
        post = sorted((h, j) for j, r in enumerate(refs) for h in r.hashes)
        self.keys = [h for h, _ in post]
        self.vals = [j for _, j in post]
        self.rlen = [len(r.hashes) for r in refs]
        self.hashes = [r.hashes for r in refs]

    def run(self, h):
        """the posting run of hash h: [lo, hi) -- the two bound searches of the count kernel"""
        return bisect_left(self.keys, h), bisect_right(self.keys, h)


def count(ix, query):
    """k_index_count: (cnt, touched, postings counted) -- cnt[r] = |Q n H_r| for every reference that shares a hash, in the order
    the references were first touched"""
    cnt, touched, n = {}, [], 0
    for h in query.hashes:
        lo, hi = ix.run(h)
        for r in ix.vals[lo:hi]:
            if r not in cnt:
                cnt[r] = 0
                touched.append(r)
            cnt[r] += 1
            n += 1
    return cnt, touched, n


def gather_index(ix, query, min_overlap=1, max_rounds=0, iq=0, counted=None, audit=None):
    """the rows of one query.  `counted`: count(ix, query), if the caller has it (it is copied).  `audit`, a dict, receives
    postings (counted), decrements, candidates, and `after`: per round the counters of every touched reference next to the
    remaining set (one flag per query position) -- what the invariant is checked on"""
    min_overlap = max(1, min_overlap)
    cnt, touched, n_post = counted if counted is not None else count(ix, query)
    cnt = dict(cnt)
    cands = sorted((r, cnt[r]) for r in touched if cnt[r] >= min_overlap)  # (r, common) by reference
    total = sum(query.counts) & GM.U64
    n = len(query.hashes)
    mask = [True] * n
    remaining = n
    bound = min(max_rounds, len(cands)) if max_rounds > 0 else len(cands)
    rows, decrements, after = [], 0, []
    for t in range(bound):
        best_c, best = 0, None
        for i, (r, _) in enumerate(cands):  # count descending, then reference ascending: the first of the largest
            if cnt[r] >= min_overlap and cnt[r] > best_c:
                best_c, best = cnt[r], i
        if best is None:
            break
        w, common = cands[best]
        abund = cleared = 0
        for h in ix.hashes[w]:  # the winner's hashes from the library's CSR, each looked up in the query
            p = bisect_left(query.hashes, h)
            if p < n and query.hashes[p] == h and mask[p]:
                mask[p] = False
                abund += query.counts[p]
                cleared += 1
                lo, hi = ix.run(h)
                for r in ix.vals[lo:hi]:
                    assert cnt[r] > 0, "a counter lowered below 0"
                    cnt[r] -= 1
                    decrements += 1
        assert cleared == best_c, "the round removed another number of hashes than the winner's counter said"
        assert cnt[w] == 0, "the winner's counter is not 0 after its round"
        remaining -= best_c
        rows.append(GM.finish({"query": iq, "reference": w, "round": t, "overlap": best_c, "common": common, "ref_len": ix.rlen[w],
                               "query_len": n, "abund": abund & GM.U64, "remaining": remaining}, total))
        if audit is not None:
            after.append(({r: cnt[r] for r in touched}, mask[:]))
    for r in touched:  # the tail: every touched counter, candidates or not
        cnt[r] = 0
    if audit is not None:
        audit.update(postings=n_post, decrements=decrements, candidates=len(cands), after=after, final=cnt)
    return rows


def gather(queries, refs, min_overlap=1, max_rounds=0, ix=None):
    ix = ix or Index(refs)
    return [gather_index(ix, q, min_overlap, max_rounds, iq) for iq, q in enumerate(queries)]
