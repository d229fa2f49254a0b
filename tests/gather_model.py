"""The contract of finch_gather (include/finch_host.h), stated twice: with Python sets, as the contract reads, and
with sorted arrays plus a bitmask, as the device works.  tests/test_gather_model.py holds the two to each other.

gather(Q, refs, min_overlap, max_rounds) for one query sketch Q and a library refs[0 .. R):
  * min_overlap below 1 is taken as 1; max_rounds = 0 means no cap;
  * S_0 = the set of Q's hashes -- plain set semantics over the hashes as stored: no max_hash cut, no early stop of a merge
    walk.  This is deliberately NOT raw_distance's walk (dist_model.py);
  * round t: c_j(t) = |S_t n H_j|; the winner w has the largest c_j(t), among equal counts the smallest j; stop if
    c_w(t) < min_overlap, or if t == max_rounds and max_rounds > 0; otherwise one row, and S_{t+1} = S_t \\ H_w.

A sketch is a Sk: ascending distinct hashes, and the counts that go with them (the query's are what `abund` sums).  A row is a
dict of the nine integers and five doubles of finch_gather_row; the doubles are plain divisions, an IEEE result where Python
raises (x / 0)."""
import math

INTS = ("query", "reference", "round", "overlap", "common", "ref_len", "query_len", "abund", "remaining")
DOUBLES = ("f_unique_to_query", "f_orig_query", "f_match", "average_abund", "f_unique_weighted")
U64 = (1 << 64) - 1


class Sk:
    def __init__(self, hashes, counts=None):
        self.hashes = [int(h) for h in hashes]
        self.counts = [1] * len(self.hashes) if counts is None else [int(c) for c in counts]
        assert len(self.counts) == len(self.hashes)
        assert all(a < b for a, b in zip(self.hashes, self.hashes[1:])), "hashes ascend strictly"


def ieee_div(a, b):
    """float(a) / float(b) as IEEE 754 has it"""
    a, b = float(a), float(b)
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a)
    return a / b


def finish(row, query_count_sum):
    """the five doubles from a row's integers: the one function both statements use, as the library's two entry points do"""
    row["f_unique_to_query"] = ieee_div(row["overlap"], row["query_len"])
    row["f_orig_query"] = ieee_div(row["common"], row["query_len"])
    row["f_match"] = ieee_div(row["common"], row["ref_len"])
    row["average_abund"] = ieee_div(row["abund"], row["overlap"])
    row["f_unique_weighted"] = ieee_div(row["abund"], query_count_sum)
    return row


def gather_sets(query, refs, min_overlap=1, max_rounds=0, iq=0, trace=None):
    """the contract with Python sets.  `trace`, a list, receives every round's counts [c_0(t) .. c_{R-1}(t)], the round that stops
    included"""
    min_overlap = max(1, min_overlap)
    count_of = dict(zip(query.hashes, query.counts))
    total = sum(query.counts) & U64
    s = set(query.hashes)
    sets = [set(r.hashes) for r in refs]
    c0 = [len(s & h) for h in sets]
    rows = []
    t = 0
    while True:
        c = [len(s & h) for h in sets]
        if trace is not None:
            trace.append(c)
        if not c:
            break
        w = max(range(len(c)), key=lambda j: (c[j], -j))
        if c[w] < min_overlap or (max_rounds > 0 and t == max_rounds):
            break
        taken = s & sets[w]
        s = s - sets[w]
        rows.append(finish({"query": iq, "reference": w, "round": t, "overlap": c[w], "common": c0[w], "ref_len": len(sets[w]),
                            "query_len": len(query.hashes), "abund": sum(count_of[h] for h in taken) & U64, "remaining": len(s)}, total))
        t += 1
    return rows


def positions(query, ref):
    """the indices into query.hashes of the hashes the two share, ascending: a merge of two ascending lists"""
    out, i, j = [], 0, 0
    q, r = query.hashes, ref.hashes
    while i < len(q) and j < len(r):
        if q[i] < r[j]:
            i += 1
        elif r[j] < q[i]:
            j += 1
        else:
            out.append(i)
            i += 1
            j += 1
    return out


def gather_mask(query, refs, min_overlap=1, max_rounds=0, iq=0):
    """the device's form: only candidates (c_j(0) >= min_overlap) have any state -- their positions in the query, made once --;
    the remaining set is a bitmask over query positions; a candidate whose last count is below min_overlap, or cannot beat the
    best count of the round so far, is not counted again (counts never grow); the loop is bounded by the candidates"""
    min_overlap = max(1, min_overlap)
    total = sum(query.counts) & U64
    cands = []  # [reference, positions, last count], by reference
    for j, r in enumerate(refs):
        p = positions(query, r)
        if len(p) >= min_overlap:
            cands.append([j, p, len(p)])
    n = len(query.hashes)
    mask = (1 << n) - 1
    remaining = n
    bound = min(max_rounds, len(cands)) if max_rounds > 0 else len(cands)
    rows = []
    for t in range(bound):
        best_c, best = 0, None
        for cand in cands:
            if cand[2] < min_overlap or cand[2] <= best_c:
                continue
            cand[2] = sum((mask >> p) & 1 for p in cand[1])
            if cand[2] >= min_overlap and cand[2] > best_c:
                best_c, best = cand[2], cand
        if best is None:
            break
        abund = 0
        for p in best[1]:
            if (mask >> p) & 1:
                mask &= ~(1 << p)
                abund += query.counts[p]
        remaining -= best_c
        rows.append(finish({"query": iq, "reference": best[0], "round": t, "overlap": best_c, "common": len(best[1]),
                            "ref_len": len(refs[best[0]].hashes), "query_len": n, "abund": abund & U64, "remaining": remaining}, total))
    return rows


def gather(queries, refs, min_overlap=1, max_rounds=0):
    """per query its rows; queries are independent"""
    return [gather_sets(q, refs, min_overlap, max_rounds, iq) for iq, q in enumerate(queries)]


def offsets(per_query):
    out = [0]
    for rows in per_query:
        out.append(out[-1] + len(rows))
    return out


def n_candidates(queries, refs, min_overlap=1):
    """the pairs with c_j(0) >= min_overlap"""
    min_overlap = max(1, min_overlap)
    return sum(1 for q in queries for r in refs if len(set(q.hashes) & set(r.hashes)) >= min_overlap)
