"""An independent model of the library search (finch_search, include/finch_host.h) and of the two loops it stands for,
Multisketch.best_match and Multisketch.filter_to_matches (lib/src/python.rs:202-234), in Python integers and Fractions on top of
tests/dist_model.py's raw_distance counts and scale choice.  It does not import finch_rs_amd.

The contract it writes down: the rows of query q are the references r with containment(q, r) >= min_containment, ordered by
containment descending and, among equal containments, by reference index ascending; the first top_n of them if top_n > 0.  No
pair is skipped, there is no old mode.  A containment is c / j of the merge walk (0 where j = 0): kept here as a Fraction, so
that thresholds and ties are decided exactly, and turned into the double the library must return -- the exactly rounded
quotient -- only for the order, which the contract states on doubles."""
import math
from fractions import Fraction

import dist_model as M


def pair_counts(query: M.Sk, ref: M.Sk, walk: bool = False, pinned: bool = False):
    """(common, i, j) of distance(query, ref, false): raw_distance's walk with distance()'s choice of scale"""
    scale = M.min_scale(query, ref)
    if walk:
        return M.walk_counts(query.hashes, ref.hashes, scale, pinned)
    return M.counts(query.hashes, ref.hashes, M.max_hash(scale, pinned) if scale > 0.0 else None)


def containment(c: int, j: int) -> Fraction:
    return Fraction(0) if j == 0 else Fraction(c, j)


def passes(cont: Fraction, min_containment: float) -> bool:
    """`containment >= min_containment` on doubles, decided exactly: the containment's double is its exactly rounded value"""
    if min_containment != min_containment:
        return False
    if math.isinf(min_containment):
        return min_containment < 0
    return Fraction(float(cont)) >= Fraction(min_containment)


def row(query: M.Sk, c: int, i: int, j: int) -> dict:
    cont, jac, common, total = M.raw_from_counts(c, i, j)
    return {"containment": cont, "jaccard": jac, "mash_distance": M.mash_distance(jac, query.k), "common_hashes": common,
            "total_hashes": total}


def search(queries, refs, min_containment: float = 0.0, top_n: int = 0, walk: bool = False, pinned: bool = False):
    """per query the list of (reference index, row dict), in the contract's order"""
    out = []
    for q in queries:
        cands = []
        for r, ref in enumerate(refs):
            c, i, j = pair_counts(q, ref, walk, pinned)
            cont = containment(c, j)
            if passes(cont, min_containment):
                cands.append((-float(cont), r, row(q, c, i, j)))  # (the order is stated on the doubles)
        cands.sort(key=lambda x: (x[0], x[1]))
        if top_n > 0:
            cands = cands[:top_n]
        out.append([(r, d) for _, r, d in cands])
    return out


def offsets(found):
    o = [0]
    for rows in found:
        o.append(o[-1] + len(rows))
    return o


class EmptyLibrary(Exception):
    """best_match on a library without sketches: the reference indexes sketches[0] and panics"""


def best_match(refs, query: M.Sk, walk: bool = False) -> int:
    """the search's statement of best_match: the first row of a top-1 search with threshold 0"""
    if not refs:
        raise EmptyLibrary()
    return search([query], refs, 0.0, 1, walk)[0][0][0]


def filter_to_matches(refs, query: M.Sk, threshold: float, walk: bool = False):
    """the search's statement of filter_to_matches: the references of an untruncated search, back in library order"""
    return sorted(r for r, _ in search([query], refs, threshold, 0, walk)[0])
