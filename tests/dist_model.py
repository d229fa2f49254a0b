"""An independent model of the reference's sketch distances (lib/src/distance.rs and calc_sketch_distances,
cli/src/main.rs:315-333), written in Python integers and numpy from the reference's text.  It does not import finch_rs_amd:
the tests hold both of the library's paths (finch_distance on the host, finch_dist on the device) to it.

Hashes are ascending sequences of u64 (lists of int or numpy uint64 arrays).  A sketch is an `Sk`: its hashes, its
variant ("mash" or "scaled"; only the Scaled variant has a scale, SketchParams::hash_info) and its k.

Where the reference panics (a zero divisor in the scale step: scale > 1 or +inf; old_distance indexing an empty query) the
model raises ReferencePanics.  The library's documented behaviour for the scale panic (M = u64::MAX) is available with
`pinned=True`; it is the library's choice, not a reference result."""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

U64_MAX = (1 << 64) - 1


class ReferencePanics(Exception):
    """the reference would panic here"""


@dataclass
class Sk:
    hashes: object
    kind: str = "mash"
    scale: float = 0.0
    k: int = 21

    def hash_scale(self):
        """SketchParams::hash_info().3"""
        return self.scale if self.kind == "scaled" else None


def as_u64(x: float) -> int:
    """Rust's `x as u64`: truncation toward zero; NaN and values below 1 give 0; values >= 2^64 give u64::MAX"""
    if x != x or x < 1.0:
        return 0
    if x >= 2.0 ** 64:
        return U64_MAX
    return int(x)


def max_hash(scale: float, pinned: bool = False) -> int:
    """`u64::MAX / scale.recip() as u64` (raw_distance's scale step): the cast binds tighter than the division"""
    d = as_u64(1.0 / scale)
    if d == 0:
        if pinned:
            return U64_MAX
        raise ReferencePanics("attempt to divide by zero (scale %r)" % scale)
    return U64_MAX // d


def f64_min(a: float, b: float) -> float:
    """Rust's f64::min: a NaN argument is ignored"""
    if a != a:
        return b
    if b != b:
        return a
    return b if b < a else a


def f64_max(a: float, b: float) -> float:
    """Rust's f64::max: a NaN argument is ignored (of +0.0 and -0.0 this returns the first)"""
    if a != a:
        return b
    if b != b:
        return a
    return b if b > a else a


def ratio(n: int, d: int) -> float:
    """`n as f64 / d as f64` for counts below 2^53: the exactly rounded quotient; 0 / 0 is NaN"""
    if d == 0:
        return math.nan if n == 0 else math.inf
    return float(Fraction(n, d))


# ----------------------------------------------------------------------------------------------------------------------
# the literal walks
# ----------------------------------------------------------------------------------------------------------------------

def walk_counts(query, ref, scale: float, pinned: bool = False):
    """raw_distance's merge walk and scale step, one hash at a time: (common, i, j)"""
    q, r = [int(x) for x in query], [int(x) for x in ref]
    i = j = common = 0
    while i < len(q) and j < len(r):
        if q[i] < r[j]:
            i += 1
        elif q[i] > r[j]:
            j += 1
        else:
            common += 1
            i += 1
            j += 1
    if scale > 0.0:
        m = max_hash(scale, pinned)
        while i < len(q) and q[i] < m:
            i += 1
        while j < len(r) and r[j] < m:
            j += 1
    return common, i, j


def raw_from_counts(common: int, i: int, j: int):
    """the tail of raw_distance: (containment, jaccard, common, total)"""
    containment = 0.0 if j == 0 else ratio(common, j)
    total = i - common + j
    jaccard = 1.0 if total == 0 else ratio(common, total)
    return containment, jaccard, common, total


def raw_distance(query, ref, scale: float, pinned: bool = False):
    """distance.rs raw_distance: (containment, jaccard, common, total)"""
    return raw_from_counts(*walk_counts(query, ref, scale, pinned))


def old_walk_counts(query, ref):
    """old_distance's loop as written, the `i < len - 1` clamp included: (common, total)"""
    q, r = [int(x) for x in query], [int(x) for x in ref]
    i = common = total = 0
    for h in r:
        if not q:
            raise ReferencePanics("old_distance indexes an empty query sketch")
        while q[i] < h and i < len(q) - 1:
            i += 1
        if q[i] == h:
            common += 1
        total += 1
    return common, total


def old_from_counts(common: int, total: int):
    return ratio(common, total), ratio(common, common + 2 * (total - common)), common, total


def old_distance(query, ref):
    """distance.rs old_distance: (containment, jaccard, common, total)"""
    return old_from_counts(*old_walk_counts(query, ref))


# ----------------------------------------------------------------------------------------------------------------------
# the same counts without the walk, for large sets; trusted only because tests/test_dist_model.py holds them to the walks
# ----------------------------------------------------------------------------------------------------------------------

def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def counts(query, ref, m=None):
    """(common, i, j) of walk_counts for strictly ascending hashes; m = the scale step's max hash, or None for no step"""
    Q, R = _u64(query), _u64(ref)
    c = len(np.intersect1d(Q, R, assume_unique=True))
    i = j = 0
    if len(Q) and len(R):
        i = int(np.searchsorted(Q, R[-1], "right"))
        j = int(np.searchsorted(R, Q[-1], "right"))
    if m is not None:
        i = max(i, int(np.searchsorted(Q, np.uint64(m), "left")))
        j = max(j, int(np.searchsorted(R, np.uint64(m), "left")))
    return c, i, j


def old_counts(query, ref):
    """(common, total) of old_walk_counts for strictly ascending hashes"""
    Q, R = _u64(query), _u64(ref)
    if len(R) and not len(Q):
        raise ReferencePanics("old_distance indexes an empty query sketch")
    return len(np.intersect1d(Q, R, assume_unique=True)), len(R)


# ----------------------------------------------------------------------------------------------------------------------
# distance() and calc_sketch_distances
# ----------------------------------------------------------------------------------------------------------------------

def mash_distance(jaccard: float, k: int) -> float:
    """distance()'s `-1.0 * ((2.0 * jaccard) / (1.0 + jaccard)).ln() / k`, clamped by f64::max and f64::min"""
    x = (2.0 * jaccard) / (1.0 + jaccard)
    ln = -math.inf if x == 0.0 else math.log(x)  # (math.log refuses 0; ln(0) is -inf; x is never negative)
    md = -1.0 * ln / float(k)
    return f64_min(1.0, f64_max(0.0, md))


def min_scale(query: Sk, ref: Sk) -> float:
    """distance()'s choice of scale: f64::min of the two when both sketches have one, else 0"""
    s1, s2 = query.hash_scale(), ref.hash_scale()
    if s1 is not None and s2 is not None:
        return f64_min(s1, s2)
    return 0.0


def distance(query: Sk, ref: Sk, old_mode: bool = False, walk: bool = False, pinned: bool = False) -> dict:
    """distance.rs distance(); walk=True runs the literal walks, else the vectorized counts"""
    if old_mode:
        c, total = (old_walk_counts if walk else old_counts)(query.hashes, ref.hashes)
        cont, jac, common, total = old_from_counts(c, total)
    else:
        scale = min_scale(query, ref)
        if walk:
            cij = walk_counts(query.hashes, ref.hashes, scale, pinned)
        else:
            cij = counts(query.hashes, ref.hashes, max_hash(scale, pinned) if scale > 0.0 else None)
        cont, jac, common, total = raw_from_counts(*cij)
    return {"containment": cont, "jaccard": jac, "mash_distance": mash_distance(jac, query.k), "common_hashes": common,
            "total_hashes": total}


def calc_sketch_distances(queries, refs, old_mode=False, max_distance=1.0, equal=None, pairs=None, pinned=False):
    """main.rs calc_sketch_distances: for each reference, for each query, skip the pair if `equal(q, r)` (the sketches'
    PartialEq, by index), keep it if mash_distance <= max_distance.  [(q, r, dict)]; `pairs` restricts the loop to those
    (q, r), in the order given"""
    it = pairs if pairs is not None else ((q, r) for r in range(len(refs)) for q in range(len(queries)))
    out = []
    for q, r in it:
        if equal is not None and equal(q, r):
            continue
        d = distance(queries[q], refs[r], old_mode, pinned=pinned)
        if d["mash_distance"] <= max_distance:
            out.append((q, r, d))
    return out


def rust_eq(a, b):
    """Sketch's derived PartialEq (serialization/mod.rs:45) on two Sketch records (finch_rs_amd.host.Sketch)"""
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
