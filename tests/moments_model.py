"""The contract of compare_counts (finch_compare_counts / finch_compare_counts_pair, include/finch_host.h),
stated twice.  It does not import finch_rs_amd.

A sketch here is a list of (hash, count) with strictly ascending hashes; count is a u32.  For a reference sketch R and a query
sketch Q, Sketch.compare_counts (lib/src/python.rs:496-559) returns
    (common, ref_pos, query_pos, ref_count, query_count, var, skew, kurt).

1. `compare_counts` is the reference's loop as written: the merge walk, and for every shared hash, in ascending hash order, the
   recurrence of python.rs:524-535 -- n, delta, delta_n, delta_n2, term1, then the updates of mean, m4, m3, m2 in that order and
   with that association -- in IEEE doubles with no fused multiply-add (numpy.float64 scalars: one rounding per operation), and
   the three finishing doubles var = m2 / common, skew = sqrt(common) * m3 / pow(m2, 1.5), kurt = common * m4 / (m2 * m2) - 3.
   common = 0, common = 1 or all shared counts equal give NaNs, as the reference does (numpy's errstate is relaxed: Python's
   own 0.0 / 0.0 raises).
2. `integers` states the five integers without a walk, on sets: common = |Q n R|, ref_pos = #{r <= max Q}, query_pos =
   #{q <= max R} (both 0 if either sketch is empty), ref_count / query_count = the summed counts of the shared hashes; and
   `central_sums` states what the recurrence computes, exactly, in Fractions: n, the mean and the sums of (x - mean)^k for
   k = 2, 3, 4 over the query's counts of the shared hashes.

Comparisons (`same`): integers are equal, doubles are equal as bit patterns, two NaNs of any sign or payload are equal."""
import struct
from fractions import Fraction

import numpy as np

F64 = np.float64
COUNTS = (1, 2, 3, 2 ** 32 - 1)


def walk_sums(ref, query):
    """python.rs:500-543 -> (common, ref_pos, query_pos, ref_count, query_count, m2, m3, m4)"""
    common = 0
    ref_pos = 0
    ref_count = 0
    query_pos = 0
    query_count = 0
    query_mean = F64(0.0)
    query_m2 = F64(0.0)
    query_m3 = F64(0.0)
    query_m4 = F64(0.0)
    with np.errstate(all="ignore"):
        while ref_pos < len(ref) and query_pos < len(query):
            if ref[ref_pos][0] < query[query_pos][0]:
                ref_pos += 1
            elif query[query_pos][0] < ref[ref_pos][0]:
                query_pos += 1
            else:
                ref_count += ref[ref_pos][1]
                query_count += query[query_pos][1]
                n = F64(common) + F64(1.0)
                float_count = F64(query[query_pos][1])
                delta = float_count - query_mean
                delta_n = delta / n
                delta_n2 = delta_n * delta_n
                term1 = delta * delta_n * (n - F64(1.0))
                query_mean = query_mean + delta_n
                query_m4 = query_m4 + (term1 * delta_n2 * (n * n - F64(3.0) * n + F64(3.0)) + F64(6.0) * delta_n2 * query_m2
                                       - F64(4.0) * delta_n * query_m3)
                query_m3 = query_m3 + (term1 * delta_n * (n - F64(2.0)) - F64(3.0) * delta_n * query_m2)
                query_m2 = query_m2 + term1
                ref_pos += 1
                query_pos += 1
                common += 1
    return common, ref_pos, query_pos, ref_count, query_count, query_m2, query_m3, query_m4


def finish(common, m2, m3, m4):
    """python.rs:545-547 -> (var, skew, kurt)"""
    with np.errstate(all="ignore"):
        c = F64(common)
        var = F64(m2) / c
        skew = np.sqrt(c) * F64(m3) / (F64(m2) ** F64(1.5))
        kurt = c * F64(m4) / (F64(m2) * F64(m2)) - F64(3.0)
    return var, skew, kurt


def compare_counts(ref, query):
    """the reference's tuple: (common, ref_pos, query_pos, ref_count, query_count, var, skew, kurt)"""
    common, ref_pos, query_pos, ref_count, query_count, m2, m3, m4 = walk_sums(ref, query)
    return (common, ref_pos, query_pos, ref_count, query_count) + finish(common, m2, m3, m4)


def integers(ref, query):
    """the five integers on sets, without a walk"""
    r, q = dict(ref), dict(query)
    assert len(r) == len(ref) and len(q) == len(query)
    shared = set(r) & set(q)
    if not r or not q:
        ref_pos = query_pos = 0
    else:
        ref_pos = sum(1 for h in r if h <= max(q))
        query_pos = sum(1 for h in q if h <= max(r))
    return len(shared), ref_pos, query_pos, sum(r[h] for h in shared), sum(q[h] for h in shared)


def central_sums(ref, query):
    """(n, mean, S2, S3, S4) in Fractions: Sk = the sum of (x - mean)^k over the query's counts x of the shared hashes; None if
    nothing is shared"""
    r = dict(ref)
    xs = [Fraction(c) for h, c in query if h in r]
    if not xs:
        return None
    mean = sum(xs) / len(xs)
    return (len(xs), mean) + tuple(sum((x - mean) ** k for x in xs) for k in (2, 3, 4))


def bits(x):
    return struct.pack("<d", float(x))


def same_double(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or bits(a) == bits(b)


def same(a, b):
    """two 8-tuples under the contract's comparison"""
    return (len(a) == len(b) == 8 and all(int(x) == int(y) for x, y in zip(a[:5], b[:5])) and
            all(same_double(x, y) for x, y in zip(a[5:], b[5:])))


def rows(refs, queries, min_common=0):
    """finch_compare_counts' rows: [(query index, reference index, 8-tuple)] for the pairs with common >= min_common, by
    query, then by reference index"""
    out = []
    for q, query in enumerate(queries):
        for r, ref in enumerate(refs):
            t = compare_counts(ref, query)
            if t[0] >= min_common:
                out.append((q, r, t))
    return out
