"""A model of Sketch.merge (merge_sketches, lib/src/python.rs:24-100) in plain Python, stated twice.

A sketch is here what the merge looks at: a list of records (hash, count, extra_count, kmer) with ascending hashes, and the scale
of its parameters (None unless it is a Scaled sketch).

  merge_pair / fold   the reference's steps as they are written: one walk that stops when either list is exhausted, one record
                      per hash, u32 sums that wrap, then the clip by (size, the first sketch's scale); a group is the left fold
                      in the order given, every step with the same size.
  closed_form         for groups without a scale, what the fold amounts to, with no walk in it: empty if the group has two
                      members or more and any is empty; otherwise the union, with summed counts, of the records whose hash is
                      <= the smallest of the members' last hashes, cut to the first `size`.  A hash held by several members
                      takes the k-mer of the earliest.

With a scale there is no such form: a record of a later member that lies above the clipped accumulator's last hash is dropped
although it is <= max_hash, so the result depends on the order of the members (test_merge_model.py pins an example)."""

import math

U32 = 2 ** 32
U64 = 2 ** 64


def scale_divisor(scale):
    """(1. / scale) as u64: Rust's saturating cast (NaN and negatives give 0)"""
    if scale != scale:
        return 0
    if scale == 0:
        return U64 - 1 if math.copysign(1.0, scale) > 0 else 0  # 1 / 0. = inf, 1 / -0. = -inf
    inv = 1.0 / scale
    if inv != inv or inv <= 0:
        return 0
    if inv >= 18446744073709551616.0:
        return U64 - 1
    return int(inv)


def max_hash(scale):
    """u64::MAX / ((1. / scale) as u64); None where the reference panics (the divisor is 0)"""
    d = scale_divisor(scale)
    return None if d == 0 else (U64 - 1) // d


def clip(records, size, scale):
    """python.rs:70-97"""
    if scale is not None:
        mh = max_hash(scale)
        if mh is None:
            raise ZeroDivisionError("(1. / scale) as u64 is 0")
        out = []
        for ix, r in enumerate(records):
            if not (r[0] <= mh or (size is not None and ix < size)):
                break
            out.append(r)
        return out
    return list(records) if size is None else list(records[:size])


def walk(first, second):
    """python.rs:44-67: stops when either list is exhausted"""
    out, i, j = [], 0, 0
    while i < len(first) and j < len(second):
        a, b = first[i], second[j]
        if a[0] < b[0]:
            out.append(a)
            i += 1
        elif b[0] < a[0]:
            out.append(b)
            j += 1
        else:
            out.append((a[0], (a[1] + b[1]) % U32, (a[2] + b[2]) % U32, a[3]))
            i += 1
            j += 1
    return out


def merge_pair(first, second, size=None, scale=None):
    """the hashes of merge_sketches(first, second, size); scale: the FIRST sketch's, None unless it is Scaled"""
    return clip(walk(first, second), size, scale)


def fold(members, size=None, scale=None):
    """a.merge(b, size); a.merge(c, size); ... from a copy of the first member; one member: unchanged and unclipped"""
    acc = list(members[0])
    for m in members[1:]:
        acc = merge_pair(acc, m, size, scale)
    return acc


def closed_form(members, size=None):
    """the fold of a group WITHOUT a scale, without walking"""
    if len(members) == 1:
        return list(members[0])
    if any(len(m) == 0 for m in members):
        return []
    bound = min(m[-1][0] for m in members)
    merged = {}
    for m in members:
        for h, c, e, k in m:
            if h <= bound:
                if h in merged:
                    c0, e0, k0 = merged[h]
                    merged[h] = ((c0 + c) % U32, (e0 + e) % U32, k0)
                else:
                    merged[h] = (c, e, k)
    out = [(h,) + merged[h] for h in sorted(merged)]
    return out if size is None else out[:size]


def sums(values):
    """seq_length / num_valid_kmers of a group: u64, wrapping"""
    return sum(values) % U64


COMPAT_FIELDS = ("k", "hash type", "hash bits", "hash seed")


def hash_info(kind, seed):
    """SketchParams::hash_info().0 .. .2 (mod.rs:138-146)"""
    return ("None", 0, 0) if kind == "allcounts" else ("MurmurHash3_x64_128", 64, seed)


def incompatibility(a, b):
    """SketchParams::check_compatibility (mod.rs:185-212) of (kind, k, seed) tuples: None or the reference's sentence"""
    va = (a[1],) + hash_info(a[0], a[2])
    vb = (b[1],) + hash_info(b[0], b[2])
    for name, x, y in zip(COMPAT_FIELDS, va, vb):
        if x != y:
            return "First sketch has %s %s, but second sketch has %s %s" % (name, x, name, y)
    return None
