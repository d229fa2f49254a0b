"""minmer_matrix (lib/src/distance.rs:345-364) restated in plain Python/numpy, sharing no code with the library: the reference's
two-cursor loop taken literally (`minmer_matrix`), and the order-free predicate it equals on strictly ascending inputs
(`by_lookup`).  A sketch is a pair (hashes, counts) of equal length; hashes are Python ints or uint64, counts u32."""
import numpy as np


def as_i32(count):
    """`count as i32` on a u32: the same 32 bits"""
    c = int(count) & 0xFFFFFFFF
    return c - (1 << 32) if c >= (1 << 31) else c


def minmer_matrix(ref_hashes, sketches):
    """the loop as written; IndexError where the reference indexes ref_sketch[0] of an empty reference (a panic)"""
    ref = [int(h) for h in ref_hashes]
    n_ref = len(ref)
    result = np.zeros((len(sketches), n_ref), np.int32)
    for i, (hashes, counts) in enumerate(sketches):
        ref_pos = 0
        for h, c in zip(hashes, counts):
            h = int(h)
            # (ref[0] of an empty list raises IndexError here, as ref_sketch[0] panics there, before `len - 1` is looked at)
            while h > ref[ref_pos] and ref_pos < n_ref - 1:
                ref_pos += 1
            if h == ref[ref_pos]:
                result[i, ref_pos] = as_i32(c)
    return result


def by_lookup(ref_hashes, sketches):
    """cell (i, p) = the count of sketch i's entry whose hash is ref[p], else 0 -- what the loop computes when both sides are
    strictly ascending"""
    if len(ref_hashes) == 0 and any(len(h) for h, _ in sketches):
        raise IndexError("ref_sketch[0] of an empty reference sketch")
    result = np.zeros((len(sketches), len(ref_hashes)), np.int32)
    for i, (hashes, counts) in enumerate(sketches):
        held = {int(h): as_i32(c) for h, c in zip(hashes, counts)}
        for p, r in enumerate(ref_hashes):
            result[i, p] = held.get(int(r), 0)
    return result
