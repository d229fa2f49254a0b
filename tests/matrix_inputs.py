"""Inputs of the minmer_matrix tests (test_matrix_model.py, test_gpu_matrix.py): sketches given as (hashes, counts) pairs, made
into a library handle through the `.sk` JSON reader -- the one way in that takes a count of 0 and hashes in any order."""
import json

import numpy as np

from finch_rs_amd import host as H

U64_MAX = (1 << 64) - 1
U32_MAX = (1 << 32) - 1


def handle(sketches, names=None):
    """[(hashes, counts)] -> H.Sketches of as many sketches, in order (an empty list: a handle of no sketches)"""
    doc = {"kmer": 21, "alphabet": "ACGT", "preserveCase": False, "canonical": True, "sketchSize": 1000,
           "hashType": "MurmurHash3_x64_128", "hashBits": 64, "hashSeed": 0,
           "sketches": [{"name": names[i] if names else "s%d" % i, "hashes": [str(int(h)) for h in hs],
                         "counts": [int(c) for c in cs]} for i, (hs, cs) in enumerate(sketches)]}
    sk = H.sketches_from_json(json.dumps(doc))
    assert len(sk) == len(sketches)
    return sk


def pool_sketches(rng, pool, sizes):
    """one sketch per size: that many distinct hashes of `pool`, ascending, with counts from the whole u32 range"""
    out = []
    for n in sizes:
        hs = np.sort(rng.choice(pool, int(n), replace=False)) if n else np.zeros(0, np.uint64)
        cs = rng.integers(0, U32_MAX, len(hs), dtype=np.uint32, endpoint=True)
        small = rng.random(len(hs)) < 0.5  # half of them the counts a sketcher emits
        cs[small] = rng.integers(1, 40, int(small.sum()), dtype=np.uint32)
        out.append((hs, cs))
    return out


def hash_pool(rng, n):
    """n distinct u64, ascending, 0 and 2^64 - 1 among them"""
    p = np.array([0, U64_MAX], np.uint64)
    while len(p) < n:
        p = np.unique(np.concatenate([p, rng.integers(1, U64_MAX, n - len(p), dtype=np.uint64)]))
    return p


# the hand-made case: R = 5, S = 3.  Counts 0, 1, 2^31, 2^32 - 1; hashes below the first reference hash, above the last,
# between two, equal to the first and to the last; 0 and 2^64 - 1 on both sides; an empty sketch
HAND_REF = ([0, 10, 20, 30, U64_MAX], [7, 0, 1 << 31, U32_MAX, 1])
HAND_SKETCHES = [
    ([0, 5, 10, 15, 30, U64_MAX], [1 << 31, 9, 0, 9, U32_MAX, 1]),  # first and last reference hash, between, a count of 0
    ([], []),
    ([20, 25, U64_MAX - 1], [1, 9, 9]),  # between and above every inner hash; nothing for 0 or 2^64 - 1
]
HAND_WANT = np.array([[-(1 << 31), 0, 0, -1, 1], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0]], np.int32)
# a reference that starts above 0 and ends below 2^64 - 1: sketch hashes below ref[0] and above ref[R - 1]
HAND_REF_INNER = ([10, 20, 30, 40, 50], [1, 1, 1, 1, 1])
HAND_WANT_INNER = np.array([[0, 0, -1, 0, 0], [0, 0, 0, 0, 0], [0, 1, 0, 0, 0]], np.int32)


def raw_call(refs, ir, sketches, out, out_len, devices=(0,), n_devices=None):
    """finch_minmer_matrix as C sees it -> (return code, message); refs / sketches: H.Sketches or None, out: an int32 array or None"""
    import ctypes as C
    L = H.lib()
    darr = (C.c_int * max(1, len(devices)))(*devices) if devices is not None else None
    rc = L.finch_minmer_matrix(refs._p if refs is not None else None, ir, sketches._p if sketches is not None else None, darr,
                               len(devices or ()) if n_devices is None else n_devices, out.ctypes.data if out is not None else None,
                               out_len, None, None)
    return rc, (L.finch_last_error() or b"").decode(errors="replace")


def refusals():
    """[(what, arguments of raw_call, words the message must hold)]: every call FH_ERR_INVALID, decided before a device is looked
    for -- the same with and without one"""
    asc = handle([([1, 5, 9], [1, 2, 3]), ([], []), ([2, 5], [4, 4])], ["a", "empty", "b"])
    bad = handle([([1, 5, 9], [1, 1, 1]), ([3, 2, 7], [1, 1, 1]), ([4, 4], [1, 1])], ["fine", "descends", "repeats"])
    none = handle([])
    out9 = np.zeros(9, np.int32)
    return [
        ("refs NULL", (None, 0, asc, out9, 9), ["null argument"]),
        ("sketches NULL", (asc, 0, None, out9, 9), ["null argument"]),
        ("out NULL", (asc, 0, asc, None, 9), ["null argument"]),
        ("devices NULL", (asc, 0, asc, out9, 9, None, 2), ["null argument"]),
        ("17 device entries", (asc, 0, asc, out9, 9, (0,) * 17), ["at most 16"]),
        ("ir out of range", (asc, 3, asc, out9, 9), ["reference sketch 3 of 3"]),
        ("ir out of range, no sketches", (none, 0, asc, out9, 0), ["reference sketch 0 of 0"]),
        ("reference descends", (bad, 1, asc, out9, 9), ["reference sketch 1 (descends)", "not strictly ascending at 1"]),
        ("reference repeats a hash", (bad, 2, asc, np.zeros(6, np.int32), 6), ["reference sketch 2 (repeats)", "not strictly ascending at 1"]),
        ("a sketch descends", (asc, 0, bad, out9, 9), ["sketch 1 (descends)", "not strictly ascending at 1"]),
        ("empty reference, a sketch with hashes", (asc, 1, asc, out9, 0), ["reference sketch 1 (empty) is empty"]),
        ("out_len short", (asc, 0, asc, out9, 8), ["out_len 8", "3 x 3"]),
        ("out_len long", (asc, 2, asc, out9, 9), ["out_len 9", "3 x 2"]),
        ("out_len 0", (asc, 0, asc, out9, 0), ["out_len 0", "3 x 3"]),
    ]
