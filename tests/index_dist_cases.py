"""What tests/test_index_dist_host.py and tests/test_gpu_index_dist.py share: sketches made from a plain description that the
model (tests/index_dist_model.py) reads too, the derived equality of two such sketches, and the comparison of a call's rows
with the model's."""
import struct
from dataclasses import dataclass

import numpy as np

import dist_model as M
import index_dist_model as IDM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams

DOUBLES = ("containment", "jaccard", "mash_distance")


@dataclass
class Spec:
    name: str
    hashes: object
    kind: str = "mash"
    scale: float = 0.0
    k: int = 21

    def params(self):
        return SketchParams.scaled(1000, self.k, self.scale) if self.kind == "scaled" else SketchParams.mash(kmer_length=self.k, no_strict=True)


def bits(x):
    return struct.pack("<d", float(x))


def build(specs):
    """the specs as one collection (all else equal: seq_length, counts, filters)"""
    out = None
    for s in specs:
        hs = np.asarray(s.hashes, np.uint64)
        kc = np.zeros(len(hs), KC_DTYPE)
        kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
        one = H.sketches_from_arrays(s.name, 100, 100, kc, np.zeros((len(hs), s.k), np.uint8), s.params(), H.FilterParams(False))
        if out is None:
            out = one
        else:
            out.append(one)
    return out


def model(specs):
    return [M.Sk(np.asarray(s.hashes, np.uint64), s.kind, s.scale if s.kind == "scaled" else 0.0, s.k) for s in specs]


def equal_fn(qspecs, rspecs):
    """Sketch's derived PartialEq on two specs: a NaN scale is not equal to itself"""
    def equal(q, r):
        a, b = qspecs[q], rspecs[r]
        if a.name != b.name or a.kind != b.kind or a.k != b.k or (a.kind == "scaled" and not a.scale == b.scale):
            return False
        return np.array_equal(np.asarray(a.hashes, np.uint64), np.asarray(b.hashes, np.uint64))
    return equal


def rows_equal_model(rows, want):
    assert [(int(q), int(r)) for q, r in zip(rows["query"], rows["reference"])] == [(q, r) for q, r, _ in want]
    for row, (q, r, d) in zip(rows, want):
        for f in DOUBLES:
            # (a NaN -- old mode's 0 / 0 -- has a sign the model does not state; every other double bit for bit)
            assert bits(row[f]) == bits(d[f]) or (row[f] != row[f] and d[f] != d[f]), (q, r, f, row, d)
        assert int(row["common_hashes"]) == d["common_hashes"] and int(row["total_hashes"]) == d["total_hashes"], (q, r, row, d)


def model_dist(qspecs, rspecs, old_mode, max_distance):
    """index_dist_model.dist for the specs (qspecs None: pairwise)"""
    return IDM.dist(None if qspecs is None else model(qspecs), model(rspecs), old_mode, max_distance,
                    equal_fn(rspecs if qspecs is None else qspecs, rspecs))
