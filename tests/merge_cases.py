"""What tests/test_merge_host.py and tests/test_gpu_merge.py share: sketches built from the model's records (finch_sketches_from_arrays,
so that members can carry different k-mer text for the same hash), read back field by field, and the model's answer for a group."""
import ctypes as C

import numpy as np

import merge_model as MM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams

K = 21
MASH = SketchParams.mash(kmer_length=K)


def scaled(scale, k=K):
    return SketchParams.scaled(1000, k, scale)


def scale_for(max_hash):
    """a scale whose max_hash is max_hash or a little below (the divisor is an integer)"""
    return 1.0 / (2 ** 64 // (max_hash + 1))


def kmer(tag, h):
    """K bytes that say which member (tag) the record of hash h came from"""
    return (b"%c%020d" % (tag, h % 10 ** 20))[:K]


def records(hashes, tag=65, counts=None, extras=None):
    counts = [1 + (h % 5) for h in hashes] if counts is None else counts
    extras = [c // 2 for c in counts] if extras is None else extras
    return [(int(h), int(c), int(e), kmer(tag, int(h))) for h, c, e in zip(hashes, counts, extras)]


class Member:
    def __init__(self, name, recs, params=MASH, seq_length=100, num_valid_kmers=90, comment="", filters=None):
        self.name, self.recs, self.params, self.seq_length, self.num_valid_kmers = name, recs, params, seq_length, num_valid_kmers
        self.comment, self.filters = comment, filters or H.FilterParams(False)

    @property
    def scale(self):
        return self.params.scale if self.params.kind == "scaled" else None

    def build(self):
        kc = np.zeros(len(self.recs), KC_DTYPE)
        kc["hash"] = np.asarray([r[0] for r in self.recs], np.uint64)
        kc["count"] = np.asarray([r[1] for r in self.recs], np.uint32)
        kc["extra_count"] = np.asarray([r[2] for r in self.recs], np.uint32)
        k = self.params.kmer_length
        km = np.frombuffer(b"".join(r[3] for r in self.recs), np.uint8).reshape(len(self.recs), k) if self.recs else np.zeros((0, k), np.uint8)
        s = H.sketches_from_arrays(self.name, self.seq_length, self.num_valid_kmers, kc, km, self.params, self.filters)
        if self.comment:
            s.set_comment(0, self.comment)
        return s


def collect(members):
    out = members[0].build()
    for m in members[1:]:
        out.append(m.build())
    return out


def read(sk, i):
    """sketch i of a collection, every field the merge is specified on"""
    L = H.lib()
    n = L.finch_sketch_n_hashes(sk._p, i)
    p = H.CSketchParams()
    H._check(L.finch_sketch_params_of(sk._p, i, C.byref(p)))
    fp = H.CFilterParams()
    H._check(L.finch_sketch_filter_params(sk._p, i, C.byref(fp)))
    hs, cs, es = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    km = np.zeros((n, p.kmer_length), np.uint8)
    H._check(L.finch_sketch_copy(sk._p, i, hs.ctypes.data, cs.ctypes.data, es.ctypes.data, km.ctypes.data))
    kb = km.tobytes()
    k = p.kmer_length
    return {"name": L.finch_sketch_name(sk._p, i).decode(), "seq_length": L.finch_sketch_seq_length(sk._p, i),
            "num_valid_kmers": L.finch_sketch_num_valid_kmers(sk._p, i), "comment": L.finch_sketch_comment(sk._p, i).decode(),
            "params": tuple(getattr(p, f) for f, _ in H.CSketchParams._fields_ if f != "pad"),
            "filters": tuple(getattr(fp, f) for f, _ in H.CFilterParams._fields_ if f != "pad"),
            "records": list(zip(hs.tolist(), cs.tolist(), es.tolist(), [kb[j * k:(j + 1) * k] for j in range(n)]))}


def expected(members, size=None):
    """the model's answer for the group `members` (Member objects, in order): the fold, the first member's identity, the sums"""
    first = members[0]
    p, fp = H._params_c(first.params), first.filters.to_c()
    return {"name": first.name, "seq_length": MM.sums(m.seq_length for m in members),
            "num_valid_kmers": MM.sums(m.num_valid_kmers for m in members), "comment": first.comment,
            "params": tuple(getattr(p, f) for f, _ in H.CSketchParams._fields_ if f != "pad"),
            "filters": tuple(getattr(fp, f) for f, _ in H.CFilterParams._fields_ if f != "pad"),
            "records": MM.fold([m.recs for m in members], size, first.scale)}


def same(got, want):
    """field by field; on a mismatch in the records, the first differing index is what one wants to read"""
    for f in ("name", "seq_length", "num_valid_kmers", "comment", "params", "filters"):
        assert got[f] == want[f], (f, got[f], want[f])
    g, w = got["records"], want["records"]
    if g != w:
        at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
        raise AssertionError("records differ at %d of %d / %d: %r != %r" % (at, len(g), len(w), g[at:at + 2], w[at:at + 2]))
    return True
