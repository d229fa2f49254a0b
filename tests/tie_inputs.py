"""Crafted inputs whose (masked) hashes land exactly where the code compares: on a threshold, next to one another, on the
edge of a histogram bucket.  Helper module of tests/test_ties_model.py and tests/test_gpu_ties.py, not a test.

Random reads cannot be aimed; single-window records can.  A pool of random k-mers is hashed on the CPU (one Mash oracle of
10**6 rows over a random genome returns every distinct hash with its canonical k-mer), the mask of the hash_mask test hook
(include/finch_hip.h) is applied in numpy, and k-mers are CHOSEN by their masked hash.  Every chosen k-mer becomes a record of
its own (`kmer + b"\\0"`, optionally padded with N to one record length), some as their reverse complement, some several
times, in a seeded order.  What a stream holds is stated from the pool and numpy alone: the oracle's sketcher is not asked.

Masked values are addressed by RANK: rank r of a mask is the r-th smallest value `h & mask` can take (the bits of r laid
into the mask's bit positions, lowest first), so that "the next value up" means the same under a low-bit mask, a high-bit
mask and a mixed one.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from oracle import oracle as O

U64 = (1 << 64) - 1
# the device's collision log holds 65 536 occurrences (CLOG_CAP, fh_api.hip); no crafted stream comes near it
MAX_COLLIDING_OCCURRENCES = 32768
DEVICE_COLLISION_LOG = 65536


def low_mask(b):
    return (1 << b) - 1


def high_mask(b):
    """the top b bits: masked hashes span the whole u64 range"""
    return ((1 << b) - 1) << (64 - b)


MIXED_MASK = 0xFF000000000000FF  # top 8 and low 8 bits


def mask_bits(mask):
    return [p for p in range(64) if (mask >> p) & 1]


def rank_of(h, mask):
    """rank of h & mask among the values the mask lets through (order preserving); h: uint64 array"""
    h = np.asarray(h, dtype=np.uint64)
    r = np.zeros(h.shape, dtype=np.uint64)
    for i, p in enumerate(mask_bits(mask)):
        r |= ((h >> np.uint64(p)) & np.uint64(1)) << np.uint64(i)
    return r.astype(np.int64)


def value_of(r, mask):
    """the masked value of rank r (int -> int)"""
    v = 0
    for i, p in enumerate(mask_bits(mask)):
        v |= ((int(r) >> i) & 1) << p
    return v


def floor_rank(x, mask):
    """rank of the largest masked value <= x (-1: none)"""
    bits = mask_bits(mask)
    lo, hi = -1, (1 << len(bits)) - 1
    while lo < hi:  # value_of is increasing in r
        mid = (lo + hi + 1) // 2
        if value_of(mid, mask) <= x:
            lo = mid
        else:
            hi = mid - 1
    return lo


@functools.lru_cache(maxsize=16)
def pool(k, seed, n_bases, genome_seed):
    """(hashes uint64 [P], canonical k-mers uint8 [P, k]) of every distinct k-mer of a random genome, as hash_f sees them"""
    assert n_bases < 950_000  # (the 10**6-row oracle below must keep every one of them)
    rng = np.random.default_rng(genome_seed)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n_bases)
    full = O.OracleSketcher(O.MASH, 10**6, k, seed)
    full.process(genome)
    kc, km = full.to_vec()
    assert len(kc) > n_bases * 0.9
    return kc["hash"].copy(), km.copy()


_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


class Stream:
    """one crafted packed stream and what it holds, occurrence by occurrence, in stream order"""

    def __init__(self, k, mask, data, hashes, kmers, is_rev, rows, stride):
        self.k, self.mask, self.data, self.stride = k, mask, data, stride
        self.hashes, self.kmers, self.is_rev, self.rows = hashes, kmers, is_rev, rows
        self.H = set(int(h) for h in np.unique(hashes))  # the distinct masked hashes
        # occurrences whose k-mer is not the first k-mer of its masked hash (what the device may have to log), and the worst
        # the device can see if another of the colliding k-mers claims the table slot first
        first_row, per_hash = {}, {}
        colliding = 0
        for h, r in zip(hashes.tolist(), rows.tolist()):
            if first_row.setdefault(h, r) != r:
                colliding += 1
            d = per_hash.setdefault(h, {})
            d[r] = d.get(r, 0) + 1
        self.colliding_occurrences = colliding
        self.worst_logged = sum(sum(d.values()) - min(d.values()) for d in per_hash.values() if len(d) > 1)
        self.collided = set(h for h, d in per_hash.items() if len(d) > 1)  # masked hashes that stand for > 1 k-mer
        assert self.colliding_occurrences <= MAX_COLLIDING_OCCURRENCES, self.colliding_occurrences
        assert self.worst_logged < DEVICE_COLLISION_LOG, self.worst_logged

    def sorted_distinct(self):
        return sorted(self.H)

    def triples(self):
        """(masked hash, canonical k-mer bytes, is_reverse) per occurrence: what the reference's push sees"""
        return [(int(h), bytes(km), int(r)) for h, km, r in zip(self.hashes, self.kmers, self.is_rev)]

    def __len__(self):
        return len(self.hashes)


class Crafter:
    """chooses k-mers of a pool by masked hash; dense / around / filler add to the plan, build() emits a Stream"""

    def __init__(self, k, mask, hash_seed=0, pool_bases=None, rng_seed=1):
        self.k, self.mask = k, mask
        if pool_bases is None:  # (a dozen k-mers or more per masked value)
            pool_bases = 300_000 if len(mask_bits(mask)) <= 14 else 900_000
        self.rng = np.random.default_rng(rng_seed)
        ph, pk = pool(k, hash_seed, pool_bases, 977 + k)
        self.pool_hash, self.pool_kmer = ph, pk
        self.masked = ph & np.uint64(mask)
        self.rank = rank_of(ph, mask)
        order = np.argsort(self.rank, kind="stable")
        ranks, starts, counts = np.unique(self.rank[order], return_index=True, return_counts=True)
        self._order = order
        self._group = {int(r): (int(s), int(c)) for r, s, c in zip(ranks, starts, counts)}
        self.n_ranks = 1 << len(mask_bits(mask))
        self.plan = {}  # rank -> number of distinct k-mers

    def available(self, r):
        return self._group.get(int(r), (0, 0))[1]

    def _want(self, r, n):
        assert 0 <= r < self.n_ranks, r
        assert self.available(r) >= n, "the pool holds %d k-mers of rank %d, %d wanted" % (self.available(r), r, n)
        self.plan[int(r)] = max(self.plan.get(int(r), 0), n)

    def dense(self, ranks, multi=(0.6, 0.25, 0.15)):
        """every masked value of the given ranks occurs, from 1..3 distinct k-mers each (as far as the pool has them)"""
        for r in ranks:
            n = 1 + int(self.rng.choice(3, p=multi))
            self._want(r, max(1, min(n, self.available(r))))
        return self

    def around(self, x_rank, below, above):
        """ranks x - below .. x + above all occur, x itself from two distinct k-mers: the tie is also a collision"""
        lo, hi = max(0, x_rank - below), min(self.n_ranks - 1, x_rank + above)
        self.dense(range(lo, hi + 1))
        self._want(x_rank, max(2, self.plan.get(int(x_rank), 0)))
        return self

    def filler(self, n, lo_rank=0, hi_rank=None):
        """n ordinary masked hashes drawn from [lo_rank, hi_rank], one k-mer each: something for a selection to cut"""
        hi_rank = self.n_ranks - 1 if hi_rank is None else hi_rank
        have = np.array([r for r in self._group if lo_rank <= r <= hi_rank], dtype=np.int64)
        for r in self.rng.choice(have, size=min(n, len(have)), replace=False):
            self._want(int(r), max(1, self.plan.get(int(r), 0)))
        return self

    def without(self, ranks):
        for r in ranks:
            self.plan.pop(int(r), None)
        return self

    def values(self):
        return sorted(value_of(r, self.mask) for r in self.plan)

    def build(self, order="shuffle", record_len=None, max_reps=3):
        """order: 'shuffle' (seeded), 'ascending' / 'descending' by masked hash.  record_len: pad every record with N to that
        many bytes (a stride of record_len + 1)."""
        rows = []
        for r, n in self.plan.items():
            s, _ = self._group[r]
            rows.extend(self._order[s:s + n].tolist())
        rows = np.array(rows, dtype=np.int64)
        reps = 1 + self.rng.choice(3, size=len(rows), p=(0.6, 0.3, 0.1)) if max_reps > 1 else np.ones(len(rows), dtype=np.int64)
        occ = np.repeat(rows, np.minimum(reps, max_reps))
        if order == "shuffle":
            occ = self.rng.permutation(occ)
        else:
            occ = occ[np.argsort(self.masked[occ], kind="stable")]
            if order == "descending":
                occ = occ[::-1].copy()
        is_rev = (self.rng.random(len(occ)) < 0.5).astype(np.uint8)
        canon = self.pool_kmer[occ]
        text = canon.copy()
        rc = _COMP[canon[:, ::-1]]
        text[is_rev == 1] = rc[is_rev == 1]
        # (a palindrome would be pushed with is_reverse = 1 whichever way it is written: none in these pools)
        assert not (canon == rc).all(axis=1).any()
        L = self.k if record_len is None else record_len
        assert L >= self.k
        rec = np.full((len(occ), L + 1), ord("N"), dtype=np.uint8)
        rec[:, :self.k] = text
        rec[:, L] = 0
        return Stream(self.k, self.mask, rec.reshape(-1).copy(), self.masked[occ].copy(), canon, is_rev, occ, L + 1)


def qoct_edges():
    """q -> the largest hash of quarter-octave bucket q (qoct_upper_edge, fh_core.h), from the host build of that header
    which tests/test_core_logic_host.py also uses"""
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "hostcore", "fhcore_host.cpp")
    so = os.path.join(here, "hostcore", "libfhcore_host.so")
    hdr = os.path.join(here, "..", "finch_rs_amd", "csrc", "fh_core.h")
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = "%s.tmp.%d" % (so, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.fhcore_qoct_upper_edge.restype = C.c_uint64
    L.fhcore_qoct_upper_edge.argtypes = [C.c_uint32]
    L.fhcore_qoct_index.restype = C.c_uint32
    L.fhcore_qoct_index.argtypes = [C.c_uint64]
    return (lambda q: int(L.fhcore_qoct_upper_edge(q))), (lambda x: int(L.fhcore_qoct_index(x)))
