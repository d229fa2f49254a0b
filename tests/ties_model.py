"""The reference's two hashing sketchers and the library's partial-sketch merge, restated in plain Python for inputs whose
hashes tie: a `heapq` where the reference holds a BinaryHeap, a `dict` where it holds a HashMap.  Takes (masked hash, k-mer,
is_reverse) triples, so it needs neither the library nor the oracle's sketcher (a caller may take raw hashes from O.hash_f).
Helper module of tests/test_ties_model.py and tests/test_gpu_ties.py, not a test.
"""
import heapq

U32_MAX = (1 << 32) - 1
U64_MAX = (1 << 64) - 1


def scaled_max_hash(scale):
    """scaled.rs:23,31: u64::MAX / ((1. / scale) as u64); `as u64` truncates and saturates"""
    inv = 1.0 / scale
    iscale = U64_MAX if inv >= 18446744073709551616.0 else int(inv)
    return U64_MAX // iscale


class _Heap:
    """a max-heap of (hash, k-mer) ordered by hash alone, as BinaryHeap<HashedItem> is (hashing.rs: Ord on the hash); the
    hashes in it are distinct (the counts map guards every push), so the k-mer is never compared"""

    def __init__(self):
        self.h = []

    def __len__(self):
        return len(self.h)

    def push(self, hash_, kmer):
        heapq.heappush(self.h, (-hash_, kmer))

    def peek(self):
        return -self.h[0][0]

    def pop(self):
        return -heapq.heappop(self.h)[0]

    def into_sorted_vec(self):
        return sorted((-nh, km) for nh, km in self.h)


class _Sketcher:
    def __init__(self, size):
        self.hashes, self.counts, self.size, self.total_kmers = _Heap(), {}, size, 0

    def _count_or_insert(self, new_hash, kmer, extra_count):
        if new_hash in self.counts:                       # mash.rs:45-50 / scaled.rs:42-47: saturating adds
            c = self.counts[new_hash]
            self.counts[new_hash] = (min(c[0] + 1, U32_MAX), min(c[1] + extra_count, U32_MAX))
            return False
        self.hashes.push(new_hash, kmer)                  # mash.rs:52-56 / scaled.rs:49-53: the first occurrence's bytes
        self.counts[new_hash] = (1, extra_count)
        return True

    def to_vec(self):
        """mash.rs:86-102 / scaled.rs:84-100 -> [(hash, kmer, count, extra_count)] ascending"""
        return [(h, km) + self.counts[h] for h, km in self.hashes.into_sorted_vec()]

    def feed(self, triples):
        for h, km, rev in triples:
            self.push(h, km, rev)
        return self


class MashModel(_Sketcher):
    def push(self, new_hash, kmer, extra_count):
        self.total_kmers += 1                             # mash.rs:35
        if len(self.hashes) == 0:                         # mash.rs:37-42
            add_hash = True
        else:
            add_hash = new_hash <= self.hashes.peek() or len(self.hashes) < self.size
        if add_hash and self._count_or_insert(new_hash, kmer, extra_count):
            if len(self.hashes) > self.size:              # mash.rs:57-60
                del self.counts[self.hashes.pop()]


class ScaledModel(_Sketcher):
    def __init__(self, size, scale=None, max_hash=None):
        super().__init__(size)
        self.max_hash = scaled_max_hash(scale) if max_hash is None else max_hash

    def push(self, new_hash, kmer, extra_count):
        self.total_kmers += 1                             # scaled.rs:38
        # scaled.rs:41: a hash above max_hash is let in while the heap holds at most `size` ...
        if new_hash <= self.max_hash or (len(self.hashes) <= self.size and self.size != 0):
            if self._count_or_insert(new_hash, kmer, extra_count):
                # scaled.rs:54-58: ... and the largest goes again once there are more, if IT is above max_hash
                if len(self.hashes) > self.size and self.hashes.peek() > self.max_hash:
                    del self.counts[self.hashes.pop()]


def merge_model(kind, size, max_hash, parts):
    """The partial-sketch merge as include/finch_hip.h states it: union of the parts' rows, counts summed and clamped at
    u32::MAX, the k-mer (and position) of the smallest first_pos, re-selection per kind -- Mash keeps the `size` smallest,
    Scaled everything at or below max_hash and, while that is fewer than `size`, the smallest above it.
    parts: lists of (hash, count, extra_count, kmer, first_pos); -> the same, ascending by hash."""
    rows = {}
    for part in parts:
        for h, c, e, km, pos in part:
            if h not in rows:
                rows[h] = [c, e, km, pos]
            else:
                r = rows[h]
                r[0], r[1] = r[0] + c, r[1] + e
                if pos < r[3]:
                    r[2], r[3] = km, pos
    out = [(h, min(r[0], U32_MAX), min(r[1], U32_MAX), r[2], r[3]) for h, r in sorted(rows.items())]
    if kind == "mash":
        return out[:size]
    n_le = sum(1 for r in out if r[0] <= max_hash)
    return out[:max(n_le, min(len(out), size))]
