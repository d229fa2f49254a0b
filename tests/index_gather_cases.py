"""The cases tests/test_index_gather_model.py and tests/test_gpu_index_gather.py share, on top of tests/gather_cases.py's: the
smallest shapes at which a piece of finch_index_gather's device form can go wrong.  Each is built once."""
from functools import lru_cache

import numpy as np

import gather_cases as GC

ROUNDS_THREADS = 1024  # k_index_gather_rounds' workgroup: the winner's hashes are walked that many at a time
MIN_OVERLAPS = (1, 3, 10 ** 6)
MAX_ROUNDS = (0, 1, 2, 5)
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 1023, 1025, 65537)
WINNER_LENGTHS = (0, 1, 63, 64, 65, 1023, 1025, 1200)


@lru_cache(None)
def hand_case():
    return GC.hand_case()


@lru_cache(None)
def random_case(n_refs):
    """tests/test_gpu_gather.py's: five queries, 70 and 130 references"""
    return GC.random_case(1000 + n_refs, 5, n_refs, pool_size=150, max_q=120, max_r=10)


@lru_cache(None)
def common_hash_case(n_refs):
    """every reference holds one hash X that query 0 has: a posting run of n_refs -- 300: longer than the count's workgroup of
    256; 1100: longer than the rounds' of 1024 and across two batches of its flat deal.  The first winner removes X and lowers
    all n_refs counters at once.  Each reference also holds three hashes of its own, of which query 0 has some, so that rounds
    follow; query 1 has private hashes only, query 2 only X"""
    rng = np.random.default_rng(n_refs)
    pool = np.unique(rng.integers(1 << 20, GC.U64_MAX, 3 * n_refs + 200, dtype=np.uint64))
    x, private = pool[len(pool) // 2], np.delete(pool, len(pool) // 2)[:3 * n_refs].reshape(n_refs, 3)
    refs = [(np.sort(np.concatenate([[x], private[j]])), None) for j in range(n_refs)]
    q0 = np.unique(np.concatenate([[x], private[::7, :2].ravel(), private[3::50].ravel(), private[n_refs - 1]]))
    q1 = np.sort(private[1::9, 1:].ravel())
    return GC.Case([(q0, rng.integers(1, 1 << 16, len(q0))), (q1, None), ([x], [77])], refs)


@lru_cache(None)
def equal_case():
    """query 0 is exactly reference 2; references 0 and 3 are equal (the tie goes to index 0, and 3 is used up with it);
    query 1 is exactly those two"""
    a, b = list(range(100, 160)), list(range(500, 530))
    refs = [(b, None), (a[:20], None), (a, None), (b, None), (a[30:] + b[:5], None)]
    return GC.Case([(a, list(range(1, 61))), (b, None)], refs)


@lru_cache(None)
def winner_length_case():
    """one query; a reference of every length in WINNER_LENGTHS.  A reference's hashes ascend, and the rounds kernel walks them
    1024 at a time: each reference takes query hashes at its low end (the first batch of the walk) and at its high end (the last
    batch: the second one for 1025 and 1200), and hashes no query has in between.  The numbers taken differ, so every one wins
    a round of its own; the reference of length 0 is never a candidate"""
    low = np.arange(1000, 1200, dtype=np.uint64) * 3
    high = (np.uint64(1) << np.uint64(63)) + np.arange(200, dtype=np.uint64) * 5
    refs, lo_at, hi_at = [], 0, 0
    for i, n in enumerate(WINNER_LENGTHS):
        if n == 0:
            refs.append(([], None))
        elif n == 1:
            refs.append((high[-1:], None))
        else:
            a, b = i + 1, i + 2
            filler = (np.uint64(1) << np.uint64(40)) + np.arange(n - a - b, dtype=np.uint64) * 7 + np.uint64(i)
            refs.append((np.concatenate([low[lo_at:lo_at + a], filler, high[hi_at:hi_at + b]]), None))
            lo_at, hi_at = lo_at + a, hi_at + b
    q = np.concatenate([low, high])
    return GC.Case([(q, np.arange(1, len(q) + 1))], refs)


@lru_cache(None)
def used_up_case():
    """tests/test_gpu_gather.py's test_reference_lengths_and_a_candidate_used_up: candidates that the first winner uses up, one
    that falls to 60 (below min_overlap 61), a tie at round 0"""
    rng = np.random.default_rng(11)
    h = np.unique(rng.integers(0, GC.U64_MAX // 2, 700, dtype=np.uint64))[:600]
    other = np.unique(rng.integers(GC.U64_MAX // 2, GC.U64_MAX, 1200, dtype=np.uint64))[:1000]
    long_ref = np.sort(np.concatenate([h[:200], other]))
    refs = [(h[100:180], None), (long_ref, None), ([], None), (h[150:260], None), (h[190:200], None), (h[400:], None)]
    return GC.Case([(h, rng.integers(1, 50, 600))], refs)


@lru_cache(None)
def length_case():
    """tests/test_gpu_gather.py's: one query of every length in LENGTHS -- the word edges of the bitmask --; the references take
    the first hash and the last three, every third, a block in the middle, and hashes no query has"""
    rng = np.random.default_rng(77)
    queries, all_h = [], []
    for n in LENGTHS:
        h = np.unique(rng.integers(0, GC.U64_MAX, n + 50, dtype=np.uint64))[:n]
        assert len(h) == n
        queries.append((h, rng.integers(1, 1 << 30, n)))
        all_h.append(h)
    refs = []
    for h in all_h:
        if len(h):
            refs.append((np.unique(np.concatenate([h[:1], h[-3:]])), None))
            refs.append((h[::3], None))
            refs.append((h[len(h) // 3:len(h) // 3 + 40], None))
    refs.append((np.unique(np.concatenate([a[-2:] for a in all_h if len(a)])), None))
    refs.append(([5, 6, 7], None))
    return GC.Case(queries, refs)


@lru_cache(None)
def longest_case():
    """1 048 576 hashes: all of the rounds kernel's 128 KiB mask; three small references at its first word, its last word and
    across the middle"""
    n = 1 << 20
    h = np.arange(n, dtype=np.uint64) * 7 + 3
    counts = (np.arange(n, dtype=np.uint64) % 1000 + 1).astype(np.uint32)
    refs = [(np.concatenate([h[:2], h[-33:]]), None), (np.concatenate([[np.uint64(1)], h[31:34], h[n // 2 - 1:n // 2 + 1]]), None),
            (h[-40:], None)]
    return GC.Case([(h, counts)], refs)


LONG_ORDERS = ("long_last", "long_first", "long_between")


@lru_cache(None)
def long_without_candidates_case(order):
    """tests/test_gpu_gather.py's: with min_overlap 10 the long query shares hashes with every reference (its counters are
    touched, and lowered by no one) but is no one's candidate; it must not size or touch the mask"""
    n = 300_000
    long_h = np.arange(n, dtype=np.uint64) * 11 + 5
    short_h = np.arange(20, dtype=np.uint64) * 11 + 7
    other_h = np.arange(33, dtype=np.uint64) * 11 + 9
    refs = [(np.sort(np.concatenate([short_h[:12], long_h[:3], long_h[-3:]])), None),
            (np.sort(np.concatenate([short_h[10:], other_h[:11], long_h[n // 2:n // 2 + 9]])), None),
            (long_h[1000:1009], None)]
    queries = {"long_last": [(short_h, None), (other_h, None), (long_h, None)],
               "long_first": [(long_h, None), (short_h, None), (other_h, None)],
               "long_between": [(short_h, None), (long_h, None), (other_h, None)]}[order]
    case = GC.Case(queries, refs)
    case.long_at = [len(h) for h, _ in queries].index(n)
    return case


def pairs_sharing_a_hash(case):
    """the (query, reference) pairs with a shared hash, counted in numpy: what the device's count touches"""
    qs = [np.asarray(q.hashes, np.uint64) for q in case.mq]
    rs = [np.asarray(r.hashes, np.uint64) for r in case.mr]
    return sum(1 for q in qs for r in rs if len(np.intersect1d(q, r, assume_unique=True)))
