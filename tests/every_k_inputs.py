"""The per-k input of the every-k sweep (tests/test_gpu_every_k.py): one small packed stream per k-mer length, built to sit on the
edges that depend on k -- records around k bases long whose breakers land at every lane offset, windows that span lane and tile
boundaries at every alignment, runs between non-bases of exactly k - 2 .. k + 2 bases, k-mers seen from both strands, reverse-
complement palindromes (even k), and N on both sides of a tile edge.  Plain numpy, no GPU; tests/test_every_k_inputs.py holds the
generator to what the sweep relies on.

    parts(k)  -> {name: [records]}      the named pieces, every record a uint8 array without its breaker
    stream(k) -> (records, packed)      all records in order, and their concatenation with one \\0 breaker behind each
    small(k, limit) -> packed prefix    the longest prefix of whole records of `packed` with at most `limit` positions
    stream_records(k) -> [records]      k <= 32: three records on the edges of the STREAMED record sketcher -- round seams, folds
"""
import functools

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NON_BASES = np.frombuffer(b"NRYKMSWn-", dtype=np.uint8)
TILE = 2048          # positions a wave takes at a time (64 lanes of 32)
N_RAGGED = 300       # records of max(1, k - 2) .. k + 70 bases

_COMP = np.zeros(256, np.uint8)
for _x, _y in zip(b"ACGT", b"TGCA"):
    _COMP[_x] = _y


def revcomp(a):
    return _COMP[a[::-1]]


def long_n_positions(k):
    """where the long record holds N: invalid windows start and end on both sides of the edges of its second and third tile"""
    return (TILE - 1, TILE + k - 1, 2 * TILE - 1 - k, 2 * TILE)


def gap_runs(k):
    """the gap record's runs of bases, each followed by a single N"""
    return [max(0, k - 2), k - 1, k, k + 1, k + 2, k]


def _noisy(rng, n):
    """n random bases, about 2 % of them lower case and about 0.3 % no base at all"""
    r = rng.choice(ACGT, size=n)
    m = rng.random(n)
    r[m > 0.98] |= 0x20
    bad = m < 0.003
    r[bad] = rng.choice(NON_BASES, size=int(bad.sum()))
    return r


def _filler_lengths(rng, lo, hi, total):
    """record lengths in [lo, hi] whose records, breakers included, take exactly `total` positions"""
    m = -(-total // (hi + 1))
    assert m * (lo + 1) <= total <= m * (hi + 1), (lo, hi, total)
    lens = np.full(m, lo, np.int64)
    spare = total - m * (lo + 1)
    while spare:
        i = int(rng.integers(0, m))
        add = min(spare, hi - int(lens[i]), int(rng.integers(1, hi - lo + 1)))
        lens[i] += add
        spare -= add
    return [int(x) for x in lens]


@functools.lru_cache(maxsize=None)
def parts(k):
    rng = np.random.default_rng(64000 + k)
    bases = lambda n: rng.choice(ACGT, size=n)  # noqa: E731
    p = {}
    p["exact"] = [bases(k - 1), bases(k), bases(k + 1)]
    p["repeats"] = [np.full(3 * k, ord("A"), np.uint8), np.full(3 * k, ord("T"), np.uint8)]
    if k % 2 == 0:
        blocks = []
        for _ in range(8):
            half = bases(k // 2)
            blocks += [half, revcomp(half), bases(3)]
        p["palindromes"] = [np.concatenate(blocks)]
    gap = []
    for run in gap_runs(k):
        gap += [bases(run), np.frombuffer(b"N", dtype=np.uint8)]
    p["gaps"] = [np.concatenate(gap)]
    lo, hi = max(1, k - 2), k + 70
    p["ragged"] = [_noisy(rng, int(n)) for n in rng.integers(lo, hi + 1, size=N_RAGGED)]
    # records of the same kind that bring the long record to the start of a tile of the stream
    used = sum(len(r) + 1 for name in p for r in p[name])
    p["filler"] = [_noisy(rng, n) for n in _filler_lengths(rng, lo, hi, TILE + (-used) % TILE)]
    long = bases(3 * TILE + k)
    long[list(long_n_positions(k))] = ord("N")
    p["long"] = [long]
    for recs in p.values():
        for r in recs:
            r.setflags(write=False)
    return p


def pack(records):
    out = np.zeros(sum(len(r) + 1 for r in records), np.uint8)
    at = 0
    for r in records:
        out[at:at + len(r)] = r
        at += len(r) + 1
    return out


@functools.lru_cache(maxsize=None)
def stream(k):
    records = [r for recs in parts(k).values() for r in recs]
    packed = pack(records)
    packed.setflags(write=False)
    return records, packed


def long_offset(k):
    """where the long record begins in stream(k)'s packed form"""
    return len(stream(k)[1]) - (3 * TILE + k + 1)


ROUND = 4096            # window starts the streamed record sketcher takes between two decision points (eight waves, two tiles)
STREAM_ROUNDS = 6       # rounds of the long streamed record, the last one partial
STREAM_SCALE = 0.02     # the sweep's Scaled records: about 400 of the long record's 20 000 hashes, within the streamed form's cap
COPIED = (1000, 600, 3 * ROUND + 1000)  # a block of the first round (start, length), and where its reverse complement lies


def stream_long_n_positions(k):
    """where the long streamed record holds N.  Behind an odd seam's N no window that spans the seam from the left is valid;
    an even seam's N invalidates every window that starts at the seam or up to k - 1 behind it.  The N two in front of the
    fourth seam closes a run of exactly k bases with that seam's N: see stream_seam_window"""
    seams = [r * ROUND - 1 if r % 2 else r * ROUND + k - 1 for r in range(1, STREAM_ROUNDS)]
    return sorted(seams + [4 * ROUND - 2])


def stream_seam_window(k):
    """the start of the one valid window between two N around the fourth seam: it begins in one round and (k >= 2) ends in the next"""
    return 4 * ROUND - 1


def stream_a_run(k):
    """(start, length) of the run of A: it ends just in front of the second seam's N, so for k >= 2 k - 1 windows of A^k span the seam"""
    return 2 * ROUND - 2 * k - 1, 3 * k


@functools.lru_cache(maxsize=None)
def stream_records(k):
    """the three records of the streamed record sketcher's sweep, k = 1..32:
    1. 5 x 4096 + k + 37 positions -- six rounds, the last partial and no whole tile -- with N around every round seam
       (stream_long_n_positions), one window alone between two N across a seam, A^(3k) across a seam, a block of the first round
       again as its reverse complement in the fourth (its k-mers are in the list when they recur behind at least one fold) and
       about 2 % lower case;
    2. 8193 random positions, one above the LDS form's bound;
    3. k + 1 bases."""
    rng = np.random.default_rng(96000 + k)
    long = rng.choice(ACGT, size=(STREAM_ROUNDS - 1) * ROUND + k + 37)
    src, n, dst = COPIED
    long[dst:dst + n] = revcomp(long[src:src + n])
    at, run = stream_a_run(k)
    long[at:at + run] = ord("A")
    long[rng.random(len(long)) > 0.98] |= 0x20
    long[stream_long_n_positions(k)] = ord("N")
    records = [long, rng.choice(ACGT, size=2 * ROUND + 1), rng.choice(ACGT, size=k + 1)]
    for r in records:
        r.setflags(write=False)
    return records


def small(k, limit):
    records, packed = stream(k)
    at = 0
    for r in records:
        if at + len(r) + 1 > limit:
            break
        at += len(r) + 1
    return packed[:at]
