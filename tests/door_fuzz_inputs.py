"""The cases of the door fuzz (tests/test_gpu_fuzz_doors.py): a randomised differential of every many-per-launch way to a sketch
against the oracle, and -- from the oracle alone -- WHICH blocks each door must take.  Plain numpy and the oracle, no GPU;
tests/test_door_fuzz_inputs.py holds this module to what the GPU test relies on.

    DOORS                       the seven doors
    case(door, seed0, i)        -> Case: the constructor parameters, the packed blocks, two_bit, slot, max_files / max_records,
                                   stage_bytes; deterministic from default_rng([seed0, door, i])
    predict(door, params, block) -> MUST_TAKE / MUST_NOT / EITHER
    expected_below, tau, taken  bplan's rules of finch_rs_amd/csrc/fh_batch_plan.h restated in Python's integers

A block is a packed stream: sequence bytes, a 0 byte (the breaker) behind a record.  The batch doors take a file of many records
a block; the record doors take one record a block, and a block of theirs holds no breaker.

The blocks follow tools/fuzz_batch.py's make_file -- empty, tiny, lengths on tile edges and on the edges of the threshold, a tiled
repeat, N-rich and lower-case text, many short records -- capped at the smallest sizes that reach every path: 60 000 positions a
block (120 000 for the large door, whose threshold appears only above 4 x 16 384), twelve blocks a case."""
import functools
import os
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O

DOORS = ("batch_mash", "batch_scaled", "wide", "large", "counts", "records", "records_stream")
MUST_TAKE, MUST_NOT, EITHER = "must_take", "must_not", "either"
# the classes a door can have at all: a count is exact for any input, a record door has no guess that may or may not hold
CLASSES = {"batch_mash": (MUST_TAKE, MUST_NOT, EITHER), "batch_scaled": (MUST_TAKE, MUST_NOT), "wide": (MUST_TAKE, MUST_NOT, EITHER),
           "large": (MUST_TAKE, MUST_NOT, EITHER), "counts": (MUST_TAKE,), "records": (MUST_TAKE, MUST_NOT),
           "records_stream": (MUST_TAKE, MUST_NOT)}

KIND_MASH, KIND_SCALED, KIND_ALL_COUNTS = 0, 1, 2
K_RANGE = {"batch_mash": (1, 32), "batch_scaled": (1, 32), "wide": (33, 64), "large": (1, 32), "counts": (1, 7), "records": (1, 32),
           "records_stream": (1, 32)}
MASH_SIZES = {"batch_mash": (1, 10, 200, 1000, 2000, 2001, 3000), "wide": (1, 10, 200, 1000, 2000, 2001, 3000),
              "large": (3001, 4096, 10000, 16384), "records": (1, 10, 200, 1000, 2000, 2001, 3000), "records_stream": (1, 50, 1000, 1024)}
SCALED_SIZES = (0, 10, 1000)
SCALES = (0.001, 0.01, 0.1, 1.0)
SEEDS = (0, 42, 2**63 + 5)
MAX_FILES = (1, 3, 8)
MAX_RECORDS = (4, 16, 512)
MAX_BLOCKS = 12
MAX_POSITIONS = 60_000
MAX_POSITIONS_LARGE = 120_000
SCALE_ONE_POSITIONS = 2000   # a scale of 1.0 keeps every distinct hash: only for blocks of at most this many positions

# --- fh_batch_plan.h (bplan) and the record doors' bounds, restated ---
EMPTY = (1 << 64) - 1
SMALL_ROWS = 12288           # keys the batch epilogue's workgroup holds in LDS (SMALL_MAX, FH_BATCH_SCALED_MAX)
LARGE_WANT = 4               # a large file's threshold: LARGE_WANT x n hashes expected below it
FIN_OK = 2
LDS_POSITIONS = 8192         # max_positions of the record sketcher's LDS form
STREAM_POSITIONS = 1 << 24   # ... of the streamed form
STREAM_CAP = 1024            # hashes the streamed form keeps of a record

N_CASES = int(os.environ.get("FH_DOOR_FUZZ_CASES", "12"))
SEED0 = int(os.environ.get("FH_DOOR_FUZZ_SEED", "7100"))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def expected_below(n):
    """fh_batch_plan.h, expected_below: the small and wide doors"""
    return 4 * n if n <= 2000 else 3 * n


def tau(E_, length):
    """fh_batch_plan.h, tau: the threshold of a Mash file of `length` positions with E_ hashes expected below it"""
    if length <= E_:
        return EMPTY
    t = (E_ << 64) // length
    return EMPTY if t >= EMPTY - 1 else t


def taken(kind, size, file_tau, sorted_, overflow, need_big, n_coll, n_live, sp_count, inserted_total):
    """fh_batch_plan.h, taken: the epilogue finished the sketch and left the partition reset, the guess held (or admitted
    everything), no collision record, the hash that cannot be a table key did not occur, no more rows than the result holds"""
    scaled = kind == KIND_SCALED
    fin = sorted_ == FIN_OK and overflow == 0 and need_big == 0
    full = n_live >= size if scaled else (file_tau == EMPTY or inserted_total >= size)
    rows = n_live <= (SMALL_ROWS if scaled else size)
    return bool(fin and full and n_coll == 0 and sp_count == 0 and rows)


def wanted_below(door, size):
    """E of a Mash door: the hashes expected at or below a file's threshold"""
    return LARGE_WANT * size if door == "large" else expected_below(size)


# --- the blocks ---

def _text(rng, n, p_n=0.0, p_low=0.0):
    seq = rng.choice(ACGT, size=n)
    m = rng.random(n)
    seq[m < p_n] = ord("N")
    low = m > 1 - p_low
    seq[low] |= 0x20
    return seq


def _log_uniform(rng, lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))) if hi > lo else lo


def _cut_into_records(rng, seq, n_rec):
    cuts = np.sort(rng.integers(0, len(seq) + 1, size=n_rec - 1)) if n_rec > 1 else np.zeros(0, np.int64)
    parts, prev = [], 0
    for c in list(cuts) + [len(seq)]:
        parts += [seq[prev:c], np.zeros(1, np.uint8)]
        prev = int(c)
    return np.concatenate(parts)


def make_block(rng, door, edge, cap):
    """one block of at most `cap` positions; `edge`: the length at which a Mash file's threshold appears (0: the door has none)"""
    one_record = door in ("records", "records_stream")
    edges = [2047, 2048, 2049, 8191, 8192, 8193, 16384] + ([edge - 1, edge, edge + 1] * 2 if edge else [])
    # the large door's threshold appears at 12 004 .. 65 536 positions, and every file above it that holds its guess has more than
    # SMALL_ROWS hashes below it -- `either`, for all but n = 3001: most of its blocks stay at or below the edge
    weights = {"large": (1, 2, 5, 1, 2, 2, 7)}.get(door, (1, 2, 4, 1, 3, 3, 6))
    kind = int(rng.choice(7, p=np.array(weights) / sum(weights)))
    if kind == 0:
        return np.zeros(0, np.uint8)
    if kind == 1:  # tiny
        L = int(rng.integers(1, 201))
    elif kind == 2:  # tile edges, the LDS form's bound, the threshold's edge
        L = int(rng.choice([e for e in edges if 1 <= e <= cap] or [cap]))
    elif door == "large" and rng.random() < 0.7:
        L = _log_uniform(rng, 200, min(cap, max(200, edge)))
    else:
        L = _log_uniform(rng, 200, cap)
    L = min(L, cap)
    if kind == 3:  # a tiled repeat
        unit = rng.choice(ACGT, size=int(rng.integers(1, 401)))
        seq = np.tile(unit, L // len(unit) + 1)[:L]
        return seq if one_record else np.concatenate([seq[:L - 1], np.zeros(1, np.uint8)])
    if kind == 4:  # N-rich and lower-case text
        seq = _text(rng, L, p_n=float(rng.choice([0.0005, 0.01, 0.2])), p_low=float(rng.choice([0.0, 0.02, 0.5])))
        if rng.random() < 0.2:
            seq[rng.random(L) < 0.01] = ord("U")
    else:
        seq = _text(rng, L, p_n=float(rng.choice([0.0, 0.0, 0.0005])), p_low=float(rng.choice([0.0, 0.02])))
    if one_record:
        return seq
    if kind == 5:  # many short records in one file
        n_rec = int(rng.integers(2, 2 + max(1, min(50, L // 20))))
    else:
        n_rec = int(rng.integers(1, 4))
    # the block has exactly L positions, breakers included -- the length the threshold is worked out from
    n_rec = min(n_rec, L)
    return _cut_into_records(rng, seq[:L - n_rec], n_rec)[:L]


class Case(SimpleNamespace):
    pass


@functools.lru_cache(maxsize=None)
def _k_order(door, seed0):
    """a door's k, uniform over its range: a permutation of the range walked case by case, so that every k occurs in every
    run of as many cases as the range has"""
    lo, hi = K_RANGE[door]
    return [int(x) for x in np.random.default_rng([seed0, DOORS.index(door)]).permutation(np.arange(lo, hi + 1))]


def case(door, seed0, i):
    rng = np.random.default_rng([seed0, DOORS.index(door), i])
    order = _k_order(door, seed0)
    c = Case(door=door, seed0=seed0, index=i, k=order[i % len(order)], kind=KIND_MASH, size=0, scale=0.0, seed=0)
    if door == "counts":
        c.kind = KIND_ALL_COUNTS
    else:
        scaled = {"batch_mash": 0.0, "batch_scaled": 1.0, "large": 0.0, "wide": 0.4}.get(door, 0.5)
        c.kind = KIND_SCALED if rng.random() < scaled else KIND_MASH
        c.seed = SEEDS[int(rng.integers(0, len(SEEDS)))]
        if c.kind == KIND_MASH:
            c.size = int(rng.choice(MASH_SIZES[door]))
        else:
            # (a batch door takes a Scaled file only if `size` hashes lie at or below max_hash, and a size of 1000 at a scale of
            # 0.001 asks for a million positions: the small sizes and the large scales are drawn more often there)
            batch = door in ("batch_scaled", "wide")
            c.size = int(rng.choice(SCALED_SIZES, p=[0.5, 0.35, 0.15] if batch else None))
            # (... and the streamed record door refuses a Scaled record only above `stream_cap` rows: 10 240 positions at 0.1)
            c.scale = float(rng.choice(SCALES, p=[0.15, 0.25, 0.35, 0.25] if batch or door == "records_stream" else None))
    cap = MAX_POSITIONS_LARGE if door == "large" else MAX_POSITIONS
    if c.kind == KIND_SCALED and c.scale == 1.0:
        cap = SCALE_ONE_POSITIONS
    edge = wanted_below(door, c.size) if c.kind == KIND_MASH and door in ("batch_mash", "wide", "large") else 0
    c.blocks = [make_block(rng, door, edge, cap) for _ in range(int(rng.integers(3, MAX_BLOCKS + 1)))]
    for b in c.blocks:
        b.setflags(write=False)
    if door in ("records", "records_stream"):
        c.max_records, c.max_files = int(rng.choice(MAX_RECORDS)), None
        c.two_bit = True  # the record doors have the two-bit form only
        c.max_positions = STREAM_POSITIONS if door == "records_stream" else LDS_POSITIONS
        c.stream_cap = STREAM_CAP
    else:
        c.max_files, c.max_records = int(rng.choice(MAX_FILES)), None
        c.two_bit = bool(rng.integers(0, 2))
    c.slot = int(rng.integers(0, 2))
    # the smallest staging buffer that holds the longest block (a submit per block or two), a quarter of a MiB, or everything
    least = max(4096, (max(len(b) for b in c.blocks) + 64 + 4095) & ~4095)
    c.stage_bytes = int(rng.choice([least, max(least, 1 << 18), 1 << 20]))
    return c


def cases(door, seed0=None, n=None):
    return [case(door, SEED0 if seed0 is None else seed0, i) for i in range(N_CASES if n is None else n)]


# --- what the oracle says ---

def oracle_all(block, k, seed):
    """an unbounded Mash oracle of the block: every distinct hash with its counts -> (kc, kmers, total valid k-mers)"""
    o = O.OracleSketcher(O.MASH, len(block) + 1, k, seed)
    o.process_packed(np.ascontiguousarray(block), 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1]


def oracle_sketch(block, kind, size, k, seed, scale):
    """the oracle's sketch of the block at the handle's parameters -> (kc, kmers, total valid k-mers)"""
    o = O.OracleSketcher(O.SCALED if kind == KIND_SCALED else O.MASH, size, k, seed, scale if kind == KIND_SCALED else 0.001)
    o.process_packed(np.ascontiguousarray(block), 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1]


def max_hash_of(c):
    return O.OracleSketcher(O.SCALED, c.size, c.k, c.seed, c.scale).max_hash


def predict(door, c, block):
    """whether `door`, made with the parameters of `c`, takes `block`: from the oracle alone"""
    if door == "counts":
        return MUST_TAKE
    if door in ("records", "records_stream"):
        if len(block) > c.max_positions:
            return MUST_NOT
        if door == "records_stream" and c.kind == KIND_SCALED:
            if len(oracle_sketch(block, c.kind, c.size, c.k, c.seed, c.scale)[0]) > c.stream_cap:
                return MUST_NOT
        return MUST_TAKE
    kc = oracle_all(block, c.k, c.seed)[0]
    twice = door == "wide" and len(kc) > 0 and int(kc["count"].max()) >= 2  # the collision log may hold a record of it
    if c.kind == KIND_SCALED:
        mh = max_hash_of(c)
        assert mh < EMPTY or not (kc["hash"] == np.uint64(EMPTY)).any()  # (scale 1.0: the block does not need the hash 2^64 - 1)
        D = int((kc["hash"] <= np.uint64(mh)).sum())
        if c.size <= D <= SMALL_ROWS:
            return EITHER if twice else MUST_TAKE
        return MUST_NOT
    t = tau(wanted_below(door, c.size), len(block))
    D = int((kc["hash"] <= np.uint64(t)).sum())
    if t != EMPTY and D < c.size:
        return MUST_NOT
    if t != EMPTY and D > SMALL_ROWS:
        return EITHER  # the partition's lists decide
    return EITHER if twice else MUST_TAKE
