"""Every k-mer length through every per-k kernel family.  The sketch kernels are templates on K -- the key's word geometry, the
murmur tail, the lookup-table set, the window mask, a lane's halo and the one- or two-word canonical compare all change with it --
so each family is 32 or 64 different programs, and each of them sketches tests/every_k_inputs.py's stream for its k here: a small
input that sits on the k-dependent edges.  The result is held bit for bit to the CPU oracle (hashes, counts, extra_counts, k-mer
bytes, total valid k-mers), and WHICH files a batch door takes is asserted from the prediction tests/test_every_k_inputs.py holds:
`small` at every k, `packed` iff k >= 7.

    tile kernels              fh_k2.hip (k <= 32), fh_k2w.hip (k >= 33)      HipSketcher.push_block of the ragged stream
    two-word segment kernel   fh_k2ws.hip (k >= 33)                          fixed-length reads, stride told
    batch / wide batch        fh_k2b.hip (k <= 32), fh_k2bw.hip (k >= 33)    F.BatchSketcher / .wide, bytes and two-bit form
    large batch               fh_k2b.hip + fh_batch_large.hip (k <= 32)      F.BatchSketcher.large, n = 3001
    record sketcher           fh_records.hip (k <= 32)                       F.RecordSketcher, seed 0 / seed != 0, Scaled
    streamed record sketcher  fh_records.hip, k_record_stream (k <= 32)      F.RecordSketcher(stream=True), the same three; E.stream_records

(fh_k2s.hip has its own sweep: test_gpu_segments.py, test_every_k_on_two_and_four_lanes.)

What the sweep found when it was written: the wide batch door did not take `small` at ANY k = 33..64.  The file is admitted whole,
so A^k from the runs of A and T reaches the table 2 (2 k + 1) times, several of them in one drain; the occurrence that claimed
the entry stored the k-mer's high word, and an occurrence of the same k-mer that read the word before the store had landed
logged itself as a possible collision (fh_k2_common.h, wide_kmer_update) -- never a wrong sketch, but the file went the long
way.  Both words are now set by compare-and-swap; test_wide_batch's `small` file is the regression test.

Needs a real MI355X (`-m gpu`)."""
import functools

import numpy as np
import pytest

import every_k_inputs as E
import finch_rs_amd as F
from finch_rs_amd._lib import KIND_MASH, KIND_SCALED
from oracle import oracle as O
from test_gpu_batch_wide import same_as
from test_gpu_parity import assert_same
from test_gpu_records import run as run_records
from test_gpu_records_stream import run as run_streamed
from test_gpu_segments import fixed_reads, oracle_of, packed as pack_reads, sketch_on_device

pytestmark = pytest.mark.gpu

K_ALL = list(range(1, 65))
K_ONE = list(range(1, 33))    # one-word k-mers
K_TWO = list(range(33, 65))   # two-word k-mers
SEEDS = [0, 42]               # the kernels are instantiated for seed 0 and for any other
N_SMALL, SMALL_LIMIT = 200, 700       # (tests/test_every_k_inputs.py holds the taken prediction at these)
N_LARGE, LARGE_LIMIT = 3001, 11000
FIRST_TAKEN_K = 7             # `packed` has fewer than n distinct hashes below its threshold for k <= 6


@pytest.fixture(autouse=True)
def _release_parked_handles():
    """handles are parked by their parameters when freed: 64 k x five doors would keep gigabytes"""
    yield
    F.load().fh_release_cached()


def file_of(k, which):
    return E.stream(k)[1] if which == "packed" else E.small(k, SMALL_LIMIT if which == "small" else LARGE_LIMIT)


@functools.lru_cache(maxsize=None)
def oracle(k, which, kind, n, seed, scale=0.001):
    """the oracle's sketcher after one file of the k's input: computed once, shared by the doors, never changed"""
    o = O.OracleSketcher(kind, n, k, seed, scale)
    o.process_packed(file_of(k, which), 0)
    return o


def oracle_rows(k, which, n, seed):
    o = oracle(k, which, O.MASH, n, seed)
    return o.to_vec() + (o.total_bases_and_kmers()[1],)


# --- the tile kernels ---

@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", K_ALL)
def test_tile_kernels(k, seed):
    sk = F.SketchParams.mash(N_SMALL, N_SMALL, True, k, seed).create_sketcher()
    sk.push_block(E.stream(k)[1])
    assert_same(sk, oracle(k, "packed", O.MASH, N_SMALL, seed), "k=%d seed=%d" % (k, seed))
    assert sk.debug_segments()[0] == 0  # a ragged stream: the segment kernels stayed out
    sk.close()


@pytest.mark.parametrize("k", K_ALL)
def test_tile_kernels_scaled(k):
    sk = F.SketchParams.scaled(10, k, 0.05, 0).create_sketcher()
    sk.push_block(E.stream(k)[1])
    assert_same(sk, oracle(k, "packed", O.SCALED, 10, 0, 0.05), "scaled k=%d" % k)
    assert sk.debug_segments()[0] == 0
    sk.close()


# --- the two-word segment kernel ---

@functools.lru_cache(maxsize=None)
def genome():
    return np.random.default_rng(77).choice(E.ACGT, size=100_000)


@pytest.mark.parametrize("k", K_TWO)
def test_two_word_segment_kernel(k):
    """reads of k + 38 bases: 39 windows a read, the stride in the range that gives a read to one lane; 600 + k reads are no
    multiple of the 64 a tile holds"""
    L = k + 38
    rng = np.random.default_rng(33000 + k)
    stream = pack_reads(fixed_reads(rng, 600 + k, L, genome()))
    sk, _ = sketch_on_device(F.SketchParams.mash(N_SMALL, N_SMALL, True, k, 0), stream, L + 1)
    launches, _, stride = sk.debug_segments()
    assert launches > 0 and stride == L + 1  # (through another kernel the case would prove nothing)
    assert_same(sk, oracle_of(O.MASH, N_SMALL, k, stream), "k=%d" % k)
    sk.close()


# --- the batch doors ---

def through_a_sketcher(k, which, n, seed):
    """what the caller does with a file the batch path did not take"""
    sk = F.SketchParams.mash(n, n, True, k, seed).create_sketcher()
    sk.push_block(file_of(k, which))
    assert_same(sk, oracle(k, which, O.MASH, n, seed), "k=%d %s through a sketcher" % (k, which))
    sk.close()


def check_batch(b, k, files, n, seed, two_bit):
    res = b.sketch_many([file_of(k, w) for w in files], two_bit=two_bit)
    assert len(res) == len(files)
    taken = 0
    for i, (which, r) in enumerate(zip(files, res)):
        ctx = "k=%d seed=%d two_bit=%s file %d (%s)" % (k, seed, two_bit, i, which)
        if which == "packed" and k < FIRST_TAKEN_K:
            assert r is None, ctx  # fewer than n distinct hashes at or below its threshold: never a sketch
            through_a_sketcher(k, which, n, seed)
        else:
            assert r is not None, (ctx, "not taken", b.counters())
            same_as(r, oracle_rows(k, which, n, seed), ctx)
            taken += 1
    assert b.counters() == {"taken": taken, "not_taken": len(files) - taken}
    b.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("two_bit", [False, True])
@pytest.mark.parametrize("k", K_ONE)
def test_batch(k, two_bit, seed):
    """two files to a batch: the third file goes to the partition the first one used"""
    b = F.BatchSketcher(N_SMALL, k, seed, max_files=2, stage_bytes=1 << 20)
    check_batch(b, k, ["packed", "small", "packed"], N_SMALL, seed, two_bit)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("two_bit", [False, True])
@pytest.mark.parametrize("k", K_TWO)
def test_wide_batch(k, two_bit, seed):
    b = F.BatchSketcher.wide(N_SMALL, k, seed, max_files=2, stage_bytes=1 << 20)
    check_batch(b, k, ["packed", "small", "packed"], N_SMALL, seed, two_bit)


@pytest.mark.parametrize("two_bit", [False, True])
@pytest.mark.parametrize("k", K_ONE)
def test_large_batch(k, two_bit):
    b = F.BatchSketcher.large(N_LARGE, k, 0, max_files=2, stage_bytes=1 << 20)
    check_batch(b, k, ["packed", "small_large"], N_LARGE, 0, two_bit)


# --- the record sketcher ---

@pytest.mark.parametrize("kind,size,seed,scale", [(KIND_MASH, 50, 0, 0.0), (KIND_MASH, 50, 42, 0.0), (KIND_SCALED, 10, 7, 0.05)],
                         ids=["mash-seed0", "mash-seed42", "scaled-seed7"])
@pytest.mark.parametrize("k", K_ONE)
def test_record_sketcher(k, kind, size, seed, scale):
    """the records of the stream one by one: every one is taken (all are within max_positions, and random records of these
    lengths have no 64-bit collision) and equals the oracle's sketch of that record; the counters say the same"""
    records = E.stream(k)[0]
    res = run_records(records, size, k, seed, kind=kind, scale=scale, ctx="k=%d" % k, max_records=512)
    assert len(res) == len(records) and all(r is not None for r in res)


# --- the streamed record sketcher ---

@pytest.mark.parametrize("kind,size,seed,scale", [(KIND_MASH, 1000, 0, 0.0), (KIND_MASH, 50, 42, 0.0), (KIND_SCALED, 10, 7, E.STREAM_SCALE)],
                         ids=["mash-seed0", "mash-seed42", "scaled-seed7"])
@pytest.mark.parametrize("k", K_ONE)
def test_streamed_record_sketcher(k, kind, size, seed, scale):
    """E.stream_records(k): a record of six rounds with N around every round seam, a window alone across one, a block that recurs
    as its reverse complement behind a fold; one of 8193 positions; one of k + 1.  All three are taken (tests/test_every_k_inputs.py
    holds the Scaled row counts within the cap) and each equals the oracle's sketch of that record; the counters say the same.
    The other fold rule runs the same records in tests/test_gpu_records_stream.py's `every_k`."""
    records = E.stream_records(k)
    res, folds = run_streamed(records, size, k, seed, kind=kind, scale=scale, ctx="k=%d" % k, max_records=16)
    assert len(res) == len(records) and all(r is not None for r in res)
    if size == 1000:
        # the long record folds behind its second round (the key array could not take a third) and at its end; for k <= 5 the
        # list never fills, the threshold never falls and every round's keys survive: a fold behind every round from the second
        assert folds >= 2, folds
