"""Many sketches per launch at Mash sizes 3001..16384 (fh_batch_new_large, k_batch_epilogue_large in fh_batch_large.hip): every
file the batch path TAKES carries the oracle's sketch bit for bit -- hashes, k-mer bytes, counts, extra counts, total k-mers --
and which files it takes is predicted, not merely counted: a random genome of ~12 n positions has Binomial(len, 4 n / len)
hashes below its threshold (mean 4 n, sd <= 256), more than 20 sd away from both n and the live capacity (4 n + 8192), so it
MUST be taken; a file with fewer than n distinct hashes below its threshold must NOT be, and the partition it used must come
back clean.  Through the C ABI and through sketch_files; needs a real MI355X (`-m gpu`)."""
import functools

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd import sketch_schemes as S
from finch_rs_amd.sketch_schemes import SketchParams
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SIZES = [3001, 4096, 4097, 8192, 8193, 10000, 12288, 12289, 16384]  # both sides of every chunk of the sort, and the ends
KS = [11, 21, 31, 32]


@pytest.fixture(autouse=True)
def _options_back():
    yield
    F.debug_set(batch_large_want=None, batch_large_files=None, file_batch=None, pool=None)


def oracle_sketch(block, n, k, seed):
    ora = O.OracleSketcher(O.MASH, n, k, seed)
    ora.process_packed(np.ascontiguousarray(block, dtype=np.uint8), 0)
    okc, okm = ora.to_vec()
    return okc, okm, ora.total_bases_and_kmers()[1]


def same_as(res, want, ctx=""):
    assert res is not None, (ctx, "not taken")
    kc, km, _, tk = res
    okc, okm, otk = want
    assert len(kc) == len(okc), (ctx, len(kc), len(okc))
    assert np.array_equal(kc["hash"], okc["hash"]), ctx
    assert np.array_equal(kc["count"], okc["count"]), ctx
    assert np.array_equal(kc["extra_count"], okc["extra_count"]), ctx
    assert km.shape == okm.shape and np.array_equal(km, okm), ctx
    assert tk == otk, (ctx, tk, otk)


def genome_block(rng, length, n_records=1, p_n=0.0, p_lower=0.0, n_runs=0):
    """a packed stream: n_records records of random bases (some lower case, single N and runs of N), a breaker byte behind each"""
    parts = []
    per = max(1, length // n_records)
    for _ in range(n_records):
        r = rng.choice(ACGT, size=per)
        m = rng.random(per)
        r[m < p_n] = ord("N")
        if p_lower:
            low = m > 1 - p_lower
            r[low] = r[low] | 0x20
        for _ in range(n_runs):
            at = int(rng.integers(0, max(1, per - 40)))
            r[at:at + int(rng.integers(2, 40))] = ord("N")
        parts.append(r)
        parts.append(np.zeros(1, np.uint8))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def parity_blocks(n):
    """two files of ~12 n positions: a plain genome, and one of several records with N runs and lower case"""
    rng = np.random.default_rng(n)
    return (genome_block(rng, 12 * n), genome_block(rng, 12 * n + 777, n_records=5, p_n=0.0003, p_lower=0.02, n_runs=3))


@functools.lru_cache(maxsize=None)
def parity_oracle(n, k, seed):
    return tuple(oracle_sketch(b, n, k, seed) for b in parity_blocks(n))


# --- parity: every n around the sort's chunks, every compile part of k2_batch, both seeds' kernels, both input forms ---

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_genomes_match_the_oracle(n, k):
    blocks = parity_blocks(n)
    for seed in (0, 42):
        want = parity_oracle(n, k, seed)
        b = F.BatchSketcher.large(n, k, seed, max_files=2, stage_bytes=1 << 20)
        for two_bit in (False, True):
            res = b.sketch_many(blocks, two_bit=two_bit)
            for i, (r, w) in enumerate(zip(res, want)):
                assert len(w[0]) == n
                same_as(r, w, "n %d k %d seed %d two_bit %s file %d" % (n, k, seed, two_bit, i))  # (taken, and the oracle's)
        assert b.counters() == {"taken": 4, "not_taken": 0}
        b.close()
    _lib.load().fh_release_cached()


# --- files that come up short ---

def test_too_few_distinct_kmers_are_not_taken_and_the_partition_comes_back_clean():
    """a 3 kb genome repeated (3000 distinct 21-mers, a finite threshold) and a file at k = 7 (at most 8192 canonical 7-mers): not
    taken; the next batch in the same slot -- files that use the same partitions -- is the oracle's"""
    rng = np.random.default_rng(1)
    n, k = 4096, 21
    unit = rng.choice(ACGT, size=3000)
    repeat = np.concatenate([np.tile(unit, 20), np.zeros(1, np.uint8)])
    good = [genome_block(rng, 12 * n), genome_block(rng, 11 * n, n_records=3)]
    b = F.BatchSketcher.large(n, k, 0, max_files=2, stage_bytes=1 << 20)
    for two_bit in (False, True):
        res = b.sketch_many([repeat, good[0]], two_bit=two_bit)
        assert res[0] is None
        same_as(res[1], oracle_sketch(good[0], n, k, 0))
        res = b.sketch_many(good[::-1], two_bit=two_bit)  # (file 0's partition was swept, file 1's reset slot by slot)
        for r, blk in zip(res, good[::-1]):
            same_as(r, oracle_sketch(blk, n, k, 0))
    assert b.counters() == {"taken": 6, "not_taken": 2}
    b.close()
    # k = 7: 120 kb at n = 10 000 are sketched at a threshold that admits a third of the 8192 possible hashes: short.  A 30 kb
    # file lies below 4 n positions, everything is admitted, and its < n hashes ARE the sketch (mash.rs:37-60): taken.
    n, k = 10000, 7
    short, whole = genome_block(rng, 120_000), genome_block(rng, 30_000, n_records=2)
    b = F.BatchSketcher.large(n, k, 5, max_files=2, stage_bytes=1 << 20)
    res = b.sketch_many([short, whole])
    assert res[0] is None
    want = oracle_sketch(whole, n, k, 5)
    assert 7000 < len(want[0]) <= 8192  # (most of the 8192 canonical 7-mers, all below n)
    same_as(res[1], want)
    res = b.sketch_many([whole, short], two_bit=True)
    same_as(res[0], want)
    assert res[1] is None
    b.close()


def distinct_below(block, n, k, seed, want):
    """distinct hashes of `block` at or below the threshold a large handle sketches it at with batch_large_want = want"""
    tau = ((want * n) << 64) // len(block)
    okc = oracle_sketch(block, 3 * want * n, k, seed)[0]
    assert len(okc) < 3 * want * n or int(okc["hash"][-1]) > tau  # (the oracle saw past the threshold)
    return int((okc["hash"] <= np.uint64(tau)).sum())


def test_a_short_guess_is_not_taken_never_wrong():
    """batch_large_want=1: a file's threshold has n hashes expected below it, so about half the files come up short -- WHICH is
    predicted from the oracle; the rest are the oracle's sketches"""
    rng = np.random.default_rng(2)
    n, k = 5000, 21
    blocks = [genome_block(rng, 12 * n + 1000 * i) for i in range(8)]
    F.debug_set(batch_large_want="1")
    D = [distinct_below(blk, n, k, 0, 1) for blk in blocks]
    assert any(d < n for d in D) and any(d >= n for d in D), D
    b = F.BatchSketcher.large(n, k, 0, max_files=8, stage_bytes=2 << 20)
    for two_bit in (False, True):
        res = b.sketch_many(blocks, two_bit=two_bit)
        for i, (r, blk, d) in enumerate(zip(res, blocks, D)):
            if d < n:
                assert r is None, (i, d)
            else:
                same_as(r, oracle_sketch(blk, n, k, 0), "file %d D %d" % (i, d))
    b.close()


def test_a_full_live_list_is_not_taken_and_leaves_the_handle_clean():
    """batch_large_want=8 at n = 4096: 32 768 hashes expected below the threshold, the live list holds 24 576 -- every file
    overflows it and is not taken; with the option cleared the same handle, and a fresh one, are exact"""
    rng = np.random.default_rng(3)
    n, k = 4096, 31
    blocks = [genome_block(rng, 12 * n), genome_block(rng, 13 * n, n_records=2), genome_block(rng, 12 * n + 99)]
    b = F.BatchSketcher.large(n, k, 9, max_files=4, stage_bytes=1 << 20)
    F.debug_set(batch_large_want="8")
    assert b.sketch_many(blocks) == [None, None, None]
    assert b.sketch_many(blocks, slot=1, two_bit=True) == [None, None, None]
    F.debug_set(batch_large_want=None)
    for slot in (0, 1):
        for r, blk in zip(b.sketch_many(blocks, slot=slot), blocks):
            same_as(r, oracle_sketch(blk, n, k, 9))
    assert b.counters() == {"taken": 6, "not_taken": 6}
    b.close()
    _lib.load().fh_release_cached()
    b = F.BatchSketcher.large(n, k, 9, max_files=4, stage_bytes=1 << 20)
    for r, blk in zip(b.sketch_many(blocks), blocks):
        same_as(r, oracle_sketch(blk, n, k, 9))
    b.close()


# --- slots and handles ---

def test_two_slots_alternate_over_four_batches():
    rng = np.random.default_rng(4)
    n, k = 3001, 21
    batches = [[genome_block(rng, 12 * n + 500 * (3 * j + i), n_records=1 + i) for i in range(3)] for j in range(4)]
    b = F.BatchSketcher.large(n, k, 0, max_files=3, stage_bytes=1 << 20)

    def submit(slot, blocks):
        buf = b.stage(slot)
        offs, lens, pos = [], [], 0
        for blk in blocks:
            buf[pos:pos + len(blk)] = blk
            offs.append(pos)
            lens.append(len(blk))
            pos = (pos + len(blk) + 63) & ~63
        b.submit(slot, offs, lens)

    def collect(slot, blocks):
        st = b.wait(slot, len(blocks))
        assert not st.any()
        for i, blk in enumerate(blocks):
            same_as(b.result(slot, i), oracle_sketch(blk, n, k, 0), "slot %d file %d" % (slot, i))

    submit(0, batches[0])
    submit(1, batches[1])  # (both in flight)
    collect(0, batches[0])
    submit(0, batches[2])
    collect(1, batches[1])
    submit(1, batches[3])
    collect(0, batches[2])
    collect(1, batches[3])
    assert b.counters() == {"taken": 12, "not_taken": 0}
    b.close()


def test_a_full_batch_with_an_empty_and_a_one_record_file():
    """max_files files in one batch, among them an empty file, one shorter than k, and a single short record whose every hash is
    admitted (fewer than n of them: that IS the sketch)"""
    rng = np.random.default_rng(6)
    n, k, F_MAX = 3001, 21, 8
    blocks = [genome_block(rng, 12 * n + 64 * i) for i in range(F_MAX - 3)]
    blocks.insert(1, np.zeros(0, np.uint8))
    blocks.insert(3, np.frombuffer(b"ACGTACGT\0", dtype=np.uint8))
    blocks.append(genome_block(rng, 2500))
    assert len(blocks) == F_MAX
    b = F.BatchSketcher.large(n, k, 0, max_files=F_MAX, stage_bytes=1 << 20)
    for two_bit in (False, True):
        res = b.sketch_many(blocks, two_bit=two_bit)
        for i, (r, blk) in enumerate(zip(res, blocks)):
            want = oracle_sketch(blk, n, k, 0)
            same_as(r, want, "file %d" % i)
        assert len(res[1][0]) == 0 and len(res[3][0]) == 0 and 2000 < len(res[-1][0]) < n
    b.close()


def test_parked_handles_are_matched_on_large_n_k_seed():
    """a parked large handle goes to fh_batch_new_large with the same n, k and seed only -- not to a small or wide request, not
    to another n -- and with pool=0 nothing is parked"""
    rng = np.random.default_rng(7)
    blk = genome_block(rng, 60_000)
    kw = dict(max_files=2, stage_bytes=1 << 20)
    _lib.load().fh_release_cached()
    assert F.BatchSketcher.parked() == (0, 0, 0)
    a = F.BatchSketcher.large(5000, 21, 0, **kw)
    same_as(a.sketch_many([blk])[0], oracle_sketch(blk, 5000, 21, 0))
    a.close()
    all_, large, nbytes = F.BatchSketcher.parked()
    assert (all_, large) == (1, 1) and nbytes > 2 * 28672 * 128  # (two partitions of live_cap 28 672)
    for other in (lambda: F.BatchSketcher(1000, 21, 0, **kw), lambda: F.BatchSketcher.wide(1000, 33, 0, **kw),
                  lambda: F.BatchSketcher.large(5001, 21, 0, **kw), lambda: F.BatchSketcher.large(5000, 22, 0, **kw),
                  lambda: F.BatchSketcher.large(5000, 21, 1, **kw)):
        o = other()
        assert F.BatchSketcher.parked()[1] == 1  # (the parked one stayed where it was)
        res = o.sketch_many([blk])[0]
        same_as(res, oracle_sketch(blk, o.size, o.kmer_length, o.seed))
        F.debug_set(pool="0")
        o.close()  # (a large one is not parked under pool=0; the small and wide ones follow their own rule)
        F.debug_set(pool=None)
        assert F.BatchSketcher.parked()[1] == 1
    again = F.BatchSketcher.large(5000, 21, 0, **kw)
    assert F.BatchSketcher.parked()[1] == 0  # ... and was handed out for the same parameters
    same_as(again.sketch_many([blk], two_bit=True)[0], oracle_sketch(blk, 5000, 21, 0))
    F.debug_set(pool="0")
    again.close()
    assert F.BatchSketcher.parked()[1] == 0
    F.debug_set(pool=None)
    _lib.load().fh_release_cached()


# --- the host layer on top: finch_sketch_files forms groups for these sizes (fh_host.cpp) ---

def _fasta(seq: bytes, name=b"g", width=70):
    return b">" + name + b"\n" + b"\n".join(seq[j:j + width] for j in range(0, len(seq), width)) + b"\n"


def _stream_oracle(data, n, k, seed):
    o = O.OracleSketcher(O.MASH, n, k, seed)
    o.sketch_stream(data)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()


def _write(tmp_path, datas):
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("f%02d.fa" % i)
        p.write_bytes(d)
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("n", [5000, 10000])
def test_sketch_files_groups_match_the_oracle_and_the_one_by_one_path(tmp_path, n):
    """12 files in groups of 4: one sketch per file in input order, each equal in every field to what file_batch=0 gives and to
    the oracle's sketch_stream.  Eleven genomes have enough k-mers and are taken; a short genome repeated has not, is handed
    to a sketcher of its own and is still the oracle's"""
    k = 21
    datas = [_fasta(bytes(S.synth_genome_host(12 * n + 997 * i, 300 + i)), b"g%d" % i) for i in range(10)]
    datas.insert(4, _fasta(bytes(S.synth_genome_host(3000, 5)) * (5 * n // 3000 + 1), b"repeat"))  # > 4 n positions, 3000 distinct k-mers
    datas.append(b"".join(_fasta(bytes(S.synth_genome_host(3 * n + c, 900 + c)), b"contig%d" % c, width=60) for c in range(4)))
    assert len(datas) == 12
    paths = _write(tmp_path, datas)
    params = SketchParams.mash(n, n, True, k, 0)  # (no_strict: the repeat has fewer than n k-mers)
    F.debug_set(batch_large_files="4")
    t0, n0 = H.debug_file_batch()
    res = H.sketch_files(paths, params, H.FilterParams(None), n_threads=2)
    t1, n1 = H.debug_file_batch()
    assert (t1 - t0, n1 - n0) == (11, 1)
    F.debug_set(file_batch="0")
    ref = H.sketch_files(paths, params, H.FilterParams(None), n_threads=2)
    assert H.debug_file_batch() == (t1, n1)
    F.debug_set(file_batch=None)
    for i, d in enumerate(datas):
        a, b = res.sketch(i), ref.sketch(i)
        assert a.name == b.name == paths[i]
        assert np.array_equal(a.arrays[0], b.arrays[0]) and np.array_equal(a.arrays[1], b.arrays[1]), i
        assert (a.seq_length, a.num_valid_kmers) == (b.seq_length, b.num_valid_kmers), i
        assert a.filter_params == b.filter_params and a.sketch_params == b.sketch_params, i
        okc, okm, totals = _stream_oracle(d, n, k, 0)
        assert np.array_equal(a.arrays[0], okc) and np.array_equal(a.arrays[1], okm), i
        assert (a.seq_length, a.num_valid_kmers) == totals, i
        assert (len(okc) < n) if i == 4 else (len(okc) == n)


def test_sketch_files_keeps_small_groups_at_3000_and_goes_one_by_one_at_k33(tmp_path):
    datas = [_fasta(bytes(S.synth_genome_host(60_000 + 500 * i, 40 + i))) for i in range(4)]
    paths = _write(tmp_path, datas)
    _lib.load().fh_release_cached()
    t0, n0 = H.debug_file_batch()
    res = H.sketch_files(paths, SketchParams.mash(3000, 3000, False, 21, 0), H.FilterParams(None), n_threads=1)
    t1, n1 = H.debug_file_batch()
    assert (t1 - t0, n1 - n0) == (4, 0)
    assert F.BatchSketcher.parked()[1] == 0 and F.BatchSketcher.parked()[0] >= 1  # (a small handle did it)
    for i, d in enumerate(datas):
        okc, okm, _ = _stream_oracle(d, 3000, 21, 0)
        assert np.array_equal(res.sketch(i).arrays[0], okc) and np.array_equal(res.sketch(i).arrays[1], okm)
    res = H.sketch_files(paths, SketchParams.mash(5000, 5000, False, 33, 0), H.FilterParams(None), n_threads=1)
    assert H.debug_file_batch() == (t1, n1)  # k = 33..64 above 3000 hashes: neither taken nor not taken
    for i, d in enumerate(datas):
        okc, okm, _ = _stream_oracle(d, 5000, 33, 0)
        assert np.array_equal(res.sketch(i).arrays[0], okc) and np.array_equal(res.sketch(i).arrays[1], okm)
