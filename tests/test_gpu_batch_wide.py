"""Many sketches per launch at k = 33..64 (fh_batch_new_wide, k2_batch_w in fh_k2bw.hip): every file the batch path TAKES carries
the oracle's sketch bit for bit -- hashes, counts, extra_counts, all k k-mer bytes (two words), total k-mers -- and every file it
does not take is sketched through a HipSketcher and equals the oracle too.  With two-word k-mers the collision log also receives
records that are no collision (fh_k2_common.h, wide_kmer_update), so a file with repeated k-mers may be "not taken" where a
k <= 32 file would be taken: that costs time, never a wrong sketch, and the assertions below say which files MUST be taken.
Through the C ABI and through sketch_files; needs a real MI355X (`-m gpu`)."""
import functools

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd import sketch_schemes as S
from finch_rs_amd._lib import KIND_SCALED
from finch_rs_amd.sketch_schemes import SketchParams
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def oracle_sketch(block, n, k, seed):
    ora = O.OracleSketcher(O.MASH, n, k, seed)
    ora.process_packed(np.frombuffer(block, dtype=np.uint8) if not isinstance(block, np.ndarray) else block, 0)
    okc, okm = ora.to_vec()
    return okc, okm, ora.total_bases_and_kmers()[1]


def same_as(res, want, ctx=""):
    kc, km, _, tk = res
    okc, okm, otk = want
    assert len(kc) == len(okc), (ctx, len(kc), len(okc))
    assert np.array_equal(kc["hash"], okc["hash"]), ctx
    assert np.array_equal(kc["count"], okc["count"]), ctx
    assert np.array_equal(kc["extra_count"], okc["extra_count"]), ctx
    assert km.shape == okm.shape and np.array_equal(km, okm), ctx
    assert tk == otk, (ctx, tk, otk)


def same(res, block, n, k, seed, ctx=""):
    same_as(res, oracle_sketch(block, n, k, seed), ctx)


def genome_block(rng, length, n_records=1, p_n=0.0005, p_lower=0.0):
    """a packed stream: n_records records of random bases, one breaker byte behind each"""
    parts = []
    per = max(1, length // n_records)
    for _ in range(n_records):
        r = rng.choice(ACGT, size=per)
        m = rng.random(per)
        r[m < p_n] = ord("N")
        if p_lower:
            low = m > 1 - p_lower
            r[low] = r[low] | 0x20
        parts.append(r)
        parts.append(np.zeros(1, np.uint8))
    return np.concatenate(parts)


def rec(*pieces):
    """one record from byte strings / arrays, its breaker behind it"""
    return np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, (bytes, bytearray)) else p for p in pieces] + [np.zeros(1, np.uint8)])


def through_sketcher_equals_oracle(block, n, k, seed=0):
    sk = F.SketchParams.mash(n, n, True, k, seed).create_sketcher()
    sk.push_block(block)
    kc, km, _ = sk.to_arrays()
    okc, okm, otk = oracle_sketch(block, n, k, seed)
    assert np.array_equal(kc, okc) and np.array_equal(km, okm) and sk.finish()[1] == otk


# --- parity over K: both ends of every compile part ---

PARITY = [(33, 1000, 0), (40, 1000, 42), (41, 500, 0), (48, 1000, 0), (49, 3000, 7), (56, 1000, 0), (57, 100, 42), (64, 1000, 0)]


@functools.lru_cache(maxsize=None)
def parity_case(k, n, seed):
    """the fifteen blocks of a case and the oracle's sketches of them: computed once, shared by both input forms, never changed"""
    rng = np.random.default_rng(k * 1000 + n + seed)
    lens = [int(x) for x in rng.integers(150_000, 900_000, size=11)] + [2_000_000, 65_536, 2048 * 7, 2048 * 7 + 1]
    blocks = [genome_block(rng, L, n_records=int(rng.integers(1, 6)), p_lower=0.01) for L in lens]
    for b in blocks:
        b.setflags(write=False)
    return blocks, [oracle_sketch(b, n, k, seed) for b in blocks]


@pytest.mark.parametrize("k,n,seed,two_bit", [c + (False,) for c in PARITY] + [c + (True,) for c in PARITY if c[0] in (33, 49, 64)])
def test_batch_of_genomes_matches_oracle(k, n, seed, two_bit):
    blocks, want = parity_case(k, n, seed)
    b = F.BatchSketcher.wide(n, k, seed, max_files=8, stage_bytes=8 << 20)  # (several batches, through both forms of phase A)
    res = b.sketch_many(blocks, two_bit=two_bit)
    assert len(res) == len(blocks)
    # random sequence has no repeated 33-mers: no record can reach the collision log, and the guess of ~4 n hashes below the
    # threshold holds as it does for k <= 32 -- every block is taken
    assert all(r is not None for r in res), (b.counters(), [i for i, r in enumerate(res) if r is None])
    for i, (r, w) in enumerate(zip(res, want)):
        same_as(r, w, "file %d (%d bytes)" % (i, len(blocks[i])))
    assert b.counters() == {"taken": len(blocks), "not_taken": 0}
    b.close()


def test_both_slots_of_one_handle_serve_sketch_many():
    blocks, want = parity_case(33, 1000, 0)
    b = F.BatchSketcher.wide(1000, 33, 0, max_files=8, stage_bytes=8 << 20)
    for slot in (1, 0):
        res = b.sketch_many(blocks[11:], slot=slot, two_bit=bool(slot))
        for r, w in zip(res, want[11:]):
            assert r is not None
            same_as(r, w, "slot %d" % slot)
    b.close()


# --- edges ---

def rc(seq):
    return seq[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def edge_blocks(k):
    rng = np.random.default_rng(500 + k)
    rnd = lambda m: bytes(rng.choice(ACGT, size=m))  # noqa: E731
    six = bytearray(rnd(6000))
    for p in (31, 32, 63, 64, 2047, 2048):
        six[p] = ord("N")
    blocks = {
        "empty": np.zeros(0, np.uint8),
        "short": rec(b"ACGT"),
        "k": rec(rnd(k)),
        "k+1": rec(rnd(k + 1)),
        "900": genome_block(rng, 900, 1),                       # fewer k-mers than n: everything is admitted, all of it kept
        "lane63": rec(b"N" * 2040, rnd(k)),                     # one valid window: starts at 2040 (lane 63 of tile 0), ends in tile 1
        "N-at-word-ends": rec(bytes(six)),
        "repeat18": np.tile(np.frombuffer(b"ACGTTGCATGCATGACCA", dtype=np.uint8), 20000),  # 360 kb, 18 distinct k-mers
        "N5000": rec(b"N" * 5000),                              # no valid window at all, behind a threshold
        "genome": genome_block(rng, 300_000, 1),
    }
    if k == 64:
        # 64-mers whose low word (the last 32 bases) is all ones, the value that doubles as "unclaimed": A^32 T^32 is its own
        # reverse complement (the tie of the canonical choice) on top; a random 32-mer in front of T^32 is not
        blocks["A32T32"] = rec(rnd(1500), b"A" * 32 + b"T" * 32, rnd(1436))
        blocks["x32T32"] = rec(rnd(1500), rnd(32) + b"T" * 32, rnd(1436))
    if k % 2 == 0:
        # reverse-complement palindromes of k bases (even k only): forward and reverse window are the same word
        pals = []
        for _ in range(6):
            h = rnd(k // 2)
            pals += [rnd(200), h + rc(h)]
        blocks["palindromes"] = rec(*pals, rnd(500))
    return blocks


@pytest.mark.parametrize("k", [33, 64, 34])
def test_small_empty_and_degenerate_files(k):
    n = 1000
    blocks = edge_blocks(k)
    names, blks = list(blocks), list(blocks.values())
    b = F.BatchSketcher.wide(n, k, 0, max_files=16, stage_bytes=4 << 20)
    res = dict(zip(names, b.sketch_many(blks)))
    for name in names:
        if res[name] is not None:
            same(res[name], blocks[name], n, k, 0, name)
    # what MUST be taken: the files whose threshold admits everything and hold no k-mer twice, and the plain genome
    for name in ("empty", "short", "900", "genome"):
        assert res[name] is not None, name
    # what must NOT be: fewer than n distinct k-mers below the threshold the file was sketched at
    assert res["N5000"] is None and res["repeat18"] is None
    # ... and whatever was not taken goes through a HipSketcher, which is exact for anything
    for name in names:
        if res[name] is None:
            through_sketcher_equals_oracle(blocks[name], n, k)
    c = b.counters()
    assert c["taken"] + c["not_taken"] == len(blocks)
    assert c["taken"] == sum(1 for r in res.values() if r is not None)
    b.close()


def test_edges_in_the_two_bit_form():
    k, n = 64, 1000
    blocks = edge_blocks(k)
    b = F.BatchSketcher.wide(n, k, 0, max_files=16, stage_bytes=4 << 20)
    res = b.sketch_many(list(blocks.values()), two_bit=True)
    for name, r in zip(blocks, res):
        if r is not None:
            same(r, blocks[name], n, k, 0, name)
    got = dict(zip(blocks, res))
    for name in ("empty", "short", "900", "genome", "lane63"):
        assert got[name] is not None, name
    assert got["N5000"] is None and got["repeat18"] is None
    b.close()


def test_two_slots_alternate_and_partitions_come_back_clean():
    """batch after batch through both slots at k = 48: a partition that held file A's hashes -- and the high words of its k-mers
    -- must hold nothing of them when file B comes to it, including after files that were not taken (whose partition the
    epilogue sweeps, high words included)"""
    rng = np.random.default_rng(11)
    k, n = 48, 1000
    b = F.BatchSketcher.wide(n, k, 0, max_files=4, stage_bytes=2 << 20)
    rounds = []
    for r in range(6):
        blocks = [genome_block(rng, int(rng.integers(50_000, 400_000)), int(rng.integers(1, 4))) for _ in range(4)]
        if r % 2:
            blocks[1] = np.tile(np.frombuffer(b"ACGTTGCATGCATGACCATT", dtype=np.uint8), 5000)  # not taken
        rounds.append(blocks)
    pending = None
    results = []
    for r, blocks in enumerate(rounds):
        slot = r & 1
        buf = b.stage(slot)
        offs, lens, pos = [], [], 0
        for blk in blocks:
            buf[pos:pos + len(blk)] = blk
            offs.append(pos)
            lens.append(len(blk))
            pos = (pos + len(blk) + 15) & ~15
        b.submit(slot, offs, lens)
        if pending is not None:
            ps, pn = pending
            st = b.wait(ps, pn)
            results.append([b.result(ps, j) if st[j] == 0 else None for j in range(pn)])
        pending = (slot, len(blocks))
    ps, pn = pending
    st = b.wait(ps, pn)
    results.append([b.result(ps, j) if st[j] == 0 else None for j in range(pn)])
    for r, (blocks, res) in enumerate(zip(rounds, results)):
        for j, (blk, x) in enumerate(zip(blocks, res)):
            if r % 2 and j == 1:
                assert x is None
            else:
                assert x is not None, (r, j)
                same(x, blk, n, k, 0, "round %d file %d" % (r, j))
    b.close()


# --- Scaled ---

def test_scaled_batch_matches_the_oracle():
    k, size, scale = 51, 1000, 0.001
    rng = np.random.default_rng(51)
    lens = [1_200_000, 2_000_000, 4_000_000, 6_000_000, 500_000]
    blocks = [genome_block(rng, L, n_records=int(rng.integers(1, 5)), p_n=0.0002, p_lower=0.01) for L in lens]
    b = F.BatchSketcher.wide(size, k, 0, max_files=4, stage_bytes=16 << 20, kind=KIND_SCALED, scale=scale)
    res = b.sketch_many(blocks, two_bit=True)
    rows = []
    for i, (r, blk) in enumerate(zip(res, blocks)):
        o = O.OracleSketcher(O.SCALED, size, k, 0, scale)
        o.process_packed(blk, 0)
        okc, okm = o.to_vec()
        D = int((okc["hash"] <= np.uint64(o.max_hash)).sum())
        rows.append(D)
        if i == 4:
            assert D < size and r is None, (D, r is None)  # fewer rows than `size`: the reference keeps hashes above max_hash too
            continue
        assert r is not None, (i, D)
        assert len(okc) == D
        same_as(r, (okc, okm, o.total_bases_and_kmers()[1]), "file %d" % i)
    assert all(1200 * 0.8 < d for d in rows[:4]) and rows[3] > 4096 > rows[1], rows  # the inputs are what the comment says
    assert b.counters() == {"taken": 4, "not_taken": 1}
    b.close()


# --- the host layer on top: finch_sketch_files forms groups for kmer_length 33..64 too ---

def _fasta(seq: bytes, name=b"g", width=70):
    return b">" + name + b"\n" + b"\n".join(seq[j:j + width] for j in range(0, len(seq), width)) + b"\n"


def test_sketch_files_groups_two_word_kmers(tmp_path):
    rng = np.random.default_rng(64)
    datas = [_fasta(bytes(S.synth_genome_host(int(rng.integers(200_000, 600_000)), 700 + i)), b"g%d" % i) for i in range(8)]
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("w%02d.fa" % i)
        p.write_bytes(d)
        paths.append(str(p))
    for k in (51, 64):
        t0, n0 = H.debug_file_batch()
        res = H.sketch_files(paths, SketchParams.mash(1000, 1000, False, k, 0), H.FilterParams(None), n_threads=2)
        t1, n1 = H.debug_file_batch()
        assert (t1 - t0, n1 - n0) == (8, 0), (k, t1 - t0, n1 - n0)  # every file went many-per-launch
        for i, d in enumerate(datas):
            o = O.OracleSketcher(O.MASH, 1000, k, 0)
            o.sketch_stream(d)
            okc, okm = o.to_vec()
            sk = res.sketch(i)
            assert sk.name == paths[i]
            assert np.array_equal(sk.arrays[0], okc) and np.array_equal(sk.arrays[1], okm), (k, i)
            assert (sk.seq_length, sk.num_valid_kmers) == o.total_bases_and_kmers(), (k, i)
