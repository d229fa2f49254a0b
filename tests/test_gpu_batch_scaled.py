"""Scaled sketches many per launch (fh_batch_* with FH_KIND_SCALED, the chunk sort of k_batch_epilogue): every file the batch
path takes carries the oracle's ScaledSketcher sketch bit for bit -- hashes, counts, extra counts, k-mer bytes, total k-mers
(scaled.rs:37-61, 83-101) -- and WHICH files it takes is predicted from the oracle, not merely counted: with D = the file's
distinct hashes at or below max_hash, size <= D <= cap must be taken, D < size and D > cap must not.  The inputs are random
genomes at k >= 11 (plus k = 1 on a tiny file), which have no 64-bit collision, so no file is excused.
Through the C ABI and through sketch_files; needs a real MI355X (`-m gpu`)."""
import gzip

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd import sketch_schemes as S
from finch_rs_amd._lib import KIND_MASH, KIND_SCALED
from finch_rs_amd.sketch_schemes import SketchParams
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAP = F.BatchSketcher.SCALED_MAX_ROWS


def genome_block(rng, length, n_records=1, p_n=0.0002, p_lower=0.01):
    """a packed stream: n_records records of random bases (some lower case, a few N), one breaker byte behind each"""
    parts = []
    per = max(1, length // n_records)
    for _ in range(n_records):
        r = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=per)
        m = rng.random(per)
        r[m < p_n] = ord("N")
        low = m > 1 - p_lower
        r[low] = r[low] | 0x20
        parts.append(r)
        parts.append(np.zeros(1, np.uint8))
    return np.concatenate(parts)


def oracle_scaled(block, size, k, seed, scale):
    """-> (records, k-mers, total k-mers, D)"""
    o = O.OracleSketcher(O.SCALED, size, k, seed, scale)
    o.process_packed(np.frombuffer(block, dtype=np.uint8) if not isinstance(block, np.ndarray) else block, 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1], int((kc["hash"] <= np.uint64(o.max_hash)).sum())


def check(res, block, size, k, seed, scale, ctx=""):
    """the prediction and, for a taken file, the sketch; returns D"""
    okc, okm, otk, D = oracle_scaled(block, size, k, seed, scale)
    if D < size or D > CAP:
        assert res is None, (ctx, "taken with D = %d, size %d" % (D, size))
        return D
    assert res is not None, (ctx, "not taken with D = %d, size %d" % (D, size))
    kc, km, _, tk = res
    assert len(okc) == D  # (the rule: the oracle's sketch holds nothing above max_hash then)
    assert len(kc) == D, (ctx, len(kc), D)
    assert np.array_equal(kc["hash"], okc["hash"]), ctx
    assert np.array_equal(kc["count"], okc["count"]), ctx
    assert np.array_equal(kc["extra_count"], okc["extra_count"]), ctx
    assert np.array_equal(km, okm), ctx
    assert tk == otk, (ctx, tk, otk)
    return D


def scaled_batch(size, k, seed, scale, **kw):
    return F.BatchSketcher(size, k, seed, kind=KIND_SCALED, scale=scale, **kw)


CASES = [
    # k, size, scale, seed, lengths (D ~ length x scale)
    (21, 500, 0.001, 0, [600_000, 900_000, 1_100_000, 2_000_000, 4_000_000, 4_250_000, 5_000_000]),  # both sides of 1024 and of 4096
    (21, 1000, 0.002, 0, [4_000_000, 6_000_000, 300_000, 2_100_000, 5_500_000, 600_000]),             # ~7932, ~12 000 (under the cap), 600 < size
    (31, 0, 0.001, 42, [4_500_000, 100_000, 3_000, 1_000_000]),                                       # size 0: everything is taken
    (32, 2000, 0.004, 7, [1_000_000, 2_500_000, 400_000]),
    (11, 300, 0.01, 0, [200_000, 50_000, 20_000]),
    (1, 2, 1.0, 0, [500, 40]),                                                                         # two canonical 1-mers
    (21, 100, 1.0, 3, [3_000, 9_000, 60]),                                                             # scale 1: max_hash = u64::MAX
]


@pytest.mark.parametrize("two_bit", [False, True])
@pytest.mark.parametrize("k,size,scale,seed,lens", CASES)
def test_batches_of_genomes_match_the_oracle(k, size, scale, seed, lens, two_bit):
    rng = np.random.default_rng(k * 1000 + size + seed)
    blocks = [genome_block(rng, L, n_records=int(rng.integers(1, 5))) for L in lens]
    b = scaled_batch(size, k, seed, scale, max_files=4, stage_bytes=16 << 20)  # (more files than max_files: several batches)
    res = b.sketch_many(blocks, two_bit=two_bit)
    assert len(res) == len(blocks)
    Ds = [check(r, blk, size, k, seed, scale, "file %d (%d bytes)" % (i, len(blk))) for i, (r, blk) in enumerate(zip(res, blocks))]
    c = b.counters()
    assert c["taken"] == sum(1 for d in Ds if size <= d <= CAP) and c["taken"] + c["not_taken"] == len(blocks), (c, Ds)
    b.close()


def test_sizes_around_the_sort_chunks_and_the_cap():
    """D on both sides of 4096 (the LDS network), of 8192 (two chunks / three) and within a few hundred of the cap on either
    side: the chunk merge's ranks"""
    rng = np.random.default_rng(77)
    k, size, scale = 21, 1000, 0.002
    lens = [2_000_000, 2_120_000, 4_040_000, 4_190_000, 6_000_000, 6_080_000, 6_330_000, 1_000_000]
    blocks = [genome_block(rng, L) for L in lens]
    b = scaled_batch(size, k, 0, scale, max_files=8, stage_bytes=48 << 20)
    res = b.sketch_many(blocks, two_bit=True)
    Ds = [check(r, blk, size, k, 0, scale, "file %d" % i) for i, (r, blk) in enumerate(zip(res, blocks))]
    # the inputs are what the comment says they are
    assert Ds[0] < 4096 < Ds[1] and Ds[2] < 8192 < Ds[3], Ds
    assert CAP - 600 < Ds[4] <= CAP and CAP - 500 < Ds[5] <= CAP and CAP < Ds[6] < CAP + 800, Ds
    b.close()


def test_small_empty_and_degenerate_files():
    rng = np.random.default_rng(5)
    k, scale = 21, 0.01
    g = genome_block(rng, 200_000, 2)
    D = oracle_scaled(g, 0, k, 0, scale)[3]
    assert 1500 < D < 2500
    blocks = [
        np.zeros(0, np.uint8),                                   # an empty file
        np.frombuffer(b"ACGT\0", dtype=np.uint8),                # shorter than k
        np.frombuffer(b"N" * 5000 + b"\0", dtype=np.uint8),      # no valid window at all
        np.tile(np.frombuffer(b"ACGTTGCATGCATGACCA", dtype=np.uint8), 20000),  # 18 distinct k-mers
        g,
        genome_block(rng, 1_400_000, 1),                         # D ~ 14 000: above the cap
        genome_block(rng, 300_000, 1),
        genome_block(rng, 500_000, 3),
    ]
    # size == D exactly: taken; size == D + 1: the same file is not; size 0: the empty files are empty sketches
    for size in (D, D + 1, 0, D - 1):
        b = scaled_batch(size, k, 0, scale, max_files=3, stage_bytes=4 << 20)
        res = b.sketch_many(blocks)
        Ds = [check(r, blk, size, k, 0, scale, "size %d file %d" % (size, i)) for i, (r, blk) in enumerate(zip(res, blocks))]
        assert Ds[4] == D and Ds[5] > CAP and Ds[0] == Ds[1] == Ds[2] == 0
        assert (res[4] is not None) == (size <= D)
        assert res[5] is None and res[6] is not None and res[7] is not None  # the partition of the file above the cap came back clean
        if size == 0:
            assert all(res[i] is not None and len(res[i][0]) == 0 for i in (0, 1, 2))
        # what was not taken goes through a HipSketcher, which is exact for anything
        for i, r in enumerate(res):
            if r is None and len(blocks[i]):
                sk = SketchParams.scaled(size, k, scale, 0).create_sketcher()
                sk.push_block(blocks[i])
                kc, km, _ = sk.to_arrays()
                okc, okm, otk, _ = oracle_scaled(blocks[i], size, k, 0, scale)
                assert np.array_equal(kc, okc) and np.array_equal(km, okm) and sk.finish()[1] == otk
                sk.close()
        b.close()


def test_two_slots_alternate_and_partitions_come_back_clean():
    """batch after batch through both slots, files above the cap and below `size` among them: every partition holds nothing
    of its previous file when the next one comes to it"""
    rng = np.random.default_rng(11)
    k, size, scale = 21, 200, 0.004
    b = scaled_batch(size, k, 0, scale, max_files=4, stage_bytes=8 << 20)
    rounds = []
    for r in range(6):
        blocks = [genome_block(rng, int(rng.integers(100_000, 1_500_000)), int(rng.integers(1, 4))) for _ in range(4)]
        if r % 2:
            blocks[1] = genome_block(rng, 3_400_000)  # D ~ 13 600: not taken, swept
        if r % 3 == 0:
            blocks[2] = genome_block(rng, 20_000)     # D ~ 80 < size
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
            D = check(x, blk, size, k, 0, scale, "round %d file %d" % (r, j))
            if r % 2 and j == 1:
                assert D > CAP
            if r % 3 == 0 and j == 2:
                assert D < size
    b.close()


def test_parked_handles_keep_their_kind_and_scale():
    """fh_batch_free parks a handle, fh_batch_new hands a parked one back when the parameters match: kind and scale are
    parameters"""
    rng = np.random.default_rng(13)
    k, n = 21, 1000
    blocks = [genome_block(rng, 1_500_000), genome_block(rng, 2_500_000, 2)]
    kw = dict(max_files=2, stage_bytes=8 << 20)

    def mash_ok(res):
        for r, blk in zip(res, blocks):
            o = O.OracleSketcher(O.MASH, n, k, 0)
            o.process_packed(blk, 0)
            okc, okm = o.to_vec()
            assert r is not None and np.array_equal(r[0], okc) and np.array_equal(r[1], okm)

    def scaled_ok(res, scale):
        for i, (r, blk) in enumerate(zip(res, blocks)):
            D = check(r, blk, n, k, 0, scale, "scale %g file %d" % (scale, i))
            assert n <= D <= CAP

    for _ in range(2):
        b = F.BatchSketcher(n, k, 0, **kw)
        mash_ok(b.sketch_many(blocks))
        b.close()
        b = scaled_batch(n, k, 0, 0.001, **kw)
        scaled_ok(b.sketch_many(blocks), 0.001)
        b.close()
        b = scaled_batch(n, k, 0, 0.002, **kw)
        scaled_ok(b.sketch_many(blocks), 0.002)
        b.close()
        b = F.BatchSketcher(n, k, 0, kind=KIND_MASH, **kw)
        mash_ok(b.sketch_many(blocks, two_bit=True))
        b.close()


def test_argument_errors():
    with pytest.raises(F.FinchHipError):
        scaled_batch(CAP + 1, 21, 0, 0.001)
    with pytest.raises(F.FinchHipError):
        scaled_batch(1000, 33, 0, 0.001)
    with pytest.raises(F.FinchHipError, match="scale must be in"):
        scaled_batch(1000, 21, 0, 0.0)
    with pytest.raises(F.FinchHipError, match="AllCounts"):
        F.BatchSketcher(0, 8, 0, kind=2)
    b = scaled_batch(CAP, 21, 0, 0.5, max_files=2, stage_bytes=1 << 20)
    b.close()


# --- the host layer on top: finch_sketch_files forms groups for Scaled parameters (fh_host.cpp) ---

def _fasta(seq: bytes, name=b"g", width=70, eol=b"\n", last_eol=True):
    body = eol.join(seq[j:j + width] for j in range(0, len(seq), width))
    return b">" + name + eol + body + (eol if last_eol else b"")


def _stream_oracle(data, n, k, seed, scale):
    o = O.OracleSketcher(O.SCALED, n, k, seed, scale)
    o.sketch_stream(data)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers(), int((kc["hash"] <= np.uint64(o.max_hash)).sum())


def test_sketch_files_groups_match_the_oracle_and_the_one_by_one_path(tmp_path):
    """a mixed list: plain genomes (grouped), CRLF and unterminated files, several contigs, a repeat and a short genome (staged,
    D < size: not taken), FASTQ and gzip'd FASTA (never grouped) -- one
    sketch per file in input order (lib.rs:29-49), each equal in every field to what option file_batch=0 gives and, for the
    FASTA files, to the oracle's sketch_stream; which files the groups took is predicted from the oracle's D"""
    rng = np.random.default_rng(21)
    n, k, scale = 100, 21, 0.001
    datas = []
    for i in range(18):
        L = int(rng.integers(200_000, 900_000))
        datas.append(_fasta(bytes(S.synth_genome_host(L, 500 + i)), b"g%d len=%d" % (i, L)))
    datas.append(_fasta(bytes(S.synth_genome_host(5_200_000, 77)), b"big"))         # ~5200 rows: the chunk sort
    datas.append(_fasta(bytes(S.synth_genome_host(390_000, 7)), eol=b"\r\n"))
    datas.append(_fasta(bytes(S.synth_genome_host(277_777, 8)), last_eol=False))
    datas.append(b"".join(_fasta(bytes(S.synth_genome_host(int(rng.integers(20_000, 90_000)), 900 + c)), b"contig%d" % c, width=60) for c in range(9)))
    datas.append(_fasta(b"ACGTTGCATGCATGACCATT" * 20_000))                          # 20 distinct k-mers: D < size
    datas.append(_fasta(bytes(S.synth_genome_host(40_000, 9))))                     # D ~ 40 < size
    n_fasta = len(datas)
    reads = S.synth_reads_host(S.synth_genome_host(50_000, 3), 0, 3000, 100, 1, 5000, 500)
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(reads[i * 101:i * 101 + 100]), b"I" * 100) for i in range(3000))
    datas.append(fq)
    datas.append(gzip.compress(datas[0], 1))
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("f%02d" % i)
        p.write_bytes(d)
        paths.append(str(p))
    oracles = [_stream_oracle(d, n, k, 0, scale) for d in datas[:n_fasta]]
    want_taken = sum(1 for o in oracles if n <= o[3] <= CAP)
    want_not = n_fasta - want_taken
    assert want_not == 2 and oracles[18][3] > 4096
    params = SketchParams.scaled(n, k, scale)
    t0, n0 = H.debug_file_batch()
    res = H.sketch_files(paths, params, H.FilterParams(None), n_threads=3)
    t1, n1 = H.debug_file_batch()
    assert len(res) == len(paths)
    assert (t1 - t0, n1 - n0) == (want_taken, want_not)
    F.debug_set(file_batch="0")
    ref = H.sketch_files(paths, params, H.FilterParams(None), n_threads=3)
    assert H.debug_file_batch() == (t1, n1)
    for i, d in enumerate(datas):
        a, b = res.sketch(i), ref.sketch(i)
        assert a.name == b.name == paths[i]
        assert np.array_equal(a.arrays[0], b.arrays[0]) and np.array_equal(a.arrays[1], b.arrays[1]), i
        assert (a.seq_length, a.num_valid_kmers) == (b.seq_length, b.num_valid_kmers), i
        assert a.filter_params == b.filter_params and a.sketch_params == b.sketch_params, i
        if i < n_fasta:
            okc, okm, totals, _ = oracles[i]
            assert np.array_equal(a.arrays[0], okc) and np.array_equal(a.arrays[1], okm), i
            assert (a.seq_length, a.num_valid_kmers) == totals, i
    for opts in (dict(batch_two_bit="0"), dict(pack_scalar="1"), dict(batch_read_piece="4099")):
        F.debug_set(file_batch=None, **opts)
        t2, n2 = H.debug_file_batch()
        alt = H.sketch_files(paths, params, H.FilterParams(None), n_threads=3)
        t3, n3 = H.debug_file_batch()
        assert (t3 - t2, n3 - n2) == (want_taken, want_not), opts
        for i in range(len(datas)):
            a, b = res.sketch(i), alt.sketch(i)
            assert np.array_equal(a.arrays[0], b.arrays[0]) and np.array_equal(a.arrays[1], b.arrays[1]), (opts, i)
            assert (a.seq_length, a.num_valid_kmers) == (b.seq_length, b.num_valid_kmers), (opts, i)
        F.debug_set(**{key: None for key in opts})
    F.debug_set(file_batch=None)


def test_sketch_files_does_not_stage_what_cannot_fit(tmp_path):
    """a file whose size puts its expected rows a quarter above the cap is not staged (neither taken nor not taken); its
    sketch is the one-by-one path's"""
    n, k, scale = 1000, 21, 0.01
    datas = [_fasta(bytes(S.synth_genome_host(L, 60 + i))) for i, L in enumerate((400_000, 2_000_000, 800_000, 1_000_000))]
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("s%d.fa" % i)
        p.write_bytes(d)
        paths.append(str(p))
    t0, n0 = H.debug_file_batch()
    res = H.sketch_files(paths, SketchParams.scaled(n, k, scale, 5), H.FilterParams(None), n_threads=2)
    t1, n1 = H.debug_file_batch()
    assert (t1 - t0, n1 - n0) == (3, 0)  # 4000, 8000 and 10 000 rows; 20 000 expected rows are never sent
    for i, d in enumerate(datas):
        okc, okm, totals, _ = _stream_oracle(d, n, k, 5, scale)
        a = res.sketch(i)
        assert np.array_equal(a.arrays[0], okc) and np.array_equal(a.arrays[1], okm), i
        assert (a.seq_length, a.num_valid_kmers) == totals, i
