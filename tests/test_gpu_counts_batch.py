"""Batches of AllCounts files on the GPU (fh_batch_new_counts, k_ac_batch_count / k_ac_batch_epilogue in fh_counts.hip):
every file's rows, k-mer bytes and total_kmers against the model of counts.rs (tests/allcounts_model.py) and against a kind-2
HipSketcher on the same block, in both input forms; the groups of sketch_files; parked handles.  Run with -m gpu."""
import gzip

import numpy as np
import pytest

import allcounts_model as M
import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd import sketch_schemes as S
from finch_rs_amd.sketch_schemes import BatchSketcher, SketchParams

pytestmark = pytest.mark.gpu

AC = SketchParams.all_counts
TILE = 2048
STAGE = 1 << 20


def bases(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def edge_blocks(k, rng):
    """packed streams (sequence bytes, a 0 byte behind a record) that can go wrong at this k"""
    blocks = [
        b"",                                                   # an empty file
        b"ACGTACG"[:k - 1],                                    # k - 1 positions: no window
        b"GATTACA"[:k],                                        # exactly k: one window
        bases(rng, TILE - 1), bases(rng, TILE), bases(rng, TILE + 1),
        bases(rng, TILE + k - 1),                              # the last window ends on the last position, across the tile edge
        bases(rng, 3 * TILE + 5) + b"\0",
    ]
    for at in (TILE - 1, TILE, TILE + 1):                      # a record's breaker on the tile edge and either side of it
        blocks.append(bases(rng, at) + b"\0" + bases(rng, 700) + b"\0")
    blocks += [
        bases(rng, 300) + b"N" * 40 + bases(rng, 2000) + b"NNN" + bases(rng, 5) + b"N" + bases(rng, 900) + b"\0",  # runs of N
        b"N" * 5000 + b"\0",                                   # no window at all
        bases(rng, 3000, b"acgtuUACGT") + b"\0",               # lower case and U
        bases(rng, 2500, b"ACGTACGTACGTRY-.*x") + b"\0",       # bytes that are no bases
        b"A" * 5000 + b"\0",                                   # one repeated base: one bin, at k windows per k-mer
        b"T" * 4099,                                           # only the reverse-complement side of the pair (A..A, T..T) occurs
        b"ACGT" * 1500 + b"\0",                                # even k: palindromes, rows (2 c, c)
        b"GGTGTTGGGT" * 300 + b"\0",                           # rc < ix for every window, and no rc occurs
    ]
    return blocks


def tiny_files(rng, n=200):
    return [bases(rng, int(rng.integers(30, 301)), b"ACGTACGTACGTN") + (b"\0" if i % 2 else b"") for i in range(n)]


def records_of(block):
    return bytes(block).split(b"\0")


def run_both_slots(bs, blocks, two_bit):
    """what sketch_many does, with two batches in flight: slot 1 is filled and submitted while slot 0 is on the device"""
    bufs = [bs.stage(0), bs.stage(1)]
    out, pending, i, slot = [], [], 0, 0

    def collect():
        sl, n = pending.pop(0)
        st = bs.wait(sl, n)
        assert not st.any()  # a count is exact for any input: every file is taken
        out.extend(bs.result(sl, j) for j in range(n))

    while i < len(blocks):
        if len(pending) == 2:
            collect()
        buf, offs, lens, pos = bufs[slot], [], [], 0
        while i < len(blocks) and len(offs) < bs.max_files:
            b = np.frombuffer(blocks[i], dtype=np.uint8)
            need = bs.packed_bytes(len(b)) if two_bit else len(b)
            if pos + need > len(buf):
                break
            if two_bit:
                bs.pack(b, buf[pos:pos + need])
            else:
                buf[pos:pos + need] = b
            offs.append(pos)
            lens.append(len(b))
            pos = (pos + need + 63) & ~63
            i += 1
        assert offs
        bs.submit(slot, offs, lens, two_bit)
        pending.append((slot, len(offs)))
        slot ^= 1
    while pending:
        collect()
    return out


def check_blocks(results, blocks, k, sk, what):
    assert len(results) == len(blocks)
    for i, (r, blk) in enumerate(zip(results, blocks)):
        kc, km, ps, tk = r
        okc, okm, _, onvk = M.sketch(records_of(blk), k)
        assert len(kc) == len(okc), (what, i)
        assert np.array_equal(kc, okc) and np.array_equal(km, okm) and tk == onvk, (what, i)
        assert not ps.any(), (what, i)
        sk.reset()
        sk.push_block(bytes(blk) + b"\0")
        skc, skm, _ = sk.to_arrays()
        assert np.array_equal(kc, skc) and np.array_equal(km, skm) and tk == sk.finish()[1], (what, i)


@pytest.mark.parametrize("two_bit", [False, True], ids=["bytes", "two_bit"])
@pytest.mark.parametrize("k", range(1, 8))
def test_every_file_equals_the_model_and_a_sketcher(k, two_bit):
    rng = np.random.default_rng(1000 + k)
    sk = AC(k).create_sketcher(device=0)
    bs = BatchSketcher.all_counts(k, max_files=64, stage_bytes=STAGE)
    # the edge cases, then 200 files of 30..300 bases: four batches over both slots, a workgroup's run crossing many files
    first = edge_blocks(k, rng) + tiny_files(rng)
    check_blocks(run_both_slots(bs, first, two_bit), first, k, sk, "first call")
    assert bs.counters() == {"taken": len(first), "not_taken": 0}
    # the same handle again with other files -- one of ~300 K positions between tiny ones, so that several workgroups add into one
    # file's table (and, every k-mer occurring at k <= 7, the file has as many rows as the result columns hold): the tables
    # came back zeroed, nothing of the first call is in these
    big = bytes(S.synth_genome_host(300_000 + 17 * k, 40 + k))
    second = [b"ACGTTGCA" * 9, big, bases(rng, 77), b"", big[:TILE * 9 + 3] + b"\0" + big[5000:9000], b"CCCCCCCCCCCC"]
    res = bs.sketch_many(second, slot=1, two_bit=two_bit)
    assert all(r is not None for r in res)
    check_blocks(res, second, k, sk, "second call")
    assert len(res[1][0]) == (4 ** k + (2 ** k if k % 2 == 0 else 0)) // 2
    bs.close()


def test_known_answer():
    bs = BatchSketcher.all_counts(2, max_files=4, stage_bytes=STAGE)
    for two_bit in (False, True):
        (kc, km, ps, tk), = bs.sketch_many([b"ACGT\0"], two_bit=two_bit)
        assert [(int(r["hash"]), bytes(m), int(r["count"]), int(r["extra_count"])) for r, m in zip(kc, km)] == \
            [(1, b"AC", 2, 1), (6, b"CG", 2, 1)]
        assert tk == 3
    bs.close()


def test_refusals_on_the_device():
    with pytest.raises(F.FinchHipError, match="AllCounts"):
        BatchSketcher.all_counts(8)
    with pytest.raises(F.FinchHipError, match="kmer_length"):
        BatchSketcher.all_counts(0)
    with pytest.raises(F.FinchHipError, match="AllCounts"):  # the door that was there keeps refusing
        BatchSketcher(1000, 4, kind=S.KIND_ALL_COUNTS)
    bs = BatchSketcher.all_counts(3, max_files=2, stage_bytes=STAGE)
    with pytest.raises(F.FinchHipError, match="2 files|at most"):
        bs.submit(0, [0, 64, 128], [4, 4, 4])
    bs.close()


def fasta(records, width, eol=b"\n"):
    out = []
    for i, r in enumerate(records):
        out.append(b">rec%d some text" % i + eol)
        out += [r[j:j + width] + eol for j in range(0, len(r), width)]
    return b"".join(out)


@pytest.fixture(scope="module")
def file_set(tmp_path_factory):
    """~40 small plain FASTA files (multi-line, CRLF among them), one gzip'd, one FASTQ and one file without sequence -> (paths,
    records per file, eligible for a group)"""
    d = tmp_path_factory.mktemp("counts_files")
    rng = np.random.default_rng(77)
    paths, recs, eligible = [], [], []
    for i in range(40):
        n_rec = 1 + i % 4
        rs = [bases(rng, int(rng.integers(1, 6000)), b"ACGTACGTACGTACGTacgtNnU") for _ in range(n_rec)]
        if i == 5:
            rs = [bases(rng, 3)]  # shorter than k = 4
        if i == 6:
            rs = [bases(rng, TILE), bases(rng, 2 * TILE - 1)]  # with the breakers, records that end on tile edges
        p = d / ("g%02d.fa" % i)
        p.write_bytes(fasta(rs, (60, 70, 80, 10000)[i % 4], b"\r\n" if i % 5 == 2 else b"\n"))
        paths.append(str(p)), recs.append(rs), eligible.append(True)
    rs = [bases(rng, 5000)]
    (d / "z.fa.gz").write_bytes(gzip.compress(fasta(rs, 60), 1))
    paths.insert(7, str(d / "z.fa.gz")), recs.insert(7, rs), eligible.insert(7, False)
    rs = [bases(rng, 150) for _ in range(50)]
    (d / "reads.fastq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(rs)))
    paths.insert(20, str(d / "reads.fastq")), recs.insert(20, rs), eligible.insert(20, False)
    # the empty file: a header and no sequence (a file of zero bytes is "empty input: not a FASTA/FASTQ file", the error of the
    # whole call on every path, as needletail has it) -- eligible, taken, no rows
    (d / "empty.fa").write_bytes(b">nothing here\n")
    paths.append(str(d / "empty.fa")), recs.append([b""]), eligible.append(True)
    return paths, recs, eligible


def same_sketch(a, b):
    assert a.name == b.name
    assert np.array_equal(a.arrays[0], b.arrays[0]) and np.array_equal(a.arrays[1], b.arrays[1])
    assert (a.seq_length, a.num_valid_kmers) == (b.seq_length, b.num_valid_kmers)
    assert a.filter_params == b.filter_params and a.sketch_params == b.sketch_params


def check_sketches(res, paths, recs, k, fastq_filtered=False):
    assert len(res) == len(paths)
    for i, (p, rs) in enumerate(zip(paths, recs)):
        sk = res.sketch(i)
        okc, okm, _, onvk = M.sketch(rs, k, fastq=p.endswith(".fastq") and fastq_filtered)
        assert sk.name == p, i
        assert np.array_equal(sk.arrays[0], okc) and np.array_equal(sk.arrays[1], okm), (i, p)
        assert sk.seq_length == 0 and sk.num_valid_kmers == onvk, (i, p)


@pytest.mark.parametrize("k", [4, 7])
def test_sketch_files_groups(file_set, k):
    paths, recs, eligible = file_set
    nofilt = H.FilterParams(False)
    t0, n0 = H.debug_file_batch()
    res = H.sketch_files(paths, AC(k), nofilt, n_threads=3)
    t1, n1 = H.debug_file_batch()
    assert (t1 - t0, n1 - n0) == (sum(eligible), 0)  # every eligible file went many-per-launch, and every one of them was taken
    check_sketches(res, paths, recs, k)
    for i, p in enumerate(paths):  # a call with one file never forms a group
        one = H.sketch_files([p], AC(k), nofilt)
        same_sketch(res.sketch(i), one.sketch(0))
    assert H.debug_file_batch() == (t1, n1)
    # the byte form on the link, and the default filter setting (off for FASTA, on for FASTQ: lib.rs:70-76)
    F.debug_set(batch_two_bit="0")
    try:
        alt = H.sketch_files(paths, AC(k), nofilt, n_threads=2)
    finally:
        F.debug_set(batch_two_bit=None)
    t2, n2 = H.debug_file_batch()
    assert (t2 - t1, n2 - n1) == (sum(eligible), 0)
    for i in range(len(paths)):
        same_sketch(res.sketch(i), alt.sketch(i))


def test_sketch_files_outside_the_groups(file_set):
    paths, recs, eligible = file_set
    plain = [p for p, e in zip(paths, eligible) if e][:12]
    plain_recs = [r for r, e in zip(recs, eligible) if e][:12]
    # filtering asked for: no group, the sketches are the filtered model's
    t0 = H.debug_file_batch()
    filt = H.FilterParams(True, (2, None), 0.0, 0.0)
    res = H.sketch_files(plain, AC(4), filt, n_threads=3)
    assert H.debug_file_batch() == t0
    for i, rs in enumerate(plain_recs):
        okc, okm, _, onvk = M.sketch(rs, 4, filter_on=True, abun=(2, None), err_filter=0.0, strand_filter=0.0)
        sk = res.sketch(i)
        assert np.array_equal(sk.arrays[0], okc) and np.array_equal(sk.arrays[1], okm) and sk.num_valid_kmers == onvk
    # k = 8: a sketcher per file as before
    res8 = H.sketch_files(plain, AC(8), H.FilterParams(False), n_threads=3)
    assert H.debug_file_batch() == t0
    check_sketches(res8, plain, plain_recs, 8)
    # groups switched off
    F.debug_set(file_batch="0")
    try:
        off = H.sketch_files(plain, AC(4), H.FilterParams(False), n_threads=3)
    finally:
        F.debug_set(file_batch=None)
    assert H.debug_file_batch() == t0
    check_sketches(off, plain, plain_recs, 4)


def test_parked_handles_keep_their_kind():
    from oracle import oracle as O
    rng = np.random.default_rng(9)
    sk5, sk3 = AC(5).create_sketcher(device=0), AC(3).create_sketcher(device=0)
    blocks = [bases(rng, 4000) + b"\0", bases(rng, 100), b"ACGTACGTAC\0"]
    a = BatchSketcher.all_counts(5, max_files=8, stage_bytes=STAGE)
    check_blocks(a.sketch_many(blocks), blocks, 5, sk5, "k = 5")
    a.close()  # parked
    # a Mash handle of the same sizes and k must not be the parked counts handle
    g = bases(rng, 350) + b"\0"  # (few enough positions that everything is admitted: the file is taken)
    mash = BatchSketcher(100, 5, max_files=8, stage_bytes=STAGE)
    (r,) = mash.sketch_many([g])
    o = O.OracleSketcher(O.MASH, 100, 5, 0)
    o.process(g[:-1])
    okc, okm = o.to_vec()
    assert r is not None and np.array_equal(r[0], okc) and np.array_equal(r[1], okm)
    mash.close()
    # ... nor a counts handle of another k
    c3 = BatchSketcher.all_counts(3, max_files=8, stage_bytes=STAGE)
    check_blocks(c3.sketch_many(blocks, two_bit=True), blocks, 3, sk3, "k = 3")
    # the first k again (may be the parked one): fresh input, nothing carried over
    fresh = [bases(rng, 2500, b"ACGTN"), b"TTTTTTTT\0", bases(rng, 9000) + b"\0"]
    again = BatchSketcher.all_counts(5, max_files=8, stage_bytes=STAGE)
    check_blocks(again.sketch_many(fresh, two_bit=True), fresh, 5, sk5, "k = 5 again")
    # ... and a parked Mash handle is not handed to a counts caller
    c5b = BatchSketcher.all_counts(5, max_files=8, stage_bytes=STAGE)
    check_blocks(c5b.sketch_many(fresh), fresh, 5, sk5, "k = 5, a second handle")
    for h in (c3, again, c5b):
        h.close()
