"""The key-word tables on the device (fh_core.h: a k2 word's cross term comes from its A and B records): every kernel that builds
them -- segment and tile kernels of one-word k-mers, the two-word kernels, the batch kernel -- at the k where the key's last k2
word is absent (9), a single merged group (13, 29), full (16, 32; 24: full in a block, no tail k2 word), short and served by
table P (31), behind a k1 word with a short group (21), and in keys of more than two blocks (33, 48).  Needs a real MI355X."""
import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd import sketch_schemes as S
from oracle import oracle as O
from test_gpu_parity import random_reads

pytestmark = pytest.mark.gpu

N = 100
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def streams():
    """2 000 noisy 150-base reads of a 3 000-base genome: as records behind breakers, and the same bytes as one sequence"""
    genome = S.synth_genome_host(3000, 91)
    rng = np.random.default_rng(91)
    reads = random_reads(rng, 2000, 150, 150, p_n=0.004, p_lower=0.02, genome=genome)
    records = np.frombuffer(b"".join(r + b"\0" for r in reads), dtype=np.uint8)
    unbroken = np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8)
    return records, unbroken


def first_occurrence(text: bytes, kmer: bytes) -> int:
    """where the k-mer or its reverse complement first begins in the upper-case text"""
    hits = [p for p in (text.find(kmer), text.find(kmer.translate(COMP)[::-1])) if p >= 0]
    return min(hits)


def check(stream, k, seed, stride, ctx):
    sk = F.SketchParams.mash(N, N, True, k, seed).create_sketcher()
    sk.set_record_stride(stride)
    d = F.DeviceBuffer(stream.size + 256)
    d.upload(stream)
    sk.push_device(d.ptr, stream.size)
    sk.sync()
    assert (sk.debug_segments()[0] > 0) == (stride > 1), ctx  # the segment kernel with the records' stride, else the tile kernel
    kc, km, pos = sk.to_arrays()
    ora = O.OracleSketcher(O.MASH, N, k, seed)
    ora.process_packed(stream, 0)
    okc, okm = ora.to_vec()
    assert len(kc) == len(okc) == N, ctx
    assert np.array_equal(kc["hash"], okc["hash"]), ctx
    assert np.array_equal(kc["count"], okc["count"]), ctx
    assert np.array_equal(kc["extra_count"], okc["extra_count"]), ctx
    assert np.array_equal(km, okm), ctx
    assert sk.finish()[1] == ora.total_bases_and_kmers()[1], ctx
    text = bytes(stream).upper()
    want = [first_occurrence(text, bytes(row)) for row in okm]
    assert [int(p) for p in pos] == want, ctx


@pytest.mark.parametrize("seed", [0, 42])
@pytest.mark.parametrize("k", [9, 13, 16, 21, 24, 29, 31, 32, 33, 48])
def test_segment_and_tile_kernels_match_the_oracle(streams, k, seed):
    records, unbroken = streams
    check(records, k, seed, 151, "records k=%d seed=%d" % (k, seed))
    check(unbroken, k, seed, 1, "one sequence k=%d seed=%d" % (k, seed))


def test_batch_of_four_small_fastas(tmp_path):
    """fh_k2b.hip builds the same tables: four FASTA files of one launch, through the batch handle and through sketch_files"""
    k, n = 21, 1000
    rng = np.random.default_rng(92)
    paths, datas, blocks = [], [], []
    for i in range(4):
        L = int(rng.integers(20_000, 60_000))
        seq = bytes(S.synth_genome_host(L, 200 + i))
        data = b">g%d\n" % i + b"\n".join(seq[j:j + 70] for j in range(0, L, 70)) + b"\n"
        p = tmp_path / ("g%d.fa" % i)
        p.write_bytes(data)
        paths.append(str(p))
        datas.append(data)
        blocks.append(np.frombuffer(seq + b"\0", dtype=np.uint8))
    oracles = []
    for data in datas:
        o = O.OracleSketcher(O.MASH, n, k, 0)
        o.sketch_stream(data)
        oracles.append(o)
    b = F.BatchSketcher(n, k, 0, max_files=4, stage_bytes=1 << 20)
    res = b.sketch_many(blocks)
    assert b.counters()["taken"] == 4
    b.close()
    for i, (r, o) in enumerate(zip(res, oracles)):
        kc, km, _, tk = r
        okc, okm = o.to_vec()
        assert np.array_equal(kc, okc) and np.array_equal(km, okm) and tk == o.total_bases_and_kmers()[1], i
    files = H.sketch_files(paths, S.SketchParams.mash(n, n, False, k, 0), H.FilterParams(None), n_threads=2)
    for i, o in enumerate(oracles):
        okc, okm = o.to_vec()
        sk = files.sketch(i)
        assert np.array_equal(sk.arrays[0], okc) and np.array_equal(sk.arrays[1], okm), i
        assert (sk.seq_length, sk.num_valid_kmers) == o.total_bases_and_kmers(), i
