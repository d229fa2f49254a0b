"""The AllCounts sketcher on the GPU (FH_KIND_ALL_COUNTS, fh_counts.hip) against the model of counts.rs
(tests/allcounts_model.py): hashes, k-mer bytes, counts, extra counts, num_valid_kmers and seq_length, bit for bit, through
every push route, the host layer, merges, saturation, the three file formats and finch_dist.  Run with -m gpu."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import allcounts_model as M
import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd import sharding
from finch_rs_amd import sketch_schemes as S
from finch_rs_amd.sketch_schemes import FinchError, SketchParams

pytestmark = pytest.mark.gpu

AC = SketchParams.all_counts


def sketcher(k, **kw):
    return AC(k).create_sketcher(device=0, **kw)


def same_as_model(kc, km, records, k, nvk=None):
    okc, okm, _, onvk = M.sketch(records, k, fastq=False)
    assert len(kc) == len(okc)
    assert np.array_equal(kc, okc)
    assert np.array_equal(km, okm)
    if nvk is not None:
        assert nvk == onvk


def packed(records):
    return b"".join(bytes(b for b in r if b not in b" \t\r\n") + b"\0" for r in records)


def random_records(rng, n, lo, hi, alphabet=b"ACGTACGTACGTACGTacgtuUNRY-.~*"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return [bytes(a[rng.integers(0, len(a), int(rng.integers(lo, hi)))]) for _ in range(n)]


def genome_records(n, rl, seed, gl=200_000):
    g = S.synth_genome_host(gl, seed)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        st = int(rng.integers(0, gl - rl))
        r = bytearray(g[st:st + rl].tobytes())
        if rng.random() < 0.3:
            r[int(rng.integers(0, rl))] = ord("N")
        out.append(bytes(r))
    return out


def test_known_answer_on_the_device():
    sk = sketcher(2)
    sk.push_block(b"ACGT\0")
    kc, km, _ = sk.to_arrays()
    assert [(int(r["hash"]), bytes(m), int(r["count"]), int(r["extra_count"])) for r, m in zip(kc, km)] == \
        [(1, b"AC", 2, 1), (6, b"CG", 2, 1)]
    assert sk.total_bases_and_kmers() == (0, 3)


@pytest.mark.parametrize("k", list(range(1, 17)))
def test_every_k_equals_the_model(k):
    rng = np.random.default_rng(100 + k)
    recs = random_records(rng, 300 if k >= 13 else 3000, 0, 400) + genome_records(200 if k >= 13 else 2000, 150, k)
    recs += [b"A" * 1000, b"acgu" * 50]
    sk = sketcher(k)
    sk.push_block(packed(recs))
    kc, km, _ = sk.to_arrays()
    n, nvk = sk.finish()
    same_as_model(kc, km, recs, k, nvk)
    assert sk.total_bases_and_kmers()[0] == 0


@pytest.mark.parametrize("k", [3, 8, 15])
def test_windows_across_staging_blocks(k):
    # records far longer than the staging buffer: fh_process cuts them, the k-1 carry makes each seam window count once
    rng = np.random.default_rng(k)
    recs = [bytes(S.synth_genome_host(50_000, 7 + i)) for i in range(3)] + random_records(rng, 50, 100, 20_000)
    sk = sketcher(k, stage_bytes=4096)
    for r in recs:
        sk.process(r)
    kc, km, _ = sk.to_arrays()
    same_as_model(kc, km, recs, k, sk.finish()[1])
    # the same through fh_push_block_ex with FH_PUSH_CONTINUE: one record in pieces of 1000 bytes
    sk2 = sketcher(k)
    big = recs[0]
    L = _lib.load()
    for i in range(0, len(big), 1000):
        piece = np.frombuffer(big[i:i + 1000] + (b"\0" if i + 1000 >= len(big) else b""), dtype=np.uint8).copy()
        _lib.check(L.fh_push_block_ex(sk2._h, piece.ctypes.data_as(C.c_void_p), piece.size, 1 if i else 0))
    kc2, km2, _ = sk2.to_arrays()
    same_as_model(kc2, km2, [big], k, sk2.finish()[1])
    # fh_push_block with a small staging buffer: blocks are cut between records only, never inside a window
    sk3 = sketcher(k, stage_bytes=4096)
    sk3.push_block(packed(recs[3:]))
    kc3, km3, _ = sk3.to_arrays()
    same_as_model(kc3, km3, recs[3:], k, sk3.finish()[1])


def test_process_records_and_reset():
    recs = genome_records(5000, 120, 3)
    buf = np.frombuffer(b"".join(recs), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64)
    lens = np.array([len(r) for r in recs], dtype=np.uint64)
    sk = sketcher(6)
    sk.push_block(b"TTTTTTTTTTTT\0")  # thrown away by the reset
    sk.reset()
    sk.process_records(buf, offs, lens)
    kc, km, _ = sk.to_arrays()
    same_as_model(kc, km, recs, 6, sk.finish()[1])


def bgzf(data: bytes, block=65280) -> bytes:
    out = []
    for ch in [data[i:i + block] for i in range(0, len(data), block)] + [b""]:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        c = co.compress(ch) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(c) + 25) + c +
                   struct.pack("<II", zlib.crc32(ch), len(ch)))
    return b"".join(out)


def fasta_text(records, width=60):
    return b"".join(b">r%d desc\n" % i + b"\n".join(r[j:j + width] for j in range(0, len(r), width)) + b"\n"
                    for i, r in enumerate(records))


def fastq_text(records):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(records))


@pytest.mark.parametrize("device_parse", ["0", "1"])
def test_files_and_buffers_every_format(tmp_path, device_parse):
    F.set_option("device_parse", device_parse)
    try:
        k = 5
        fa_recs = [r.lower() if i % 3 == 0 else r for i, r in enumerate(genome_records(400, 700, 5))]
        fq_recs = genome_records(3000, 150, 6)
        fa, fq = fasta_text(fa_recs), fastq_text(fq_recs)
        files = {"a.fa": fa, "b.fastq": fq, "c.fa.gz": gzip.compress(fa, 1), "d.fastq.gz": gzip.compress(fq, 1),
                 "e.fastq.bgz": bgzf(fq), "f.fa.bgz": bgzf(fa)}
        paths = []
        for name, data in files.items():
            (tmp_path / name).write_bytes(data)
            paths.append(str(tmp_path / name))
        nofilt = H.FilterParams(False)
        res = H.sketch_files(paths, AC(k), nofilt, n_threads=3)
        for i, name in enumerate(files):
            recs = fq_recs if "fastq" in name else fa_recs
            sk = res.sketch(i)
            same_as_model(sk.arrays[0], sk.arrays[1], recs, k)
            assert sk.seq_length == 0 and sk.num_valid_kmers == M.sketch(recs, k)[3]
        one = H.sketch_stream(gzip.compress(fa, 1), "buf", AC(k), nofilt).sketch(0)
        same_as_model(one.arrays[0], one.arrays[1], fa_recs, k)
        assert one.seq_length == 0
    finally:
        F.set_option("device_parse", None)


def test_fastq_default_filters_on(tmp_path):
    k = 7
    recs = genome_records(20000, 150, 9, gl=20_000)
    p = tmp_path / "reads.fq"
    p.write_bytes(fastq_text(recs))
    filt = H.FilterParams(None, (None, None), 0.21, 0.1)
    sk = H.sketch_files([str(p)], AC(k), filt).sketch(0)
    ix, c = M.sparse_counts(recs, k)
    okc, okm = M.to_vec_sparse(ix, M.saturate(c), k)
    b, bk, abun = M.filter_counts(okc, okm, True, None, (None, None), 0.21, 0.1)
    assert sk.filter_params.filter_on is True and sk.filter_params.abun_filter == abun
    assert np.array_equal(sk.arrays[0], b) and np.array_equal(sk.arrays[1], bk)
    assert sk.seq_length == 0


def test_device_blocks_and_merge():
    k = 9
    recs = genome_records(20000, 150, 11)
    blocks = [packed(recs[:7000]), packed(recs[7000:])]
    bufs = []
    try:
        for b in blocks:
            d = S.DeviceBuffer(len(b) + 64)
            d.upload(np.frombuffer(b, dtype=np.uint8))
            bufs.append(d)
        sks = [sketcher(k), sketcher(k)]
        sharding.sketch_device_blocks(sks, [d.ptr for d in bufs], [len(b) for b in blocks], [0, len(blocks[0])])
        kc, km, _ = sks[0].to_arrays()
        same_as_model(kc, km, recs, k, sks[0].finish()[1])
    finally:
        for d in bufs:
            d.free()
    a, b = sketcher(k), sketcher(k)
    a.push_block(blocks[0])
    b.push_block(blocks[1])
    a.finish(), b.finish()
    a.merge(b)
    kc, km, _ = a.to_arrays()
    same_as_model(kc, km, recs, k, a.finish()[1])


def test_saturation_and_wrapping_through_the_debug_hook():
    recs = [b"ACGTTT", b"AAAAAAAAAAGA"]
    sk = sketcher(2)
    sk.push_block(packed(recs))
    sk.debug_add_counts(2 ** 32 - 3, 0)  # every nonzero bin to c + 2^32 - 3: most saturate, count + extra wraps
    kc, km, _ = sk.to_arrays()
    c = M.forward_counts(recs, 2)
    c[c > 0] += 2 ** 32 - 3
    okc, okm = M.to_vec_arrays(M.saturate(c), 2)
    assert np.array_equal(kc, okc) and np.array_equal(km, okm)
    assert sk.finish()[1] == int(M.saturate(c).astype(np.uint64).sum())
    assert np.any(kc["count"] < kc["extra_count"])  # a wrapped count + extra_count


def test_more_than_2_pow_32_windows_of_one_kmer():
    # a device-resident block of 2^32 + 100 'A' bytes, a breaker and five 'T': A saturates (4.3 G windows at k = 1), and
    # A's row is then (u32::MAX + 5) mod 2^32 = 4 with extra 5
    n_a = 2 ** 32 + 100
    total = n_a + 7
    d = S.DeviceBuffer(total + 64)
    try:
        piece = np.full(1 << 28, ord("A"), dtype=np.uint8)
        for off in range(0, n_a, piece.size):
            d.upload(piece[:min(piece.size, n_a - off)], off)
        d.upload(np.frombuffer(b"\0TTTTT\0", dtype=np.uint8), n_a)
        sk = sketcher(1)
        sk.push_device(d.ptr, total)
        kc, km, _ = sk.to_arrays()
        assert [(int(r["hash"]), bytes(m), int(r["count"]), int(r["extra_count"])) for r, m in zip(kc, km)] == [(0, b"A", 4, 5)]
        assert sk.finish()[1] == 2 ** 32 - 1 + 5
    finally:
        d.free()


def test_refusals(tmp_path):
    with pytest.raises(_lib.FinchHipError, match="AllCounts"):
        sketcher(17)
    with pytest.raises(_lib.FinchHipError, match="hash_mask"):
        sketcher(4, hash_mask=0xFF)
    L = _lib.load()
    p = _lib.FhParams(_lib.KIND_ALL_COUNTS, 4, 1000, 0, 0.001, 0, 0, 0)
    assert not L.fh_batch_new(C.byref(p), 0, 4, 1 << 20)
    assert b"AllCounts" in L.fh_last_error()
    n = C.c_uint64()
    assert L.fh_merge_partials(2, 0, 0.0, 4, 0, None, None, None, None, None, 0, None, None, None, None, None,
                               C.byref(n), None, None, None, None, None) == _lib.FH_ERR_UNSUPPORTED
    bufs = (C.c_void_p * 1)()
    z = np.zeros(4, dtype=np.uint64)
    assert L.fh_merge_wire(2, 0, 0.0, 4, 0, 1, bufs, C.byref(n), z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                           z.ctypes.data, None) == _lib.FH_ERR_UNSUPPORTED
    sk = sketcher(4)
    sk.push_block(b"ACGTACGT\0")
    with pytest.raises(_lib.FinchHipError, match="add_extra"):
        sk.debug_add_counts(1, 1)
    sk.finish()
    kc, km, ps = sk.to_arrays()
    with pytest.raises(_lib.FinchHipError, match="AllCounts"):
        sk.merge_arrays(kc, km, ps, 5)
    fa = tmp_path / "x.fa"
    fa.write_bytes(b">a\nACGTACGTAAAC\n")
    with pytest.raises(_lib.FinchHipError, match="AllCounts"):
        H.sketch_file_sharded(str(fa), AC(4), H.FilterParams(False), [0, 0])
    with pytest.raises(_lib.FinchHipError, match="AllCounts"):
        H.sketch_stream_sharded(fa.read_bytes(), "x", AC(4), H.FilterParams(False), [0, 0])


def test_round_trip_through_every_format_and_dist(tmp_path):
    k = 6
    paths = []
    for i in range(4):
        p = tmp_path / ("g%d.fa" % i)
        p.write_bytes(fasta_text(genome_records(300 + 100 * i, 200, 20 + i)))
        paths.append(str(p))
    res = H.sketch_files(paths, AC(k), H.FilterParams(False))
    for ext in ("sk", "bsk", "msh"):
        out = str(tmp_path / ("all." + ext))
        res.write(out)
        back = H.open_sketch_file(out)
        assert len(back) == 4
        for i in range(4):
            a, b = res.sketch(i), back.sketch(i)
            assert [(h.hash, h.count) for h in a.hashes] == [(h.hash, h.count) for h in b.hashes]
            if ext == "bsk":
                assert [h.extra_count for h in a.hashes] == [h.extra_count for h in b.hashes]
            else:  # (the readers of .sk and .msh make extra_count = count / 2: json.rs:124, mash.rs:116)
                assert [h.extra_count for h in b.hashes] == [h.count // 2 for h in a.hashes]
            if ext != "msh":  # (.msh keeps no k-mer bytes)
                assert [h.kmer for h in a.hashes] == [h.kmer for h in b.hashes]
                assert (b.seq_length, b.num_valid_kmers) == (0, a.num_valid_kmers)
            assert back.params_of(i).kmer_length == k
            if ext != "msh":  # (the .msh reader knows Mash sketches only: mash.rs)
                assert back.params_of(i).kind == "allcounts"
    rows = H.dist(res, res)
    assert len(rows) > 0
    for r in rows:
        want = H.distance(res, int(r["query"]), res, int(r["reference"]))
        for f in ("containment", "jaccard", "mash_distance", "common_hashes", "total_hashes"):
            assert r[f] == want[f] or (np.isnan(r[f]) and np.isnan(want[f])), f
