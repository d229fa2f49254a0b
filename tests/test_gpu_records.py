"""One sketch per record in a workgroup's LDS (fh_records_*, k_record_sketch of fh_records.hip) through F.RecordSketcher: every
record the door takes carries the oracle's sketch of that record bit for bit -- hashes, counts, extra counts, k-mer bytes, total
k-mers (mash.rs:34-63, scaled.rs:37-61) -- and WHICH records it takes is predicted: all of them up to `max_positions`, none above
(random records at these k have no 64-bit collision).  Needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd._lib import KIND_MASH, KIND_SCALED
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NOISE = np.frombuffer(b"NRYKMSWnx-", dtype=np.uint8)  # N, IUPAC codes and other bytes that are no base: they break k-mers


def bases(rng, n, p_noise=0.0, p_lower=0.02):
    r = rng.choice(ACGT, size=n)
    m = rng.random(n)
    r[m > 1 - p_lower] |= 0x20  # lower case is a base
    if p_noise:
        bad = m < p_noise
        r[bad] = rng.choice(NOISE, size=int(bad.sum()))
    return r


def revcomp(a):
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    return comp[a[::-1]]


def oracle_sketch(block, kind, size, k, seed, scale):
    o = O.OracleSketcher(kind, size, k, seed, scale if kind == KIND_SCALED else 0.001)
    o.process_packed(np.ascontiguousarray(block), 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1]


def check_all(rs, blocks, res, ctx=""):
    """every block up to max_positions is taken and equals the oracle; every longer one is not taken; -> records taken"""
    assert len(res) == len(blocks)
    taken = 0
    for i, (blk, r) in enumerate(zip(blocks, res)):
        c = (ctx, "record %d of %d positions" % (i, len(blk)))
        if len(blk) > rs.max_positions:
            assert r is None, c
            continue
        assert r is not None, c
        taken += 1
        kc, km, tk = r
        okc, okm, otk = oracle_sketch(blk, rs.kind, rs.size, rs.kmer_length, rs.seed, rs.scale)
        assert len(kc) == len(okc), (c, len(kc), len(okc))
        assert np.array_equal(kc["hash"], okc["hash"]), c
        assert np.array_equal(kc["count"], okc["count"]), c
        assert np.array_equal(kc["extra_count"], okc["extra_count"]), c
        assert np.array_equal(km, okm), c
        assert tk == otk, (c, tk, otk)
    return taken


def run(blocks, size, k, seed=0, kind=KIND_MASH, scale=0.0, ctx="", **kw):
    rs = F.RecordSketcher(size, k, seed, kind=kind, scale=scale, **kw)
    try:
        res = rs.sketch_many(blocks)
        taken = check_all(rs, blocks, res, ctx)
        c = rs.counters()
        assert c == {"taken": taken, "not_taken": len(blocks) - taken}, (ctx, c)
        return res
    finally:
        rs.close()


def test_max_positions_is_the_headers():
    rs = F.RecordSketcher(1000, 21)
    assert rs.max_positions == 8192 and rs.rows_cap >= rs.max_positions
    rs.close()


@pytest.mark.parametrize("k,seed", [(21, 0), (21, 42), (32, 0), (1, 0), (25, 42)])
def test_window_counts(k, seed):
    """records of 0 (shorter than k), 1, 63, 64, 65, 2047, 2048, 2049 and 4097 windows, of max - 1, max and max + 1 positions (the
    last comes back None), an all-N record and an empty one, and the same lengths with N / IUPAC noise"""
    rng = np.random.default_rng(100 * k + seed)
    mp = 8192
    blocks = [bases(rng, w + k - 1) for w in (0, 1, 63, 64, 65, 2047, 2048, 2049, 4097)]
    blocks += [bases(rng, n) for n in (mp - 1, mp, mp + 1)]
    blocks += [np.full(500, ord("N"), np.uint8), np.zeros(0, np.uint8)]
    blocks += [bases(rng, n, p_noise=0.01) for n in (k, 100, 2048, 2049, 5000, mp, mp + 1)]
    res = run(blocks, 1000, k, seed, ctx="k=%d seed=%d" % (k, seed))
    assert res[11] is None and res[-1] is None and res[10] is not None
    assert len(res[0][0]) == 0 and res[0][2] == 0 and len(res[1][0]) == 1 and len(res[12][0]) == 0 and len(res[13][0]) == 0


@pytest.mark.parametrize("k", [1, 2, 11, 16, 21, 24, 25, 31, 32])
def test_every_path_of_k(k):
    rng = np.random.default_rng(k)
    blocks = [bases(rng, n, p_noise=pn) for n, pn in ((1500, 0.0), (1500, 0.005), (3000, 0.002), (k, 0.0), (k - 1, 0.0), (7000, 0.001))]
    run(blocks, 1000, k, 0, ctx="k=%d" % k)
    run(blocks[:3], 50, k, 42, ctx="k=%d seed 42" % k)


def test_repeats_have_long_runs():
    """an 18-base repeat of 6 000 bases: at most 18 distinct hashes, runs of hundreds; one piece three times.  (Three 3 000-base pieces are 9 000 positions, beyond the bound: not taken; three of 2 700 are taken.)"""
    rng = np.random.default_rng(18)
    unit = bases(rng, 18, p_lower=0)
    rep = np.tile(unit, 334)[:6000]
    piece3000, piece2700 = bases(rng, 3000), bases(rng, 2700)
    homo = np.full(8192, ord("A"), np.uint8)
    blocks = [rep, np.tile(piece3000, 3), np.tile(piece2700, 3), homo, np.tile(bases(rng, 2), 4000)]
    for k in (21, 16):
        res = run(blocks, 1000, k, ctx="repeats k=%d" % k)
        assert 1 <= len(res[0][0]) <= 18 and int(res[0][0]["count"].sum()) == 6000 - k + 1
        assert res[1] is None
        if k == 21:  # a window inside the piece occurs three times, one across the seam between two copies twice
            assert set(res[2][0]["count"].tolist()) <= {2, 3}
        assert len(res[3][0]) == 1 and res[3][0]["count"][0] == 8192 - k + 1


def test_palindromes_at_even_k():
    """a k-mer that is its own reverse complement (even k only): the tie goes to the reverse complement, extra_count says so"""
    rng = np.random.default_rng(16)
    for k in (16, 2, 32):
        half = [bases(rng, k // 2, p_lower=0) for _ in range(40)]
        parts = []
        for h in half:
            parts += [h, revcomp(h), bases(rng, 3, p_lower=0)]  # a palindromic k-mer, then a few free bases
        blk = np.concatenate(parts)
        res = run([blk, np.concatenate([blk, blk])], 1000, k, ctx="palindromes k=%d" % k)
        okc, _, _ = oracle_sketch(blk, KIND_MASH, 1000, k, 0, 0)
        assert int(okc["extra_count"].sum()) >= 40  # the input is what the comment says it is
        assert res[0] is not None


def test_size_against_the_distinct_count():
    rng = np.random.default_rng(5)
    blk = bases(rng, 920)  # 900 windows at k = 21, all distinct in a random record
    okc, _, _ = oracle_sketch(blk, KIND_MASH, 10**6, 21, 0, 0)
    d = len(okc)
    assert d == 900
    for size in (1, d - 1, d, d + 1, 5000):
        res = run([blk, bases(rng, 50), blk], size, 21, ctx="size %d" % size)
        assert len(res[0][0]) == min(size, d)


@pytest.mark.parametrize("scale", [1.0, 0.1, 0.001])
@pytest.mark.parametrize("size", [0, 10, 1000])
def test_scaled(size, scale):
    """both branches of the rows rule: every hash at or below max_hash, and the first `size` whatever their hash"""
    rng = np.random.default_rng(int(size + 1000 * scale))
    blocks = [bases(rng, n, p_noise=pn) for n, pn in ((1500, 0.0), (8192, 0.001), (300, 0.0), (20, 0.0), (0, 0.0), (4097, 0.0), (8193, 0.0))]
    res = run(blocks, size, 21, 7, kind=KIND_SCALED, scale=scale, ctx="scaled size=%d scale=%g" % (size, scale))
    o = O.OracleSketcher(O.SCALED, size, 21, 7, scale)
    below = int((res[0][0]["hash"] <= np.uint64(o.max_hash)).sum())
    if scale == 0.001 and size >= 10:
        assert below < len(res[0][0]) == min(size, 1480)  # fewer than `size` below max_hash: the sketch is filled up to `size`
    if scale >= 0.1 and size <= 10:
        assert below == len(res[0][0]) > size            # more than `size` below max_hash: all of them
    if size == 0 and scale == 0.001:
        assert len(res[0][0]) == below                   # size 0: nothing above max_hash


def test_600_short_records_in_one_submit():
    """more records than workgroups: a workgroup takes a run of several, zero-row records sit between the others"""
    rng = np.random.default_rng(600)
    blocks = []
    for i in range(600):
        n = int(rng.integers(1200, 1800)) if i % 7 else int(rng.integers(0, 21))
        blocks.append(bases(rng, n, p_noise=0.001 if i % 3 == 0 else 0.0))
    rs = F.RecordSketcher(1000, 21, max_records=1024, stage_bytes=8 << 20)
    res = rs.sketch_many(blocks)
    assert check_all(rs, blocks, res) == 600
    ms, launches, positions = rs.kernel_time()
    assert launches == 1 and positions == sum(len(b) for b in blocks) and ms > 0
    assert rs.counters() == {"taken": 600, "not_taken": 0}
    rs.close()


def test_two_slots_alternate_over_five_submits():
    rng = np.random.default_rng(55)
    blocks = [bases(rng, int(rng.integers(100, 3000)), p_noise=0.001) for _ in range(40)]
    blocks[17] = bases(rng, 8200)  # one not taken, in the middle of a submit
    rs = F.RecordSketcher(200, 21, seed=42, max_records=8)
    res = rs.sketch_many(blocks)
    assert check_all(rs, blocks, res) == 39
    assert rs.kernel_time()[1] == 5
    assert rs.counters() == {"taken": 39, "not_taken": 1}
    # the verbs by hand: a slot in flight refuses to be staged, a result is read only after the wait
    buf = rs.stage(0)
    need = rs.packed_bytes(len(blocks[0]))
    rs.pack(blocks[0], buf[:need])
    rs.submit(0, [0], [len(blocks[0])])
    with pytest.raises(F.FinchHipError):
        rs.stage(0)
    with pytest.raises(F.FinchHipError):
        rs.result(0, 0)
    assert list(rs.wait(0, 1)) == [0]
    kc, km, tk = rs.result(0, 0)
    assert np.array_equal(kc["hash"], res[0][0]["hash"]) and tk == res[0][2]
    # a submit whose regions overlap is refused by name, nothing is launched
    with pytest.raises(F.FinchHipError) as ei:
        rs.submit(0, [0, 64], [len(blocks[0]), len(blocks[0])])
    assert "overlaps" in str(ei.value)
    rs.close()


def test_rows_beyond_a_slot_are_refused():
    rng = np.random.default_rng(9)
    rs = F.RecordSketcher(5000, 21, max_records=2, stage_bytes=64 << 10)  # rows_cap: max(8192, min(budget, 2 x 5000, by stage))
    blocks = [bases(rng, 6000) for _ in range(3)]
    assert rs.rows_cap < 3 * 5000
    buf = rs.stage(0)
    offs, pos = [], 0
    for b in blocks[:2]:
        need = rs.packed_bytes(len(b))
        rs.pack(b, buf[pos:pos + need])
        offs.append(pos)
        pos = (pos + need + 63) & ~63
    if 2 * 5000 > rs.rows_cap:
        with pytest.raises(F.FinchHipError) as ei:
            rs.submit(0, offs, [6000, 6000])
        assert "submit fewer records" in str(ei.value)
    res = rs.sketch_many(blocks)  # (sketch_many closes a group at the rows, too)
    assert check_all(rs, blocks, res) == 3
    rs.close()
