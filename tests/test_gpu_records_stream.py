"""Long records streamed through a workgroup's LDS (fh_records_new_stream, k_record_stream of fh_records.hip) through
F.RecordSketcher(stream=True): every record the door takes carries the oracle's sketch of that record bit for bit -- hashes,
counts, extra counts, k-mer bytes, total k-mers -- and WHICH records it takes is predicted: all of them up to the handle's
`max_positions` whose kept hashes fit `stream_cap` (random records at these k have no 64-bit collision).

Every shape runs twice: with the default fold rule (a fold when the key array could not take another round) in this process, and
with records_stream_fold=1 (a fold behind every round, so that even short records fold many times) in a child process, which
runs the same function of this file: the option is read when a handle is made.  Needs a real MI355X (`-m gpu`)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import every_k_inputs as E  # noqa: E402
import finch_rs_amd as F  # noqa: E402
from finch_rs_amd._lib import KIND_MASH, KIND_SCALED  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NOISE = np.frombuffer(b"NRYKMSWnx-", dtype=np.uint8)  # bytes that are no base: they break k-mers
CAP, LDS_POS = 1024, 8192


def bases(rng, n, p_noise=0.0, p_lower=0.02):
    r = rng.choice(ACGT, size=n)
    m = rng.random(n)
    r[m > 1 - p_lower] |= 0x20  # lower case is a base
    if p_noise:
        bad = m < p_noise
        r[bad] = rng.choice(NOISE, size=int(bad.sum()))
    return r


def positions_of(k):
    """the lengths that matter: none, one short of a window, one window, a tile, the LDS form's bound and one more, a bound's
    worth of windows and one more (16 384 = two rounds of 4096 window starts twice over), and records of many rounds"""
    return [0, k - 1, k, 2048, LDS_POS, LDS_POS + 1, LDS_POS + k - 1, 16384, 16385, 20000, 70000]


def oracle_sketch(block, kind, size, k, seed, scale):
    o = O.OracleSketcher(kind, size, k, seed, scale if kind == KIND_SCALED else 0.001)
    o.process_packed(np.ascontiguousarray(block), 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1]


def check_all(rs, blocks, res, ctx=""):
    """a block is taken iff it is within the handle's bound and the oracle's sketch of it has no more rows than the cap (a Mash
    size never has); a taken one equals the oracle -> (taken, not taken)"""
    assert len(res) == len(blocks)
    taken = 0
    for i, (blk, r) in enumerate(zip(blocks, res)):
        c = (ctx, "record %d of %d positions" % (i, len(blk)))
        if len(blk) > rs.max_positions:
            assert r is None, c
            continue
        okc, okm, otk = oracle_sketch(blk, rs.kind, rs.size, rs.kmer_length, rs.seed, rs.scale)
        if len(okc) > rs.stream_cap:
            assert rs.kind == KIND_SCALED and r is None, c
            continue
        assert r is not None, c
        taken += 1
        kc, km, tk = r
        assert len(kc) == len(okc), (c, len(kc), len(okc))
        assert np.array_equal(kc["hash"], okc["hash"]), c
        assert np.array_equal(kc["count"], okc["count"]), c
        assert np.array_equal(kc["extra_count"], okc["extra_count"]), c
        assert np.array_equal(km, okm), c
        assert tk == otk, (c, tk, otk)
    return taken, len(blocks) - taken


def run(blocks, size, k, seed=0, kind=KIND_MASH, scale=0.0, ctx="", **kw):
    rs = F.RecordSketcher(size, k, seed, kind=kind, scale=scale, stream=True, **kw)
    try:
        res = rs.sketch_many(blocks)
        taken, not_taken = check_all(rs, blocks, res, ctx)
        assert rs.counters() == {"taken": taken, "not_taken": not_taken}, ctx
        return res, rs.folds()
    finally:
        rs.close()


# ---- the cases: plain functions, run here (default fold rule) and in a child (records_stream_fold=1) ----
def case_handle():
    rs = F.RecordSketcher(1000, 21, stream=True)
    lds = F.RecordSketcher(1000, 21)
    assert rs.stream_cap == CAP and rs.max_positions == 1 << 24 and lds.max_positions == LDS_POS
    assert rs.rows_cap >= rs.stream_cap
    assert rs.row_bound(70000) == 1000 and rs.row_bound(500) == 480 and rs.row_bound(rs.max_positions + 1) == 0
    rs.close()
    lds.close()
    sc = F.RecordSketcher(0, 21, kind=KIND_SCALED, scale=0.5, stream=True)
    assert sc.row_bound(70000) == CAP and sc.row_bound(120) == 100
    sc.close()


def case_positions(k, seed):
    rng = np.random.default_rng(1000 * k + seed)
    blocks = [bases(rng, n, p_noise=0.001 if i % 2 else 0.0) for i, n in enumerate(positions_of(k))]
    res, folds = run(blocks, 1000, k, seed, ctx="k=%d seed=%d" % (k, seed))
    assert all(r is not None for r in res)
    assert len(res[0][0]) == 0 and len(res[1][0]) == 0 and res[1][2] == 0 and len(res[2][0]) <= 1
    return folds


def case_sizes(size):
    rng = np.random.default_rng(size)
    blocks = [bases(rng, n, p_noise=0.001) for n in (10, 2048, LDS_POS + 1, 16385, 70000)]
    res, _ = run(blocks, size, 21, 42, ctx="size %d" % size)
    assert [len(r[0]) for r in res] == [0] + [size] * 4
    res, _ = run(blocks[1:4], size, 32, 0, ctx="size %d k 32" % size)
    assert [len(r[0]) for r in res] == [size] * 3


def case_scaled(size, scale, k):
    rng = np.random.default_rng(int(size + 1000 * scale))
    blocks = [bases(rng, n, p_noise=0.001 if i % 2 else 0.0) for i, n in enumerate(positions_of(k))]
    res, _ = run(blocks, size, k, 7, kind=KIND_SCALED, scale=scale, ctx="scaled size=%d scale=%g k=%d" % (size, scale, k))
    o = O.OracleSketcher(O.SCALED, size, k, 7, scale)
    if scale == 0.01:  # about 700 of the longest record's hashes are at or below max_hash: within the cap, and more than `size`
        below = int((res[-1][0]["hash"] <= np.uint64(o.max_hash)).sum())
        assert below == len(res[-1][0]) > max(size, 400)
    if scale == 1.0:  # every distinct hash is kept: short records are taken, those of more than `cap` distinct k-mers are not
        assert res[2] is not None and all(r is None for r in res[3:])


def case_repeats():
    rng = np.random.default_rng(7)
    unit = bases(rng, 3000, p_lower=0)
    homo = np.full(30000, ord("A"), np.uint8)
    for k in (21, 4):
        res, _ = run([np.tile(unit, 7), homo, np.tile(bases(rng, 2, p_lower=0), 10000)], 1000, k, ctx="repeats k=%d" % k)
        if k == 21:  # a window inside the unit occurs seven times, one across a seam six times
            assert set(res[0][0]["count"].tolist()) <= {6, 7, 12, 13, 14} and int((res[0][0]["count"] == 7).sum()) > 900
        assert len(res[1][0]) == 1 and res[1][0]["count"][0] == 30000 - k + 1


def case_scaled_list_beyond_the_cap():
    rng = np.random.default_rng(20)
    blocks = [bases(rng, 20000), bases(rng, 900), bases(rng, 20000, p_noise=0.001)]
    rs = F.RecordSketcher(0, 21, kind=KIND_SCALED, scale=1.0, stream=True)
    res = rs.sketch_many(blocks)
    assert res[0] is None and res[2] is None and res[1] is not None and len(res[1][0]) == 880
    assert rs.counters() == {"taken": 1, "not_taken": 2}
    assert check_all(rs, blocks, res) == (1, 2)
    rs.close()


def case_above_the_bound():
    rng = np.random.default_rng(24)
    rs = F.RecordSketcher(10, 21, max_records=4, stream=True)
    piece = bases(rng, 1 << 16)
    big = np.tile(piece, 257)[:rs.max_positions + 1]
    blocks = [bases(rng, 9000), big, bases(rng, 500)]
    res = rs.sketch_many(blocks)
    assert res[1] is None and rs.counters() == {"taken": 2, "not_taken": 1}
    assert check_all(rs, blocks, res) == (2, 1)
    rs.close()


def case_forty_records(slot):
    """lengths from 100 to 70 000, short beside long, on a handle that takes 16 records and 256 KiB a submit: the counter-dealt
    loop, several submits, both slots alternately from `slot` on"""
    rng = np.random.default_rng(40 + slot)
    lengths = np.rint(np.geomspace(100, 70000, 40)).astype(int)
    rng.shuffle(lengths)
    blocks = [bases(rng, int(n), p_noise=0.001 if i % 3 == 0 else 0.0) for i, n in enumerate(lengths)]
    rs = F.RecordSketcher(1000, 21, seed=42, max_records=16, stage_bytes=256 << 10, stream=True)
    res = rs.sketch_many(blocks, slot=slot)
    assert check_all(rs, blocks, res) == (40, 0)
    ms, launches, positions = rs.kernel_time()
    assert launches >= 3 and positions == int(lengths.sum()) and ms > 0
    assert rs.folds() >= 40  # every record folds at its end
    rs.close()


def case_parked_handles_keep_their_form():
    """a freed handle is parked; the next constructor of the OTHER form with the same parameters, records and stage must not get it"""
    rng = np.random.default_rng(77)
    blk = bases(rng, 20000)
    kw = dict(max_records=32, stage_bytes=1 << 20)
    for stream in (False, True, False, True):
        rs = F.RecordSketcher(1000, 21, stream=stream, **kw)
        assert rs.max_positions == ((1 << 24) if stream else LDS_POS), stream
        res = rs.sketch_many([blk])
        assert (res[0] is not None) == stream
        if stream:
            assert check_all(rs, [blk], res) == (1, 0)
        assert rs.counters() == {"taken": int(stream), "not_taken": int(not stream)}  # (a parked handle comes back with its counters at zero)
        rs.close()


def case_every_k():
    """every k-mer length through k_record_stream<K, SEED0> and <K, false>: the three records of tests/every_k_inputs.py's
    stream_records (round seams, a recurring block behind a fold, 8193 positions, k + 1 bases), Mash 1000"""
    for k in range(1, 33):
        for seed in (0, 42):
            res, folds = run(E.stream_records(k), 1000, k, seed, ctx="every_k k=%d seed=%d" % (k, seed), max_records=16, stage_bytes=1 << 20)
            assert all(r is not None for r in res) and folds >= 2
        F.load().fh_release_cached()  # (a parked handle per k and seed would add up)


CASES = {
    "every_k": (case_every_k, [()]),
    "handle": (case_handle, [()]),
    "parked_handles_keep_their_form": (case_parked_handles_keep_their_form, [()]),
    "positions": (case_positions, [(1, 0), (4, 42), (21, 0), (21, 42), (31, 0), (32, 42)]),
    "sizes": (case_sizes, [(1,), (10,), (1000,), (CAP,)]),
    "scaled": (case_scaled, [(0, 0.01, 21), (10, 0.01, 21), (2000, 1.0, 11)]),
    "repeats": (case_repeats, [()]),
    "scaled_list_beyond_the_cap": (case_scaled_list_beyond_the_cap, [()]),
    "above_the_bound": (case_above_the_bound, [()]),
    "forty_records": (case_forty_records, [(0,), (1,)]),
}


def both_fold_rules(name):
    fn, argsets = CASES[name]
    for args in argsets:
        fn(*args)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=F.debug_env(records_stream_fold=1), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok " + name), r.stdout[-4000:]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stream(name):
    both_fold_rules(name)


def test_fold_option_folds_behind_every_round():
    """the option does what the child runs rely on: a 20 000-position record is 10 tiles = 40 units = 5 rounds"""
    rng = np.random.default_rng(5)
    blk = bases(rng, 20000)
    _, folds = run([blk], 1000, 21)
    assert 2 <= folds <= 3  # 8192 keys behind round 2, then about 1000 + 420 + 290 + 220: one more at the end
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_records_stream as T; import numpy as np; " \
           "print('folds', T.run([T.bases(np.random.default_rng(5), 20000)], 1000, 21)[1])" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=F.debug_env(records_stream_fold=1), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.split()[-2:] == ["folds", "5"], r.stdout[-2000:]


if __name__ == "__main__":
    fn, argsets = CASES[sys.argv[1]]
    assert F.get_option("records_stream_fold") == "1"
    for args in argsets:
        fn(*args)
    print("ok " + sys.argv[1])
