"""Randomised differential of the seven many-per-launch doors against the oracle: BatchSketcher Mash and Scaled, .wide (k = 33..64),
.large (n = 3001..16384), .all_counts (k <= 7), RecordSketcher in the LDS form and streamed.  tests/door_fuzz_inputs.py draws a
case -- k over the door's whole range, sizes, scales, seeds up to 2^63 + 5, group sizes, staging buffers small enough for several
submits, both input forms, both slots, and blocks nobody thought of: files of wildly different sizes in one group, an empty or
all-N file between two genomes, lengths on tile edges and on the edges of the threshold -- and predicts from the oracle alone which
blocks the door must take, must not take, or may do either with (tests/test_door_fuzz_inputs.py holds the generator and the rule).

Per block: a result equals the oracle's sketch bit for bit (hashes, counts, extra counts, k-mer bytes, total valid k-mers; a count
equals tests/allcounts_model.py's rows); a None is sketched through a HipSketcher of the same parameters and held to the oracle
too; `must_take` blocks are taken and `must_not` blocks are None -- a door that quietly sends everything the long way fails; the
handle's counters agree with what came back.  Every third case then closes the handle and makes it again with the same parameters
-- the parked handle -- and runs the same blocks in reverse order through the other slot (a batch door: in the other input form
too): a partition, or a slot, that the group before left in any state but reset shows there.

soak runs: FH_DOOR_FUZZ_CASES=400 FH_DOOR_FUZZ_SEED=123456 python -m pytest tests/test_gpu_fuzz_doors.py -m gpu
Needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import allcounts_model as M
import door_fuzz_inputs as D
import finch_rs_amd as F

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_parked_handles():
    """handles are parked by their parameters when freed: every case has its own"""
    yield
    F.load().fh_release_cached()


@pytest.mark.parametrize("i", range(D.N_CASES))
@pytest.mark.parametrize("door", D.DOORS)
def test_random_case(door, i):
    run_case(door, D.SEED0, i)


def make(c):
    """the handle of the case's door"""
    if c.door in ("records", "records_stream"):
        h = F.RecordSketcher(c.size, c.k, c.seed, max_records=c.max_records, stage_bytes=c.stage_bytes, kind=c.kind, scale=c.scale,
                             stream=c.door == "records_stream")
        assert (h.max_positions, h.stream_cap) == (c.max_positions, c.stream_cap)  # what the prediction was worked out from
        return h
    kw = dict(max_files=c.max_files, stage_bytes=c.stage_bytes)
    if c.door == "counts":
        return F.BatchSketcher.all_counts(c.k, **kw)
    if c.door == "large":
        return F.BatchSketcher.large(c.size, c.k, c.seed, **kw)
    return (F.BatchSketcher.wide if c.door == "wide" else F.BatchSketcher)(c.size, c.k, c.seed, kind=c.kind, scale=c.scale, **kw)


def sketch_many(h, c, blocks, slot, two_bit):
    """-> per block (kc, kmers, total valid k-mers) or None"""
    if c.door in ("records", "records_stream"):
        return h.sketch_many(blocks, slot=slot)
    res = h.sketch_many(blocks, slot=slot, two_bit=two_bit)
    if c.door == "counts":
        assert all(r is not None and not r[2].any() for r in res)  # (a count has no first positions)
    return [None if r is None else (r[0], r[1], r[3]) for r in res]


def want_of(c, block):
    if c.door == "counts":
        okc, okm, _, total = M.sketch(bytes(block).split(b"\0"), c.k)
        return okc, okm, total
    return D.oracle_sketch(block, c.kind, c.size, c.k, c.seed, c.scale)


def same(got, want, ctx):
    kc, km, tk = got
    okc, okm, otk = want
    assert len(kc) == len(okc), (ctx, len(kc), len(okc))
    assert np.array_equal(kc["hash"], okc["hash"]), ctx
    assert np.array_equal(kc["count"], okc["count"]), ctx
    assert np.array_equal(kc["extra_count"], okc["extra_count"]), ctx
    assert km.shape == okm.shape and np.array_equal(km, okm), ctx
    assert tk == otk, (ctx, tk, otk)


class LongWay:
    """what the caller does with a block the door did not take: a HipSketcher of the same parameters, made when first needed"""

    def __init__(self, c):
        self.c, self.sk = c, None

    def sketch(self, block):
        c = self.c
        if self.sk is None:
            p = F.SketchParams.scaled(c.size, c.k, c.scale, c.seed) if c.kind == D.KIND_SCALED else F.SketchParams.mash(c.size, c.size, True, c.k, c.seed)
            self.sk = p.create_sketcher()
        self.sk.reset()
        self.sk.push_block(bytes(block) + (b"" if len(block) and block[-1] == 0 else b"\0"))
        kc, km, _ = self.sk.to_arrays()
        return kc, km, self.sk.finish()[1]

    def close(self):
        if self.sk is not None:
            self.sk.close()


def check(h, c, blocks, classes, wants, res, long_way, what):
    assert len(res) == len(blocks)
    taken = 0
    for j, (blk, cl, want, r) in enumerate(zip(blocks, classes, wants, res)):
        ctx = "%s seed0=%d case=%d %s: k=%d kind=%d size=%d scale=%g seed=%d two_bit=%s block %d of %d positions, %s" % (
            c.door, c.seed0, c.index, what, c.k, c.kind, c.size, c.scale, c.seed, c.two_bit, j, len(blk), cl)
        if cl == D.MUST_TAKE:
            assert r is not None, (ctx, "not taken", h.counters())
        if cl == D.MUST_NOT:
            assert r is None, (ctx, "taken", h.counters())
        if r is None:
            same(long_way.sketch(blk), want, ctx + ", through a sketcher")
        else:
            same(r, want, ctx)
            taken += 1
    assert h.counters() == {"taken": taken, "not_taken": len(blocks) - taken}, (c.door, c.seed0, c.index, what)


def run_case(door, seed0, i):
    c = D.case(door, seed0, i)
    classes = [D.predict(door, c, b) for b in c.blocks]
    wants = [want_of(c, b) for b in c.blocks]
    long_way = LongWay(c)
    h = make(c)
    try:
        res = sketch_many(h, c, c.blocks, c.slot, c.two_bit)
        check(h, c, c.blocks, classes, wants, res, long_way, "first handle")
        if i % 3 == 2:
            h.close()
            h = make(c)  # the parked one, for the same parameters and sizes: its counters at zero, its partitions reset
            # (a batch door's other input form too: the two-bit form next to the byte form on the same partitions)
            back = sketch_many(h, c, c.blocks[::-1], c.slot ^ 1, not c.two_bit)
            check(h, c, c.blocks[::-1], classes[::-1], wants[::-1], back, long_way, "parked handle, reversed, other slot and form")
            for j, (a, b, cl) in enumerate(zip(res, back[::-1], classes)):
                if cl != D.EITHER:
                    assert (a is None) == (b is None), (door, seed0, i, j)
    finally:
        h.close()
        long_way.close()
