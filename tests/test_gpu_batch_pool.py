"""The pool of parked batch handles behind the four doors of the batch sketcher (fh_batch_new, _new_wide, _new_large,
_new_counts): one match predicate (fh_batch_plan.h, pool_match) serves them all -- a handle parked by one door comes back
through that door for the same parameters, never through another, and what comes back sketches as a new one does.
Through the C ABI; needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import allcounts_model as M
from finch_rs_amd import _lib
from finch_rs_amd._lib import KIND_SCALED
from finch_rs_amd.sketch_schemes import BatchSketcher
from test_gpu_batch import genome_block, same
from test_gpu_batch_scaled import check as check_scaled

pytestmark = pytest.mark.gpu

SIZES = dict(max_files=2, stage_bytes=256 << 10)
DOORS = {
    "mash": lambda: BatchSketcher(1000, 21, 0, **SIZES),
    "scaled": lambda: BatchSketcher(1000, 21, 0, kind=KIND_SCALED, scale=0.01, **SIZES),
    "wide": lambda: BatchSketcher.wide(1000, 33, 0, **SIZES),
    "large": lambda: BatchSketcher.large(3001, 21, 0, **SIZES),
    "counts": lambda: BatchSketcher.all_counts(7, **SIZES),
}


def parked():
    return BatchSketcher.parked()[0]


def test_every_door_gets_its_own_handle_back():
    L = _lib.load()
    L.fh_release_cached()
    assert parked() == 0
    for make in DOORS.values():
        make().close()
    assert parked() == 5 and BatchSketcher.parked()[1] == 1
    # k and n of parked handles (counts k = 7, Mash n = 1000), but no handle of the small door's: a new one
    other = BatchSketcher(1000, 7, 0, **SIZES)
    assert parked() == 5
    held = {}
    for left, (name, make) in zip((4, 3, 2, 1, 0), DOORS.items()):
        held[name] = make()
        assert parked() == left, name
    rng = np.random.default_rng(20)
    blocks = [genome_block(rng, 30_000), genome_block(rng, 30_000, n_records=2)]
    for name, b in held.items():
        res = b.sketch_many(blocks)
        assert len(res) == 2
        for i, (r, blk) in enumerate(zip(res, blocks)):
            ctx = "%s, file %d" % (name, i)
            if name == "scaled":  # (taken iff the file holds at least `size` hashes at or below max_hash: the oracle says which)
                check_scaled(r, blk, 1000, 21, 0, 0.01, ctx)
            elif name == "counts":
                okc, okm, _, onvk = M.sketch(bytes(blk).split(b"\0"), 7)
                assert np.array_equal(r[0], okc) and np.array_equal(r[1], okm) and r[3] == onvk, ctx
            else:
                assert r is not None, ctx
                same(r, blk, b.size, b.kmer_length, 0, ctx)
    for b in list(held.values()) + [other]:
        b.close()
    assert parked() == 6
    L.fh_release_cached()
    assert parked() == 0
