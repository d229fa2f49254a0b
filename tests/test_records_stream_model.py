"""The streamed rule (tests/records_stream_model.py: drop above T, fold at a given capacity, cut) gives the sketch of the whole
record: compared with O.OracleSketcher over the record, field for field, for Mash and Scaled, sizes 1 / 10 / 1000, a fold after
every 1, 7 and 4096 windows.  No GPU and nothing of the library: this pins the exactness argument of DESIGN 3.22 on its own."""
import numpy as np
import pytest

from oracle import oracle as O
from records_stream_model import MASH, SCALED, streamed_sketch, windows_of

K, SEED = 21, 42
FOLDS = (1, 7, 4096)


def rand_record(rng, n, p_noise=0.0):
    r = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    if p_noise:
        r[rng.random(n) < p_noise] = ord("N")
    return r.tobytes()


def _records():
    rng = np.random.default_rng(322)
    unit = rand_record(rng, 700)
    return {
        "random": rand_record(rng, 9000, p_noise=0.001),  # more than two folds of 4096
        "few": rand_record(rng, 300),                     # fewer distinct hashes than 1000
        "repeat": unit * 7,                                # every count a multiple of 7 but at the seams: counts add across folds
        "homopolymer": b"A" * 5000,                        # one hash, EQUAL to T at every window behind the first fold
    }


RECORDS = _records()
_WINDOWS = {}


def windows(name):
    if name not in _WINDOWS:  # computed once, shared, never changed
        _WINDOWS[name] = tuple(windows_of(RECORDS[name], K, SEED, O.hash_f, O.reverse_complement))
    return _WINDOWS[name]


def oracle(name, kind, size, scale):
    o = O.OracleSketcher(kind, size, K, SEED, scale)
    o.process_packed(np.frombuffer(RECORDS[name], dtype=np.uint8), 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1], o.max_hash if kind == SCALED else 0


def check(name, kind, size, scale, fold_every):
    kc, km, total, max_hash = oracle(name, kind, size, scale)
    w = windows(name)
    assert len(w) == total
    got = streamed_sketch(w, kind, size, max_hash, fold_every)
    assert got is not None
    rows, folds, dropped = got
    ctx = (name, kind, size, scale, fold_every)
    assert [r[0] for r in rows] == kc["hash"].tolist(), ctx
    assert [r[2] for r in rows] == kc["count"].tolist(), ctx
    assert [r[3] for r in rows] == kc["extra_count"].tolist(), ctx
    assert [r[1] for r in rows] == [bytes(x) for x in km], ctx
    assert folds >= -(-len(w) // fold_every)
    return rows, dropped, kc, max_hash


@pytest.mark.parametrize("fold_every", FOLDS)
@pytest.mark.parametrize("size", [1, 10, 1000])
@pytest.mark.parametrize("name", sorted(RECORDS))
def test_mash(name, size, fold_every):
    rows, dropped, kc, _ = check(name, MASH, size, 0.0, fold_every)
    if name == "random" and size <= 10:
        # the threshold does its work: everything survives up to the first fold, behind it a window survives with probability
        # about size / (windows so far): 10 ln 9000 = 91 in all, 300 is far out
        assert dropped > len(windows(name)) - fold_every - 300
    if name == "few":
        assert len(rows) == min(size, 280) and (size < 280 or dropped == 0)  # fewer distinct hashes than `size`: T never falls
    if name == "repeat" and size == 1000:
        assert len(rows) == 700 and sorted(set(r[2] for r in rows)) == [6, 7]  # (windows across a seam occur six times)
    if name == "homopolymer":
        assert len(rows) == 1 and rows[0][2] == 5000 - K + 1 and dropped == 0


# Scaled: size 0 (nothing above max_hash); scale 0.1 keeps about 900 of the random record's 9000 hashes -- more than a size of
# 10, fewer than 1000; scale 0.0002 about 2 -- fewer than 10
@pytest.mark.parametrize("fold_every", FOLDS)
@pytest.mark.parametrize("size,scale", [(0, 0.1), (0, 0.001), (10, 0.1), (10, 0.0002), (1000, 0.1), (1000, 1.0)])
@pytest.mark.parametrize("name", ["random", "few", "repeat"])
def test_scaled(name, size, scale, fold_every):
    rows, dropped, kc, max_hash = check(name, SCALED, size, scale, fold_every)
    below = sum(1 for r in rows if r[0] <= max_hash)
    if size == 0:
        assert below == len(rows)
    if name == "random":
        if (size, scale) == (10, 0.1):
            assert below == len(rows) > size       # more than `size` below max_hash: all of them, nothing else
        if (size, scale) == (10, 0.0002):
            assert below < len(rows) == size       # fewer: filled up to `size` with hashes above max_hash
        if (size, scale) == (1000, 0.1):
            assert below < len(rows) == size
        if scale == 1.0:
            assert dropped == 0 and len(rows) > 8000  # max_hash is 2^64 - 1: T never falls below it


def test_the_cap_refuses_a_scaled_list_that_outgrows_it():
    _, _, _, max_hash = oracle("random", SCALED, 0, 1.0)
    assert streamed_sketch(windows("random"), SCALED, 0, max_hash, 4096, cap=1024) is None
    _, _, _, max_hash = oracle("random", SCALED, 0, 0.1)
    assert streamed_sketch(windows("random"), SCALED, 0, max_hash, 4096, cap=1024) is not None
