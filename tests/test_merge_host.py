"""merge without a device: finch_merge_pair (the reference's loop on the host, the judge of the GPU tests) against
tests/merge_model.py bit for bit in all four clip modes, the new symbols, options and ABI version, and everything
finch_merge_groups decides before it looks for a device.  (The refusal of one member of 2^32 - 1 hashes or more is not exercised:
such a sketch does not fit a test.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finch_rs_amd as F
import merge_cases as MC
import merge_model as MM
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError, SketchParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_merge_pair", "finch_merge_groups")
BIG = 2 ** 32 - 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def random_member(rng, name, tag, params=MC.MASH, universe=60, spread=1):
    n = int(rng.integers(0, universe // 2))
    hs = np.sort(rng.choice(universe, size=n, replace=False)) * spread
    counts = rng.choice([1, 2, 9, BIG], size=n)
    extras = [int(rng.integers(0, int(c) + 1)) if c < BIG else int(rng.choice([0, 1, BIG])) for c in counts]
    return MC.Member(name, MC.records(hs.tolist(), tag, counts.tolist(), extras), params, int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 40)))


def check_pair(a, b, size):
    got = MC.read(H.merge_pair(a.build(), 0, b.build(), 0, size), 0)
    return MC.same(got, MC.expected([a, b], size))


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("with_size", [False, True])
def test_pair_against_the_model(built, with_scale, with_size):
    rng = np.random.default_rng(21 + 2 * with_scale + with_size)
    clipped = 0
    for it in range(120):
        # max_hash falls inside the hashes in use, so the scaled clip cuts somewhere; the second sketch is Mash or Scaled at will
        first = MC.scaled(MC.scale_for(int(rng.integers(0, 70)))) if with_scale else MC.MASH
        second = MC.scaled(0.5) if rng.integers(0, 2) else MC.MASH
        a, b = random_member(rng, "first", 65, first), random_member(rng, "second", 66, second)
        size = int(rng.integers(0, 40)) if with_size else None
        check_pair(a, b, size)
        clipped += len(MM.fold([a.recs, b.recs], size, a.scale)) < len(MM.walk(a.recs, b.recs))
    assert clipped > 20 or not (with_scale or with_size)


def test_pair_keeps_the_first_sketchs_identity_and_wraps(built):
    filt = H.FilterParams(True, (2, None), 0.5, 0.25)
    a = MC.Member("alpha", MC.records([3, 7, 9], 65, [BIG, 1, 5], [BIG, 0, 2]), MC.scaled(1.0), 2 ** 64 - 3, 2 ** 64 - 1, "first comment", filt)
    b = MC.Member("beta", MC.records([3, 8, 9, 11], 66, [2, 1, BIG, 1], [3 - 1, 0, BIG, 0]), MC.MASH, 10, 2, "second comment")
    got = MC.read(H.merge_pair(a.build(), 0, b.build(), 0), 0)
    MC.same(got, MC.expected([a, b]))
    assert got["name"] == "alpha" and got["comment"] == "first comment" and got["seq_length"] == 7 and got["num_valid_kmers"] == 1
    assert [r[:3] for r in got["records"]] == [(3, 1, 1), (7, 1, 0), (8, 1, 0), (9, 4, 1)]  # sums mod 2^32; 11 is past the first list's end
    assert [r[3][:1] for r in got["records"]] == [b"A", b"A", b"B", b"A"]  # a shared hash keeps the first sketch's k-mer


def test_pair_refusals(built):
    a, b = MC.Member("a", MC.records([1, 2])).build(), MC.Member("b", MC.records([2, 3])).build()
    out = C.c_void_p()
    assert built.finch_merge_pair(None, 0, b._p, 0, None, C.byref(out)) == _lib.FH_ERR_INVALID
    assert built.finch_merge_pair(a._p, 0, None, 0, None, C.byref(out)) == _lib.FH_ERR_INVALID
    assert built.finch_merge_pair(a._p, 0, b._p, 0, None, None) == _lib.FH_ERR_INVALID
    assert built.finch_merge_pair(a._p, 1, b._p, 0, None, C.byref(out)) == _lib.FH_ERR_INVALID
    assert b"first sketch 1 of 1" in built.finch_last_error()
    assert built.finch_merge_pair(a._p, 0, b._p, 4, None, C.byref(out)) == _lib.FH_ERR_INVALID
    assert b"second sketch 4 of 1" in built.finch_last_error()
    k31 = MC.Member("c", [(5, 1, 0, b"A" * 31)], SketchParams.mash(kmer_length=31)).build()
    with pytest.raises(FinchError, match="First sketch has k 21, but second sketch has k 31"):
        H.merge_pair(a, 0, k31, 0)
    seeded = MC.Member("d", MC.records([5]), SketchParams.mash(kmer_length=MC.K, hash_seed=42)).build()
    with pytest.raises(FinchError, match="First sketch has hash seed 0, but second sketch has hash seed 42"):
        H.merge_pair(a, 0, seeded, 0)
    for bad_scale in (1.5, -0.25, float("nan")):
        bad = MC.Member("wide", MC.records([1, 2]), MC.scaled(bad_scale)).build()
        with pytest.raises(FinchError, match=r"first sketch 0 \(wide\) has scale .*1 / scale as an integer is 0"):
            H.merge_pair(bad, 0, b, 0)
        H.merge_pair(b, 0, bad, 0)  # only the first sketch's scale counts
    zero = MC.Member("z", MC.records([1, 2]), MC.scaled(0.0))  # 1 / 0. is inf, the cast saturates: max_hash = 1, no refusal
    assert [r[0] for r in MC.read(H.merge_pair(zero.build(), 0, b, 0), 0)["records"]] == [1]


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in H._SYMS
    assert "wrap" in hdr.lower() and "STOPS WHEN EITHER LIST IS EXHAUSTED" in hdr
    assert len(H._SYMS["finch_merge_groups"][1]) == 12  # the statistics are out-parameters


def test_abi_version_is_at_least_12(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 12 and _lib.load().fh_abi_version() == want
    assert re.search(r"\b%d: fh_batch_new_wide" % want, hdr) and "finch_merge_groups" in hdr


def test_options_listed(built):
    names = [n for n, _ in F.option_list()]
    assert "merge_tile" in names and "merge_chunk_records" in names
    F.set_option("merge_tile", 7)
    assert F.get_option("merge_tile") == "7"
    F.set_option("merge_tile", None)
    assert F.get_option("merge_tile") is None


def c_groups(built, s, groups, size=None, devs=(0,), n_devices=None, offsets="ok", members="ok", out="ok", n_groups=None):
    off = np.zeros(len(groups) + 1, np.uint64)
    off[1:] = np.cumsum([len(g) for g in groups])
    flat = np.asarray([i for g in groups for i in g] or [0], np.uint32)
    if isinstance(offsets, np.ndarray):
        off = offsets
    darr = (C.c_int * max(len(devs), 1))(*devs) if devs is not None else None
    p = C.c_void_p()
    sz = C.c_uint64(size) if size is not None else None
    rc = built.finch_merge_groups(s, off.ctypes.data if offsets is not None else None, flat.ctypes.data if members is not None else None,
                                  len(groups) if n_groups is None else n_groups, C.byref(sz) if sz is not None else None, darr,
                                  len(devs) if n_devices is None else n_devices, C.byref(p) if out == "ok" else None, None, None, None, None)
    return rc, p, (built.finch_last_error() or b"").decode()


@pytest.fixture(scope="module")
def lib5(built):
    members = [MC.Member("s%d" % i, MC.records(range(i, 40, 3), 65 + i)) for i in range(3)]
    members.append(MC.Member("k31", [(5, 1, 0, b"C" * 31)], SketchParams.mash(kmer_length=31)))
    members.append(MC.Member("seeded", MC.records([4, 5]), SketchParams.mash(kmer_length=MC.K, hash_seed=7)))
    return members, MC.collect(members)


def test_groups_null_arguments_and_too_many_entries(built, lib5):
    _, s = lib5
    for kw in ({"offsets": None}, {"members": None}, {"out": None}, {"devs": None, "n_devices": 1}):
        rc, _, msg = c_groups(built, s._p, [[0, 1]], **kw)
        assert rc == _lib.FH_ERR_INVALID and "null argument" in msg, kw
    rc, _, msg = c_groups(built, None, [[0, 1]])
    assert rc == _lib.FH_ERR_INVALID and "null argument" in msg
    rc, _, msg = c_groups(built, s._p, [[0, 1]], devs=[0] * 17)
    assert rc == _lib.FH_ERR_INVALID and "at most 16 device entries (got 17)" in msg


def test_groups_shape_refusals_name_the_group(built, lib5):
    _, s = lib5
    rc, _, msg = c_groups(built, s._p, [[0, 1], [], [2]])
    assert rc == _lib.FH_ERR_INVALID and "group 1 is empty" in msg
    rc, _, msg = c_groups(built, s._p, [[0, 1], [2]], offsets=np.asarray([0, 2, 1], np.uint64))
    assert rc == _lib.FH_ERR_INVALID and "group 1" in msg and "offsets do not ascend" in msg
    rc, _, msg = c_groups(built, s._p, [[0], [1, 2, 5]])
    assert rc == _lib.FH_ERR_INVALID and "group 1 member 2: sketch 5 of 5 sketches" in msg
    with pytest.raises(FinchError, match="group 0 member 1: sketch 9 of 5"):
        H.merge(s, [[0, 9]])


def test_groups_incompatible_member_named_with_the_references_words(built, lib5):
    _, s = lib5
    rc, _, msg = c_groups(built, s._p, [[0, 1], [1, 2, 3]])
    assert rc == _lib.FH_ERR_INVALID and "group 1 member 2: First sketch has k 21, but second sketch has k 31" in msg
    rc, _, msg = c_groups(built, s._p, [[4, 0]])
    assert rc == _lib.FH_ERR_INVALID and "group 0 member 1: First sketch has hash seed 7, but second sketch has hash seed 0" in msg
    rc, p, _ = c_groups(built, s._p, [[3], [4]])  # alone in their groups they are compared with nothing
    assert rc == _lib.FH_OK
    built.finch_sketches_free(p)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
def test_groups_unsorted_member_refused_by_name(built, bad):
    s = MC.collect([MC.Member("good", MC.records([1, 2, 3])), MC.Member("bad sketch", MC.records(bad))])
    rc, _, msg = c_groups(built, s._p, [[0], [0, 0, 1]])
    assert rc == _lib.FH_ERR_INVALID
    assert "group 1 member 2" in msg and "sketch 1 (bad sketch): hashes not strictly ascending at" in msg
    assert MC.read(H.merge_pair(s, 0, s, 1), 0)["name"] == "good"  # the pair call takes any input the reference's loop takes


def test_group_of_2_to_the_32_records_refused(built):
    s = MC.Member("wide", MC.records(range(1 << 16))).build()
    rc, _, msg = c_groups(built, s._p, [[0], [0] * (1 << 16)])
    assert rc == _lib.FH_ERR_INVALID and "group 1" in msg and "2^32 records or more" in msg


def test_first_member_scale_with_divisor_zero_refused(built):
    s = MC.collect([MC.Member("wide", MC.records([1, 2]), MC.scaled(1.5)), MC.Member("ok", MC.records([2, 3]))])
    rc, _, msg = c_groups(built, s._p, [[1, 0], [0, 1]])
    assert rc == _lib.FH_ERR_INVALID and "group 1 member 0: sketch 0 (wide) has scale 1.5" in msg
    rc, p, _ = c_groups(built, s._p, [[0]])  # a group of one member merges nothing
    assert rc == _lib.FH_OK
    built.finch_sketches_free(p)


def test_no_groups_needs_no_device(built, lib5):
    _, s = lib5
    rc, p, _ = c_groups(built, s._p, [])
    assert rc == _lib.FH_OK and p.value and built.finch_sketches_len(p) == 0
    built.finch_sketches_free(p)
    st = {}
    assert len(H.merge(s, [], stats=st)) == 0
    assert st == {"kernel_ms": 0.0, "launches": 0, "records_copied": 0, "upload_ms": 0.0, "copy_ms": 0.0, "gather_ms": 0.0}


@pytest.mark.parametrize("size", [None, 0, 3])
def test_groups_of_one_member_are_the_members_and_need_no_device(built, lib5, size):
    members, s = lib5
    groups = [[2], [0], [3], [0], [4], [1]]
    st = {}
    out = H.merge(s, groups, size, stats=st)
    assert len(out) == len(groups) and st["launches"] == 0 and st["records_copied"] == 0
    for g, (i,) in enumerate(groups):
        got = MC.read(out, g)
        MC.same(got, MC.expected([members[i]], size))
        assert got == MC.read(s, i)  # unchanged and unclipped


def test_no_device_is_an_error(built, lib5):
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    _, s = lib5
    rc, _, msg = c_groups(built, s._p, [[0], [1, 2]])
    assert rc == _lib.FH_ERR_NO_DEVICE and "no usable HIP device" in msg
    with pytest.raises(F.FinchHipError) as ei:
        H.merge(s, [[0, 1]])
    assert "no usable HIP device" in str(ei.value)
