"""The door of the batch sketcher for Mash sketches of 3001..16384 hashes (fh_batch_new_large, include/finch_hip.h) without a GPU:
the symbol is in the library, the header and the ctypes table; its parameter checks come before the device check, so what it
accepts gets as far as "no usable HIP device" and what it refuses is refused by a message that names the limit; fh_batch_new
keeps refusing 3001."""
import ctypes as C
import os
import re

import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd._lib import KIND_ALL_COUNTS, KIND_MASH, KIND_SCALED, FhParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N = 16384


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    return _lib.load()


def _new(L, fn, kind, k, size, scale=0.0, seed=0, mask=0, max_files=4, stage=1 << 20):
    p = FhParams(kind, k, size, seed, scale, 0, mask, 0)
    h = getattr(L, fn)(C.byref(p), 0, max_files, stage)
    msg = "" if h else (L.fh_last_error() or b"").decode(errors="replace")
    if h:
        L.fh_batch_free(h)
    return bool(h), msg


def test_symbol_exported_and_declared(L):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    assert re.search(r"fh_batch \*fh_batch_new_large\(const fh_params \*params, int device, uint32_t max_files, uint64_t stage_bytes\);", hdr)
    assert re.search(r"int fh_batch_parked\(uint64_t \*handles, uint64_t \*large_handles, uint64_t \*large_device_bytes\);", hdr)
    for name in ("fh_batch_new_large", "fh_batch_parked"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 13 and L.fh_abi_version() == want  # (12 was finch_merge_groups)
    assert re.search(r"\b13: [^;]*fh_batch_new_large", hdr)  # the header says what the version added
    assert int(re.search(r"#define\s+FH_BATCH_LARGE_MAX_N\s+(\d+)u", hdr).group(1)) == MAX_N == _lib.LARGE_MAX_N == F.BatchSketcher.LARGE_MAX_N
    assert hasattr(F.BatchSketcher, "large")
    listed = {line.split("\t")[0] for line in L.fh_option_list().decode().splitlines()}
    for opt in ("batch_large_want", "batch_large_files"):
        assert opt in listed and L.fh_set_option(opt.encode(), None) == 0  # a known option
        assert "| `%s` |" % opt in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.parametrize("k,size,seed", [(21, 3001, 0), (1, 10000, 42), (32, MAX_N, 7), (11, 5000, 0)])
def test_accepted_parameters_reach_the_device_check(L, k, size, seed):
    ok, msg = _new(L, "fh_batch_new_large", KIND_MASH, k, size, seed=seed)
    if L.fh_device_count() > 0:
        assert ok, msg
    else:
        assert not ok and "no usable HIP device" in msg, msg
    L.fh_release_cached()


@pytest.mark.parametrize("kind,k,size,scale,mask,words", [
    (KIND_MASH, 21, 3000, 0.0, 0, ("3001..16384", "fh_batch_new's")),             # <= 3000 is the other constructor's
    (KIND_MASH, 21, 1, 0.0, 0, ("3001..16384", "fh_batch_new's")),
    (KIND_MASH, 21, 0, 0.0, 0, ("3001..16384", "fh_batch_new's")),
    (KIND_MASH, 21, MAX_N + 1, 0.0, 0, ("3001..16384", "FH_BATCH_LARGE_MAX_N")),
    (KIND_MASH, 21, 1 << 40, 0.0, 0, ("3001..16384", "FH_BATCH_LARGE_MAX_N")),
    (KIND_SCALED, 21, 5000, 0.001, 0, ("Mash sketches only", "Scaled", "fh_batch_new")),
    (KIND_ALL_COUNTS, 5, 5000, 0.0, 0, ("Mash sketches only", "AllCounts", "fh_batch_new_counts")),
    (7, 21, 5000, 0.0, 0, ("unknown sketch kind 7",)),
    (KIND_MASH, 0, 5000, 0.0, 0, ("k = 1..32", "k = 0")),
    (KIND_MASH, 33, 5000, 0.0, 0, ("k = 1..32", "k = 33")),
    (KIND_MASH, 64, 10000, 0.0, 0, ("k = 1..32", "k = 64")),
    (KIND_MASH, 21, 5000, 0.0, 0xFFFF, ("no test mask",)),
])
def test_refusals_name_the_limit(L, kind, k, size, scale, mask, words):
    ok, msg = _new(L, "fh_batch_new_large", kind, k, size, scale, mask=mask)
    assert not ok
    for w in words:
        assert w in msg, (w, msg)
    assert "no usable HIP device" not in msg  # refused by its parameters, with or without a device


def test_sizes_and_the_two_bit_tile_space(L):
    limit = (1 << 21) * 768 - 4096  # a slot of fewer than 2^21 tiles of the two-bit form
    for max_files, stage in ((0, 1 << 20), (4097, 1 << 20), (4, 100), (4, limit + 1), (4, 1 << 36)):
        ok, msg = _new(L, "fh_batch_new_large", KIND_MASH, 21, 5000, max_files=max_files, stage=stage)
        assert not ok and "max_files 1..4096" in msg and "two-bit" in msg and str(limit) in msg, msg
        assert "no usable HIP device" not in msg
    assert not L.fh_batch_new_large(None, 0, 4, 1 << 20)


def test_fh_batch_new_still_refuses_3001(L):
    for fn, k in (("fh_batch_new", 21), ("fh_batch_new_wide", 51)):
        for size in (3001, 10000, MAX_N):
            ok, msg = _new(L, fn, KIND_MASH, k, size)
            assert not ok and "Mash sketches of 1..3000" in msg, msg
            assert "no usable HIP device" not in msg
    ok, msg = _new(L, "fh_batch_new", KIND_MASH, 21, 3001)
    assert "fh_batch_new_large" in msg and "k = 1..32" in msg and "fh_batch_new_wide" in msg  # ... and says where 3001.. is served


def test_nothing_parked_without_a_device(L):
    a, b, c = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    L.fh_release_cached()
    assert L.fh_batch_parked(C.byref(a), C.byref(b), C.byref(c)) == 0
    assert (a.value, b.value, c.value) == (0, 0, 0)
    assert L.fh_batch_parked(None, None, None) == 0
