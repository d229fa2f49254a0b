"""The door of the batch sketcher for k = 33..64 (fh_batch_new_wide, include/finch_hip.h) without a GPU: the symbol is in the
library, the header and the ctypes table; its parameter checks come before the device check, so what it accepts gets as far as
"no usable HIP device" and what it refuses is refused by a message that names the limit; fh_batch_new keeps refusing k = 33."""
import ctypes as C
import os
import re

import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd._lib import KIND_ALL_COUNTS, KIND_MASH, KIND_SCALED, FhParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = F.BatchSketcher.SCALED_MAX_ROWS


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    return _lib.load()


def _new(L, fn, kind, k, size, scale, seed=0, mask=0):
    p = FhParams(kind, k, size, seed, scale, 0, mask, 0)
    h = getattr(L, fn)(C.byref(p), 0, 4, 1 << 20)
    msg = "" if h else (L.fh_last_error() or b"").decode(errors="replace")
    if h:
        L.fh_batch_free(h)
    return bool(h), msg


def test_symbol_exported_and_declared(L):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    assert re.search(r"fh_batch \*fh_batch_new_wide\(const fh_params \*params, int device, uint32_t max_files, uint64_t stage_bytes\);", hdr)
    assert "fh_batch_new_wide" in _lib.SYMBOLS
    assert hasattr(L, "fh_batch_new_wide")
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 9 and L.fh_abi_version() == want  # (8 was taken by finch_minmer_matrix)
    assert re.search(r"\b%d: fh_batch_new_wide" % want, hdr)  # the header says what the version added
    assert hasattr(F.BatchSketcher, "wide")


@pytest.mark.parametrize("kind,k,size,scale", [(KIND_MASH, 33, 1000, 0.0), (KIND_SCALED, 64, 0, 1.0), (KIND_MASH, 64, 3000, 0.0),
                                               (KIND_SCALED, 51, CAP, 0.001)])
def test_accepted_parameters_reach_the_device_check(L, kind, k, size, scale):
    ok, msg = _new(L, "fh_batch_new_wide", kind, k, size, scale, seed=42)
    if L.fh_device_count() > 0:
        assert ok, msg
    else:
        assert not ok and "no usable HIP device" in msg, msg
    L.fh_release_cached()


@pytest.mark.parametrize("kind,k,size,scale,mask,words", [
    (KIND_MASH, 32, 1000, 0.0, 0, ("k = 33..64", "fh_batch_new")),           # k <= 32 is the other constructor's
    (KIND_SCALED, 1, 0, 1.0, 0, ("k = 33..64", "fh_batch_new")),
    (KIND_MASH, 65, 1000, 0.0, 0, ("k = 33..64",)),
    (KIND_MASH, 51, 3001, 0.0, 0, ("Mash sketches of 1..3000",)),
    (KIND_MASH, 51, 0, 0.0, 0, ("Mash sketches of 1..3000",)),
    (KIND_SCALED, 51, CAP + 1, 0.001, 0, ("Scaled sketches of size 0..%d" % CAP,)),
    (KIND_SCALED, 51, 1000, 0.0, 0, ("scale must be in (0, 1]",)),
    (KIND_SCALED, 51, 1000, 1.5, 0, ("scale must be in (0, 1]",)),
    (KIND_SCALED, 51, 1000, float("nan"), 0, ("scale must be in (0, 1]",)),
    (KIND_ALL_COUNTS, 51, 0, 0.0, 0, ("AllCounts", "fh_batch_new_counts", "k = 1..7")),
    (7, 51, 1000, 0.001, 0, ("unknown sketch kind 7", "0 Mash, 1 Scaled")),
    (KIND_MASH, 51, 1000, 0.0, 0xFFFF, ("no test mask",)),
])
def test_refusals_name_the_limit(L, kind, k, size, scale, mask, words):
    ok, msg = _new(L, "fh_batch_new_wide", kind, k, size, scale, mask=mask)
    assert not ok
    for w in words:
        assert w in msg, (w, msg)
    assert "no usable HIP device" not in msg  # refused by its parameters, with or without a device


def test_sizes_are_checked_like_fh_batch_new(L):
    p = FhParams(KIND_MASH, 48, 1000, 0, 0.0, 0, 0, 0)
    for max_files, stage in ((0, 1 << 20), (4097, 1 << 20), (4, 100)):
        assert not L.fh_batch_new_wide(C.byref(p), 0, max_files, stage)
        assert "max_files 1..4096" in (L.fh_last_error() or b"").decode()
    assert not L.fh_batch_new_wide(None, 0, 4, 1 << 20)


def test_fh_batch_new_still_refuses_two_word_kmers(L):
    for kind, size, scale in ((KIND_MASH, 1000, 0.0), (KIND_SCALED, 1000, 0.001)):
        ok, msg = _new(L, "fh_batch_new", kind, 33, size, scale)
        assert not ok and "k = 1..32" in msg, msg
        assert "fh_batch_new_wide" in msg  # ... and says where k = 33..64 is served
