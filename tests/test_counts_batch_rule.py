"""The AllCounts batch sketcher's door (fh_batch_new_counts, include/finch_hip.h) without a GPU: the symbol is in the library,
the header and the ctypes table; its parameter checks come before the device check; and the row bound its result columns
are sized from, (4^k + P) / 2 with P the palindromes of an even k, is the most rows to_vec emits from 4^k bins
(tests/allcounts_model.py)."""
import os
import re

import numpy as np
import pytest

import allcounts_model as M
from finch_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STAGE = (1 << 21) * 768 - 4096  # the header: a slot holds fewer than 2^21 tiles of the two-bit form


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    return _lib.load()


def refused(L, *args):
    assert not L.fh_batch_new_counts(*args)
    return (L.fh_last_error() or b"").decode()


def test_symbol_in_library_header_and_table(L):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    assert re.search(r"fh_batch \*fh_batch_new_counts\(uint32_t k, int device, uint32_t max_files, uint64_t stage_bytes\);", hdr)
    assert "fh_batch_new_counts" in _lib.SYMBOLS
    assert hasattr(L, "fh_batch_new_counts")
    assert int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 7


def test_parameter_checks_come_before_the_device_check(L):
    no_device = "no usable HIP device"
    msg = refused(L, 0, 0, 64, 1 << 20)
    assert "kmer_length" in msg and no_device not in msg
    for k in (8, 9, 16, 17, 33):
        msg = refused(L, k, 0, 64, 1 << 20)
        assert "AllCounts" in msg and "1..7" in msg and no_device not in msg
    for stage in (MAX_STAGE + 1, 1 << 31, 1 << 32, 1 << 36, (1 << 64) - 1):
        msg = refused(L, 4, 0, 64, stage)
        assert "stage_bytes" in msg and "2^32 positions" in msg and no_device not in msg
    for stage in (0, 4095):
        assert "stage_bytes" in refused(L, 4, 0, 64, stage)
    for files in (0, 4097):
        assert "max_files" in refused(L, 4, 0, files, 1 << 20)
    if L.fh_device_count() == 0:  # what passes the checks gets as far as the device check, the bound itself included
        for k in range(1, 8):
            assert no_device in refused(L, k, 0, 64, 1 << 20)
        assert no_device in refused(L, 7, 0, 4096, MAX_STAGE)


def test_the_largest_slot_holds_fewer_than_2_pow_32_positions():
    # two-bit form: a file of t tiles of 2048 positions takes (t + 1) * 768 bytes; byte form: a byte per position
    assert MAX_STAGE % 4096 == 0  # (the library rounds stage_bytes up to 4 KiB: the bound is not passed by that)
    assert (MAX_STAGE // 768 - 1) * 2048 < 2 ** 32 and MAX_STAGE < 2 ** 32
    # ... and the first size refused is 2^21 tiles' worth of bytes: 2^32 positions, the tile of zeroes behind a file not counted
    assert (MAX_STAGE + 4096) // 768 * 2048 == 2 ** 32


@pytest.mark.parametrize("k", range(1, 8))
def test_row_bound_is_what_to_vec_emits_at_most(k):
    bins = 4 ** k
    palindromes = 2 ** k if k % 2 == 0 else 0
    bound = (bins + palindromes) // 2
    ix = np.arange(bins, dtype=np.uint64)
    assert int((M.revcomp_ix(ix, k) == ix).sum()) == palindromes
    kc, km = M.to_vec_arrays(np.ones(bins, dtype=np.uint32), k)
    assert len(kc) == bound
    # no count vector emits more: a pair is reported once, whichever members occurred
    rng = np.random.default_rng(k)
    for _ in range(20):
        c = rng.integers(0, 3, bins).astype(np.uint32)
        assert len(M.to_vec_arrays(c, k)[0]) <= bound
    assert bound <= 8192
