"""The streamed record sketcher's boundary without a device: the new symbols exist, the ABI version is still 21, the LDS form's
bound is still 8192, the three options are listed (library and README), and every refusal of fh_records_new_stream comes with its
text before any device is looked at (so these run the same with and without a GPU)."""
import ctypes as C
import os
import re

import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd._lib import FhParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH, SCALED, ALL_COUNTS = 0, 1, 2
OPTIONS = ("records_stream", "records_stream_max_pos", "records_stream_fold")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def test_symbols_and_version(L):
    for name in ("fh_records_new_stream", "fh_records_max_positions_of", "fh_records_stream_cap", "fh_records_stream_folds", "finch_sketch_records_stream_stats"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    assert int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1)) == 21 == L.fh_abi_version()
    comment = hdr[hdr.index(" * 21: "):hdr.index("#define FH_ABI_VERSION")]
    for name in ("fh_records_new_stream", "fh_records_max_positions_of", "fh_records_stream_cap", "finch_sketch_records_stream_stats") + OPTIONS:
        assert name in comment, name
    assert L.fh_records_max_positions() == 8192
    assert L.fh_records_stream_cap() >= 1024
    assert L.fh_records_max_positions_of(None) == 0 and L.fh_records_stream_folds(None) == 0
    for decl in ("fh_records *fh_records_new_stream(const fh_params *params, int device, uint32_t max_records, uint64_t stage_bytes);",
                 "uint32_t fh_records_max_positions_of(fh_records *r);", "uint32_t fh_records_stream_cap(void);"):
        assert decl in hdr, decl
    host_hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    assert "int finch_sketch_records_stream_stats(uint64_t *streamed, double *kernel_ms, uint64_t *launches);" in host_hdr


def test_options_are_listed_in_order(L):
    names = [n for n, _ in F.option_list()]
    i = names.index("records_lds")
    assert tuple(names[i + 1:i + 4]) == OPTIONS
    readme = open(os.path.join(ROOT, "README.md")).read()
    table = readme[readme.index("| option | effect |"):]
    listed = re.findall(r"^\| `([a-z0-9_]+)` \|", table, re.M)
    assert tuple(listed[listed.index("records_lds") + 1:][:3]) == OPTIONS
    for n in OPTIONS:  # off / unset by default
        assert F.get_option(n) is None


def test_stream_stats_start_at_zero(L):
    a, ms, nl = C.c_uint64(7), C.c_double(7.0), C.c_uint64(7)
    assert L.finch_sketch_records_stream_stats(C.byref(a), C.byref(ms), C.byref(nl)) == 0
    assert (a.value, ms.value, nl.value) == (0, 0.0, 0)
    assert L.finch_sketch_records_stream_stats(None, None, None) == 0


def _refusals(cap):
    too_many = "the streamed record sketcher keeps at most %d hashes of a record in LDS: a Mash sketch of %d goes through an fh_sketcher"
    return [
        ((ALL_COUNTS, 4, 0, 0.0, 0, 16, 1 << 20), "the record sketcher serves Mash and Scaled sketches: AllCounts (kind 2) records go through an fh_sketcher"),
        ((5, 21, 1000, 0.0, 0, 16, 1 << 20), "unknown sketch kind 5 (0 Mash, 1 Scaled)"),
        ((MASH, 0, 1000, 0.0, 0, 16, 1 << 20), "kmer_length must be at least 1"),
        ((MASH, 33, 1000, 0.0, 0, 16, 1 << 20), "the record sketcher serves k = 1..32: k = 33 goes through an fh_sketcher"),
        ((MASH, 21, 1000, 0.0, 0xFFFF, 16, 1 << 20), "the record sketcher takes no test mask (hash_mask must be 0)"),
        ((MASH, 21, 0, 0.0, 0, 16, 1 << 20), "a Mash sketch has at least one hash (size 0)"),
        ((SCALED, 21, 10, 0.0, 0, 16, 1 << 20), "scale must be in (0, 1]"),
        ((MASH, 21, 1000, 0.0, 0, 0, 1 << 20), "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
        ((MASH, 21, 1000, 0.0, 0, 16, 4095), "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
        ((MASH, 21, cap + 1, 0.0, 0, 16, 1 << 20), too_many % (cap, cap + 1)),
        ((MASH, 21, 5000, 0.0, 0, 16, 1 << 20), too_many % (cap, 5000)),
    ]


def test_fh_records_new_stream_refusals(L):
    cap = L.fh_records_stream_cap()
    for (kind, k, size, scale, mask, nrec, stage), msg in _refusals(cap):
        p = FhParams(kind, k, size, 0, scale, 0, mask, 0)
        # device 99 does not exist anywhere: the refusal speaks before the device is looked at
        assert not L.fh_records_new_stream(C.byref(p), 99, nrec, stage)
        assert L.fh_last_error().decode() == msg
        if mask == 0:
            with pytest.raises(F.FinchHipError) as ei:
                F.RecordSketcher(size, k, device=99, max_records=nrec, stage_bytes=stage, kind=kind, scale=scale, stream=True)
            assert msg in str(ei.value)
    # the same size is no refusal of the LDS form, whose rows a record's windows bound (what it then says is about the device)
    p = FhParams(MASH, 21, cap + 1, 0, 0.0, 0, 0, 0)
    assert not L.fh_records_new(C.byref(p), 99, 16, 1 << 20)
    assert "hashes of a record in LDS" not in L.fh_last_error().decode()


def test_fh_records_new_stream_null(L):
    assert not L.fh_records_new_stream(None, 0, 16, 1 << 20)
    assert L.fh_last_error().decode() == "null params"
