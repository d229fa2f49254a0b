"""The record sketcher's boundary without a device: the new symbols exist, the ABI version is the header's, and every refusal of
finch_sketch_records / finch_sketch_records_buffer and of fh_records_new comes with its code and its text before any device is
looked at (so these run the same with and without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd._lib import FhParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH, SCALED, ALL_COUNTS = 0, 1, 2
INVALID, UNSUPPORTED = _lib.FH_ERR_INVALID, _lib.FH_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def test_symbols_and_version(L):
    for name in ("fh_records_new", "fh_records_free", "fh_records_max_positions", "fh_records_rows_cap", "fh_records_stage", "fh_records_submit_packed",
                 "fh_records_wait", "fh_records_result", "fh_records_copy_out_records", "fh_records_kernel_time", "fh_records_counters",
                 "finch_sketch_records", "finch_sketch_records_buffer", "finch_sketch_records_stats"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    assert int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1)) == 21 == L.fh_abi_version()
    assert re.search(r"^ \* 21: .*record sketcher", hdr, re.M)
    assert int(re.search(r"#define\s+FH_RECORDS_MAX_POS\s+(\d+)u", hdr).group(1)) == L.fh_records_max_positions() == 8192
    assert "records_lds" in [n for n, _ in F.option_list()]
    assert hasattr(F, "RecordSketcher") and hasattr(H, "sketch_records")


NEW_REFUSALS = [
    ((ALL_COUNTS, 4, 0, 0.0, 0, 16, 1 << 20), UNSUPPORTED, "the record sketcher serves Mash and Scaled sketches: AllCounts (kind 2) records go through an fh_sketcher"),
    ((5, 21, 1000, 0.0, 0, 16, 1 << 20), INVALID, "unknown sketch kind 5 (0 Mash, 1 Scaled)"),
    ((MASH, 0, 1000, 0.0, 0, 16, 1 << 20), INVALID, "kmer_length must be at least 1"),
    ((MASH, 33, 1000, 0.0, 0, 16, 1 << 20), UNSUPPORTED, "the record sketcher serves k = 1..32: k = 33 goes through an fh_sketcher"),
    ((SCALED, 64, 0, 0.5, 0, 16, 1 << 20), UNSUPPORTED, "the record sketcher serves k = 1..32: k = 64 goes through an fh_sketcher"),
    ((MASH, 21, 1000, 0.0, 0xFFFF, 16, 1 << 20), UNSUPPORTED, "the record sketcher takes no test mask (hash_mask must be 0)"),
    ((MASH, 21, 0, 0.0, 0, 16, 1 << 20), INVALID, "a Mash sketch has at least one hash (size 0)"),
    ((SCALED, 21, 10, 0.0, 0, 16, 1 << 20), INVALID, "scale must be in (0, 1]"),
    ((SCALED, 21, 10, 2.0, 0, 16, 1 << 20), INVALID, "scale must be in (0, 1]"),
    ((MASH, 21, 1000, 0.0, 0, 0, 1 << 20), INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
    ((MASH, 21, 1000, 0.0, 0, (1 << 20) + 1, 1 << 20), INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
    ((MASH, 21, 1000, 0.0, 0, 16, 4095), INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
    ((MASH, 21, 1000, 0.0, 0, 16, (1 << 32) + 1), INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
]


@pytest.mark.parametrize("case,code,msg", NEW_REFUSALS)
def test_fh_records_new_refusals(L, case, code, msg):
    kind, k, size, scale, mask, nrec, stage = case
    p = FhParams(kind, k, size, 0, scale, 0, mask, 0)
    # device 99 does not exist anywhere: the refusal speaks before the device is looked at
    assert not L.fh_records_new(C.byref(p), 99, nrec, stage)
    assert L.fh_last_error().decode() == msg
    # (a constructor returns no code: tests/test_records_plan_host.py holds the code to each of these texts; the Python
    # wrapper raises with the same text)
    if mask == 0:
        with pytest.raises(F.FinchHipError) as ei:
            F.RecordSketcher(size, k, device=99, max_records=nrec, stage_bytes=stage, kind=kind, scale=scale)
        assert msg in str(ei.value)


def test_fh_records_new_null(L):
    assert not L.fh_records_new(None, 0, 16, 1 << 20)
    assert L.fh_last_error().decode() == "null params"


def _call_files(L, paths, sp, fp, n_devices=1, out=True):
    arr = (C.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths]) if paths is not None else None
    darr = (C.c_int * max(1, n_devices))(*([0] * max(1, n_devices)))
    o = C.c_void_p()
    rc = L.finch_sketch_records(arr, len(paths) if paths is not None else 1, C.byref(sp) if sp is not None else None,
                                C.byref(fp) if fp is not None else None, darr, n_devices, 1, C.byref(o) if out else None)
    return rc, (L.finch_last_error() or b"").decode()


def _params():
    sp = H._params_c(F.SketchParams.mash(kmers_to_sketch=100, final_size=100, no_strict=True, kmer_length=21))
    fp = H.FilterParams().to_c()
    return sp, fp


def test_finch_sketch_records_refusals(L, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r1\nACGTACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r1\nACGT\n+\nIIII\n")
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    sp, fp = _params()
    # null arguments
    for args in ((None, sp, fp, 1, True), ([str(fa)], None, fp, 1, True), ([str(fa)], sp, None, 1, True), ([str(fa)], sp, fp, 1, False)):
        assert _call_files(L, *args) == (INVALID, "null argument")
    # more than 16 device entries
    assert _call_files(L, [str(fa)], sp, fp, 17) == (INVALID, "more than 16 device entries")
    # filtering: 1 is refused (and speaks before the input is opened), -1 and 0 mean off
    fon = H.FilterParams(filter_on=True).to_c()
    assert _call_files(L, [str(tmp_path / "missing.fa")], sp, fon) == \
        (UNSUPPORTED, "finch_sketch_records: filtering a single record's sketch is not offered (filter_on must be 0 or -1)")
    # FASTQ: the message names the file
    rc, msg = _call_files(L, [str(fa), str(fq)], sp, fp)
    assert rc == UNSUPPORTED and msg == "%s: a FASTQ input (first byte '@'): finch_sketch_records makes one sketch per FASTA record, one sketch per read is not offered" % fq
    # an empty input: finch_sketch_files' error for it
    assert _call_files(L, [str(empty)], sp, fp) == (INVALID, "empty input: not a FASTA/FASTQ file")
    # a file that is not there
    rc, msg = _call_files(L, [str(tmp_path / "missing.fa")], sp, fp)
    assert rc == INVALID and msg.startswith(str(tmp_path / "missing.fa") + ": No such file")


def test_finch_sketch_records_buffer_refusals(L):
    sp, fp = _params()
    darr = (C.c_int * 17)(*([0] * 17))

    def call(data, sp_, fp_, nd=1, out=True):
        o = C.c_void_p()
        buf = np.frombuffer(data, dtype=np.uint8) if data else None
        rc = L.finch_sketch_records_buffer(buf.ctypes.data if data else None, len(data) if data is not None else 5, C.byref(sp_) if sp_ is not None else None,
                                           C.byref(fp_) if fp_ is not None else None, darr, nd, 1, C.byref(o) if out else None)
        return rc, (L.finch_last_error() or b"").decode()
    fa = b">r\nACGT\n"
    assert call(None, sp, fp) == (INVALID, "null argument")
    assert call(fa, None, fp) == (INVALID, "null argument") and call(fa, sp, None) == (INVALID, "null argument") and call(fa, sp, fp, out=False) == (INVALID, "null argument")
    assert call(fa, sp, fp, nd=17) == (INVALID, "more than 16 device entries")
    assert call(fa, sp, H.FilterParams(filter_on=True).to_c())[0] == UNSUPPORTED
    rc, msg = call(b"@r\nACGT\n+\nIIII\n", sp, fp)
    assert rc == UNSUPPORTED and "first byte '@'" in msg and "one sketch per read is not offered" in msg
    assert call(b"", sp, fp) == (INVALID, "empty input: not a FASTA/FASTQ file")
    assert call(b"ACGT\n", sp, fp) == (INVALID, "not a FASTA/FASTQ file (first byte 0x41)")


def test_python_wrapper_raises(L, tmp_path):
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@r1\nACGT\n+\nIIII\n")
    with pytest.raises(F.FinchHipError) as ei:
        H.sketch_records(str(fq), F.SketchParams.mash(no_strict=True))
    assert ei.value.code == UNSUPPORTED and str(fq) in str(ei.value)
    with pytest.raises(F.FinchHipError) as ei:
        H.sketch_records(b">a\nACGT\n", F.SketchParams.mash(no_strict=True), filters=H.FilterParams(filter_on=True))
    assert ei.value.code == UNSUPPORTED
    with pytest.raises(H.FinchError):
        H.sketch_records(b"", F.SketchParams.mash(no_strict=True))
