"""The screen's host side without a GPU (include/finch_host.h, finch_index_screen / finch_screen_host): the
symbols and options are there, the refusals carry their messages, the empty cases touch nothing, and finch_screen_host -- the
contract in plain host code -- equals tests/screen_model.py row for row and field for field on every case of
tests/screen_cases.py."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import finch_rs_amd as F
import screen_cases as SC
import screen_model as SM
from finch_rs_amd import _lib
from finch_rs_amd import host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("finch_index_screen", "finch_index_screen_buffer", "finch_screen_host", "finch_screen_len", "finch_screen_copy",
           "finch_screen_stats", "finch_screen_free")


def test_symbols_version_and_options():
    L = H.lib()
    for s in SYMBOLS:
        assert s in H._SYMS and hasattr(L, s), s
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want == 21 and _lib.load().fh_abi_version() == want
    names = [n for n, _ in F.option_list()]
    readme = open(os.path.join(ROOT, "README.md")).read()
    for o in ("screen_piece", "screen_dir_bits"):
        assert o in names and "| `%s` |" % o in readme, o
    assert H.SCREEN_DTYPE.itemsize == 40


def empty_index():
    return H.LibraryIndex(SC.build(SC.case("empty_library")))


def raw_screen(ix, data, k, out=None):
    """finch_index_screen_buffer with its arguments as they are -> the return code"""
    p = H._P()
    buf = np.frombuffer(data, np.uint8)
    return H.lib().finch_index_screen_buffer(ix, buf.ctypes.data if len(buf) else None, len(buf), k, 0, 1, 0, C.byref(p) if out is None else out)


def last_error():
    return H.lib().finch_last_error().decode()


def test_refusals():
    text = SC.fasta([SC.S[:100]])
    refs = SC.build(SC.case("one_hash"))
    with empty_index() as ix:  # (an index of a library without a hash: no device behind it, and the checks come first)
        assert raw_screen(None, text, 21) == _lib.FH_ERR_INVALID and "null argument" in last_error()
        assert H.lib().finch_index_screen_buffer(ix._p, None, 5, 21, 0, 1, 0, C.byref(H._P())) == _lib.FH_ERR_INVALID
        assert "null argument" in last_error()
        assert H.lib().finch_index_screen_buffer(ix._p, None, 0, 21, 0, 1, 0, None) == _lib.FH_ERR_INVALID and "null argument" in last_error()
        assert H.lib().finch_index_screen(ix._p, None, 1, 21, 0, 1, 0, C.byref(H._P())) == _lib.FH_ERR_INVALID and "null argument" in last_error()
        with pytest.raises(F.FinchError, match="kmer_length 0"):
            ix.screen(text, kmer_length=0, hash_seed=0)
        for k in (33, 48, 64):
            with pytest.raises(F.FinchHipError, match="finch_index_screen_buffer: kmer_length %d: the screen serves kmer_length <= 32" % k) as ei:
                ix.screen(text, kmer_length=k, hash_seed=0)
            assert ei.value.code == _lib.FH_ERR_UNSUPPORTED
        with pytest.raises(F.FinchError, match="kmer_length 65"):
            ix.screen(text, kmer_length=65, hash_seed=0)
    with pytest.raises(F.FinchError, match="kmer_length 0"):
        H.screen_host(refs, text, 0)
    with pytest.raises(F.FinchHipError, match="finch_screen_host: kmer_length 33: the screen serves kmer_length <= 32"):
        H.screen_host(refs, text, 33)
    assert H.lib().finch_screen_host(None, None, 0, 21, 0, 1, C.byref(H._P())) == _lib.FH_ERR_INVALID and "null argument" in last_error()
    with pytest.raises(F.FinchError, match="not a FASTA/FASTQ file"):
        H.screen_host(refs, b"ACGT\n", 21)
    assert H.lib().finch_screen_stats(None, *[None] * 8) == _lib.FH_ERR_INVALID


def test_unreadable_file_named(tmp_path):
    good = tmp_path / "good.fa"
    good.write_bytes(SC.fasta([SC.S[:100]]))
    with empty_index() as ix:
        with pytest.raises(F.FinchError, match="no_such_file.fa: No such file"):
            ix.screen([str(good), str(tmp_path / "no_such_file.fa")], kmer_length=21, hash_seed=0)
        assert len(ix.screen([str(good)], kmer_length=21, hash_seed=0)) == 0


def test_empty_index_and_empty_input():
    text = SC.fasta([SC.S])
    with empty_index() as ix:
        st = {}
        rows = ix.screen(text, stats=st)  # (kmer_length and hash_seed from the library's sketches)
        assert rows.dtype == H.SCREEN_DTYPE and len(rows) == 0
        assert st == dict(positions=0, kmers=0, hits=0, distinct=0, table_bytes=0, table_ms=0.0, kernel_ms=0.0, launches=0)
        assert len(ix.screen(b"", kmer_length=21, hash_seed=0)) == 0 and len(ix.screen([], kmer_length=21, hash_seed=0)) == 0
    st = {}
    assert len(H.screen_host(SC.build(SC.case("empty_library")), text, 21, stats=st)) == 0 and st["kmers"] == 0
    st = {}
    assert len(H.screen_host(SC.build(SC.case("one_hash")), b"", 21, stats=st)) == 0 and st["distinct"] == 0


def test_library_parameters_must_agree():
    a = SC.build(SC.Case([], 21, [SC.Ref([1, 2])]))
    a.append(SC.build(SC.Case([], 31, [SC.Ref([3])])))
    with H.LibraryIndex(SC.build(SC.case("empty_library"))) as ix:
        ix.refs = a
        with pytest.raises(F.FinchError, match="different"):
            ix.screen(b"")


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_equals_model(name):
    case = SC.case(name)
    st = {}
    rows = H.screen_host(SC.build(case), b"".join(case.texts), case.k, case.seed, case.min_shared, stats=st)
    SC.check(rows, st, case)
    assert st["launches"] == 0 and st["table_bytes"] == 0


def test_host_reads_containers_and_min_shared():
    case = SC.case("medians")
    refs, text = SC.build(case), b"".join(case.texts)
    plain = H.screen_host(refs, text, case.k)
    assert np.array_equal(plain, H.screen_host(refs, gzip.compress(text), case.k))
    for ms in (0, 1, 5, 1000):
        st = {}
        SC.check(H.screen_host(refs, text, case.k, 0, ms, stats=st), st, case, min_shared=ms)
    assert len(H.screen_host(refs, text, case.k, 0, 1000)) == 0


def test_revcomp_sample_gives_the_forward_rows():
    f, r = SC.case("forward"), SC.case("revcomp")
    assert np.array_equal(H.screen_host(SC.build(f), f.texts[0], f.k), H.screen_host(SC.build(r), r.texts[0], r.k))
    assert SM.screen([x.hashes for x in f.refs], f.texts, f.k, 0)[0] == SM.screen([x.hashes for x in r.refs], r.texts, r.k, 0)[0]
