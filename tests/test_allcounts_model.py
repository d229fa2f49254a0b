"""The AllCounts model (tests/allcounts_model.py) against hand-worked answers, its literal to_vec walk against its vectorised
form, SketchParams.all_counts, and the host build of the kernel's window logic (finch_rs_amd/csrc/fh_counts.h) against the
model.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import allcounts_model as M
from finch_rs_amd.sketch_schemes import SketchParams

HERE = os.path.dirname(os.path.abspath(__file__))


def rows(records, k):
    kc, km = M.to_vec_arrays(M.saturate(M.forward_counts(records, k)), k)
    return [(int(r["hash"]), bytes(m), int(r["count"]), int(r["extra_count"])) for r, m in zip(kc, km)]


def test_known_answer_acgt_k2():
    # AC (1), CG (6), GT (11): GT folds into AC, CG is a palindrome
    assert rows([b"ACGT"], 2) == [(1, b"AC", 2, 1), (6, b"CG", 2, 1)]
    kc, km, seq_length, nvk = M.sketch([b"ACGT"], 2)
    assert (seq_length, nvk) == (0, 3)
    assert [(int(r["hash"]), bytes(m)) for r, m in zip(kc, km)] == [(1, b"AC"), (6, b"CG")]


def test_known_answers_more():
    # odd k: no palindromes; AAA (0) with TTT (63) folded in
    assert rows([b"AAAA", b"TTT"], 3) == [(0, b"AAA", 3, 1)]
    # a k-mer whose reverse complement never occurred keeps extra 0; one that only occurs reverse-complemented is
    # reported under its own (larger) index with extra 0
    assert rows([b"GG"], 1) == [(2, b"G", 2, 0)]
    assert rows([b"C"], 1) == [(1, b"C", 1, 0)]
    # N, IUPAC codes and '-' break windows; lower case and U count; a multi-line FASTA record joins its lines
    assert rows([b"ACNGT"], 2) == [(1, b"AC", 2, 1)]
    assert rows([b"AC-GT"], 2) == [(1, b"AC", 2, 1)]
    assert rows([b"ACRGT"], 2) == [(1, b"AC", 2, 1)]
    assert rows([b"acgu"], 2) == [(1, b"AC", 2, 1), (6, b"CG", 2, 1)]
    assert rows([b"AC\nGT"], 2) == [(1, b"AC", 2, 1), (6, b"CG", 2, 1)]
    assert rows([b"AC\r\n GT\n"], 4) == [(27, b"ACGT", 2, 1)]
    # windows never span records
    assert rows([b"AC", b"GT"], 2) == [(1, b"AC", 2, 1)]
    # k = 4 palindrome AATT: 2c, extra c
    assert rows([b"AATTAATT"], 4)[0] == (15, b"AATT", 4, 2)


def test_revcomp_index():
    for k in (1, 2, 5, 8, 16):
        rng = np.random.default_rng(k)
        for ix in rng.integers(0, 4 ** k, 50):
            t = M.kmer_text(int(ix), k)
            rc = bytes({65: 84, 67: 71, 71: 67, 84: 65}[b] for b in reversed(t))
            assert M.kmer_text(M.revcomp_ix(int(ix), k), k) == rc


def test_loop_equals_predicate_on_random_counts():
    rng = np.random.default_rng(7)
    for trial in range(300):
        k = int(rng.integers(1, 6))
        n = 4 ** k
        c = np.zeros(n, dtype=np.uint64)
        nz = rng.random(n) < rng.random()
        c[nz] = rng.integers(1, 50, int(nz.sum()))
        if trial % 3 == 0:  # saturated and wrapping counts
            big = rng.random(n) < 0.3
            c[big & nz] = rng.integers(2 ** 31, 2 ** 33, int((big & nz).sum()))
        s = M.saturate(c)
        kc, km = M.to_vec_arrays(s, k)
        got = [(int(r["hash"]), bytes(m), int(r["count"]), int(r["extra_count"])) for r, m in zip(kc, km)]
        assert got == M.to_vec_loop(s, k)
        ix, cs = M.sparse_counts([], k)
        assert len(ix) == 0
        assert all(a[0] < b[0] for a, b in zip(got, got[1:]))


def test_wrapping_add_and_saturation():
    k = 1
    c = M.saturate([2 ** 33, 0, 0, 5])  # A saturated, T five times
    assert M.to_vec_loop(c, k) == [(0, b"A", (M.U32 + 5) & M.U32, 5)]
    assert M.to_vec_loop(M.saturate([0, 3, 2 ** 40, 0]), k) == [(1, b"C", (3 + M.U32) & M.U32, M.U32)]


def test_sketch_params_all_counts():
    p = SketchParams.all_counts()
    assert (p.kind, p.kmer_length) == ("allcounts", 4)
    assert p.hash_info() == ("None", 0, 0, None)
    assert p.expected_size() == 256
    assert SketchParams.all_counts(9).expected_size() == 4 ** 9


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("achost") / "libachost.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "hostcore", "allcounts_host.cpp")])
    L = C.CDLL(so)
    L.ac_host_windows.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.ac_host_windows.restype = C.c_int64
    L.ac_host_revcomp.argtypes = [C.c_uint32, C.c_int]
    L.ac_host_revcomp.restype = C.c_uint32
    L.ac_host_emit.argtypes = [C.c_uint32] * 4
    return L


def packed(records):
    return b"".join(bytes(b for b in r if b not in b" \t\r\n") + b"\0" for r in records)


def random_records(rng, n, maxlen, alphabet=b"ACGTACGTACGTacgtuUNRY-.~ \n"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return [bytes(a[rng.integers(0, len(a), int(rng.integers(0, maxlen)))]) for _ in range(n)]


def test_host_window_logic_equals_model(host_lib):
    rng = np.random.default_rng(11)
    for k in range(1, 17):
        recs = random_records(rng, 40, 300) + [b"A" * 100, b"ACGT" * 30, b"acgu" * 9]
        buf = np.frombuffer(packed(recs), dtype=np.uint8).copy()
        got = np.zeros(buf.size + 1, dtype=np.uint32)
        n = host_lib.ac_host_windows(buf.ctypes.data, buf.size, k, got.ctypes.data)
        want = np.concatenate([M.window_indices(r, k) for r in recs])
        assert n == len(want) and np.array_equal(got[:n].astype(np.uint64), want), k
        for ix in rng.integers(0, 4 ** k, 200):
            rc = M.revcomp_ix(int(ix), k)
            assert host_lib.ac_host_revcomp(int(ix), k) == rc
            for c, crc in ((0, 0), (1, 0), (3, 5), (0, 2)):
                assert host_lib.ac_host_emit(int(ix), rc, c, crc) == int(c > 0 and (rc >= ix or crc == 0))
