"""The key-word tables of the sketch kernels (finch_rs_amd/csrc/fh_core.h: lut_rec_A, lut_rec_B, lut_rec_P, key_word_mix), compiled
for the HOST.  A k2 word's cross term w * hi(2 c1) comes from the tables (the A group's share in the high word of the A record's
U, the B group's in the B record's second dword): every pair of groups of both word kinds must give rotl(x * c, R) * C, and the
hash made of the words must be murmur3's for every k."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "kword_tables_host.cpp")
SO = os.path.join(HERE, "hostcore", "libkword_tables_host.so")


@pytest.fixture(scope="module")
def shim():
    hdr = os.path.join(HERE, "..", "finch_rs_amd", "csrc", "fh_core.h")
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        tmp = "%s.tmp.%d" % (SO, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, SO)
    L = C.CDLL(SO)
    L.kword_pairs.restype = C.c_int64
    L.kword_pairs.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    L.kword_last_pair.restype = C.c_int
    L.kword_last_pair.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.kword_hashes.restype = C.c_int
    L.kword_hashes.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("what,pairs", [(0, 65536), (1, 65536)])
def test_every_pair_of_full_groups(shim, what, pairs):
    """k1 (0) and k2 (1) words: 256 x 256 pairs of 4-base groups"""
    n = C.c_uint64()
    assert shim.kword_pairs(what, C.byref(n)) == 0
    assert n.value == pairs


@pytest.mark.parametrize("k,is_k2,nb", [(6, 0, 2), (7, 0, 3), (14, 1, 2), (15, 1, 3), (22, 0, 2), (23, 0, 3), (30, 1, 2), (31, 1, 3)])
def test_every_short_high_group_from_table_p(shim, k, is_k2, nb):
    """the word whose high group has 2 or 3 bases takes its B record from table P's builder (lut_rec_P<K>): 256 x 4^nb pairs"""
    geom = (C.c_int * 3)()
    assert shim.kword_last_pair(k, geom) >= 0
    assert list(geom) == [is_k2, nb, 1]
    n = C.c_uint64()
    assert shim.kword_pairs(k, C.byref(n)) == 0
    assert n.value == 256 * 4 ** nb


def test_which_k_have_a_short_high_group(shim):
    """the K the test above walks are all there are, up to the key's whole blocks in front (K and K + 16 share the word)"""
    short = {}
    for k in range(1, 33):
        geom = (C.c_int * 3)()
        if shim.kword_last_pair(k, geom) >= 0 and geom[2]:
            short[k] = (geom[0], geom[1])
    assert short == {6: (0, 2), 7: (0, 3), 14: (1, 2), 15: (1, 3), 22: (0, 2), 23: (0, 3), 30: (1, 2), 31: (1, 3)}


def canonical_words(rng, k, n):
    """n random k-mers as ASCII and their canonical m-form words (A 0, C 1, G 2, T 3, first base on top)"""
    codes = rng.integers(0, 4, size=(n, k), dtype=np.uint64)
    rc = (np.uint64(3) - codes)[:, ::-1]
    weights = np.uint64(1) << (np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64))
    f, r = (codes * weights).sum(axis=1, dtype=np.uint64), (rc * weights).sum(axis=1, dtype=np.uint64)
    canon = np.where((f < r)[:, None], codes, rc)
    words = np.ascontiguousarray(np.minimum(f, r))
    ascii_ = np.frombuffer(b"ACGT", np.uint8)[canon.astype(np.intp)]
    return words, [bytes(row) for row in ascii_]


@pytest.mark.parametrize("seed", [0, 2**63 + 5])
@pytest.mark.parametrize("k", list(range(1, 33)))
def test_hashes_of_random_canonical_words(shim, k, seed):
    rng = np.random.default_rng(7000 + k)
    words, kmers = canonical_words(rng, k, 2000)
    fast, lut = np.zeros(len(words), np.uint64), np.zeros(len(words), np.uint64)
    assert shim.kword_hashes(k, words.ctypes.data, len(words), seed, fast.ctypes.data, lut.ctypes.data) == 0
    assert np.array_equal(fast, lut)
    want = np.array([O.hash_f(km, seed) for km in kmers], dtype=np.uint64)
    assert np.array_equal(fast, want)
