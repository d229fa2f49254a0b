"""finch_index_cluster / finch_cluster_host without a device (include/finch_host.h): the symbols, the ABI
version, the option and its range, every refusal finch_index_cluster decides before it looks for a device, finch_cluster_host
against tests/index_cluster_model.py's literal loop, and the whole call on an index of a library without a hash, which has no
device entries."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import finch_rs_amd as F
import index_cluster_model as ICM
import index_dist_cases as X
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError
from index_dist_cases import Spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = (1 << 64) - 1
BELOW_ONE = math.nextafter(1.0, 0.0)
BOUNDS = (0.0, 0.01, 0.1, BELOW_ONE)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def last_error(built):
    return (built.finch_last_error() or b"").decode()


def scaled_m(scale):
    return U64_MAX // int(1.0 / scale)


def mixed_specs(empties, seed=21, n=15, scaled_only=False):
    """Mash and Scaled sketches of three scales and a NaN scale over a pool that straddles the scales' max hashes, kmer_length
    11 and 31 in one library (and 21), near copies, and `empties` empty sketches of three kinds"""
    rng = np.random.default_rng(seed)
    lo, hi = scaled_m(0.001), scaled_m(0.01)
    pool = np.unique(np.concatenate([rng.integers(0, lo, 20, dtype=np.uint64), rng.integers(lo, hi, 20, dtype=np.uint64),
                                     rng.integers(hi, U64_MAX, 20, dtype=np.uint64), np.array([lo - 1, lo, hi - 1, hi], np.uint64)]))
    kinds = [("mash", 0.0, U64_MAX), ("scaled", 0.001, lo), ("scaled", 0.01, hi), ("scaled", 0.5, scaled_m(0.5)), ("scaled", math.nan, U64_MAX)]
    if scaled_only:  # (an empty sketch beside a Mash sketch has no scale step: total 0, distance 0 -- it links every one of them)
        kinds = kinds[1:]
    specs = []
    for s in range(n):
        kind, scale, below = kinds[s % len(kinds)]
        own = pool[pool < np.uint64(below)]
        specs.append(Spec("s%d" % s, own[rng.random(len(own)) < (0.95 if s % 2 == 0 else 0.6)], kind, scale, (11, 31, 21)[s % 3]))
    specs.append(Spec("twin", specs[0].hashes, specs[0].kind, specs[0].scale, 31))  # equal content, another kmer_length
    specs.append(Spec("s5", specs[5].hashes, specs[5].kind, specs[5].scale, specs[5].k))  # equal name and content: linked all the same
    specs.append(Spec("near", specs[0].hashes[:-1], specs[0].kind, specs[0].scale, 11))
    empty = [Spec("e_mash", []), Spec("e_s01", [], "scaled", 0.01), Spec("e_nan", [], "scaled", math.nan, 31), Spec("e_mash2", [], k=11)]
    if scaled_only:
        empty = [Spec("e_s001", [], "scaled", 0.001), Spec("e_s01", [], "scaled", 0.01), Spec("e_nan", [], "scaled", math.nan, 31), Spec("e_s5", [], "scaled", 0.5, 11)]
    return specs + empty[:empties]


def c_cluster_host(built, sk, old_mode, d, n_labels=None, want_edges=True):
    n = len(sk) if n_labels is None else n_labels
    labels = np.full(max(n, 1), 0xdead, np.uint32)
    edges = C.c_uint64(1234)
    rc = built.finch_cluster_host(sk._p, int(old_mode), d, labels.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(edges) if want_edges else None)
    return rc, labels[:n], edges.value


def c_index_cluster(built, ix, sk, old_mode, d, n_labels=None):
    n = len(sk) if n_labels is None else n_labels
    labels = np.full(max(n, 1), 0xdead, np.uint32)
    st = H.CClusterStats()
    rc = built.finch_index_cluster(ix, sk._p, int(old_mode), d, labels.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(st))
    return rc, labels[:n], st


@pytest.fixture()
def hashless(built):
    """an index of four empty sketches: built and clustered without a device"""
    lib = X.build(mixed_specs(4)[-4:])
    p = C.c_void_p()
    assert built.finch_index_new(lib._p, None, 0, C.byref(p)) == _lib.FH_OK and p.value, last_error(built)
    yield p, lib
    built.finch_index_free(p)


def test_symbols_exported_declared_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "finch_host.h")).read()
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("finch_index_cluster", "finch_cluster_host"):
        assert re.search(r"\bint %s\s*\(const finch_" % name, hdr), name
        assert hasattr(raw, name) and name in H._SYMS, name
    assert "finch_cluster_stats;" in hdr and C.sizeof(H.CClusterStats) == 64
    assert H._SYMS["finch_index_cluster"][1][5] == C.c_uint64 and H._SYMS["finch_cluster_host"][1][4] == C.c_uint64


def test_abi_version_is_at_least_20(built):
    hdr = open(os.path.join(ROOT, "include", "finch_hip.h")).read()
    want = int(re.search(r"#define\s+FH_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want >= 20 and _lib.load().fh_abi_version() == want
    assert re.search(r"\b20: .*finch_index_cluster, finch_cluster_host .*index_cluster_margin", hdr.replace("\n", " "))


def test_the_option_and_its_range(built, hashless):
    ix, lib = hashless
    assert "index_cluster_margin" in [n for n, _ in F.option_list()]
    try:
        for value in (2.0 ** -20, 0.25, 0.5, "9.5367431640625e-07"):
            F.set_option("index_cluster_margin", value)
            rc, labels, _ = c_index_cluster(built, ix, lib, False, 0.1)
            assert rc == _lib.FH_OK and labels.tolist() == [0, 0, 0, 0], (value, last_error(built))
        for value in (2.0 ** -21, 0.6, 0, -0.25, "nan", "x", math.nextafter(2.0 ** -20, 0.0)):
            F.set_option("index_cluster_margin", value)
            rc, labels, _ = c_index_cluster(built, ix, lib, False, 0.1)
            assert rc == _lib.FH_ERR_INVALID and "index_cluster_margin" in last_error(built) and "2^-20" in last_error(built), value
            assert labels.tolist() == [0xdead] * 4  # refused before anything is written
    finally:
        F.set_option("index_cluster_margin", None)
    assert c_index_cluster(built, ix, lib, False, 0.1)[0] == _lib.FH_OK


def test_refusals_that_need_no_device(built, hashless):
    ix, lib = hashless
    labels = (C.c_uint32 * 8)()
    assert built.finch_index_cluster(None, lib._p, 0, 0.1, labels, 4, None) == _lib.FH_ERR_INVALID and "null argument" in last_error(built)
    assert built.finch_index_cluster(ix, None, 0, 0.1, labels, 4, None) == _lib.FH_ERR_INVALID and "null argument" in last_error(built)
    assert built.finch_index_cluster(ix, lib._p, 0, 0.1, None, 4, None) == _lib.FH_ERR_INVALID and "null argument" in last_error(built)
    assert built.finch_cluster_host(None, 0, 0.1, labels, 4, None) == _lib.FH_ERR_INVALID
    assert built.finch_cluster_host(lib._p, 0, 0.1, None, 4, None) == _lib.FH_ERR_INVALID
    assert built.finch_index_cluster(ix, lib._p, 0, 0.1, labels, 4, None) == _lib.FH_OK  # stats may be NULL
    for d in (1.0, 1.5, math.inf):
        rc, _, _ = c_index_cluster(built, ix, lib, False, d)
        assert rc == _lib.FH_ERR_INVALID and "every pair is within a bound >= 1" in last_error(built), d
    for n in (0, 3, 5):
        rc, _, _ = c_index_cluster(built, ix, lib, False, 0.1, n_labels=n)
        assert rc == _lib.FH_ERR_INVALID and "n_labels %d" % n in last_error(built)
        rc, _, _ = c_cluster_host(built, lib, False, 0.1, n_labels=n)
        assert rc == _lib.FH_ERR_INVALID and "n_labels %d" % n in last_error(built)
    # refs must be the library of the index: another sketch count, another hash count
    three, full = X.build(mixed_specs(3)[-3:]), X.build(mixed_specs(3)[-3:] + [Spec("h", [1, 2])])
    for other in (three, full):
        rc, _, _ = c_index_cluster(built, ix, other, False, 0.1)
        assert rc == _lib.FH_ERR_INVALID and "refs must be the library of the index" in last_error(built)
    # hashes that do not ascend strictly; old mode with an empty sketch next to a non-empty one
    bad = X.build([Spec("a", [1, 2, 3]), Spec("b", [5, 5, 6])])
    rc, _, _ = c_cluster_host(built, bad, False, 0.1)
    assert rc == _lib.FH_ERR_INVALID and "not strictly ascending" in last_error(built)
    rc, _, _ = c_cluster_host(built, full, True, 0.1)
    assert rc == _lib.FH_ERR_INVALID and "old_distance: empty query sketch" in last_error(built)
    with pytest.raises(ICM.M.ReferencePanics):
        ICM.cluster(X.model(mixed_specs(3)[-3:] + [Spec("h", [1, 2])]), True, 0.1)


@pytest.mark.parametrize("which,old_mode", [("mixed", False), ("mixed", True), ("mixed_empties", False), ("scaled_empties", False)])
def test_cluster_host_is_the_model(built, which, old_mode):
    specs = mixed_specs(0 if which == "mixed" else 4, scaled_only=which == "scaled_empties")
    sk, model = X.build(specs), X.model(specs)
    seen = set()
    for d in BOUNDS + (-0.0, 0.3):
        want_labels, want_edges = ICM.cluster(model, old_mode, d)
        rc, labels, edges = c_cluster_host(built, sk, old_mode, d)
        assert rc == _lib.FH_OK, last_error(built)
        assert labels.tolist() == want_labels and edges == want_edges, (old_mode, d)
        got = []
        assert H.cluster_host(sk, d, old_mode, edges=got).tolist() == want_labels and got == [want_edges]
        assert c_cluster_host(built, sk, old_mode, d, want_edges=False)[1].tolist() == want_labels  # edges may be NULL
        seen.add(len(set(want_labels)))
        assert want_labels[16] == want_labels[5]  # equal name and content: linked, whatever finch_dist's self-skip does
    if which == "mixed_empties":  # the empty Mash sketch is at distance 0 of every sketch
        assert seen == {1}
    else:
        assert len(seen) >= 2 and 1 < max(seen) < len(specs)  # the bounds tell clusterings apart, and none is the identity
    labels0 = ICM.cluster(model, old_mode, 0.0)[0]
    assert labels0[15] == labels0[0] and (which == "mixed" or labels0[-1] == labels0[-4])  # the twin at distance 0; empty beside empty


@pytest.mark.parametrize("old_mode", [False, True])
def test_a_bound_that_links_nothing_and_one_that_links_everything(built, old_mode):
    specs = mixed_specs(0 if old_mode else 2)
    sk = X.build(specs)
    for d in (math.nan, -1.0, -5e-324, -math.inf):
        rc, labels, edges = c_cluster_host(built, sk, old_mode, d)
        assert rc == _lib.FH_OK and labels.tolist() == list(range(len(specs))) and edges == 0
    rc, labels, edges = c_cluster_host(built, sk, old_mode, 1.0)
    assert rc == _lib.FH_OK and not labels.any() and edges == len(specs) * (len(specs) - 1)


@pytest.mark.parametrize("old_mode", [False, True])
def test_an_index_without_a_hash_clusters_on_the_host(built, hashless, old_mode):
    ix, lib = hashless
    model = X.model(mixed_specs(4)[-4:])
    for d in BOUNDS:
        want_labels, want_edges = ICM.cluster(model, old_mode, d)
        rc, labels, st = c_index_cluster(built, ix, lib, old_mode, d)
        assert rc == _lib.FH_OK, last_error(built)
        assert labels.tolist() == want_labels == [0, 0, 0, 0] and st.edges == want_edges == 12
        assert labels.tolist() == c_cluster_host(built, lib, old_mode, d)[1].tolist()
        assert (st.launches, st.pairs_touched, st.pairs_united, st.pairs_copied, st.pairs_kept_host, st.clusters, st.kernel_ms) == (0, 0, 0, 0, 0, 1, 0.0)
    for d in (math.nan, -1.0):
        rc, labels, st = c_index_cluster(built, ix, lib, old_mode, d)
        assert rc == _lib.FH_OK and labels.tolist() == [0, 1, 2, 3] and (st.edges, st.clusters) == (0, 4)
    with H.LibraryIndex(lib) as pix:  # the Python layer on the same library
        st = {}
        assert pix.cluster(0.1, old_mode, stats=st).tolist() == [0, 0, 0, 0] and st["edges"] == 12 and st["clusters"] == 1
        assert pix.cluster(math.nan, old_mode).tolist() == [0, 1, 2, 3]
        with pytest.raises(FinchError):
            pix.cluster(1.0, old_mode)
        assert pix.dereplicate(0.1, old_mode).tolist() == [0, 0, 0, 0] and len(pix.refs) == 1
