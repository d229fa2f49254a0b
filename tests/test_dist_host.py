"""finch_dist (the `dist` subcommand, cli/src/main.rs:85-125) without a device: argument checks, the ascending-hash check,
old_mode's empty-query error, the missing-device error, and the query selection of dist_command."""
import ctypes as C

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


def mk(name, hashes, params=None, k=21):
    hs = np.asarray(hashes, np.uint64)
    kc = np.zeros(len(hs), KC_DTYPE)
    kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
    km = np.zeros((len(hs), k), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, params or SketchParams.mash(kmer_length=k), H.FilterParams(False))


def collect(*sks):
    out = mk(sks[0][0], sks[0][1])
    for name, hs in sks[1:]:
        out.append(mk(name, hs))
    return out


def test_null_arguments(built):
    a = collect(("a", [1, 2, 3]))
    out = C.c_void_p()
    dev = (C.c_int * 1)(0)
    assert built.finch_dist(None, a._p, 0, 1.0, dev, 1, C.byref(out)) == -1
    assert built.finch_dist(a._p, None, 0, 1.0, dev, 1, C.byref(out)) == -1
    assert built.finch_dist(a._p, a._p, 0, 1.0, dev, 1, None) == -1
    assert built.finch_dist(a._p, a._p, 0, 1.0, None, 1, C.byref(out)) == -1
    assert b"null argument" in built.finch_last_error()
    devs = (C.c_int * 17)(*([0] * 17))
    assert built.finch_dist(a._p, a._p, 0, 1.0, devs, 17, C.byref(out)) == -1
    assert built.finch_dist_len(None) == 0
    assert built.finch_dist_copy(None, None, None, None) == -1
    assert built.finch_dist_to_json(None, None, None) == -1
    built.finch_dist_free(None)


@pytest.mark.parametrize("bad", [[5, 3, 9], [3, 3, 9], [1, 2, 2]])
@pytest.mark.parametrize("side", ["query", "reference"])
def test_unsorted_or_duplicate_hashes_refused(built, bad, side):
    good = collect(("g0", [1, 2, 3]), ("g1", [2, 4]))
    bad_set = collect(("g0", [1, 2, 3]), ("bad sketch", bad))
    q, r = (bad_set, good) if side == "query" else (good, bad_set)
    with pytest.raises(FinchError) as ei:
        H.dist(q, r)
    msg = str(ei.value)
    assert "%s sketch 1 (bad sketch)" % side in msg and "strictly ascending" in msg


def test_unsorted_hashes_from_sk_text_refused(built):
    text = mk("from text", [10, 20, 30]).to_json()
    assert '"hashes":["10","20","30"]' in text
    sk = H.sketches_from_json(text.replace('"hashes":["10","20","30"]', '"hashes":["40","20","30"]').encode())
    hs = sk.sketch(0).arrays[0]["hash"]
    assert list(hs) != sorted(set(hs.tolist())), "the .sk text was not altered"
    with pytest.raises(FinchError) as ei:
        H.dist(sk, mk("x", [1]))
    assert "query sketch 0 (from text)" in str(ei.value)


def test_old_mode_empty_query_is_the_distance_error(built):
    qs = collect(("full", [1, 2]), ("empty", []))
    rs = collect(("r", [1, 5]))
    with pytest.raises(FinchError) as ref:
        H.distance(qs, 1, rs, 0, old_mode=True)
    with pytest.raises(FinchError) as ei:
        H.dist(qs, rs, old_mode=True)
    assert str(ei.value) == str(ref.value) == "old_distance: empty query sketch"


def test_no_device_is_an_error(built):
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    a = collect(("a", [1, 2, 3]), ("b", [2, 3]))
    with pytest.raises(F.FinchHipError) as ei:
        H.dist(a, a)
    assert "no usable HIP device" in str(ei.value)
    with pytest.raises(F.FinchHipError):
        H.dist_command(a, pairwise=True)
    # an empty call needs a device too: there is no CPU path at all
    with pytest.raises(F.FinchHipError):
        H.dist(H.select(a, []), a)


def test_select(built):
    a = collect(("a", [1]), ("b", [2, 3]), ("c", [4, 5, 6]))
    s = H.select(a, [2, 0, 2])
    assert len(s) == 3
    assert [built.finch_sketch_name(s._p, i).decode() for i in range(3)] == ["c", "a", "c"]
    assert [built.finch_sketch_n_hashes(s._p, i) for i in range(3)] == [3, 1, 3]
    with pytest.raises(FinchError):
        H.select(a, [3])


def test_dist_queries_selection():
    names = ["a", "b", "a", "c"]
    assert H.dist_queries(names, pairwise=True) is None
    assert H.dist_queries(names, pairwise=True, queries={"b"}) is None  # --pairwise wins (main.rs:92)
    assert H.dist_queries(names, queries={"a", "zz"}) == [0, 2]
    assert H.dist_queries(names, queries=[]) == []
    assert H.dist_queries(names) == [0]
    with pytest.raises(FinchError, match="No sketches present!"):
        H.dist_queries([])
    assert H.dist_queries([], queries={"a"}) == []


def test_dist_command_selection_through_a_stub(monkeypatch, built):
    a = collect(("a", [1]), ("b", [2]), ("c", [3]))
    calls = []

    def fake_dist(q, r, max_distance, old_mode, devices):
        calls.append(([built.finch_sketch_name(q._p, i).decode() for i in range(len(q))], len(r), max_distance, old_mode))
        rows = np.zeros(len(q), H.DIST_DTYPE)
        rows["query"] = np.arange(len(q))
        return rows

    monkeypatch.setattr(H, "dist", fake_dist)
    rows = H.dist_command(a, queries={"c", "b"}, max_distance=0.5, old_mode=True)
    assert calls[-1] == (["b", "c"], 3, 0.5, True)
    assert list(rows["query"]) == [1, 2]  # indices into the sketches given
    H.dist_command(a)
    assert calls[-1][0] == ["a"]
    H.dist_command(a, pairwise=True)
    assert calls[-1][0] == ["a", "b", "c"]
