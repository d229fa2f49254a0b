"""finch_index_cluster on the GPU (include/finch_host.h).  Every case holds the call's labels and its `edges`
against finch_cluster_host, the contract's loop on the host; where the names are distinct, `edges` also against the rows
finch_dist gives for the library beside itself (its diagonal aside: a NaN-scaled sketch is not equal to itself); the stats
against each other; and, where tests/index_cluster_model.py has followed the device's path, against its counts."""
import math
from functools import lru_cache

import numpy as np
import pytest

import finch_rs_amd as F
import index_cluster_model as ICM
import index_dist_cases as X
from finch_rs_amd import host as H
from index_dist_cases import Spec

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
SHARED_HASH = 1 << 62


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def index_with_chunk(refs, chunk, devices=(0,)):
    try:
        F.set_option("index_chunk_queries", chunk)  # (read when the index is built)
        return H.LibraryIndex(refs, devices=devices)
    finally:
        F.set_option("index_chunk_queries", None)


@lru_cache(None)
def host_answer(lib, old_mode, d):
    """finch_cluster_host for a library of this module (by its builder's name): (labels, edges, ordered rows of finch_dist)"""
    sk = built(lib)
    edges = []
    labels = H.cluster_host(sk, d, old_mode, edges=edges)
    rows = H.dist(sk, sk, d, old_mode)
    return labels.tolist(), edges[0], int((rows["query"] != rows["reference"]).sum())


def check(ix, sk, want, old_mode, d, distinct_names=True):
    """one call against (labels, edges, rows of finch_dist) -> its labels and stats"""
    st = {}
    labels = ix.cluster(d, old_mode, stats=st)
    assert labels.dtype == np.uint32 and labels.tolist() == want[0], (old_mode, d, st)
    assert st["edges"] == want[1], (old_mode, d, st)
    if distinct_names:
        assert st["edges"] == want[2], (old_mode, d, st)
    assert st["clusters"] == len(set(want[0])) and st["pairs_kept_host"] <= st["pairs_copied"]
    assert st["pairs_united"] + st["pairs_copied"] <= st["pairs_touched"]
    assert st["pairs_united"] + st["pairs_kept_host"] <= st["edges"]
    return labels, st


def near(base, n_drop, fresh):
    """`base` with its last n_drop hashes replaced by larger ones from `fresh` on: the walk gives jaccard 1 - n_drop / len"""
    base = np.asarray(base, np.uint64)
    return np.concatenate([base[:len(base) - n_drop], np.arange(fresh, fresh + n_drop, dtype=np.uint64)])


# ----------------------------------------------------------------------------------------------------------------------
# the libraries, by name; built once
# ----------------------------------------------------------------------------------------------------------------------

CHAIN_D = 0.004
# where chain position p sits in the library: reversed -- the links come 9-8, 8-7, ... as the queries ascend --, and scrambled
CHAIN_ORDERS = {"reversed": [9 - p for p in range(10)], "scrambled": [9, 4, 7, 0, 2, 8, 5, 1, 6, 3]}


def chain_specs(order):
    """ten windows of 40 over a run of hashes, each 4 further: neighbours are within CHAIN_D (jaccard 36 / 40 by the walk), no
    other pair is (32 / 40 at best)"""
    specs = [None] * 10
    for p in range(10):
        specs[order[p]] = Spec("c%d" % p, [1000 + 7 * (4 * p + t) for t in range(40)])
    return specs


def star_specs():
    """two stars, 0..3 around sketch 0 and 4..7 around sketch 4, over ranges of their own; sketches 3 (kmer_length 11) and 7
    (kmer_length 31) share 15 hashes of 85: within 0.05 only with 7 as the query, the last one"""
    a, b, x = np.arange(10_000, 10_050, dtype=np.uint64), np.arange(20_000, 20_050, dtype=np.uint64), np.arange(100, 115, dtype=np.uint64)
    tail = lambda n, at: np.arange(at, at + n, dtype=np.uint64)  # noqa: E731
    return [Spec("a", a), Spec("a1", near(a, 2, 30_000)), Spec("a2", near(a, 8, 31_000)), Spec("a3", np.concatenate([x, a[:25], tail(10, 32_000)]), k=11),
            Spec("b", b), Spec("b1", near(b, 5, 33_000)), Spec("b2", near(b, 1, 34_000)), Spec("b3", np.concatenate([x, b[:25], tail(10, 35_000)]), k=31)]


def apart_specs():
    """40 sketches of 20 hashes of their own and one that all share: every pair is touched, none is within 0.05"""
    return [Spec("r%d" % r, [1000 * (r + 1) + t for t in range(20)] + [SHARED_HASH]) for r in range(40)]


def identical_specs():
    return [Spec("d%d" % r, [11 * t + 5 for t in range(64)]) for r in range(300)]


def one_way_specs():
    """jaccard 15 / 85 at 0.05: within the bound for a query of kmer_length 31, not for one of 11; and a third sketch apart"""
    s = star_specs()
    return [s[3], s[7], Spec("apart", [7, 8, 9])]


def old_asym_specs():
    """old mode: 20 hashes inside 60.  Query the 60, reference the 20: c / |R| = 1; the other way 20 / (20 + 2 * 40)"""
    big = np.arange(500, 560, dtype=np.uint64)
    return [Spec("big", big), Spec("small", big[::3]), Spec("other", np.arange(900, 930, dtype=np.uint64)), Spec("other2", np.arange(905, 935, dtype=np.uint64))]


def scaled_m(scale):
    return U64_MAX // int(1.0 / scale)


def mixed_specs(scaled_only):
    """Mash and Scaled sketches of three scales and a NaN scale over a pool that straddles the scales' max hashes, kmer_length
    11, 21 and 31, and empty sketches: with an empty Mash sketch, which is at distance 0 of every sketch, or Scaled ones only"""
    rng = np.random.default_rng(31)
    lo, hi = scaled_m(0.001), scaled_m(0.01)
    pool = np.unique(np.concatenate([rng.integers(0, lo, 20, dtype=np.uint64), rng.integers(lo, hi, 20, dtype=np.uint64),
                                     rng.integers(hi, U64_MAX, 20, dtype=np.uint64), np.array([lo - 1, lo, hi - 1, hi], np.uint64)]))
    kinds = [("mash", 0.0, U64_MAX), ("scaled", 0.001, lo), ("scaled", 0.01, hi), ("scaled", 0.5, scaled_m(0.5)), ("scaled", math.nan, U64_MAX)]
    kinds = kinds[1:] if scaled_only else kinds
    specs = []
    for s in range(20):
        kind, scale, below = kinds[s % len(kinds)]
        own = pool[pool < np.uint64(below)]
        specs.append(Spec("s%d" % s, own[rng.random(len(own)) < (0.95 if s % 2 == 0 else 0.6)], kind, scale, (11, 31, 21)[s % 3]))
    specs.append(Spec("s5", specs[5].hashes, specs[5].kind, specs[5].scale, specs[5].k))  # equal name and content: linked all the same
    if scaled_only:
        return specs + [Spec("e_s001", [], "scaled", 0.001), Spec("e_s01", [], "scaled", 0.01), Spec("e_nan", [], "scaled", math.nan, 31)]
    return specs + [Spec("e_mash", []), Spec("e_s01", [], "scaled", 0.01), Spec("e_nan", [], "scaled", math.nan, 31)]


def pool_specs():
    """140 sketches: 14 groups, each drawing 30..64 hashes from 80 of its own -- jaccards from a fifth to four fifths --, two
    exact copies per group, kmer_length 21, 31 and 11 in turn, and one hash that all share: 140 x 140 pairs are touched, and
    few of them are near a bound"""
    rng = np.random.default_rng(41)
    specs = []
    for g in range(14):
        own = np.unique(rng.integers(1 << 20, 1 << 30, 100, dtype=np.uint64))[:80] + np.uint64(g << 32)
        for t in range(10):
            hs = np.sort(rng.choice(own, int(rng.integers(30, 64)), replace=False)) if t < 8 else specs[-2].hashes[:-1]
            specs.append(Spec("p%d_%d" % (g, t), np.concatenate([hs, [np.uint64(SHARED_HASH)]]), k=(21, 31, 11)[len(specs) % 3]))
    return specs


BUILDERS = {"chain_reversed": lambda: chain_specs(CHAIN_ORDERS["reversed"]), "chain_scrambled": lambda: chain_specs(CHAIN_ORDERS["scrambled"]),
            "stars": star_specs, "apart": apart_specs, "identical": identical_specs, "one_way": one_way_specs, "old_asym": old_asym_specs,
            "mixed_empties": lambda: mixed_specs(False), "scaled_empties": lambda: mixed_specs(True), "pools": pool_specs}


@lru_cache(None)
def specs_of(lib):
    return BUILDERS[lib]()


@lru_cache(None)
def built(lib):
    return X.build(specs_of(lib))


@lru_cache(None)
def model_bands(lib, old_mode, d, m):
    return ICM.bands(X.model(specs_of(lib)), old_mode, d, m)


def pairs_of(lib, old_mode, d):
    rows = H.dist(built(lib), built(lib), d, old_mode)
    return {(int(q), int(r)) for q, r in zip(rows["query"], rows["reference"]) if q != r}


# ----------------------------------------------------------------------------------------------------------------------
# by hand
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["reversed", "scrambled"])
def test_a_chain_whose_links_arrive_one_launch_at_a_time(order):
    lib = "chain_" + order
    place = CHAIN_ORDERS[order]
    neighbours = {(place[p], place[p + 1]) for p in range(9)}
    assert pairs_of(lib, False, CHAIN_D) == neighbours | {(b, a) for a, b in neighbours}  # the ends are not within the bound
    want = host_answer(lib, False, CHAIN_D)
    assert want[0] == [0] * 10 and want[1] == 18
    for chunk, launches in ((1, 10), (2, 5), (None, 1)):  # the parent array has to survive the launches
        with index_with_chunk(built(lib), chunk) as ix:
            _, st = check(ix, built(lib), want, False, CHAIN_D)
            assert st["launches"] == launches and st["pairs_united"] == 18 and st["pairs_copied"] == 0 and st["kernel_ms"] > 0
            check(ix, built(lib), host_answer(lib, False, 0.0), False, 0.0)  # ten clusters on the same index
            assert host_answer(lib, False, 0.0)[0] == list(range(10))
            check(ix, built(lib), host_answer(lib, True, CHAIN_D), True, CHAIN_D)


def test_two_stars_joined_by_one_late_pair():
    across = {(q, r) for q, r in pairs_of("stars", False, 0.05) if (q < 4) != (r < 4)}
    assert across == {(7, 3)}  # the last query's pair, and one way only
    want = host_answer("stars", False, 0.05)
    assert want[0] == [0] * 8
    for chunk in (1, 3, None):
        with index_with_chunk(built("stars"), chunk) as ix:
            _, st = check(ix, built("stars"), want, False, 0.05)
            assert st["pairs_united"] == want[1] and st["pairs_touched"] == 8 + 2 * (6 + 6 + 1)
            check(ix, built("stars"), host_answer("stars", False, 0.01), False, 0.01)
    assert host_answer("stars", False, 0.01)[0] == [0, 0, 0, 3, 4, 4, 4, 7]


def test_a_library_with_no_pair_within_the_bound():
    want = host_answer("apart", False, 0.05)
    assert want[0] == list(range(40)) and want[1] == 0
    with H.LibraryIndex(built("apart")) as ix:
        for old_mode in (False, True):
            _, st = check(ix, built("apart"), host_answer("apart", old_mode, 0.05), old_mode, 0.05)
            assert st["pairs_united"] == 0 and st["pairs_copied"] == 0 and st["pairs_touched"] == 40 * 40 and st["clusters"] == 40


def test_300_identical_sketches_at_distance_zero():
    """one cluster through the jaccard-1 rule: 300 x 299 unions that contend for one root, and nothing for the host"""
    want = host_answer("identical", False, 0.0)
    assert want[0] == [0] * 300 and want[1] == 300 * 299
    with H.LibraryIndex(built("identical")) as ix:
        _, st = check(ix, built("identical"), want, False, 0.0)
        assert st["pairs_united"] == 300 * 299 and st["pairs_touched"] == 300 * 300
        assert st["pairs_copied"] <= 300  # the band's share: the self pairs at most
        check(ix, built("identical"), host_answer("identical", True, 0.0), True, 0.0)


def test_a_pair_that_passes_with_one_kmer_length_only():
    assert pairs_of("one_way", False, 0.05) == {(1, 0)}  # query of kmer_length 31, reference of 11
    want = host_answer("one_way", False, 0.05)
    assert want[0] == [0, 0, 2] and want[1] == 1
    with H.LibraryIndex(built("one_way")) as ix:
        _, st = check(ix, built("one_way"), want, False, 0.05)
        assert st["pairs_united"] == 1


def test_old_mode_links_a_pair_that_passes_one_way():
    assert pairs_of("old_asym", True, 0.05) >= {(0, 1)} and (1, 0) not in pairs_of("old_asym", True, 0.05)
    want = host_answer("old_asym", True, 0.05)
    assert want[0][:2] == [0, 0]
    with H.LibraryIndex(built("old_asym")) as ix:
        _, st = check(ix, built("old_asym"), want, True, 0.05)
        assert st["pairs_united"] >= 1  # c == |R|: jaccard 1
        check(ix, built("old_asym"), host_answer("old_asym", False, 0.05), False, 0.05)


@pytest.mark.parametrize("lib", ["mixed_empties", "scaled_empties"])
def test_empty_sketches_among_the_others(lib):
    """the host-made pairs: both sides empty, one side empty beside Mash (always distance 0) and beside Scaled (only with no
    hash below the pair's max hash)"""
    specs = specs_of(lib)
    empties = [v for v, s in enumerate(specs) if not len(s.hashes)]
    with index_with_chunk(built(lib), 5) as ix:
        for d in (0.4, 0.1, 0.0):
            want = host_answer(lib, False, d)
            labels, st = check(ix, built(lib), want, False, d, distinct_names=False)
            assert labels[20] == labels[5]  # equal name and content: no self-skip
            host_made = st["edges"] - st["pairs_united"] - st["pairs_kept_host"]
            assert host_made >= len(empties) * (len(empties) - 1)  # empty beside empty
            b = model_bands(lib, False, d, ICM.MARGIN_DEFAULT)
            assert (st["pairs_touched"], st["pairs_united"], st["pairs_copied"], st["pairs_kept_host"]) == \
                (b["touched"], b["united"], b["copied"], b["kept_host"])
        if lib == "mixed_empties":
            assert not labels.any()  # the empty Mash sketch links every sketch
        else:
            assert 1 < st["clusters"] < len(specs)  # (at 0: an empty Scaled sketch links only what has no hash below the pair's max hash)


# ----------------------------------------------------------------------------------------------------------------------
# pools: the bands at work
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("old_mode", [False, True])
@pytest.mark.parametrize("d", [0.01, 0.1])
def test_pools(old_mode, d):
    b = model_bands("pools", old_mode, d, ICM.MARGIN_DEFAULT)
    assert b["united"] > 0 and 100 * b["copied"] <= b["touched"]  # the library was chosen for this, with room
    with H.LibraryIndex(built("pools")) as ix:
        labels, st = check(ix, built("pools"), host_answer("pools", old_mode, d), old_mode, d)
        assert st["pairs_united"] > 0 and 10 * st["pairs_copied"] <= st["pairs_touched"] == 140 * 140
        assert (st["pairs_united"], st["pairs_copied"], st["pairs_kept_host"]) == (b["united"], b["copied"], b["kept_host"])
        assert 14 <= st["clusters"] < 140


@pytest.mark.parametrize("old_mode", [False, True])
@pytest.mark.parametrize("d", [0.01, 0.1])
def test_pools_with_a_wide_band(old_mode, d):
    """index_cluster_margin 0.25: the pairs up to a quarter above the bound cross to the host's exact test, which keeps them"""
    b = model_bands("pools", old_mode, d, 0.25)
    assert b["kept_host"] > 0
    try:
        F.set_option("index_cluster_margin", 0.25)
        with H.LibraryIndex(built("pools")) as ix:
            labels, st = check(ix, built("pools"), host_answer("pools", old_mode, d), old_mode, d)
    finally:
        F.set_option("index_cluster_margin", None)
    assert st["pairs_kept_host"] > 0 and st["pairs_copied"] > model_bands("pools", old_mode, d, ICM.MARGIN_DEFAULT)["copied"]
    assert (st["pairs_united"], st["pairs_copied"], st["pairs_kept_host"]) == (b["united"], b["copied"], b["kept_host"])


def test_three_device_entries():
    """chunks of two queries dealt over three entries: three label arrays for the host to merge"""
    for lib, d in (("pools", 0.1), ("chain_scrambled", CHAIN_D), ("scaled_empties", 0.1)):
        with index_with_chunk(built(lib), 2, (0, 0, 0)) as ix:
            _, st = check(ix, built(lib), host_answer(lib, False, d), False, d, distinct_names=lib != "scaled_empties")
            assert st["launches"] == (len(specs_of(lib)) + 1) // 2
            if lib == "pools":
                b = model_bands("pools", False, d, ICM.MARGIN_DEFAULT)
                assert (st["pairs_united"], st["pairs_copied"]) == (b["united"], b["copied"])


def test_a_cluster_leaves_the_counters_clean():
    queries = H.select(built("pools"), [3, 17, 64, 139])
    with H.LibraryIndex(built("pools")) as ix:
        first = ix.search(queries, 0.05, 5)
        assert len(first[1]) > 5
        check(ix, built("pools"), host_answer("pools", False, 0.1), False, 0.1)
        again = ix.search(queries, 0.05, 5)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        check(ix, built("pools"), host_answer("pools", True, 0.01), True, 0.01)
        again = ix.search(queries, 0.05, 5)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        assert ix.dist(None, 0.1).tobytes() == H.dist(built("pools"), built("pools"), 0.1).tobytes()


def as_records(sk):
    """name, kmer_length and hashes of every sketch (a library of several kmer_lengths has no JSON form)"""
    L, out = H.lib(), []
    for i in range(len(sk)):  # (column by column: Sketches.sketch sizes its k-mer buffer by the collection's kmer_length)
        hs = np.zeros(L.finch_sketch_n_hashes(sk._p, i), np.uint64)
        assert L.finch_sketch_copy(sk._p, i, hs.ctypes.data, None, None, None) == 0
        out.append((L.finch_sketch_name(sk._p, i).decode(), sk.params_of(i).kmer_length, hs.tolist()))
    return out


def fresh_cluster(sk, d):
    with H.LibraryIndex(sk) as ix:
        st = {}
        return ix.cluster(d, stats=st).tolist(), st["edges"]


def test_after_add_and_after_keep():
    stars, chain = built("stars"), built("chain_scrambled")
    lib = H.select(stars, np.arange(len(stars)))
    with H.LibraryIndex(lib) as ix:
        ix.add(H.select(chain, np.arange(len(chain))))
        for d in (CHAIN_D, 0.05):
            st = {}
            labels = ix.cluster(d, stats=st).tolist()
            assert (labels, st["edges"]) == fresh_cluster(ix.refs, d)
            assert labels == H.cluster_host(ix.refs, d).tolist() and len(labels) == 18
        assert ix.cluster(0.05).tolist()[:8] == [0] * 8
        ix.keep([0, 1, 2, 4, 5, 6, 7, 9, 10, 12, 17])  # without the stars' joint; a chain with gaps
        for d in (CHAIN_D, 0.05):
            st = {}
            labels = ix.cluster(d, stats=st).tolist()
            assert (labels, st["edges"]) == fresh_cluster(ix.refs, d)
            assert labels == H.cluster_host(ix.refs, d).tolist() and len(labels) == 11
        assert ix.cluster(0.05).tolist()[:7] == [0, 0, 0, 3, 3, 3, 3]


@pytest.mark.parametrize("lib,d", [("pools", 0.1), ("stars", 0.05), ("apart", 0.05)])
def test_dereplicate(lib, d):
    sk = built(lib)
    with H.LibraryIndex(H.select(sk, np.arange(len(sk)))) as ix:
        labels = ix.dereplicate(d)
        assert labels.tolist() == host_answer(lib, False, d)[0]
        keep = np.unique(labels)
        assert as_records(ix.refs) == as_records(H.select(sk, keep)) and ix.stats()["n_refs"] == len(keep)
        # (single linkage promises no singletons; the contract's loop over the survivors is the judge)
        edges = []
        again = H.cluster_host(ix.refs, d, edges=edges)
        st = {}
        assert ix.cluster(d, stats=st).tolist() == again.tolist() and st["edges"] == edges[0]
