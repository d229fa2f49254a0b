"""Hashes that land exactly on a threshold, on the CPU: the oracle's sketchers against a literal Python restatement of
mash.rs / scaled.rs (tests/ties_model.py) on crafted streams (tests/tie_inputs.py), and the two host merges
(fh_merge_partials, fh_merge_wire) against a model of the merge rule that include/finch_hip.h states.  No GPU.

With the hash_mask hook the hash space is as small and dense as a case wants, and a Scaled sketch's max_hash
(u64::MAX / ((1/scale) as u64)) can be put in the middle of it: max_hash itself is a hash of the input, so is max_hash + 1,
and the n-th smallest hash of a Mash sketch has its successor right behind it.  Every comparison is exact."""
import numpy as np
import pytest

import tie_inputs as T
from ties_model import MashModel, ScaledModel, merge_model, scaled_max_hash
from oracle import oracle as O

K = 21
MASK = T.low_mask(12)
# (1/scale) as u64 = 2^53 -> max_hash 2047 (inside the masked range); 3 * 2^51 (not a power of two) -> 2730; 2^52 -> 4095, the
# mask's top value; 2^50 -> 16383, above every masked hash; 1 -> u64::MAX
SCALES = {"pow2": 2.0 ** -53, "nonpow2": 1.0 / (3 * 2.0 ** 51), "top": 2.0 ** -52, "above": 2.0 ** -50, "one": 1.0}


def rows_of(model):
    v = model.to_vec()
    return (np.array([r[0] for r in v], dtype=np.uint64), np.array([r[2] for r in v], dtype=np.uint32),
            np.array([r[3] for r in v], dtype=np.uint32),
            np.frombuffer(b"".join(r[1] for r in v), dtype=np.uint8).reshape(len(v), -1) if v else None)


def hold_oracle_to_model(kind, size, st, scale=0.001, ctx=""):
    ora = O.OracleSketcher(kind, size, st.k, 0, scale)
    ora.set_hash_mask(st.mask)
    ora.process_packed(st.data, 0)
    model = (MashModel(size) if kind == O.MASH else ScaledModel(size, scale)).feed(st.triples())
    kc, km = ora.to_vec()
    h, c, e, kmers = rows_of(model)
    assert len(kc) == len(h), (ctx, len(kc), len(h))
    assert np.array_equal(kc["hash"], h), ctx
    assert np.array_equal(kc["count"], c), ctx
    assert np.array_equal(kc["extra_count"], e), ctx
    if len(h):
        assert np.array_equal(km, kmers), ctx
    assert ora.total_bases_and_kmers()[1] == model.total_kmers == len(st), ctx
    return kc


def test_ranks_and_values_of_the_masks():
    for mask in (T.low_mask(12), T.high_mask(10), T.MIXED_MASK):
        n = 1 << len(T.mask_bits(mask))
        vals = [T.value_of(r, mask) for r in (0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1)]
        assert vals == sorted(set(vals)) and vals[-1] == mask and all(v & mask == v for v in vals)
        assert T.rank_of(np.array(vals, dtype=np.uint64), mask).tolist() == [0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1]
        assert T.floor_rank(mask, mask) == n - 1 and T.floor_rank(T.U64, mask) == n - 1 and T.floor_rank(0, mask) == 0
        v = T.value_of(n // 2, mask)
        assert T.floor_rank(v, mask) == n // 2 and T.floor_rank(v - 1, mask) == n // 2 - 1
    rng = np.random.default_rng(0)
    h = rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64)
    for mask in (T.high_mask(10), T.MIXED_MASK):  # order preserving
        m = h & np.uint64(mask)
        o = np.argsort(m, kind="stable")
        assert (np.diff(T.rank_of(h, mask)[o]) >= 0).all()


def test_crafted_streams_hold_what_they_say():
    """the helper's statement of a stream (from the pool and numpy) against hashing its records one by one"""
    for mask, k in ((MASK, 21), (T.high_mask(10), 33), (T.MIXED_MASK, 21)):
        c = T.Crafter(k, mask, rng_seed=5)
        x = c.n_ranks // 2
        st = c.around(x, 20, 20).filler(100).build(record_len=None if k == 21 else 47)
        assert all(T.value_of(r, mask) in st.H for r in range(x - 20, x + 21))
        assert T.value_of(x, mask) in st.collided
        assert st.stride == (k + 1 if k == 21 else 48) and len(st.data) == len(st) * st.stride
        assert st.colliding_occurrences <= T.MAX_COLLIDING_OCCURRENCES and st.colliding_occurrences > 0
        recs = bytes(st.data).split(b"\0")[:-1]
        assert len(recs) == len(st)
        for rec, (h, km, rev) in list(zip(recs, st.triples()))[::7]:
            seq = rec.rstrip(b"N")
            rc = O.reverse_complement(seq)
            assert min(seq, rc) == km and (seq != km) == bool(rev)
            assert O.hash_f(km, 0) & mask == h


def test_the_collision_bound_is_asserted():
    c = T.Crafter(K, T.low_mask(3), rng_seed=2)  # 8 values: nearly every occurrence collides
    for r in range(8):
        c._want(r, 3)
    c.build()
    old = T.MAX_COLLIDING_OCCURRENCES
    T.MAX_COLLIDING_OCCURRENCES = 3
    try:
        with pytest.raises(AssertionError):
            c.build()
    finally:
        T.MAX_COLLIDING_OCCURRENCES = old


def scaled_case(variant, scale_name, order, k=K, mask=MASK, rng_seed=11, record_len=None):
    """-> (stream, max_hash, x_rank).  variant: 'both' max_hash and max_hash + 1 are hashes of the input; 'absent': max_hash is
    not, its neighbours are; 'no_successor': max_hash is, max_hash + 1 is not"""
    mh = scaled_max_hash(SCALES[scale_name])
    c = T.Crafter(k, mask, rng_seed=rng_seed)
    x = T.floor_rank(mh, mask)
    c.around(min(x, c.n_ranks - 1), 30, 30).filler(150)
    if variant == "absent":
        c.without([x])
    elif variant == "no_successor":
        c.without([x + 1])
    return c.build(order=order, record_len=record_len), mh, x


@pytest.mark.parametrize("scale_name", ["pow2", "nonpow2", "top", "above", "one"])
@pytest.mark.parametrize("variant", ["both", "absent", "no_successor"])
def test_scaled_oracle_at_max_hash(variant, scale_name):
    """scaled.rs:37-61 with max_hash in the input, absent from it, and with max_hash + 1 there; `size` below, equal to and
    above the number of distinct hashes at or below max_hash (above: hashes beyond max_hash are let in and popped again,
    which depends on the order, so three orders), size 0, scale 1"""
    iscale = int(1.0 / SCALES[scale_name])
    assert (iscale & (iscale - 1) != 0) == (scale_name == "nonpow2")
    for order in ("shuffle", "ascending", "descending"):
        st, mh, x = scaled_case(variant, scale_name, order)
        assert O.OracleSketcher(O.SCALED, 1, K, 0, SCALES[scale_name]).max_hash == mh
        H = st.H
        if scale_name in ("pow2", "nonpow2"):
            assert T.value_of(x, MASK) == mh and mh + 1 == T.value_of(x + 1, MASK)
            assert (mh in H) == (variant != "absent") and (mh + 1 in H) == (variant != "no_successor") and mh - 1 in H
            if variant != "absent":
                assert mh in st.collided
        elif scale_name == "top":
            assert mh == MASK and (mh in H) == (variant != "absent") and max(H) <= mh
        else:
            assert max(H) < mh
        n_le = sum(1 for h in H if h <= mh)
        assert 30 < n_le <= len(H)
        for size in (0, 1, n_le - 7, n_le - 1, n_le, n_le + 1, n_le + 9, len(H), len(H) + 5):
            kc = hold_oracle_to_model(O.SCALED, size, st, SCALES[scale_name], (variant, scale_name, order, size))
            assert len(kc) == max(n_le, min(len(H), size))  # scaled.rs:41-58, net effect


@pytest.mark.parametrize("mask", [MASK, T.high_mask(11), T.MIXED_MASK])
def test_mash_oracle_at_the_nth_hash(mask):
    """mash.rs:34-63 where the n-th smallest hash has its successor in the input: n equal to, one below and one above the
    number of distinct hashes, and cuts inside a run of consecutive values"""
    c = T.Crafter(K, mask, rng_seed=13)
    st = c.dense(range(0, 120)).around(700, 25, 25).filler(60, 800).build()
    d = st.sorted_distinct()
    assert [T.value_of(r, mask) for r in range(120)] == d[:120]
    for n in (0, 1, 2, 64, 119, 120, 121, len(d) - 1, len(d), len(d) + 1):
        if 0 < n < 120:
            t = d[n - 1]
            assert T.value_of(T.floor_rank(t, mask) + 1, mask) in st.H  # the successor of the n-th smallest is a hash too
        kc = hold_oracle_to_model(O.MASH, n, st, ctx=(hex(mask), n))
        assert kc["hash"].tolist() == d[:n]
        assert any(h in st.collided for h in kc["hash"].tolist()) or n < 3


# ---- the host merges ----

def random_part(rng, hashes, k, pos_base, big_counts=False):
    n = len(hashes)
    kc = np.zeros(n, dtype=O.KC_DTYPE)
    kc["hash"] = np.array(sorted(hashes), dtype=np.uint64)
    choices = np.array([1, 2, 7, 2**31, 2**32 - 1] if big_counts else [1, 2, 3, 9], dtype=np.uint64)
    kc["count"] = rng.choice(choices, size=n).astype(np.uint32)
    kc["extra_count"] = (kc["count"] // rng.integers(1, 4, n)).astype(np.uint32)
    km = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(n, k))
    pos = (rng.permutation(1_000_000)[:n] * 2 + pos_base).astype(np.uint64)  # (distinct across the parts: bases 0 / 1)
    return kc, km, pos, int(rng.integers(0, 2**40))


def as_rows(part):
    kc, km, pos, _ = part
    return [(int(kc["hash"][i]), int(kc["count"][i]), int(kc["extra_count"][i]), bytes(km[i]), int(pos[i])) for i in range(len(kc))]


def hold_merges_to_model(kind, size, scale, parts, k, ctx):
    from finch_rs_amd import sharding as SH
    from finch_rs_amd.sketch_schemes import SketchParams
    params = SketchParams.mash(size, size, True, k, 0) if kind == "mash" else SketchParams.scaled(size, k, scale, 0)
    want = merge_model(kind, size, scaled_max_hash(scale) if kind == "scaled" else 0, [as_rows(p) for p in parts])
    pad = max(len(p[0]) for p in parts) + 3
    got = {"fh_merge_partials": SH.merge_partials(params, parts),
           "fh_merge_wire": SH.merge_wire(params, [SH.pack_partial(p[0], p[1], p[2], p[3], pad, k) for p in parts], pad)}
    for name, (kc, km, pos, tk) in got.items():
        c = (name,) + tuple(ctx)
        assert len(kc) == len(want), (c, len(kc), len(want))
        assert np.array_equal(kc["hash"], np.array([r[0] for r in want], dtype=np.uint64)), c
        assert np.array_equal(kc["count"], np.array([r[1] for r in want], dtype=np.uint32)), c
        assert np.array_equal(kc["extra_count"], np.array([r[2] for r in want], dtype=np.uint32)), c
        assert [bytes(r) for r in km] == [r[3] for r in want], c
        assert np.array_equal(np.asarray(pos, dtype=np.uint64), np.array([r[4] for r in want], dtype=np.uint64)), c
        assert tk == sum(p[3] for p in parts), c
    return want


@pytest.mark.parametrize("k", [21, 40])
@pytest.mark.parametrize("where", ["A", "B", "both", "neither"])
def test_scaled_merges_at_max_hash(where, k):
    """consecutive hashes around max_hash = 2047, max_hash itself in A only, in B only, in both, in neither while its two
    neighbours are there; `size` on either side of the number at or below max_hash and of the union's count"""
    import __graft_entry__ as G
    G.build()
    scale = SCALES["pow2"]
    mh = scaled_max_hash(scale)
    assert mh == 2047
    rng = np.random.default_rng(31 + k)
    run = list(range(mh - 12, mh + 13))
    for trial in range(4):
        a = set(rng.choice([h for h in run if h != mh], size=14, replace=False).tolist()) | {mh - 1}
        b = set(rng.choice([h for h in run if h != mh], size=14, replace=False).tolist()) | {mh + 1}
        a |= {mh} if where in ("A", "both") else set()
        b |= {mh} if where in ("B", "both") else set()
        a |= {5, 90, 70000}
        b |= {5, 91, 70001, 2**63}
        union = sorted(a | b)
        assert (mh in union) == (where != "neither") and mh - 1 in union and mh + 1 in union
        n_le = sum(1 for h in union if h <= mh)
        parts = [random_part(rng, a, k, 0, big_counts=trial % 2 == 1), random_part(rng, b, k, 1, big_counts=trial % 2 == 1)]
        for size in (0, 1, n_le - 1, n_le, n_le + 1, len(union) - 1, len(union), len(union) + 1):
            want = hold_merges_to_model("scaled", size, scale, parts, k, (where, trial, size))
            assert len(want) == max(n_le, min(len(union), size))
            # the rule of the model is the net effect of scaled.rs' push: the same set, whatever the order of the union
            for order in (union, union[::-1], rng.permutation(union).tolist()):
                m = ScaledModel(size, scale).feed((h, b"", 0) for h in order)
                assert [r[0] for r in m.to_vec()] == [r[0] for r in want]
        # three parts: A, B and A again (every count of A doubled, clamped)
        hold_merges_to_model("scaled", n_le, scale, parts + [parts[0]], k, (where, trial, "three"))


@pytest.mark.parametrize("k", [21, 64])
def test_mash_merges_where_the_cut_falls_between_neighbours(k):
    """the size-th hash of the union in A only, in B only, in both, with its successor always there"""
    import __graft_entry__ as G
    G.build()
    rng = np.random.default_rng(41 + k)
    for trial in range(6):
        base = int(rng.choice([0, 1000, 2**32 - 20, 2**63 - 20]))
        run = [base + i for i in range(40)]
        a = set(run[i] for i in rng.choice(40, size=25, replace=False))
        b = set(run[i] for i in rng.choice(40, size=25, replace=False)) | (set(run) - a)  # the union is the whole run
        union = sorted(a | b)
        assert union == run
        parts = [random_part(rng, a, k, 0, big_counts=trial % 2 == 1), random_part(rng, b, k, 1, big_counts=trial % 2 == 1)]
        seen = set()
        for size in range(0, 43):
            want = hold_merges_to_model("mash", size, 0.0, parts, k, (trial, size))
            assert [r[0] for r in want] == union[:size]
            if 0 < size < 40:
                t = union[size - 1]
                seen.add(("A" if t in a else "") + ("B" if t in b else ""))
        assert seen == {"A", "B", "AB"}
