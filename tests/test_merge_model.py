"""tests/merge_model.py against itself: the fold as the reference writes it against the closed form where there is no scale,
the order dependence where there is one (pinned as a literal), the dropped records that never come back, the wrapping sums."""
import itertools

import numpy as np
import pytest

import merge_model as MM

BIG = 2 ** 32 - 1


def rec(h, c=1, e=0, k=b""):
    return (h, c, e, k)


def random_group(rng, universe=40):
    members = []
    for m in range(int(rng.integers(1, 6))):
        n = int(rng.integers(0, 12))
        hs = sorted(rng.choice(universe, size=n, replace=False).tolist())
        members.append([(h, int(rng.choice([1, 2, 7, BIG])), int(rng.integers(0, 2)), bytes([65 + m])) for h in hs])
    return members


def test_divisor_and_max_hash():
    assert MM.scale_divisor(0.001) == 1000 and MM.max_hash(0.001) == (2 ** 64 - 1) // 1000
    assert MM.scale_divisor(1.0) == 1 and MM.max_hash(1.0) == 2 ** 64 - 1
    assert MM.scale_divisor(0.3) == 3
    assert MM.scale_divisor(0.0) == 2 ** 64 - 1 and MM.max_hash(0.0) == 1  # 1 / 0. is inf: the cast saturates
    assert MM.scale_divisor(1e-30) == 2 ** 64 - 1
    for bad in (1.5, 2.0, -0.5, -0.0, float("nan"), float("inf")):
        assert MM.scale_divisor(bad) == 0 and MM.max_hash(bad) is None
    with pytest.raises(ZeroDivisionError):
        MM.merge_pair([rec(1)], [rec(1)], None, 2.0)


def test_walk_stops_when_either_list_is_exhausted():
    a = [rec(1), rec(5), rec(9)]
    b = [rec(2), rec(5, 3, 1), rec(6), rec(20), rec(30)]
    assert MM.merge_pair(a, b) == [rec(1), rec(2), rec(5, 4, 1), rec(6), rec(9)]  # 20 and 30 are dropped
    assert MM.merge_pair(b, a) == [rec(1), rec(2), rec(5, 4, 1), rec(6), rec(9)]
    assert MM.merge_pair(a, []) == [] and MM.merge_pair([], a) == []
    assert MM.merge_pair([rec(100)], [rec(1), rec(2)]) == [rec(1), rec(2)]  # one list entirely above the other: the lower alone


def test_wrapping_adds():
    a, b = [rec(7, BIG, BIG - 1, b"A")], [rec(7, 2, 3, b"B")]
    assert MM.merge_pair(a, b) == [(7, 1, 1, b"A")]
    assert MM.merge_pair(b, a) == [(7, 1, 1, b"B")]
    assert MM.fold([a, a]) == [(7, BIG - 1, BIG - 3, b"A")]  # a.merge(a) doubles, mod 2^32
    assert MM.sums([2 ** 64 - 1, 5]) == 4


def test_clip_modes():
    a = [rec(h) for h in (10, 20, 30, 40)]
    b = [rec(h) for h in (15, 20, 35, 40)]
    full = [rec(10), rec(15), rec(20, 2), rec(30), rec(35), rec(40, 2)]
    assert MM.merge_pair(a, b) == full
    assert MM.merge_pair(a, b, 3) == full[:3] and MM.merge_pair(a, b, 0) == [] and MM.merge_pair(a, b, 99) == full
    scale = 1.0 / (2 ** 64 // 32)  # max_hash lands a little above 30
    mh = MM.max_hash(scale)
    assert 30 <= mh < 35
    assert MM.merge_pair(a, b, None, scale) == full[:4]
    assert MM.merge_pair(a, b, 2, scale) == full[:4]  # the size is below the scaled length: hash <= max_hash keeps more
    assert MM.merge_pair(a, b, 5, scale) == full[:5]  # ix < size keeps a record above max_hash
    assert MM.merge_pair(a, b, 0, scale) == full[:4]


def test_fold_equals_the_closed_form_without_a_scale():
    rng = np.random.default_rng(11)
    nonempty = 0
    for _ in range(3000):
        members = random_group(rng)
        size = None if rng.integers(0, 2) else int(rng.integers(0, 15))
        got = MM.fold(members, size)
        assert got == MM.closed_form(members, size), (members, size)
        if len(members) >= 2 and any(len(m) == 0 for m in members):
            assert got == []
        nonempty += bool(got)
    assert nonempty > 1000


def test_order_matters_without_a_scale_only_for_the_tie_kmer():
    rng = np.random.default_rng(12)
    differed = 0
    for _ in range(300):
        members = random_group(rng, 20)
        if len(members) < 2 or len(members) > 4:
            continue
        size = None if rng.integers(0, 2) else int(rng.integers(0, 15))
        base = MM.fold(members, size)
        for perm in itertools.permutations(range(len(members))):
            other = MM.fold([members[p] for p in perm], size)
            assert [r[:3] for r in other] == [r[:3] for r in base]
            first_holder = {}
            for p in perm:
                for r in members[p]:
                    first_holder.setdefault(r[0], r[3])
            assert all(r[3] == first_holder[r[0]] for r in other)
            differed += other != base
    assert differed > 0


def test_a_scaled_group_depends_on_the_order():
    """max_hash is a little above 50.  Where every member reaches past the accumulator's end the order does not show; it shows
    once a step's clip has shortened the accumulator below max_hash: what a later member holds above that end is dropped."""
    scale = 1.0 / (2 ** 64 // 52)
    assert 50 <= MM.max_hash(scale) < 60
    A = [rec(10, 1, 0, b"A"), rec(40, 1, 0, b"A"), rec(70, 1, 0, b"A")]
    B = [rec(20, 1, 0, b"B"), rec(60, 1, 0, b"B")]
    C = [rec(30, 1, 0, b"C"), rec(80, 1, 0, b"C")]
    ab = MM.merge_pair(A, B, None, scale)
    assert ab == [rec(10, 1, 0, b"A"), rec(20, 1, 0, b"B"), rec(40, 1, 0, b"A")]  # 60 is clipped: the accumulator now ends at 40
    abc = MM.fold([A, B, C], None, scale)
    acb = MM.fold([A, C, B], None, scale)
    assert abc == [rec(10, 1, 0, b"A"), rec(20, 1, 0, b"B"), rec(30, 1, 0, b"C"), rec(40, 1, 0, b"A")]
    assert acb == abc
    # a member that ends low first: everything later is cut at its last hash
    D = [rec(5, 1, 0, b"D"), rec(25, 1, 0, b"D")]
    E = [rec(15, 2, 1, b"E"), rec(45, 1, 0, b"E"), rec(90, 1, 0, b"E")]
    ade = MM.fold([A, D, E], None, scale)
    aed = MM.fold([A, E, D], None, scale)
    assert ade == aed == [rec(5, 1, 0, b"D"), rec(10, 1, 0, b"A"), rec(15, 2, 1, b"E"), rec(25, 1, 0, b"D")]
    # the order dependence: F's 45 is <= max_hash, but after (G, H) the accumulator ends at 40 (H's 55 was clipped), so 45 is dropped
    G = [rec(10, 1, 0, b"G"), rec(40, 1, 0, b"G"), rec(70, 1, 0, b"G")]
    H = [rec(20, 1, 0, b"H"), rec(55, 1, 0, b"H"), rec(75, 1, 0, b"H")]
    F = [rec(45, 1, 0, b"F"), rec(58, 1, 0, b"F"), rec(90, 1, 0, b"F")]
    ghf = MM.fold([G, H, F], None, scale)
    gfh = MM.fold([G, F, H], None, scale)
    assert ghf == [rec(10, 1, 0, b"G"), rec(20, 1, 0, b"H"), rec(40, 1, 0, b"G")]
    assert gfh == [rec(10, 1, 0, b"G"), rec(20, 1, 0, b"H"), rec(40, 1, 0, b"G"), rec(45, 1, 0, b"F")]
    assert ghf != gfh


def test_with_a_scale_random_groups_do_depend_on_the_order():
    rng = np.random.default_rng(13)
    scale = 1.0 / (2 ** 64 // 25)
    differ = 0
    for _ in range(2000):
        members = random_group(rng)
        if len(members) < 3:
            continue
        size = None if rng.integers(0, 2) else int(rng.integers(0, 15))
        differ += MM.fold(members, size, scale) != MM.fold(members[:1] + members[1:][::-1], size, scale)
    assert differ > 0


def test_a_dropped_record_never_comes_back():
    """after every step the accumulator's last hash only goes down (or the accumulator is empty for good), with and without scale"""
    rng = np.random.default_rng(14)
    for _ in range(2000):
        members = random_group(rng)
        size = None if rng.integers(0, 2) else int(rng.integers(1, 15))
        scale = None if rng.integers(0, 2) else 1.0 / (2 ** 64 // 25)
        acc = list(members[0])
        for m in members[1:]:
            nxt = MM.merge_pair(acc, m, size, scale)
            if not acc:
                assert nxt == []
            elif nxt:
                assert nxt[-1][0] <= acc[-1][0]
                assert all(r[0] <= acc[-1][0] for r in nxt)
            acc = nxt


def test_incompatibility_sentences():
    mash21 = ("mash", 21, 0)
    assert MM.incompatibility(mash21, ("scaled", 21, 0)) is None  # the variant is not compared
    assert MM.incompatibility(mash21, ("mash", 31, 0)) == "First sketch has k 21, but second sketch has k 31"
    assert MM.incompatibility(mash21, ("mash", 21, 42)) == "First sketch has hash seed 0, but second sketch has hash seed 42"
    assert MM.incompatibility(mash21, ("allcounts", 21, 0)) == \
        "First sketch has hash type MurmurHash3_x64_128, but second sketch has hash type None"
    assert MM.incompatibility(("allcounts", 4, 0), ("allcounts", 4, 9)) is None  # AllCounts reports seed 0 whatever it holds
