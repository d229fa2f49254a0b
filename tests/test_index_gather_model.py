"""tests/index_gather_model.py -- the gather over live counters, as finch_index_gather's device works -- against
tests/gather_model.py, the contract: the same rows, and the invariant that makes the form exact, checked after every round on
every touched reference."""
from functools import lru_cache

import pytest

import gather_cases as GC
import gather_model as GM
import index_gather_cases as IC
import index_gather_model as IM

SETTINGS = [(mo, mr) for mo in IC.MIN_OVERLAPS for mr in IC.MAX_ROUNDS]

CASES = {
    "hand": IC.hand_case,
    "random_70": lambda: IC.random_case(70),
    "random_130": lambda: IC.random_case(130),
    "common_hash_300": lambda: IC.common_hash_case(300),
    "common_hash_1100": lambda: IC.common_hash_case(1100),
    "equal": IC.equal_case,
    "winner_lengths": IC.winner_length_case,
    "used_up": IC.used_up_case,
    "query_lengths": IC.length_case,
    "longest": IC.longest_case,
    "long_last": lambda: IC.long_without_candidates_case("long_last"),
    "long_first": lambda: IC.long_without_candidates_case("long_first"),
    "long_between": lambda: IC.long_without_candidates_case("long_between"),
}


@lru_cache(None)
def counted(name):
    """the case, its index and the count of every query: made once, copied by every setting"""
    case = CASES[name]()
    ix = IM.Index(case.mr)
    counts = [IM.count(ix, q) for q in case.mq]
    # per query, per touched reference: the query positions of the hashes the two share (a merge walk, not the index)
    where = [{r: GM.positions(q, case.mr[r]) for r in c[1]} for q, c in zip(case.mq, counts)]
    return case, ix, counts, where


def check(name, min_overlap, max_rounds):
    case, ix, counts, where = counted(name)
    want = case.want(min_overlap, max_rounds)
    sets = [set(r.hashes) for r in case.mr]
    rows = 0
    for iq, q in enumerate(case.mq):
        audit = {}
        got = IM.gather_index(ix, q, min_overlap, max_rounds, iq, counted=counts[iq], audit=audit)
        assert len(got) == len(want[iq]), (name, iq)
        for a, b in zip(got, want[iq]):
            assert all(a[f] == b[f] for f in GM.INTS), (name, iq, a, b)
            assert all(GC.bits(a[f]) == GC.bits(b[f]) or (a[f] != a[f] and b[f] != b[f]) for f in GM.DOUBLES), (name, iq, a, b)
        cnt0, touched, n_post = counts[iq]
        common = [len(s.intersection(q.hashes)) if len(s) < len(q.hashes) else len(s & set(q.hashes)) for s in sets]
        assert n_post == sum(common)  # the count is the plain count
        assert all(cnt0[r] == common[r] for r in touched) and len(touched) == sum(1 for c in common if c)
        assert audit["candidates"] == sum(1 for r in touched if cnt0[r] >= max(1, min_overlap))
        assert len(audit["after"]) == len(got)
        for cnt, left in audit["after"]:  # after every round, on EVERY touched reference, candidate or not
            for r in touched:
                assert cnt[r] == sum(left[p] for p in where[iq][r]) and cnt[r] >= 0, (name, iq, r)
        for row, (cnt, _) in zip(got, audit["after"]):
            assert cnt[row["reference"]] == 0  # the winner's counter
        assert all(v == 0 for v in audit["final"].values()) and set(audit["final"]) == set(touched)  # the tail
        assert audit["decrements"] <= audit["postings"]
        rows += len(got)
    return rows


@pytest.mark.parametrize("min_overlap, max_rounds", SETTINGS)
@pytest.mark.parametrize("name", [n for n in CASES if n != "longest" and not n.startswith("long_")])
def test_the_rows_and_the_invariant(name, min_overlap, max_rounds):
    rows = check(name, min_overlap, max_rounds)
    if min_overlap == 10 ** 6:
        assert rows == 0
    elif min_overlap == 1:
        assert rows > 0


@pytest.mark.parametrize("min_overlap, max_rounds", SETTINGS)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_cases(seed, min_overlap, max_rounds):
    name = "seed_%d" % seed
    CASES.setdefault(name, lambda: GC.random_case(seed, 6, 40))
    check(name, min_overlap, max_rounds)


@pytest.mark.parametrize("name", ["longest", "long_last", "long_first", "long_between"])
def test_the_long_queries(name):
    """a million bisections each: every setting, one test per case"""
    for min_overlap, max_rounds in SETTINGS:
        check(name, min_overlap, max_rounds)
    if name != "longest":  # with min_overlap 10 the long query is touched, never a candidate, and cleaned
        case, ix, counts, _ = counted(name)
        audit = {}
        assert IM.gather_index(ix, case.mq[case.long_at], 10, 0, case.long_at, counted=counts[case.long_at], audit=audit) == []
        assert audit["candidates"] == 0 and len(audit["final"]) == 3 and audit["decrements"] == 0


def test_a_hash_every_reference_holds_lowers_every_counter():
    case, ix, counts, _ = counted("common_hash_1100")
    audit = {}
    rows = IM.gather_index(ix, case.mq[0], 1, 0, 0, counted=counts[0], audit=audit)
    assert len(counts[0][1]) == 1100 and len(rows) > 100
    first = audit["after"][0][0]
    assert all(first[r] == counts[0][0][r] - 1 for r in counts[0][1] if r != rows[0]["reference"])
    assert audit["decrements"] == audit["postings"]  # with no threshold and no cap every counted posting is removed


def test_ties_go_to_the_lower_reference():
    case, ix, counts, _ = counted("equal")
    rows = IM.gather(case.mq, case.mr)
    assert [r["reference"] for r in rows[0]] == [2] and [r["reference"] for r in rows[1]] == [0]
