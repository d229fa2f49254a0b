"""tests/library_fuzz_inputs.py held to what tests/test_gpu_fuzz_library.py relies on, over the default list and one other seed:
every planted value is there, hashes ascend, every case has rows exactly on each threshold and a tie, every length edge and
every option value occurs, few draws are redrawn -- and THE HOST CONTRACTS agree with the models on the fuzz cases themselves, at
every state of every life, so that a disagreement on the GPU machine is the kernel's and not the judge's.

Host contracts checked against the models here (integers by value, doubles as bit patterns, two NaNs equal):
    H.distance             against dist_model.distance, in the case's mode: every pair that shares a hash and a sample of the rest
    H.compare_counts_pair  against moments_model.compare_counts: every pair that shares a hash
    H.gather_query         against gather_model.gather (== index_gather_model.gather): every query, both min_overlap values
    H.merge_pair           folded over every drawn group, against merge_model.fold, with the first member's name and the sums
    H.cluster_host         against index_cluster_model (labels and edges)
    H.screen_host          against screen_model.screen: rows at both min_shared values, and the figures
No GPU."""
import numpy as np
import pytest

import dist_model as M
import library_fuzz_inputs as L
import merge_cases as MC
from finch_rs_amd import host as H

OTHER_SEED = 97531
SEEDS = (L.SEED0, OTHER_SEED)
N = 12


def all_cases(seed0):
    return [L.case(seed0, i) for i in range(N)]


@pytest.mark.parametrize("seed0", SEEDS)
def test_hashes_ascend_and_every_planted_value_is_present(seed0):
    for c in all_cases(seed0):
        for specs in L.states(c) + [c.queries] + [arg for what, arg in c.life if what == "add"]:
            for x in specs:
                assert all(a < b for a, b in zip(x.hashes, x.hashes[1:])), (c.index, x.name)
                assert len(x.counts) == len(x.hashes) and all(0 <= n < 2 ** 32 for n in x.counts)
        st0 = L.states(c)[0]
        held = {}
        for r, x in enumerate(st0):
            for h in x.hashes:
                held.setdefault(h, []).append(r)
        for h in [0, L.U64_MAX] + c.low_run + c.high_run + c.planted_sample:
            assert h in held, (c.index, h)
        assert {h >> 32 for h in c.low_run} == {c.low_run[0] >> 32} and len({h & 0xffffffff for h in c.low_run}) == 6
        assert {h & 0xffffffff for h in c.high_run} == {c.high_run[0] & 0xffffffff} and len({h >> 32 for h in c.high_run}) == 6
        assert held[c.ALL] == [r for r, x in enumerate(st0) if x.hashes], c.index       # the posting run is as long as the library
        assert len(held[c.ONE]) == 1 and st0[held[c.ONE][0]].name == c.long_name
        assert L.LONG_RANGE[0] <= len(st0[held[c.ONE][0]].hashes) <= L.LONG_RANGE[1] + 40
        for specs in L.states(c):  # ... and stays so through the life
            assert all(c.ALL in x.hashes for x in specs if x.hashes)
            assert sum(c.ONE in x.hashes for x in specs) <= 1
        if len(c.planted_sample) and len(st0) >= 2:
            assert all(len(held[h]) >= 2 for h in c.planted_sample[:(len(c.planted_sample) + 1) // 2])  # two references hold them
        counts = [n for x in st0 for n in x.counts]
        assert max(counts) >= 2 ** 31 and (2 ** 32 - 1) in counts, c.index
        # the queries the issue names
        names = [q.name for q in c.queries]
        assert ("q_empty" in names) == (not c.old_mode) and {"q_equal", "q_stranger", "q_of_long"} <= set(names)
        q = {x.name: x for x in c.queries}
        assert q["q_equal"].hashes == st0[c.dup_of].hashes and not set(q["q_stranger"].hashes) & set(held)
        assert set(q["q_of_long"].hashes) <= set(st0[held[c.ONE][0]].hashes)
        assert 1 <= len(c.queries) <= 12 and 3 <= len(c.life) <= 6 and 1 <= len(st0) <= 202
        assert len(c.sample) == 0 or sum(len(r) for r in L.SM.records(c.sample)) <= L.MAX_SAMPLE_POSITIONS


@pytest.mark.parametrize("seed0", SEEDS)
def test_the_life(seed0):
    for c in all_cases(seed0):
        now, emptied = list(c.refs0), 0
        for at, (what, arg) in enumerate(c.life):
            if what == "add":
                assert 1 <= len(arg) <= 40
                if not c.old_mode:
                    assert any(not x.hashes for x in arg)
                if any(x.hashes and c.ONE not in x.hashes for x in now) and len(arg) >= 2:
                    assert any(x.hashes and any(x.hashes == y.hashes for y in now) for x in arg), (c.index, at)  # a duplicate
                if len(arg) >= 3 and any(x.hashes for x in now):  # hashes below, between and above the old postings
                    old = sorted({h for x in now for h in x.hashes})
                    new = {h for x in arg for h in x.hashes} - set(old)
                    assert any(old[0] < h < old[-1] for h in new), (c.index, at)
                    assert old[0] == 0 or any(h < old[0] for h in new), (c.index, at)
                    assert old[-1] == L.U64_MAX or any(h > old[-1] for h in new), (c.index, at)
                now = now + arg
            else:
                assert all(a < b for a, b in zip(arg, arg[1:])) and all(0 <= j < len(now) for j in arg)
                now = [now[j] for j in arg]
                if not any(x.hashes for x in now) and at + 1 < len(c.life) and c.life[at + 1][0] == "add":
                    emptied += 1  # an empty library, or every hash dropped, and an add follows
        assert emptied >= 1 or c.index % 3 != 1, c.index


def test_every_length_edge_occurs_in_the_default_list():
    lengths = {len(x.hashes) for c in all_cases(L.SEED0) for specs in L.states(c) for x in specs}
    assert set(L.LENGTH_EDGES) <= lengths
    assert any(100 <= n <= 300 for n in lengths) and any(n >= L.LONG_RANGE[0] for n in lengths)
    sizes = {len(c.refs0) - (len(c.refs0) >= 3) for c in all_cases(L.SEED0)}  # (the duplicate is one more)
    assert len(sizes & set(L.LIBRARY_SIZES)) >= 3, sizes


@pytest.mark.parametrize("seed0", SEEDS)
def test_every_setting_occurs_within_24_consecutive_cases(seed0):
    for start in range(0, 60, 5):
        for salt, (name, values) in enumerate(L.OPTIONS.items()):
            assert {L._walk(values, seed0, i, salt) for i in range(start, start + 24)} == set(values), (name, start)
        assert {L._walk(L.DEVICES, seed0, i, 101) for i in range(start, start + 24)} == set(L.DEVICES)
        assert {L._walk((False, True), seed0, i, 102) for i in range(start, start + 24)} == {False, True}
        assert {L._walk(L.TOP_N, seed0, i, 103) for i in range(start, start + 24)} == set(L.TOP_N)
    for c in all_cases(seed0):  # the cases carry what the walk says
        assert c.opts == {name: L._walk(values, seed0, c.index, salt) for salt, (name, values) in enumerate(L.OPTIONS.items())}
        assert c.devices == L._walk(L.DEVICES, seed0, c.index, 101)


def test_few_draws_are_redrawn():
    cases = all_cases(L.SEED0) + all_cases(OTHER_SEED)
    assert sum(c.redraws for c in cases) * 10 <= len(cases), [c.redraws for c in cases]


@pytest.mark.parametrize("seed0", SEEDS)
def test_thresholds_sit_on_realised_values_and_every_case_has_a_tie(seed0):
    for c in all_cases(seed0):
        on = dict(search=0, dist=0, gather=0, counts=0, screen=0)
        ties = 0
        for s in range(len(c.life) + 1):
            e = L.expect(c, s)
            on["search"] += e.search[e.min_containments[0]].on_threshold
            on["dist"] += e.dist.on_threshold
            on["gather"] += e.gather[e.min_overlaps[0]].on_threshold
            on["counts"] += sum(1 for t in e.moments.values() if t[0] == e.min_commons[0])
            on["screen"] += e.screen_on_threshold
            ties += min(e.containment_ties, e.gather_ties)
            assert e.min_overlaps[1] == e.min_overlaps[0] + 1 and e.min_commons == e.min_overlaps
            assert e.min_shareds[1] == e.min_shareds[0] + 1
            assert 0 < e.min_containments[0] <= 1 and 0 < e.min_containments[1] <= 1 and 0 <= e.max_distance < 1
        for what, n in on.items():
            if what == "screen" and (c.empty_sample or not c.planted_sample):
                continue
            assert n >= 1, (c.index, what, on)
        assert ties >= 1 or len(c.refs0) == 1, c.index  # (a library of one sketch has no duplicate)


# --- the host contracts against the models, on the fuzz cases, at every state ---------------------------------------------

def dist_row(d, q, r):
    return dict(d, query=q, reference=r)


@pytest.mark.parametrize("i", range(N))
@pytest.mark.parametrize("seed0", SEEDS)
def test_host_contracts_equal_the_models(seed0, i):
    c = L.case(seed0, i)
    qs = L.build(c, c.queries)
    dqs = [L.dsk(c, x) for x in c.queries]
    rng = np.random.default_rng([seed0, i, 99])
    for s, specs in enumerate(L.states(c)):
        e = L.expect(c, s)
        ctx = (L.describe(c), "state %d" % s)
        refs = L.build(c, specs)
        drefs = [L.dsk(c, x) for x in specs]
        assert len(refs) == len(specs) == e.n_refs
        # H.distance
        pairs = set(e.moments)
        if specs:
            pairs |= {(int(rng.integers(0, len(dqs))), int(rng.integers(0, len(specs)))) for _ in range(40)}
        for q, r in sorted(pairs):
            want = M.distance(dqs[q], drefs[r], c.old_mode)
            assert L.same_dist_row(dist_row(H.distance(qs, q, refs, r, c.old_mode), q, r), q, r, want), (ctx, q, r)
        # H.compare_counts_pair
        for (q, r), t in e.moments.items():
            assert L.MOM.same(H.compare_counts_pair(refs, r, qs, q), t), (ctx, q, r)
        # H.gather_query
        for mo in e.min_overlaps:
            host = [H.gather_query(refs, qs, q, mo, 0) for q in range(len(c.queries))]
            offsets = np.cumsum([0] + [len(h) for h in host])
            L.check_gather(offsets, np.concatenate(host), e.gather[mo].rows, (ctx, "gather", mo))
        # H.merge_pair, folded
        for members, want in zip(e.merge_groups, e.merge):
            acc = H.select(refs, [members[0]])
            for m in members[1:]:
                acc = H.merge_pair(acc, 0, refs, m, e.merge_size)
            L.check_merged(MC.read(acc, 0), want, (ctx, "merge", members, e.merge_size))
        # H.cluster_host
        edges = []
        labels = H.cluster_host(refs, e.max_distance, c.old_mode, edges)
        assert labels.tolist() == e.cluster.labels and edges == [e.cluster.edges], (ctx, "cluster")
        # H.screen_host
        for ms in e.min_shareds:
            st = {}
            rows = H.screen_host(refs, c.sample, c.k, c.hash_seed, ms, stats=st)
            L.check_screen(rows, st, e.screen[ms], e.screen_figures, (ctx, "screen", ms))
