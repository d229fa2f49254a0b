"""The generator of the door fuzz (tests/door_fuzz_inputs.py) held to what tests/test_gpu_fuzz_doors.py relies on, over the default
case list and with the oracle alone: the list is the same on every run, a record door's block holds no breaker, the Python
restatement of bplan::tau / expected_below / taken agrees with the host build of finch_rs_amd/csrc/fh_batch_plan.h (the program
tests/test_batch_plan_host.py builds) on every (n, length) pair of the list -- that agreement is checked here and not assumed on
the GPU -- and a wrong door cannot pass unnoticed: per door at least 60 % of the non-empty blocks must be taken, at most 25 % may
go either way, and at least one must not be taken where the door has that class.

Every k of a door's range occurs in a list of 64 cases (a door's k walks a permutation of its range, so 32 cases suffice); in the
default list of 12 only the counts door's seven do.  The shares and the draws are properties of the default seed's list: a soak
with another FH_DOOR_FUZZ_SEED is a matter of the GPU test alone.  No GPU."""
import functools
import itertools
import subprocess

import numpy as np
import pytest

import door_fuzz_inputs as D
from test_batch_plan_host import INC, LARGE, SMALL, SRC, WIDE

FORM = {"batch_mash": SMALL, "wide": WIDE, "large": LARGE}


@functools.lru_cache(maxsize=None)
def classes(door):
    """(case, block index, class) of every block of the default list"""
    return [(c.index, j, D.predict(door, c, b)) for c in D.cases(door) for j, b in enumerate(c.blocks)]


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("door_fuzz_plan") / "batch_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-I", INC, "-o", exe, SRC])

    def run(questions):
        text = "".join(" ".join(str(w) for w in q) + "\n" for q in questions)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(questions)
        return [line.split() for line in lines]
    return run


def same_case(a, b):
    da, db = dict(vars(a)), dict(vars(b))
    ba, bb = da.pop("blocks"), db.pop("blocks")
    return da == db and len(ba) == len(bb) and all(x.dtype == np.uint8 and np.array_equal(x, y) for x, y in zip(ba, bb))


@pytest.mark.parametrize("door", D.DOORS)
def test_case_list_is_deterministic_and_within_its_bounds(door):
    assert D.N_CASES >= 12 or "FH_DOOR_FUZZ_CASES" in D.os.environ
    first = D.cases(door)
    assert all(same_case(a, b) for a, b in zip(first, D.cases(door)))
    assert not same_case(D.case(door, D.SEED0, 0), D.case(door, D.SEED0 + 1, 0))
    lo, hi = D.K_RANGE[door]
    for c in first:
        assert lo <= c.k <= hi and 3 <= len(c.blocks) <= D.MAX_BLOCKS and c.slot in (0, 1)
        cap = D.MAX_POSITIONS_LARGE if door == "large" else D.MAX_POSITIONS
        if c.kind == D.KIND_SCALED and c.scale == 1.0:
            cap = D.SCALE_ONE_POSITIONS
        assert max(len(b) for b in c.blocks) <= cap
        assert c.stage_bytes >= 4096 and all(len(b) + 64 <= c.stage_bytes for b in c.blocks)
        if door in ("records", "records_stream"):
            # one record a block: the breaker occurs in none of them
            assert not any((b == 0).any() for b in c.blocks)
            assert c.max_records in D.MAX_RECORDS and c.max_files is None
        else:
            assert c.max_files in D.MAX_FILES and c.max_records is None
        if c.kind == D.KIND_MASH:
            assert c.size in D.MASH_SIZES[door] and c.seed in D.SEEDS
        elif c.kind == D.KIND_SCALED:
            assert c.size in D.SCALED_SIZES and c.scale in D.SCALES and c.seed in D.SEEDS
        else:
            assert door == "counts"


@pytest.mark.parametrize("door", D.DOORS)
def test_the_draws_reach_what_the_door_has(door):
    """over a list of 64: every k of the range (the default 12 hold every k of the counts door only), every size, seed, scale,
    group size, both slots, both input forms, staging buffers that need several submits, and every kind of block"""
    many = [D.case(door, D.SEED0, i) for i in range(64)]
    lo, hi = D.K_RANGE[door]
    assert {c.k for c in many} == set(range(lo, hi + 1))
    assert {c.k for c in many[:32]} == set(range(lo, hi + 1))
    if door == "counts":
        assert {c.k for c in D.cases(door)} == set(range(1, 8)) or D.N_CASES < 7
    else:
        assert {c.seed for c in many} == set(D.SEEDS)
    assert {c.slot for c in many} == {0, 1}
    if door in D.MASH_SIZES:
        assert {c.size for c in many if c.kind == D.KIND_MASH} == set(D.MASH_SIZES[door])
    if door in ("batch_scaled", "wide", "records", "records_stream"):
        sc = [c for c in many if c.kind == D.KIND_SCALED]
        assert {c.size for c in sc} == set(D.SCALED_SIZES) and {c.scale for c in sc} == set(D.SCALES)
    if door in ("records", "records_stream"):
        assert {c.max_records for c in many} == set(D.MAX_RECORDS)
        assert sum(len(b) > D.LDS_POSITIONS for c in many for b in c.blocks) >= 0.08 * sum(len(c.blocks) for c in many)
    else:
        assert {c.max_files for c in many} == set(D.MAX_FILES) and {c.two_bit for c in many} == {False, True}
        assert any((b[:-1] == 0).sum() >= 5 for c in many for b in c.blocks if len(b))  # many short records in one file
    assert any(sum(len(b) for b in c.blocks) > c.stage_bytes for c in D.cases(door))    # several submits, in the default list
    lens = [len(b) for c in many for b in c.blocks]
    assert 0 in lens and {2047, 2048, 2049, 8191, 8192, 8193} <= set(lens) and min(x for x in lens if x) <= 20
    if door in FORM:
        for c in many:  # the threshold's edge, at the length the handle works it out from
            e = D.wanted_below(door, c.size)
            assert all(D.tau(e, len(b)) == D.EMPTY for b in c.blocks if len(b) <= e)
        assert any(len(b) - D.wanted_below(door, c.size) == d for c in many for b in c.blocks for d in (-1, 0, 1))
        hits = {len(b) - D.wanted_below(door, c.size) for c in many for b in c.blocks}
        assert {-1, 0, 1} <= hits


def test_tau_and_expected_below_are_the_headers(ask):
    """every (door, n, length) of the default list, and the lengths around every threshold edge"""
    pairs = set()
    for door, form in FORM.items():
        for c in D.cases(door):
            if c.kind != D.KIND_MASH:
                continue
            e = D.wanted_below(door, c.size)
            pairs |= {(door, form, c.size, len(b)) for b in c.blocks}
            pairs |= {(door, form, c.size, x) for x in (0, 1, e - 1, e, e + 1, 2 * e, (1 << 32) + 1)}
    for door in ("batch_mash", "large"):
        for n in D.MASH_SIZES[door]:
            pairs.add((door, FORM[door], n, D.wanted_below(door, n) + 1))
    pairs = sorted(pairs)
    assert len(pairs) > 100
    got = ask([("tau", form, D.KIND_MASH, n, 12345, length, D.LARGE_WANT if door == "large" else 0) for door, form, n, length in pairs])
    assert [int(a[0]) for a in got] == [D.tau(D.wanted_below(door, n), length) for door, _, n, length in pairs]
    assert D.expected_below(2000) == 8000 and D.expected_below(2001) == 6003 and D.wanted_below("large", 3001) == 12004
    # Scaled: max_hash whatever the file
    for door in ("batch_scaled", "wide"):
        sc = [c for c in D.cases(door) if c.kind == D.KIND_SCALED]
        qs = [("tau", FORM.get(door, SMALL), D.KIND_SCALED, c.size, D.max_hash_of(c), len(b), 0) for c in sc for b in c.blocks]
        assert [int(a[0]) for a in ask(qs)] == [q[4] for q in qs]


def test_taken_is_the_headers(ask):
    fields = ("sorted_", "overflow", "need_big", "n_coll", "n_live", "sp_count", "inserted_total")
    real_tau = (4000 << 64) // 5_000_000
    grid = []
    for kind, size, t in itertools.product((D.KIND_MASH, D.KIND_SCALED), (0, 1, 1000), (real_tau, D.EMPTY)):
        base = dict(sorted_=2, overflow=0, need_big=0, n_coll=0, n_live=size, sp_count=0, inserted_total=size)
        changes = [{}, dict(sorted_=1), dict(overflow=1), dict(need_big=1), dict(n_coll=1), dict(sp_count=1), dict(n_live=size + 1),
                   dict(n_live=max(size, 1) - 1, inserted_total=max(size, 1) - 1), dict(n_live=12288), dict(n_live=12289),
                   dict(inserted_total=0), dict(inserted_total=size + 5)]
        grid += [(kind, size, t, dict(base, **ch)) for ch in changes]
    got = ask([("taken", kind, size) + tuple(o[f] for f in fields) + (t,) for kind, size, t, o in grid])
    want = [D.taken(kind, size, t, **o) for kind, size, t, o in grid]
    assert [int(a[0]) for a in got] == [int(w) for w in want]
    assert 0 < sum(want) < len(want)


@pytest.mark.parametrize("door", D.DOORS)
def test_a_wrong_door_cannot_pass_unnoticed(door):
    got = [(cl, len(D.case(door, D.SEED0, i).blocks[j])) for i, j, cl in classes(door)]
    assert {cl for cl, _ in got} <= set(D.CLASSES[door])
    live = [cl for cl, n in got if n > 0]
    share = {cl: live.count(cl) / len(live) for cl in (D.MUST_TAKE, D.MUST_NOT, D.EITHER)}
    assert share[D.MUST_TAKE] >= 0.60, share
    assert share[D.EITHER] <= 0.25, share
    if D.MUST_NOT in D.CLASSES[door]:
        assert live.count(D.MUST_NOT) >= 1, share
    # an empty block has no window: every door takes it, but a Scaled batch door asked for `size` > 0 hashes at or below max_hash
    for (i, j, cl), (_, n) in zip(classes(door), got):
        c = D.case(door, D.SEED0, i)
        if n == 0 and c.kind == D.KIND_SCALED and c.size > 0 and door in ("batch_scaled", "wide"):
            assert cl == D.MUST_NOT
        elif n == 0:
            assert cl == D.MUST_TAKE


def test_predictions_on_known_blocks():
    """the rule on blocks whose answer is plain"""
    rng = np.random.default_rng(1)
    genome = rng.choice(D.ACGT, size=50_000)
    c = D.Case(k=21, kind=D.KIND_MASH, size=1000, seed=0, scale=0.0, max_positions=D.LDS_POSITIONS, stream_cap=D.STREAM_CAP)
    assert D.predict("batch_mash", c, genome[:4000]) == D.MUST_TAKE           # everything is admitted
    assert D.predict("batch_mash", c, genome) == D.MUST_TAKE                  # about 4000 below the threshold
    assert D.predict("batch_mash", c, np.tile(genome[:300], 100)) == D.MUST_NOT   # 300 distinct k-mers, a threshold, n = 1000
    assert D.predict("batch_mash", c, np.full(30_000, ord("N"), np.uint8)) == D.MUST_NOT
    c.size = 3000
    assert D.predict("batch_mash", c, genome) == D.MUST_TAKE                  # about 9000
    c.size, c.k = 1000, 40
    assert D.predict("wide", c, genome) == D.MUST_TAKE
    assert D.predict("wide", c, np.concatenate([genome[:3000], genome[:3000]])) == D.EITHER  # taken by the rule, but k-mers recur
    c.size, c.k = 4096, 21
    assert D.predict("large", c, genome) == D.EITHER                          # about 16 384 below the threshold: the lists decide
    assert D.predict("large", c, genome[:16384]) == D.MUST_TAKE
    c.size = 3001
    assert D.predict("large", c, genome) == D.MUST_TAKE                       # about 12 004
    c.kind, c.size, c.scale = D.KIND_SCALED, 10, 0.01
    assert D.predict("batch_scaled", c, genome) == D.MUST_TAKE                # about 500 at or below max_hash
    assert D.predict("batch_scaled", c, genome[:200]) == D.MUST_NOT           # about 2: fewer than `size`
    c.scale = 1.0
    assert D.predict("batch_scaled", c, genome[:20_000]) == D.MUST_NOT        # more than the epilogue sorts
    assert D.predict("records_stream", c, genome[:20_000]) == D.MUST_NOT      # more rows than the running list holds
    assert D.predict("records_stream", c, genome[:900]) == D.MUST_TAKE
    assert D.predict("records", c, genome[:8192]) == D.MUST_TAKE and D.predict("records", c, genome[:8193]) == D.MUST_NOT
    assert D.predict("counts", c, genome) == D.MUST_TAKE
