"""finch_merge_groups on the GPU (include/finch_host.h): every group, field by field, against tests/merge_model.py
-- the reference's loop folded in the order given -- and, on a sample, against finch_merge_pair folded on the host, over the
shape edges of the kernel: list lengths around a wave and a workgroup, tiles and thread chunks, every clip mode with the clip on
and beside a record, folds with empty and repeated members, sums that wrap, launches, device entries."""
import ctypes as C

import numpy as np
import pytest

import finch_rs_amd as F
import merge_cases as MC
import merge_model as MM
from finch_rs_amd import host as H

pytestmark = pytest.mark.gpu

BIG = 2 ** 32 - 1
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
SCALE = 2.0 ** -40          # the divisor is 2^40 exactly: max_hash = 2^24 - 1
MAX_HASH = 2 ** 24 - 1


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")
    assert MM.max_hash(SCALE) == MAX_HASH


def merge(s, groups, size=None, tile=None, chunk=None, **kw):
    try:
        F.set_option("merge_tile", tile)
        F.set_option("merge_chunk_records", chunk)
        return H.merge(s, groups, size, **kw)
    finally:
        F.set_option("merge_tile", None)
        F.set_option("merge_chunk_records", None)


def check(members, groups, size=None, host_sample=3, **kw):
    """one call over `groups` of indices into `members`; every result against the model, the first few against the host fold too"""
    s = MC.collect(members)
    st = {}
    out = merge(s, groups, size, stats=st, **kw)
    assert len(out) == len(groups)
    want = [MC.expected([members[i] for i in g], size) for g in groups]
    for g, w in enumerate(want):
        try:
            MC.same(MC.read(out, g), w)
        except AssertionError as e:
            raise AssertionError("group %d %r: %s" % (g, groups[g][:8], e))
    for g in range(min(host_sample, len(groups))):
        acc = H.select(s, [groups[g][0]])
        for i in groups[g][1:]:
            acc = H.merge_pair(acc, 0, s, i, size)
        MC.same(MC.read(acc, 0), want[g])
    multi = [w for g, w in zip(groups, want) if len(g) >= 2]
    assert st["records_copied"] == sum(len(w["records"]) for w in multi)
    assert st["launches"] >= (1 if multi else 0)
    return want, st


def spread(rng, n, universe, tag, **kw):
    hs = np.sort(rng.choice(universe, size=n, replace=False)) * 1009 + 17
    return MC.Member("%c%d" % (tag, n), MC.records(hs.tolist(), tag), **kw)


# ---- lengths ----

def length_members():
    rng = np.random.default_rng(31)
    acc = [spread(rng, n, 6000, 65) for n in LENGTHS]     # hashes from a few thousand values: the lists share many
    mem = [spread(rng, n, 6000, 66) for n in LENGTHS]
    return acc + mem


@pytest.mark.parametrize("tile", [None, 1, 64])
def test_lengths(tile):
    """accumulator and member lengths around a wave, a workgroup and a tile; merge_tile 1 makes every position a tile of its own"""
    members = length_members()
    n = len(LENGTHS)
    pairs = [[a, n + b] for a in range(n) for b in range(n)]
    if tile == 1:
        pairs = [p for p in pairs if LENGTHS[p[0]] <= 257 and LENGTHS[p[1] - n] <= 257]
    elif tile == 64:
        pairs = [p for p in pairs if LENGTHS[p[0]] > 257 or LENGTHS[p[1] - n] > 257]
    want, _ = check(members, pairs, tile=tile)
    assert any(len(w["records"]) > 4097 for w in want) or tile == 1


# ---- patterns ----

def pattern_members(n):
    base = [h * 11 + 3 for h in range(n)]
    A = MC.Member("A", MC.records(base, 65, [2] * n, [1] * n))
    same_ = MC.Member("same", MC.records(base, 66, [3] * n, [0] * n))
    every_other = MC.Member("every other", MC.records([h if i % 2 == 0 else h + 1 for i, h in enumerate(base)], 67))
    odd_shared = MC.Member("odd shared", MC.records([h if i % 2 == 1 else h + 1 for i, h in enumerate(base)], 68))
    disjoint = MC.Member("interleaved", MC.records([h + 5 for h in base], 69))
    above = MC.Member("above", MC.records([base[-1] + 1 + h for h in range(n)], 70))
    below = MC.Member("below", MC.records(list(range(0, 3)), 71))
    runs = MC.Member("runs", MC.records([h if (i // 7) % 2 else h + 2 for i, h in enumerate(base)], 72))  # shared in runs of 7
    return [A, same_, every_other, odd_shared, disjoint, above, below, runs]


@pytest.mark.parametrize("tile", [None, 1, 64, 300, 4096])
def test_patterns(tile):
    """shared hashes on every position (so on every thread-chunk and tile boundary, whatever the tile), on the even and on the odd
    positions, in runs, nowhere; one list entirely above the other: the result is the lower list alone"""
    n = 150 if tile == 1 else 700
    members = pattern_members(n)
    groups = [[0, j] for j in range(1, len(members))] + [[j, 0] for j in range(1, len(members))]
    want, _ = check(members, groups, tile=tile, host_sample=len(groups))
    by = {tuple(g): w["records"] for g, w in zip(groups, want)}
    assert len(by[(0, 1)]) == n and all(r[1] == 5 and r[2] == 1 and r[3][:1] == b"A" for r in by[(0, 1)])
    assert all(r[3][:1] == b"B" for r in by[(1, 0)])
    assert by[(0, 5)] == members[0].recs and by[(5, 0)] == members[0].recs        # A lies entirely below "above"
    assert by[(0, 6)] == members[6].recs and by[(6, 0)] == members[6].recs        # "below" lies entirely below A
    assert len(by[(0, 4)]) == 2 * n - 1                                           # disjoint: only the last record of the higher list is lost


# ---- clip ----

def clip_members(n_a=180, n_b=150, universe=300):
    """For every place c of the clip in the walk's output and both kinds of place -- max_hash equal to record c - 1's hash, or
    between records c - 1 and c -- a Scaled first member and a second member whose hashes are laid around MAX_HASH accordingly; the
    same index sets with a Mash first member for the modes without a scale."""
    rng = np.random.default_rng(41)
    ia = np.sort(rng.choice(universe, size=n_a, replace=False))
    ib = np.sort(rng.choice(universe, size=n_b, replace=False))
    bound = min(ia[-1], ib[-1])
    order = sorted(set(ia[ia <= bound].tolist()) | set(ib[ib <= bound].tolist()))   # the walk's output, as indices
    length = len(order)
    rank = {v: r for r, v in enumerate(order)}
    top = len(order)
    for v in sorted(set(ia.tolist()) | set(ib.tolist())):
        if v not in rank:
            rank[v] = top                                                           # (past the walk's end: only their order matters)
            top += 1
    places = sorted({0, 1, 63, 64, 65, 128, length - 1, length, length + 5})
    members, groups, meta = [], [], []
    for c in places:
        for exact in (True, False):
            def hashes(idx):
                return [MAX_HASH + (rank[v] - (c - 1)) * 3 - (0 if exact else 1) for v in idx.tolist()]
            first = MC.Member("scaled c=%d %s" % (c, exact), MC.records(hashes(ia), 65), MC.scaled(SCALE), 7, 5)
            second = MC.Member("second c=%d %s" % (c, exact), MC.records(hashes(ib), 66), MC.scaled(0.5), 11, 13)
            mash = MC.Member("mash c=%d %s" % (c, exact), first.recs, MC.MASH, 7, 5)
            at = len(members)
            members += [first, second, mash]
            groups += [[at, at + 1], [at + 2, at + 1]]
            meta += [(c, True), (c, False)]
    return members, groups, meta, length


@pytest.mark.parametrize("tile", [None, 64])
@pytest.mark.parametrize("size", ["none", 0, 1, 70, "len-1", "len", "len+9"])
def test_clip_modes(size, tile):
    members, groups, meta, length = clip_members()
    size = {"none": None, "len-1": length - 1, "len": length, "len+9": length + 9}.get(size, size)
    want, _ = check(members, groups, size, tile=tile)
    for (c, is_scaled), w in zip(meta, want):
        n = len(w["records"])
        if is_scaled:   # hash <= max_hash keeps min(c, length) records; ix < size keeps records above max_hash
            assert n == (min(c, length) if size is None else max(min(c, length), min(size, length))), (c, size, n)
        else:
            assert n == (length if size is None else min(size, length))


# ---- folds ----

def fold_members():
    rng = np.random.default_rng(51)
    members = [spread(rng, int(rng.integers(40, 400)), 900, 65 + i, seq_length=int(rng.integers(0, 2 ** 50)), num_valid_kmers=1000 + i,
                      comment="comment %d" % i) for i in range(17)]
    members.append(MC.Member("empty", [], comment="nothing here"))                        # 17
    return members


@pytest.mark.parametrize("size", [None, 100])
def test_folds(size):
    members = fold_members()
    groups = [[3], [0, 1], [2, 1, 0], list(range(17)), list(range(16, -1, -1)),
              [17, 0, 1], [0, 17, 1], [0, 1, 17], [17], [17, 17],
              [4, 4], [4, 5, 4, 5, 4], [4, 6], [6, 4, 7]]          # a sketch twice in a group, and in several groups
    want, st = check(members, groups, size, host_sample=len(groups), tile=64)
    by = {tuple(g): w for g, w in zip(groups, want)}
    assert by[(3,)]["records"] == members[3].recs and len(members[3].recs) > 100     # one member: unclipped whatever the size
    for g in ((17, 0, 1), (0, 17, 1), (0, 1, 17), (17, 17)):
        assert by[g]["records"] == []
    assert [r[1] for r in by[(4, 4)]["records"]] == [2 * r[1] for r in members[4].recs][:size]
    assert by[(2, 1, 0)]["name"] == members[2].name and by[(2, 1, 0)]["comment"] == "comment 2"
    assert by[tuple(range(17))]["seq_length"] == sum(m.seq_length for m in members[:17]) % 2 ** 64
    assert st["launches"] == 1


def test_a_scaled_group_in_two_orders():
    """test_merge_model.py's literal around MAX_HASH: (G, H, F) loses F's record below max_hash, (G, F, H) keeps it"""
    at = lambda *offs: [MAX_HASH + o for o in offs]
    G = MC.Member("G", MC.records(at(-40, -10, 20), 71), MC.scaled(SCALE))
    Hm = MC.Member("H", MC.records(at(-30, 5, 25), 72), MC.scaled(SCALE))
    Fm = MC.Member("F", MC.records(at(-5, 8, 40), 70), MC.scaled(SCALE))
    want, _ = check([G, Hm, Fm], [[0, 1, 2], [0, 2, 1]])
    assert [r[0] - MAX_HASH for r in want[0]["records"]] == [-40, -30, -10]
    assert [r[0] - MAX_HASH for r in want[1]["records"]] == [-40, -30, -10, -5]
    rng = np.random.default_rng(52)
    members = [MC.Member("m%d" % i, MC.records((np.sort(rng.choice(400, size=120, replace=False)) * 7 + MAX_HASH - 1400).tolist(), 65 + i),
                         MC.scaled(SCALE)) for i in range(6)]
    groups = [list(p) for p in ([0, 1, 2, 3, 4, 5], [0, 5, 4, 3, 2, 1], [3, 1, 4, 0, 5, 2], [2, 5, 0, 4, 1, 3])]
    want, _ = check(members, groups, tile=64)
    assert len({tuple(r[0] for r in w["records"]) for w in want}) > 1   # the orders do not agree


def test_only_the_first_members_scale_counts():
    rng = np.random.default_rng(53)
    def member(i, params):
        return MC.Member("m%d" % i, MC.records((np.sort(rng.choice(400, size=150, replace=False)) * 7 + MAX_HASH - 1400).tolist(), 65 + i), params)
    members = [member(0, MC.MASH), member(1, MC.scaled(SCALE)), member(2, MC.scaled(0.25)), member(3, MC.scaled(SCALE))]
    want, _ = check(members, [[0, 1, 2], [1, 0, 2], [2, 0, 1], [3, 2, 0]], 30, tile=64)
    assert len(want[0]["records"]) == 30                                         # Mash first: the size alone
    assert 30 < len(want[1]["records"]) and want[1]["records"][-1][0] <= MAX_HASH  # Scaled first: max_hash, which lies beyond 30 records
    assert len(want[2]["records"]) > len(want[1]["records"])                     # scale 0.25: max_hash = 2^62, nothing is clipped


# ---- arithmetic ----

def test_sums_wrap_and_ties_take_the_earlier_kmer():
    hs = list(range(100, 400, 3))
    a = MC.Member("a", MC.records(hs, 65, [BIG] * len(hs), [BIG - 1] * len(hs)), seq_length=2 ** 64 - 5, num_valid_kmers=2 ** 63)
    b = MC.Member("b", MC.records(hs, 66, [7] * len(hs), [7] * len(hs)), seq_length=9, num_valid_kmers=2 ** 63)
    c = MC.Member("c", MC.records(hs[::2] + [1000], 67, [BIG] * (len(hs[::2]) + 1), [0] * (len(hs[::2]) + 1)), seq_length=1, num_valid_kmers=1)
    want, _ = check([a, b, c], [[0, 1], [1, 0], [0, 1, 2], [2, 1, 0], [0, 0, 0]])
    assert want[0]["records"][0][1:] == (6, 5, MC.kmer(65, 100)) and want[1]["records"][0][3] == MC.kmer(66, 100)
    assert want[0]["seq_length"] == 4 and want[0]["num_valid_kmers"] == 0
    assert want[2]["records"][0][1:3] == (5, 5) and want[2]["records"][1][1:3] == (6, 5)
    assert want[3]["records"][0][3] == MC.kmer(67, 100) and want[3]["records"][1][3] == MC.kmer(66, 103)
    assert want[4]["records"][0][1:3] == ((3 * BIG) % 2 ** 32, (3 * (BIG - 1)) % 2 ** 32)


# ---- scheduling ----

def random_library():
    rng = np.random.default_rng(61)
    members = [spread(rng, int(rng.integers(0, 300)), 2000, 65 + i % 26) for i in range(120)]
    groups = [rng.choice(120, size=int(rng.integers(1, 7))).tolist() for _ in range(300)]
    return members, groups


@pytest.mark.parametrize("how", ["default", "launches", "two entries"])
def test_300_random_groups(how):
    """more groups than one per compute unit; the same call cut into at least 5 launches; the same call over two device entries"""
    members, groups = random_library()
    kw = {"launches": {"chunk": 10000}, "two entries": {"devices": (0, 0), "chunk": 100000}}.get(how, {})
    want, st = check(members, groups, 250, **kw)
    if how == "default":
        assert st["launches"] == 1 and st["kernel_ms"] > 0
    elif how == "launches":
        assert st["launches"] >= 5
    else:
        assert st["launches"] >= 2
    assert sum(len(g) == 1 for g in groups) > 10 and any(len(w["records"]) == 250 for w in want)


def test_the_current_device_is_left_alone():
    hip = C.CDLL("libamdhip64.so")
    members = pattern_members(50)
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    before = dev.value
    check(members, [[0, 1], [2, 3]], devices=(F.device_count() - 1,))
    assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == before
