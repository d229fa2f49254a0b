"""The host rules of the batch sketcher (finch_rs_amd/csrc/fh_batch_plan.h) on their own and without a GPU: the sizes of a
handle, a file's threshold, the rule for "taken", the pool's match predicate, and the plan finch_sketch_files asks for its files.
tests/hostcore/batch_plan_host.cpp includes that header and answers questions line by line; what the answers must be is worked
out here, in Python's integers, so the test does not restate the C++.  Built twice into pytest's temporary directory, plainly
and under AddressSanitizer + UndefinedBehaviorSanitizer, which must stay silent."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "batch_plan_host.cpp")
INC = os.path.join(HERE, "..", "finch_rs_amd", "csrc")

SMALL, WIDE, LARGE, COUNTS = 0, 1, 2, 3
MASH, SCALED, ALL_COUNTS = 0, 1, 2
EMPTY = 2**64 - 1
MIB = 1 << 20
SIZE_EDGES = (0, 1, 3000, 3001, 12288, 12289, 16384, 16385, 1 << 40)
SCALES = ("0.0", "0.001", "1.0", "1.5", "nan")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def ask(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_plan_" + request.param) / "batch_plan_host")
    flags = ["-O2"] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-I", INC, "-o", exe, SRC])

    def run(questions):
        """the answers to a list of questions (each a sequence of words), as lists of words"""
        text = "".join(" ".join(str(w) for w in q) + "\n" for q in questions)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (request.param, r.returncode, r.stderr[-4000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(questions)
        return [line.split() for line in lines]
    return run


def ints(answer):
    return [int(w) for w in answer]


def ceil_to(x, m):
    return -(-x // m) * m


def test_geometry(ask):
    # a large handle's partitions
    ns = (3001, 10000, 16384)
    for n, a in zip(ns, ask([("geom", LARGE, MASH, 21, n, 16, 32 * MIB) for n in ns])):
        cap, live, shard = ints(a)[:3]
        assert live == ceil_to(4 * n + 8192, 1024) and cap == 2 * live and shard == live // 32
    # the small ones, whatever the size; the result columns
    cols = [((SMALL, MASH, 21, 1000), 1002, 4008), ((WIDE, MASH, 40, 1000), 1002, 5010), ((SMALL, SCALED, 21, 1000), 12290, 49160),
            ((WIDE, SCALED, 64, 0), 12290, 61450), ((LARGE, MASH, 21, 16384), 16386, 65544), ((COUNTS, ALL_COUNTS, 7, 0), 8192, 12288),
            ((COUNTS, ALL_COUNTS, 6, 0), 2080, 3120), ((SMALL, MASH, 1, 3000), 3002, 12008), ((SMALL, MASH, 32, 1), 4, 16)]
    for (case, stride, words), a in zip(cols, ask([("geom",) + c + (4, MIB) for c, _, _ in cols])):
        g = ints(a)
        assert (g[4], g[5]) == (stride, words), (case, g)
        if case[0] in (SMALL, WIDE):
            assert g[:3] == [32768, 16384, 512], (case, g)
        if case[0] == COUNTS:
            assert g[:3] == [0, 0, 0]
    # the descriptors of max_files files (40 bytes each) rounded up to 4 KiB, the staging bytes likewise
    files = (1, 64, 102, 103, 4096)
    for f, a in zip(files, ask([("geom", SMALL, MASH, 21, 1000, f, 100000) for f in files])):
        assert ints(a)[6:8] == [ceil_to(40 * f, 4096), 102400], (f, a)
    assert ceil_to(40 * 103, 4096) == 8192 and ceil_to(40 * 4096, 4096) == 40 * 4096
    # device memory: per file the table (40-byte entries, 8 more for the high k-mer words), live and dead lists (and a large
    # handle's key scratch), 256 shard lists and their cursors 32 dwords apart, the control block (3680) and 64 collision
    # records of 32 bytes; the two slots' staging buffers
    for form, k, n, f in ((SMALL, 21, 1000, 64), (WIDE, 33, 3000, 7), (LARGE, 21, 10000, 16)):
        (a,) = ask([("geom", form, MASH, k, n, f, 32 * MIB)])
        cap, live, shard, _, _, _, header, data, dev = ints(a)
        assert dev == f * (cap * (40 + (8 if form == WIDE else 0)) + live * (8 + (8 if form == LARGE else 0)) + 256 * (shard + 32) * 4 + 3680 + 64 * 32) + \
            2 * (header + data + 64), (form, a)
    assert ints(ask([("geom", SMALL, MASH, 21, 1000, 64, 32 * MIB)])[0])[8] == 64 * 2_004_576 + 2 * (4096 + 32 * MIB + 64)


def want_tau(E, length):
    if length <= E:
        return EMPTY
    t = (E << 64) // length
    return EMPTY if t >= EMPTY - 1 else t


def test_tau(ask):
    cases = [(SMALL, 1000, 0, 4000), (WIDE, 1000, 0, 4000), (SMALL, 2000, 0, 8000), (SMALL, 2001, 0, 6003), (LARGE, 5000, 4, 20000), (LARGE, 5000, 1, 5000),
             (LARGE, 5000, 0, 5000), (SMALL, 1, 0, 4)]
    qs, want = [], []
    for form, n, large_want, E in cases:
        for length in (0, E, E + 1, 2 * E, 1 << 40, E - 1, (1 << 64) - 1):
            qs.append(("tau", form, MASH, n, 12345, length, large_want))
            want.append(want_tau(E, length))
    assert [int(a[0]) for a in ask(qs)] == want
    assert want_tau(4000, 4001) == (4000 << 64) // 4001 and want_tau(4000, 8000) == 1 << 63
    # Scaled: max_hash whatever the file, u64::MAX at scale 1 included; a count has none
    mh = EMPTY // 1000
    qs = [("tau", form, SCALED, 1000, m, length, 0) for form in (SMALL, WIDE) for m in (mh, EMPTY, 0) for length in (0, 5000, 1 << 40)]
    assert [int(a[0]) for a in ask(qs)] == [q[4] for q in qs]
    assert [int(a[0]) for a in ask([("tau", COUNTS, ALL_COUNTS, 0, 0, length, 0) for length in (0, 5000, 1 << 40)])] == [0, 0, 0]


def test_taken(ask):
    real_tau = (4000 << 64) // 5_000_000
    base = dict(kind=MASH, size=1000, sorted=2, overflow=0, need_big=0, n_coll=0, n_live=1000, sp_count=0, inserted_total=4000, tau=real_tau)

    def q(**changes):
        r = dict(base, **changes)
        return ("taken",) + tuple(r[f] for f in ("kind", "size", "sorted", "overflow", "need_big", "n_coll", "n_live", "sp_count", "inserted_total", "tau"))
    cases = [
        (q(), 1),
        (q(sorted=1), 0), (q(sorted=0), 0), (q(overflow=1), 0), (q(need_big=1), 0), (q(n_coll=1), 0), (q(sp_count=1), 0),
        # Mash: the guess must have admitted `size` hashes, unless it admitted everything; never more rows than `size`
        (q(inserted_total=999, n_live=999), 0), (q(inserted_total=999, n_live=999, tau=EMPTY), 1), (q(inserted_total=1000), 1),
        (q(n_live=1001), 0), (q(n_live=0, inserted_total=0, tau=EMPTY), 1),
        # Scaled: at least `size` live entries, at most what the epilogue sorts; inserted_total and tau do not matter
        (q(kind=SCALED, n_live=999), 0), (q(kind=SCALED, n_live=1000), 1), (q(kind=SCALED, n_live=12288), 1), (q(kind=SCALED, n_live=12289), 0),
        (q(kind=SCALED, size=0, n_live=0, inserted_total=0), 1), (q(kind=SCALED, n_live=1000, inserted_total=0), 1),
        (q(kind=SCALED, n_live=1000, sorted=1), 0), (q(kind=SCALED, n_live=1000, sp_count=1, tau=EMPTY), 0),
    ]
    got = [int(a[0]) for a in ask([c for c, _ in cases])]
    assert got == [w for _, w in cases], [(c, w, g) for (c, w), g in zip(cases, got) if w != g]


def test_pool_key(ask):
    def key(form, device=0, max_files=4, data=MIB, k=7, size=3000, seed=0, kind=MASH, scale="0.0"):
        return (form, device, max_files, data, k, size, seed, kind, scale)

    def match(parked, asked):
        return int(ask([("match",) + parked + asked])[0][0])
    # one key per door, everything else equal: a handle made through one door is never handed out by another
    doors = (SMALL, WIDE, LARGE, COUNTS)
    got = ask([("match",) + key(a) + key(b) for a in doors for b in doors])
    assert [int(g[0]) for g in got] == [int(a == b) for a in doors for b in doors]
    # what every door looks at
    for form in doors:
        assert match(key(form), key(form)) == 1
        for other in (dict(device=1), dict(max_files=5), dict(data=2 * MIB), dict(k=8)):
            assert match(key(form), key(form, **other)) == 0, (form, other)
    # small and wide: size, seed and kind, the scale of a Scaled sketch only
    for form in (SMALL, WIDE):
        for other in (dict(size=2999), dict(seed=1), dict(kind=SCALED)):
            assert match(key(form), key(form, **other)) == 0, (form, other)
        assert match(key(form, kind=SCALED, scale="0.001"), key(form, kind=SCALED, scale="0.002")) == 0
        assert match(key(form, kind=SCALED, scale="0.001"), key(form, kind=SCALED, scale="0.001")) == 1
        assert match(key(form, scale="0.001"), key(form, scale="0.002")) == 1
    # large: size and seed, neither kind (Mash only) nor scale
    assert match(key(LARGE), key(LARGE, seed=1)) == 0 and match(key(LARGE), key(LARGE, size=3001)) == 0
    assert match(key(LARGE, scale="0.5"), key(LARGE, scale="0.25")) == 1
    # counts: k alone
    assert match(key(COUNTS), key(COUNTS, size=1, seed=9, scale="0.5")) == 1


def parent_rule(kind, k, n, scale, filter_on, n_files):
    """which door served a call before the plan existed (group_ok and the choice of constructor in finch_sketch_files), or None"""
    s = float(scale)
    if n_files <= 1 or filter_on > 0 or not 1 <= k <= 64:
        return None
    if kind == ALL_COUNTS:
        return COUNTS if k <= 7 else None
    if kind == SCALED:
        return (WIDE if k > 32 else SMALL) if n <= 12288 and 0.0 < s <= 1.0 else None
    if kind != MASH or n < 1:
        return None
    if n <= 3000:
        return WIDE if k > 32 else SMALL
    return LARGE if n <= 16384 and k <= 32 else None


def test_file_plan(ask):
    def plan(kind=MASH, k=21, kmers=1000, final=1000, scale="0.001", filter_on=0, n_files=2):
        ok, form, group_n = ints(ask([("plan", kind, k, kmers, final, scale, filter_on, n_files)])[0])
        return (form, group_n) if ok else None
    assert plan(kmers=3000, final=3000) == (SMALL, 3000)
    assert plan(k=32, kmers=3001, final=3001) == (LARGE, 3001)
    assert plan(k=33, kmers=3001, final=3001) is None
    assert plan(kmers=16384, final=16384) == (LARGE, 16384)
    assert plan(kmers=16385, final=16385) is None
    assert plan(k=64) == (WIDE, 1000) and plan(k=33) == (WIDE, 1000) and plan(k=32) == (SMALL, 1000)
    assert plan(k=65) is None and plan(k=0) is None
    assert plan(kind=ALL_COUNTS, k=7) == (COUNTS, 1000) and plan(kind=ALL_COUNTS, k=1) == (COUNTS, 1000)
    assert plan(kind=ALL_COUNTS, k=8) is None and plan(kind=ALL_COUNTS, k=0) is None
    assert plan(kind=SCALED, kmers=12288) == (SMALL, 12288) and plan(kind=SCALED, kmers=0) == (SMALL, 0)
    assert plan(kind=SCALED, kmers=12289) is None
    assert plan(kind=SCALED, scale="0.0") is None and plan(kind=SCALED, scale="1.5") is None and plan(kind=SCALED, scale="nan") is None
    assert plan(kind=SCALED, scale="1.0") == (SMALL, 1000) and plan(kind=SCALED, k=40, scale="1.0") == (WIDE, 1000)
    assert plan(filter_on=1) is None and plan(filter_on=-1) == (SMALL, 1000)
    assert plan(n_files=1) is None and plan(n_files=0) is None
    assert plan(kind=7) is None
    # the cut to final_size: the handle is made for what the small sketcher would keep; never for a Scaled sketch
    assert plan(kmers=5000, final=1000) == (SMALL, 1000)
    assert plan(kmers=5000, final=0) == (LARGE, 5000) and plan(kmers=1000, final=5000) == (SMALL, 1000)
    assert plan(kmers=100000, final=10000) == (LARGE, 10000)
    assert plan(kind=SCALED, kmers=5000, final=1000) == (SMALL, 5000)


def test_scaled_prefilter(ask):
    # not staged once floor(st_size x max_hash / 2^64) passes 5/4 of 12 288
    cap = 12288 + 12288 // 4
    assert cap == 15360
    for mh in (EMPTY // 1000, EMPTY // 7, EMPTY):
        first_out = -(-((cap + 1) << 64) // mh)  # the smallest size whose estimate is cap + 1
        assert (first_out * mh) >> 64 == cap + 1 and ((first_out - 1) * mh) >> 64 == cap
        sizes = (1, first_out - 1, first_out, first_out + 1, 32 * MIB)
        assert [int(a[0]) for a in ask([("fit", s, mh) for s in sizes])] == [1, 1, 0, 0, 0], mh
    assert [int(a[0]) for a in ask([("fit", s, 0) for s in (1, 32 * MIB)])] == [1, 1]


def test_what_the_plan_names_its_door_accepts(ask):
    """the property the plan adds: whenever it names a door for a call, that door's own check takes the parameters the worker will
    construct its handle with -- and over the grid the plan names exactly the door finch_sketch_files chose before"""
    grid = list(itertools.product((MASH, SCALED, ALL_COUNTS, 7), range(0, 67), SIZE_EDGES, SCALES))
    plans = ask([("plan", kind, k, n, n, scale, 0, 2) for kind, k, n, scale in grid])
    checks, named = [], 0
    for (kind, k, n, scale), a in zip(grid, plans):
        ok, form, group_n = ints(a)
        assert group_n == n
        want = parent_rule(kind, k, n, scale, 0, 2)
        assert (form if ok else None) == want, (kind, k, n, scale, a)
        if ok:
            named += 1
            checks.append(("check", form, kind, k, group_n, scale, 0, 16 if form == LARGE else 64, 32 * MIB))
    assert named > 1000 and {c[1] for c in checks} == {SMALL, WIDE, LARGE, COUNTS}
    for c, a in zip(checks, ask(checks)):
        assert a == ["0"], (c, a)
