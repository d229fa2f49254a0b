"""The host rules of the streamed record sketcher (finch_rs_amd/csrc/fh_records_plan.h: route3, stream_row_bound,
stream_assign_rows, stream_geometry, check_stream) on their own and without a GPU.  tests/hostcore/records_stream_host.cpp
includes that header and answers questions line by line; what the answers must be is worked out here.  Built twice into
pytest's temporary directory, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer, which must stay silent."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "records_stream_host.cpp")
INC = os.path.join(HERE, "..", "finch_rs_amd", "csrc")
MASH, SCALED, ALL_COUNTS = 0, 1, 2
FH_ERR_INVALID, FH_ERR_UNSUPPORTED = -1, -6
LDS, STREAM, ONE = 0, 1, 2


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def ask(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("records_stream_" + request.param) / "records_stream_host")
    flags = ["-O2"] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-I", INC, "-o", exe, SRC])

    def run(questions):
        text = "".join(" ".join(str(w) for w in q) + "\n" for q in questions)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (request.param, r.returncode, r.stderr[-4000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(questions)
        return [line.split() for line in lines]
    return run


def consts(ask):
    return [int(w) for w in ask([("consts",)])[0]]


def test_constants(ask):
    mp, cap, bound, group_records, group_stage, budget = consts(ask)
    assert mp == 8192 and cap >= 1024 and bound > mp and bound <= 1 << 30
    # a record at the bound fits a group's stage, and a group's rows fit a slot's result
    assert (-(-bound // 2048) + 1) * 768 <= group_stage and group_records * cap <= budget


def want_route3(kind, k, pos, lds_on, stream_on, max_pos, group_n, mp, cap, bound):
    served = kind in (MASH, SCALED) and 1 <= k <= 32
    if lds_on and served and pos <= mp:
        return LDS
    fits = kind != MASH or 1 <= group_n <= cap
    if stream_on and served and fits and mp < pos <= min(max_pos, bound):
        return STREAM
    return ONE


def test_three_way_route(ask):
    mp, cap, bound = consts(ask)[:3]
    qs, want = [], []
    for kind in (MASH, SCALED, ALL_COUNTS):
        for k in (1, 21, 32, 33):
            for pos in (0, mp, mp + 1, 20000, 20001, bound, bound + 1):
                for lds_on in (1, 0):
                    for stream_on in (1, 0):
                        for max_pos in (bound, 20000, 0, 1 << 40):
                            for group_n in (1, 1000, cap, cap + 1):
                                qs.append(("route3", kind, k, pos, lds_on, stream_on, max_pos, group_n))
                                want.append(want_route3(kind, k, pos, lds_on, stream_on, max_pos, group_n, mp, cap, bound))
    got = [int(a[0]) for a in ask(qs)]
    assert got == want
    # the corners by name: Mash 1000, k 21, everything on, the door's own bound
    def r(kind, k, pos, lds_on=1, stream_on=1, max_pos=bound, group_n=1000):
        return int(ask([("route3", kind, k, pos, lds_on, stream_on, max_pos, group_n)])[0][0])
    assert [r(MASH, 21, p) for p in (mp, mp + 1, bound, bound + 1)] == [LDS, STREAM, STREAM, ONE]
    assert r(MASH, 32, mp + 1) == STREAM and r(MASH, 33, mp + 1) == ONE and r(MASH, 33, 100) == ONE
    assert r(ALL_COUNTS, 4, mp + 1) == ONE
    assert r(MASH, 21, mp + 1, group_n=cap) == STREAM and r(MASH, 21, mp + 1, group_n=cap + 1) == ONE
    assert r(SCALED, 21, mp + 1, group_n=cap + 1) == STREAM  # (a Scaled size is no bound on the list)
    assert r(MASH, 21, mp + 1, stream_on=0) == ONE and r(MASH, 21, mp, stream_on=0) == LDS
    assert r(MASH, 21, 20000, max_pos=20000) == STREAM and r(MASH, 21, 20001, max_pos=20000) == ONE
    assert r(MASH, 21, mp, lds_on=0) == ONE and r(MASH, 21, mp + 1, lds_on=0) == STREAM


def test_option_off_is_the_two_way_rule(ask):
    mp, cap, bound = consts(ask)[:3]
    qs3, qs2 = [], []
    for kind in (MASH, SCALED, ALL_COUNTS):
        for k in (1, 32, 33, 64):
            for pos in (0, 1, mp, mp + 1, 50000, bound + 1):
                for on in (1, 0):
                    qs3.append(("route3", kind, k, pos, on, 0, bound, 1000))
                    qs2.append(("route", kind, k, pos, on))
    assert [LDS if int(a[0]) else ONE for a in ask(qs2)] == [int(a[0]) for a in ask(qs3)]


def want_bound(kind, size, k, pos, cap):
    w = max(0, pos - k + 1)
    return min(size, w) if kind == MASH else min(w, cap)


def test_row_bounds_and_row0(ask):
    mp, cap, bound = consts(ask)[:3]
    rng = random.Random(11)
    lens = (0, 1, 20, 21, 22, 900, 1044, cap + 20, cap + 21, 8192, 8193, 70000, bound, bound + 1)
    qs, want = [], []
    for kind in (MASH, SCALED):
        for size in (0, 1, 10, 1000, cap):
            for k in (1, 21, 32):
                for pos in lens:
                    qs.append(("bound", kind, size, k, pos))
                    want.append(want_bound(kind, size, k, pos, cap))
    assert [int(a[0]) for a in ask(qs)] == want
    qs, want = [], []
    for kind in (MASH, SCALED):
        for size in (0, 1, 1000, cap):
            for k in (1, 21, 32):
                pos = [rng.choice(lens) for _ in range(rng.randrange(1, 14))]
                qs.append(("rows", kind, size, k) + tuple(pos))
                b = [0 if p > bound else want_bound(kind, size, k, p, cap) for p in pos]  # (beyond the bound: not taken, no rows)
                want.append([sum(b[:i]) for i in range(len(b) + 1)])
    assert [[int(w) for w in a] for a in ask(qs)] == want
    assert want_bound(SCALED, 0, 21, 70000, cap) == cap and want_bound(MASH, 1000, 21, 70000, cap) == 1000 and want_bound(SCALED, 5, 21, 120, cap) == 100


def test_geometry(ask):
    mp, cap, bound, group_records, group_stage, budget = consts(ask)
    cases = [(MASH, 1000, group_records, group_stage), (MASH, 1, 1, 4096), (MASH, cap, 16, 1 << 20), (SCALED, 0, group_records, group_stage), (SCALED, 10, 3, 65536),
             (SCALED, 0, 1 << 20, 8 << 20), (MASH, 10, 257, 100000)]
    for (kind, size, nrec, stage), a in zip(cases, ask([("geom",) + c for c in cases])):
        header, data, rows = (int(w) for w in a)
        assert header == -(-16 * nrec // 4096) * 4096 and data == -(-stage // 4096) * 4096
        per = min(size, cap) if kind == MASH else cap
        assert rows == max(cap, min(budget, nrec * per)), (kind, size, nrec, stage, a)
        assert rows >= cap  # any single record the door serves fits a slot's result


def test_refusals(ask):
    cap = consts(ask)[1]
    too_many = "the streamed record sketcher keeps at most %d hashes of a record in LDS: a Mash sketch of %d goes through an fh_sketcher"
    cases = [
        ((ALL_COUNTS, 4, 0, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher serves Mash and Scaled sketches: AllCounts (kind 2) records go through an fh_sketcher"),
        ((7, 21, 1000, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "unknown sketch kind 7 (0 Mash, 1 Scaled)"),
        ((MASH, 0, 1000, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "kmer_length must be at least 1"),
        ((MASH, 33, 1000, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher serves k = 1..32: k = 33 goes through an fh_sketcher"),
        ((MASH, 33, cap + 1, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher serves k = 1..32: k = 33 goes through an fh_sketcher"),
        ((MASH, 21, 1000, "0", 255, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher takes no test mask (hash_mask must be 0)"),
        ((MASH, 21, 0, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "a Mash sketch has at least one hash (size 0)"),
        ((SCALED, 21, 0, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "scale must be in (0, 1]"),
        ((MASH, 21, 1000, "0", 0, 0, 1 << 20), FH_ERR_INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
        ((MASH, 21, cap + 1, "0", 0, 0, 1 << 20), FH_ERR_INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
        ((MASH, 21, cap + 1, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, too_many % (cap, cap + 1)),
        ((MASH, 21, 10**9, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, too_many % (cap, 10**9)),
        ((MASH, 21, cap, "0", 0, 16, 1 << 20), 0, ""),
        ((SCALED, 21, cap + 1, "1.0", 0, 16, 1 << 20), 0, ""),
        ((SCALED, 1, 0, "0.001", 0, 1 << 20, 1 << 32), 0, ""),
        ((MASH, 32, 1, "0", 0, 1, 4096), 0, ""),
    ]
    for (c, code, msg), a in zip(cases, ask([("check",) + c for c, _, _ in cases])):
        assert int(a[0]) == code and " ".join(a[1:]) == msg, (c, a)
