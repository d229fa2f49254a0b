"""The host rules of the record sketcher (finch_rs_amd/csrc/fh_records_plan.h) on their own and without a GPU: the header rule
(name / comment), where the records of a FASTA text begin and end and what seq_length is, which route a record takes, the rows
of a group, the size a handle is made for and its sizes.  tests/hostcore/records_plan_host.cpp includes that header and answers
questions line by line; what the answers must be is worked out here, in Python, so the test does not restate the C++.  Built
twice into pytest's temporary directory, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer, which must stay
silent."""
import os
import random
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "records_plan_host.cpp")
INC = os.path.join(HERE, "..", "finch_rs_amd", "csrc")
MASH, SCALED, ALL_COUNTS = 0, 1, 2
FH_ERR_INVALID, FH_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def ask(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("records_plan_" + request.param) / "records_plan_host")
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


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def max_pos(ask):
    return int(ask([("maxpos",)])[0][0])


# ---- the header rule ----
def want_header(h: bytes):
    """name = up to the first blank or tab; comment = what follows that run of blanks and tabs"""
    m = re.match(rb"([^ \t]*)[ \t]*(.*)\Z", h, re.S)
    return m.group(1), m.group(2)


HEADERS = [b"seq1", b"seq1 a comment", b"seq1\tcomment", b"seq1 \t  two  words ", b"", b" lead", b"\tx", b"id ", b"id\t", b"a b\tc", b"id  ", b"x" * 300 + b" " + b"y" * 300]


def test_header_rule(ask):
    for h, a in zip(HEADERS, ask([("header", hx(h)) for h in HEADERS])):
        name_len, c_off, c_len = (int(w) for w in a)
        name, comment = want_header(h)
        assert h[:name_len] == name and h[c_off:c_off + c_len] == comment and c_off + c_len == len(h), (h, a)
    assert want_header(b"seq1 \t  two  words ") == (b"seq1", b"two  words ") and want_header(b" lead") == (b"", b"lead") and want_header(b"id ") == (b"id", b"")


# ---- records ----
def want_records(t: bytes):
    """parse_fastx's rules, stated over lines: a record begins at a line that begins with '>'"""
    lines = t.splitlines(keepends=True)  # (bytes.splitlines also splits at a lone CR: put those lines back together)
    merged = []
    for ln in lines:
        if merged and not merged[-1].endswith(b"\n"):
            merged[-1] += ln
        else:
            merged.append(ln)
    recs, pos = [], 0
    for ln in merged:
        if ln.startswith(b">"):
            recs.append({"text0": pos, "hdr": ln, "seq": b""})
        else:
            recs[-1]["seq"] += ln
        pos += len(ln)
    out = []
    for r in recs:
        hdr = r["hdr"]
        content = hdr[1:]
        if content.endswith(b"\n"):
            content = content[:-1]
        if content.endswith(b"\r"):
            content = content[:-1]
        seq = r["seq"]
        trimmed = seq
        if trimmed.endswith(b"\r\n"):
            trimmed = trimmed[:-2]
        elif trimmed.endswith(b"\n") or trimmed.endswith(b"\r"):
            trimmed = trimmed[:-1]
        positions = len(seq) - sum(seq.count(c) for c in (b" ", b"\t", b"\r", b"\n"))
        out.append((r["text0"], r["text0"] + len(hdr) + len(seq), r["text0"] + 1, r["text0"] + 1 + len(content), r["text0"] + len(hdr), len(trimmed), positions))
    return out


TEXTS = [
    b">a\nACGT\n",
    b">a\nACGT",                                   # no final line end
    b">a\nAC\nGT\n>b\nTT\n",                       # multi-line
    b">a desc here\r\nAC\r\nGT\r\n>b\r\nTT\r\n",   # CR LF
    b">\nACGT\n",                                  # '>' alone
    b">a\nAC>GT\n>b\nA\n",                         # a '>' inside a sequence line
    b">a\nACGT\n>b",                               # a header as the last line
    b">a\nACGT\n>b\n",
    b">a\n>b\n>c\nA\n",                            # headers without sequence
    b">a\n\nAC\n\n>b\nT T\tA\n",                   # empty lines and blanks in the sequence
    b">a",
    b">a\r",
    b">a\nAC\r",
    b">a\n\n",
    b">a\n\r\n",
    b">a x\ty  \nACGT\nN\n",
]


def test_split_records(ask):
    rng = random.Random(5)
    texts = list(TEXTS)
    for _ in range(200):  # random texts over the bytes that matter
        n = rng.randrange(1, 60)
        texts.append(b">" + bytes(rng.choice(b">\n\rAC \t") for _ in range(n)))
    for t, a in zip(texts, ask([("split", hx(t)) for t in texts])):
        v = [int(w) for w in a]
        got = [tuple(v[1 + 7 * i:8 + 7 * i]) for i in range(v[0])]
        assert got == want_records(t), (t, got, want_records(t))
    # what the rule says, spelled out once
    assert want_records(b">a desc here\r\nAC\r\nGT\r\n>b\r\nTT\r\n")[0] == (0, 22, 1, 12, 14, 6, 4)
    assert want_records(b">a\nAC>GT\n>b\nA\n")[0][5:] == (5, 5) and len(want_records(b">a\nAC>GT\n>b\nA\n")) == 2
    assert want_records(b">a\nACGT\n>b")[1] == (8, 10, 9, 10, 10, 0, 0)


# ---- the route ----
def test_route(ask):
    mp = max_pos(ask)
    assert mp == 8192
    qs, want = [], []
    for kind in (MASH, SCALED, ALL_COUNTS):
        for k in (1, 21, 32, 33, 64):
            for pos in (0, 1, mp - 1, mp, mp + 1, 10 * mp):
                for on in (1, 0):
                    qs.append(("route", kind, k, pos, on))
                    want.append(int(on == 1 and kind in (MASH, SCALED) and k <= 32 and pos <= mp))
    assert [int(a[0]) for a in ask(qs)] == want


# ---- rows ----
def want_bound(kind, size, k, pos):
    w = max(0, pos - k + 1)
    return min(size, w) if kind == MASH else w


def test_row0_sums(ask):
    rng = random.Random(7)
    qs, want = [], []
    for kind in (MASH, SCALED):
        for size in (0, 1, 10, 1000, 5000, 10**9):
            for k in (1, 21, 32):
                pos = [rng.choice((0, 1, k - 1, k, k + 1, 900, 1500, 8191, 8192)) for _ in range(rng.randrange(1, 12))]
                qs.append(("rows", kind, size, k) + tuple(pos))
                b = [want_bound(kind, size, k, p) for p in pos]
                want.append([sum(b[:i]) for i in range(len(b) + 1)])
    assert [[int(w) for w in a] for a in ask(qs)] == want
    # a 900-window record asked for 5000 hashes needs 900 rows; a Scaled record may keep every window
    assert want_bound(MASH, 5000, 21, 920) == 900 and want_bound(SCALED, 10, 21, 920) == 900 and want_bound(MASH, 1000, 21, 20) == 0
    lens = (0, 1, 2047, 2048, 2049, 8192)
    assert [int(a[0]) for a in ask([("region", p) for p in lens])] == [(-(-p // 2048) + 1) * 768 for p in lens]


def test_group_n(ask):
    cases = [(MASH, 1000, 1000), (MASH, 2000, 1000), (MASH, 1000, 2000), (MASH, 1000, 0), (MASH, 1000, 1), (SCALED, 1000, 10), (SCALED, 0, 0), (MASH, 1, 1)]
    want = [kts if kind == SCALED or not (1 <= fin < kts) else fin for kind, kts, fin in cases]
    assert [int(a[0]) for a in ask([("group_n",) + c for c in cases])] == want


def test_geometry(ask):
    mp, _, group_stage, budget = (int(w) for w in ask([("maxpos",)])[0])
    cases = [(MASH, 1000, 16384, group_stage), (MASH, 1000, 1, 4096), (MASH, 10, 100, 1 << 20), (SCALED, 0, 16384, group_stage), (SCALED, 10, 3, 65536),
             (MASH, 10**6, 50, 8 << 20), (MASH, 1000, 257, 100000)]
    for (kind, size, nrec, stage), a in zip(cases, ask([("geom",) + c for c in cases])):
        header, data, rows = (int(w) for w in a)
        assert header == -(-16 * nrec // 4096) * 4096 and data == -(-stage // 4096) * 4096
        per = min(size, mp) if kind == MASH else mp
        assert rows == max(mp, min(budget, nrec * per, data // 3840 * mp + mp)), (kind, size, nrec, stage, a)
        assert rows >= mp  # any single record the door serves fits a slot's result


def test_refusals(ask):
    cases = [
        ((ALL_COUNTS, 4, 0, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher serves Mash and Scaled sketches: AllCounts (kind 2) records go through an fh_sketcher"),
        ((7, 21, 1000, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "unknown sketch kind 7 (0 Mash, 1 Scaled)"),
        ((MASH, 0, 1000, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "kmer_length must be at least 1"),
        ((MASH, 33, 1000, "0", 0, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher serves k = 1..32: k = 33 goes through an fh_sketcher"),
        ((MASH, 21, 1000, "0", 255, 16, 1 << 20), FH_ERR_UNSUPPORTED, "the record sketcher takes no test mask (hash_mask must be 0)"),
        ((MASH, 21, 0, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "a Mash sketch has at least one hash (size 0)"),
        ((SCALED, 21, 0, "0", 0, 16, 1 << 20), FH_ERR_INVALID, "scale must be in (0, 1]"),
        ((SCALED, 21, 0, "1.5", 0, 16, 1 << 20), FH_ERR_INVALID, "scale must be in (0, 1]"),
        ((MASH, 21, 1000, "0", 0, 0, 1 << 20), FH_ERR_INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
        ((MASH, 21, 1000, "0", 0, 16, 100), FH_ERR_INVALID, "max_records 1..1048576, stage_bytes 4 KiB..4 GiB"),
        ((MASH, 21, 10**9, "0", 0, 16, 1 << 20), 0, ""),
        ((SCALED, 1, 0, "1.0", 0, 1 << 20, 1 << 32), 0, ""),
        ((MASH, 32, 1, "0", 0, 1, 4096), 0, ""),
    ]
    for (c, code, msg), a in zip(cases, ask([("check",) + c for c, _, _ in cases])):
        assert int(a[0]) == code and " ".join(a[1:]) == msg, (c, a)
