"""finch_sketch_records with the option records_stream=1 (H.sketch_records in a child process): the contract of
tests/test_gpu_sketch_records.py holds -- every sketch is H.sketch_stream of the record's own text, name and comment agree --
the bytes are those of the default routes, and the statistics say which records were streamed.  A child runs one function of
this file (`python tests/test_gpu_sketch_records_stream.py <case> <dir>`) under F.debug_env(...).  Needs a real MI355X (`-m gpu`)."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import finch_rs_amd as F  # noqa: E402
from finch_rs_amd import host as H  # noqa: E402
from finch_rs_amd.sketch_schemes import FinchError, SketchParams  # noqa: E402
from test_gpu_sketch_records import OFF, assert_contract, seq, split, wrap  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_POS, BOUND, CAP = 8192, 1 << 24, 1024
LENGTHS = (900, 8192, 8193, 12000, 30000, 70000)
MASH = SketchParams.mash(1000, 1000, True, 21, 0)
PARAMS = {
    "mash": MASH,
    "mash-k40": SketchParams.mash(500, 500, True, 40, 5),
    "allcounts-k4": SketchParams.all_counts(4),
    "mash-cut-to-100": SketchParams.mash(2000, 100, True, 16, 42),
    "mash-2000": SketchParams.mash(2000, 2000, True, 21, 0),
    "scaled-0.001": SketchParams.scaled(0, 31, 0.001, 3),
    "scaled-scale1": SketchParams.scaled(10, 21, 1.0, 0),
}


def make_fasta(seed=60, n_records=60):
    rng = np.random.default_rng(seed)
    parts, lengths = [], []
    for i in range(n_records):
        n = int(LENGTHS[i % 6] if i < 12 else rng.choice(LENGTHS))
        eol = b"\r\n" if i % 5 == 0 else b"\n"
        hdr = [b"rec%d" % i, b"rec%d some comment" % i, b"rec%d\tkey=value  x" % i][i % 3]
        parts.append(b">" + hdr + eol + wrap(seq(rng, n), 70 if i % 3 else 1 << 20, eol))
        lengths.append(n)
    return b"".join(parts), lengths


def digest(res, st):
    return {"sha": hashlib.sha256(res.to_json().encode()).hexdigest(), "st": {k: v for k, v in st.items() if not k.endswith("_ms")}}


# ---- what a child does (the options are in its environment) ----
def child_contract(d, name):
    text = open(os.path.join(d, "lib.fa"), "rb").read()
    st = {}
    res = H.sketch_records(os.path.join(d, "lib.fa"), PARAMS[name], stats=st)
    assert_contract(res, text, PARAMS[name])
    streamed, stream_ms, stream_launches = H.records_stream_stats()
    assert sorted(st) == ["in_lds", "kernel_ms", "launches", "one_by_one", "records", "streamed"] and st["streamed"] == streamed
    assert stream_ms <= st["kernel_ms"] + 1e-6 and stream_launches <= st["launches"]
    assert (stream_launches > 0) == (stream_ms > 0) and (stream_launches > 0 or streamed == 0)
    return digest(res, dict(st, stream_launches=stream_launches))


def child_inputs(d, name):
    out = {}
    text = open(os.path.join(d, "lib.fa"), "rb").read()
    for key, inp, kw in (("path", os.path.join(d, "lib.fa"), {}), ("gz", os.path.join(d, "lib.fa.gz"), {}), ("bytes", text, {}), ("t1", text, {"n_threads": 1}),
                         ("t4", text, {"n_threads": 4}), ("dev00", text, {"n_threads": 4, "devices": (0, 0)})):
        st = {}
        out[key] = digest(H.sketch_records(inp, MASH, stats=st, **kw), st)
    return out


def child_strict(d, name):
    rng = np.random.default_rng(3)
    ns = seq(rng, 9000, 0).replace(b"A", b"N").replace(b"C", b"N").replace(b"G", b"N")  # a long record with few k-mers
    text = b">long1\n" + seq(rng, 20000, 0) + b"\n>big a comment\n" + ns + b"\n>long2\n" + seq(rng, 20000, 0) + b"\n"
    strict = SketchParams.mash(1000, 1000, False, 21, 0)
    msgs = []
    for fn in (lambda: H.sketch_records(text, strict, n_threads=2), lambda: H.sketch_stream(split(text)[1][0], "big", strict, OFF)):
        try:
            fn()
            msgs.append(None)
        except FinchError as e:
            msgs.append(str(e))
    return {"msgs": msgs}


CHILD = {"contract": child_contract, "inputs": child_inputs, "strict": child_strict}


def child(case, d, name="mash", **opts):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(d), name], env=F.debug_env(**opts), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("records_stream")
    text, lengths = make_fasta()
    (d / "lib.fa").write_bytes(text)
    (d / "lib.fa.gz").write_bytes(gzip.compress(text, 1))
    return d, text, lengths


def here(text, params, **kw):
    st = {}
    return digest(H.sketch_records(text, params, stats=st, **kw), st)


def test_streamed_records_are_their_own_sketch_stream(lib):
    d, text, lengths = lib
    got = child("contract", d, records_stream=1)
    long_ones = sum(1 for n in lengths if MAX_POS < n <= BOUND)
    assert long_ones >= 8 and got["st"]["streamed"] == long_ones and got["st"]["one_by_one"] == 0
    assert got["st"]["in_lds"] + got["st"]["one_by_one"] == got["st"]["records"] == 60
    # the bytes of the default routes, whose statistics say that nothing was streamed
    dflt = here(text, MASH)
    assert got["sha"] == dflt["sha"]
    assert dflt["st"]["streamed"] == 0 and H.records_stream_stats() == (0, 0.0, 0) and dflt["st"]["one_by_one"] == long_ones


def test_max_pos_option_bounds_the_route(lib):
    d, text, lengths = lib
    got = child("contract", d, records_stream=1, records_stream_max_pos=20000)
    assert got["st"]["streamed"] == sum(1 for n in lengths if MAX_POS < n <= 20000)
    assert got["st"]["one_by_one"] == sum(1 for n in lengths if n > 20000) > 0
    assert got["sha"] == here(text, MASH)["sha"]


def test_folding_behind_every_round_changes_nothing(lib):
    d, text, lengths = lib
    got = child("contract", d, records_stream=1, records_stream_fold=1)
    assert got["st"]["streamed"] == sum(1 for n in lengths if n > MAX_POS) and got["sha"] == here(text, MASH)["sha"]


@pytest.mark.parametrize("name", [n for n in sorted(PARAMS) if n != "mash"])
def test_other_parameters(lib, name):
    d, text, lengths = lib
    got = child("contract", d, name, records_stream=1)
    st = got["st"]
    long_ones = sum(1 for n in lengths if n > MAX_POS)
    assert st["in_lds"] + st["one_by_one"] == st["records"] == 60
    assert got["sha"] == here(text, PARAMS[name])["sha"]
    if name in ("mash-k40", "allcounts-k4", "mash-2000"):  # k > 32, AllCounts, a Mash size above the cap: nothing is streamed
        assert st["streamed"] == 0 and st["stream_launches"] == 0 and st["one_by_one"] >= long_ones
    elif name == "scaled-scale1":  # every long record keeps more hashes than the cap: launched, not taken, one by one, exact
        assert st["streamed"] == 0 and st["stream_launches"] > 0 and st["one_by_one"] == long_ones
    else:
        assert st["streamed"] == long_ones and st["one_by_one"] == 0


def test_inputs_workers_and_devices(lib):
    d, text, lengths = lib
    got = child("inputs", d, records_stream=1)
    sha = here(text, MASH)["sha"]
    long_ones = sum(1 for n in lengths if n > MAX_POS)
    for key, v in got.items():
        assert v["sha"] == sha and v["st"]["streamed"] == long_ones and v["st"]["one_by_one"] == 0, key


def test_strict_mode_error_of_a_long_record(lib):
    d, _, _ = lib
    msgs = child("strict", d, records_stream=1)["msgs"]
    assert msgs[0] is not None and msgs[0] == msgs[1] and msgs[0].startswith("big had too few kmers (")


if __name__ == "__main__":
    assert F.get_option("records_stream") == "1"
    print(json.dumps(CHILD[sys.argv[1]](sys.argv[2], sys.argv[3])))
