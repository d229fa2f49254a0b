"""One sketch per record of a FASTA input (finch_sketch_records through H.sketch_records): sketch j is, field for field, what
H.sketch_stream(text_j, name_j, ...) returns for the record's own text -- hashes, k-mer bytes, counts, extra counts, seq_length,
num_valid_kmers, filter_params -- with the name and the comment taken from the header by the rule; whichever route a record
takes (a workgroup's LDS, or one by one) and however the records are dealt to workers, the answer is the same.  text_j is cut
out of the input HERE, by a regular expression over line starts.  Needs a real MI355X (`-m gpu`)."""
import gzip
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError, SketchParams

pytestmark = pytest.mark.gpu

MAX_POS = 8192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = H.FilterParams(False)


def seq(rng, n, p_noise=0.002):
    r = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    m = rng.random(n)
    r[m > 0.98] |= 0x20
    bad = m < p_noise
    r[bad] = rng.choice(np.frombuffer(b"NRYn", dtype=np.uint8), size=int(bad.sum()))
    return bytes(r)


def wrap(s: bytes, width: int, eol: bytes) -> bytes:
    return b"".join(s[i:i + width] + eol for i in range(0, len(s), width)) if s else b""


def make_fasta(seed, n_records=300):
    """-> (text, lengths): mixed short and long records, above the bound too; multi-line and one-line; CR LF; duplicated ids; tabs
    and runs of blanks in the headers; header-only records; no final line end"""
    rng = np.random.default_rng(seed)
    parts, lengths = [], []
    for i in range(n_records):
        n = int(rng.choice([0, 30, 200, 900, 1500, 1500, 1800, 3000, 6000, MAX_POS - 1, MAX_POS, MAX_POS + 1, 12000, 30000],
                           p=[.03, .04, .1, .12, .2, .15, .1, .1, .06, .02, .02, .02, .02, .02]))
        eol = b"\r\n" if i % 5 == 0 else b"\n"
        hdr = [b"rec%d" % (i % 250), b"rec%d some comment" % i, b"rec%d\tkey=value  x" % i, b"rec%d   " % i, b""][i % 5 if i % 50 else 4]
        parts.append(b">" + hdr + eol + (wrap(seq(rng, n), 60 if i % 3 else 1 << 20, eol)))
        lengths.append(n)
    text = b"".join(parts)
    return text[:-1] if text.endswith(b"\n") else text, lengths


def split(text: bytes):
    """text_j, name_j, comment_j of every record, by the contract's words"""
    starts = [m.start() for m in re.finditer(rb"(?:\A|(?<=\n))>", text)]
    out = []
    for a, b in zip(starts, starts[1:] + [len(text)]):
        t = text[a:b]
        line = t[1:].split(b"\n", 1)[0]
        if line.endswith(b"\r"):
            line = line[:-1]
        m = re.match(rb"([^ \t]*)[ \t]*(.*)\Z", line, re.S)
        out.append((t, m.group(1).decode(), m.group(2).decode()))
    return out


def assert_contract(res, text, params, filters=OFF):
    recs = split(text)
    assert len(res) == len(recs)
    for j, (t, name, comment) in enumerate(recs):
        want = H.sketch_stream(t, name, params, filters).sketch(0)
        got = res.sketch(j)
        c = "record %d (%r, %d bytes)" % (j, name, len(t))
        assert got.name == name and res.comment(j) == comment, c
        assert (got.seq_length, got.num_valid_kmers) == (want.seq_length, want.num_valid_kmers), c
        assert np.array_equal(got.arrays[0], want.arrays[0]) and np.array_equal(got.arrays[1], want.arrays[1]), c
        assert got.filter_params == want.filter_params, c
        if j % 37 == 0:  # (sketch_params as the library holds them)
            assert res.params_of(j) == H.sketch_stream(t, name, params, filters).params_of(0), c
    return recs


@pytest.fixture(scope="module")
def fasta():
    return make_fasta(11)


MASH = SketchParams.mash(1000, 1000, True, 21, 0)


def test_every_record_is_its_own_sketch_stream(fasta, tmp_path):
    text, lengths = fasta
    plain, gz = tmp_path / "lib.fa", tmp_path / "lib.fa.gz"
    plain.write_bytes(text)
    gz.write_bytes(gzip.compress(text, 1))
    st = {}
    res = H.sketch_records(str(plain), MASH, stats=st)
    recs = assert_contract(res, text, MASH)
    assert len(recs) == 300
    # the routes: every record within the bound went through LDS (random records have no 64-bit collision), the others one by one
    above = sum(1 for n in lengths if n > MAX_POS)
    assert above >= 3 and st["records"] == 300 and st["in_lds"] + st["one_by_one"] == st["records"]
    assert st["one_by_one"] == above and st["launches"] >= 1 and st["kernel_ms"] > 0
    # the same file gzip'd, and as bytes: the same sketches
    st2 = {}
    assert H.sketch_records(str(gz), MASH, stats=st2).to_json() == res.to_json() and st2["in_lds"] == st["in_lds"]
    assert H.sketch_records(text, MASH).to_json() == res.to_json()
    assert H.sketch_records(gzip.compress(text, 1), MASH, filters=H.FilterParams(None)).to_json() == res.to_json()


def test_order_workers_and_devices(fasta, tmp_path):
    text, _ = fasta
    text2, _ = make_fasta(12, 40)
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_bytes(text)
    b.write_bytes(text2)
    ref = H.sketch_records([str(b), str(a)], MASH, n_threads=1)
    names = [n for _, n, _ in split(text2)] + [n for _, n, _ in split(text)]
    assert [ref.sketch(j).name for j in range(len(ref))] == names
    assert len(ref) == 340
    for kw in ({"n_threads": 4}, {"n_threads": 4, "devices": (0, 0)}, {"n_threads": 3, "devices": (0, 0, 0)}):
        assert H.sketch_records([str(b), str(a)], MASH, **kw).to_json() == ref.to_json(), kw


def test_records_lds_off_gives_the_same_bytes(fasta, tmp_path):
    text, _ = fasta
    p = tmp_path / "lib.fa"
    p.write_bytes(text)
    code = r'''
import hashlib, sys
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import SketchParams
st = {}
res = H.sketch_records(sys.argv[1], SketchParams.mash(1000, 1000, True, 21, 0), stats=st)
print(hashlib.sha256(res.to_json().encode()).hexdigest(), st["in_lds"], st["one_by_one"], st["records"])
'''
    r = subprocess.run([sys.executable, "-c", code, str(p)], env=F.debug_env(records_lds=0), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    sha, in_lds, one, n = r.stdout.split()[-4:]
    st = {}
    here = H.sketch_records(str(p), MASH, stats=st)
    assert (int(in_lds), int(one), int(n)) == (0, 300, 300) and st["in_lds"] > 0
    assert sha == hashlib.sha256(here.to_json().encode()).hexdigest()


def test_strict_mode_fails_on_the_first_short_record():
    rng = np.random.default_rng(3)
    text = b">long1\n" + seq(rng, 3000, 0) + b"\n>shorty a comment\n" + seq(rng, 520, 0) + b"\n>shorter\n" + seq(rng, 100, 0) + b"\n>long2\n" + seq(rng, 20000, 0) + b"\n"
    strict = SketchParams.mash(1000, 1000, False, 21, 0)
    with pytest.raises(FinchError) as ei:
        H.sketch_records(text, strict)
    assert str(ei.value) == "shorty had too few kmers (500) to sketch"
    # ... which is what the record's own text says through sketch_stream
    with pytest.raises(FinchError) as e2:
        H.sketch_stream(split(text)[1][0], "shorty", strict, OFF)
    assert str(e2.value) == str(ei.value)
    # the first failing record wins whichever route it takes (here the first is one that goes one by one)
    text2 = b">big\n" + seq(rng, 9000, 0)[:9000].replace(b"A", b"N").replace(b"C", b"N").replace(b"G", b"N") + b"\n" + text
    with pytest.raises(FinchError) as e3:
        H.sketch_records(text2, strict, n_threads=2)
    assert str(e3.value).startswith("big had too few kmers (")
    res = H.sketch_records(text, SketchParams.mash(1000, 1000, True, 21, 0))
    assert [len(res.sketch(j).hashes) for j in range(4)] == [1000, 500, 80, 1000]


@pytest.mark.parametrize("params", [SketchParams.mash(500, 500, True, 40, 5), SketchParams.all_counts(4), SketchParams.mash(2000, 100, True, 16, 42),
                                    SketchParams.scaled(10, 21, 0.01, 0), SketchParams.scaled(0, 31, 0.001, 3), SketchParams.scaled(2000, 11, 1.0, 0)],
                         ids=["mash-k40", "allcounts-k4", "mash-cut-to-100", "scaled-0.01", "scaled-size0", "scaled-scale1"])
def test_other_parameters(params):
    text, lengths = make_fasta(21, 40)
    st = {}
    res = H.sketch_records(text, params, stats=st)
    assert_contract(res, text, params)
    assert st["in_lds"] + st["one_by_one"] == st["records"] == 40
    if params.kmer_length > 32 or params.kind == "allcounts":
        assert st["in_lds"] == 0 and st["launches"] == 0  # the long way
    else:
        assert st["in_lds"] == sum(1 for n in lengths if n <= MAX_POS)


def test_the_sketches_feed_the_library_index():
    rng = np.random.default_rng(8)
    text = b"".join(b">p%d plasmid %d\n%s\n" % (i, i, wrap(seq(rng, int(rng.integers(1200, 5000)), 0), 70, b"\n")) for i in range(60))
    res = H.sketch_records(text, MASH)
    with H.LibraryIndex(res) as ix:
        offsets, rows = ix.search(res, 0.5, top_n=1)
    assert len(rows) == 60 and np.array_equal(rows["query"], np.arange(60)) and np.array_equal(rows["reference"], np.arange(60))
