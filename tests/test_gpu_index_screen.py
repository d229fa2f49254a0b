"""finch_index_screen on the GPU (include/finch_host.h).  Every case holds LibraryIndex.screen's rows and
figures against finch_screen_host, the contract in host code, byte for byte, and against tests/screen_model.py, the contract in
Python; the cases are those of tests/screen_cases.py plus what needs the device's own sketchers or the index's life."""
import gzip

import numpy as np
import pytest

import finch_rs_amd as F
import screen_cases as SC
import screen_model as SM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import SketchParams

pytestmark = pytest.mark.gpu

FIGURES = ("positions", "kmers", "hits", "distinct")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


def with_options(opts, fn):
    try:
        for o, v in opts.items():
            F.set_option(o, v)
        return fn()
    finally:
        for o in opts:
            F.set_option(o, None)


def screen_both(refs, inputs, text, k, seed=0, min_shared=1, opts=None, ix=None):
    """the device's (rows, figures) for `inputs`, held against the host's for `text`, the same sample as one image"""
    st, hst = {}, {}
    if ix is None:
        with H.LibraryIndex(refs) as own:
            rows = with_options(opts or {}, lambda: own.screen(inputs, k, seed, min_shared, stats=st))
    else:
        rows = with_options(opts or {}, lambda: ix.screen(inputs, k, seed, min_shared, stats=st))
    host = H.screen_host(refs, text, k, seed, min_shared, stats=hst)
    assert rows.dtype == H.SCREEN_DTYPE and rows.tobytes() == host.tobytes(), (rows, host)
    for f in FIGURES:
        assert st[f] == hst[f], (f, st, hst)
    return rows, st


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case(name):
    """window rules, strand, ownership of windows, multiplicity, lookup, every k at two seeds"""
    case = SC.case(name)
    refs = SC.build(case)
    text = b"".join(case.texts)
    rows, st = screen_both(refs, text, text, case.k, case.seed, case.min_shared, case.opts)
    SC.check(rows, st, case)
    if st["distinct"]:
        n_tiles = -(-(st["positions"] + len(SM.records(text))) // 2048)
        assert st["launches"] >= 1 and st["table_bytes"] >= 16 * st["distinct"] + 8 and st["kernel_ms"] > 0
        if "screen_piece" in case.opts:
            assert st["launches"] >= n_tiles * 2048 // case.opts["screen_piece"]
        else:
            assert st["launches"] == 1


def test_empty_input_on_an_index_with_a_device_entry():
    """b"" and [] against a library that has hashes: no rows, every figure 0 as the host's and the model's, nothing launched, and
    the screens around it are what they are alone"""
    full, empty = SC.case("extremes"), SC.case("empty_sample")
    refs = SC.build(full)
    zero = dict(positions=0, kmers=0, hits=0, distinct=0)
    assert SC.expect(SC.Case([b""], full.k, full.refs)) == ([], zero) and SC.expect(SC.Case([], full.k, full.refs)) == ([], zero)
    with H.LibraryIndex(refs) as ix:
        before, st0 = screen_both(refs, full.texts[0], full.texts[0], full.k, ix=ix)
        SC.check(before, st0, full)
        for inputs in (b"", []):
            rows, st = screen_both(refs, inputs, b"", full.k, ix=ix)
            assert len(rows) == 0 and rows.dtype == H.SCREEN_DTYPE
            assert st == dict(zero, table_bytes=0, table_ms=0.0, kernel_ms=0.0, launches=0)
        after, st1 = screen_both(refs, full.texts[0], full.texts[0], full.k, ix=ix)
        assert after.tobytes() == before.tobytes() and [st1[f] for f in FIGURES] == [st0[f] for f in FIGURES]
    assert SC.expect(empty) == ([], zero)


def test_junction_kmer_is_not_counted():
    rows, _ = SC.expect(SC.case("junction"))
    assert [r[0] for r in rows] == [1]  # (the model's own answer: the reference that holds only the junction's hash has no row)


def test_revcomp_sample_gives_the_forward_rows():
    f, r = SC.case("forward"), SC.case("revcomp")
    a, _ = screen_both(SC.build(f), f.texts[0], f.texts[0], f.k)
    b, _ = screen_both(SC.build(r), r.texts[0], r.texts[0], r.k)
    assert a.tobytes() == b.tobytes() and len(a) == 2


def test_homopolymer_is_one_hash():
    case = SC.case("homopolymer")
    rows, st = screen_both(SC.build(case), case.texts[0], case.texts[0], case.k)
    assert len(rows) == 1 and rows[0]["shared"] == 1 and rows[0]["sum_mult"] == 5001 - case.k == rows[0]["median_mult"]


def test_one_input_and_two_files(tmp_path):
    case = SC.case("two_files")
    refs = SC.build(case)
    paths = []
    for i, t in enumerate(case.texts):
        p = tmp_path / ("part%d.fa" % i)
        p.write_bytes(t)
        paths.append(str(p))
    text = b"".join(case.texts)
    one, st1 = screen_both(refs, text, text, case.k)
    two, st2 = screen_both(refs, paths, text, case.k)
    assert one.tobytes() == two.tobytes() and [st1[f] for f in FIGURES] == [st2[f] for f in FIGURES]
    SC.check(two, st2, case)
    (tmp_path / "whole.fa").write_bytes(text)
    assert screen_both(refs, str(tmp_path / "whole.fa"), text, case.k)[0].tobytes() == one.tobytes()


def test_input_forms_and_min_shared(tmp_path):
    """the same sample as FASTA, as FASTQ, gzip'd and as two files; min_shared 1, 5 and above every shared"""
    reads = [SC.S[o:o + 150] for o in range(0, 2850, 75)]
    fa, fq = SC.fasta(reads, width=60), SC.fastq(reads)
    m = SC.mult_of([fa], SC.K)
    hs = sorted(m)
    case = SC.Case([fa], SC.K, [SC.Ref(hs), SC.Ref(hs[:4]), SC.Ref(hs[10:16] + [3, 4]), SC.Ref([5, 6])])
    refs = SC.build(case)
    want, _ = SC.expect(case)
    with H.LibraryIndex(refs) as ix:
        base, st = screen_both(refs, fa, fa, SC.K, ix=ix)
        assert SM.rows_of(base) == want
        forms = {"fq": fq, "fa.gz": gzip.compress(fa), "fq.gz": gzip.compress(fq)}
        for name, image in forms.items():
            assert screen_both(refs, image, image, SC.K, ix=ix)[0].tobytes() == base.tobytes(), name
            (tmp_path / ("s." + name)).write_bytes(image)
            assert ix.screen(str(tmp_path / ("s." + name))).tobytes() == base.tobytes(), name
        half = len(reads) // 2
        (tmp_path / "a.fa").write_bytes(SC.fasta(reads[:half]))
        (tmp_path / "b.fq.gz").write_bytes(gzip.compress(SC.fastq(reads[half:])))
        assert ix.screen([str(tmp_path / "a.fa"), str(tmp_path / "b.fq.gz")]).tobytes() == base.tobytes()
        for ms in (1, 5, len(hs) + 1):
            rows, _ = screen_both(refs, fa, fa, SC.K, min_shared=ms, ix=ix)
            assert SM.rows_of(rows) == SC.expect(case, ms)[0]
        assert len(screen_both(refs, fa, fa, SC.K, min_shared=len(hs) + 1, ix=ix)[0]) == 0
        with pytest.raises(F.FinchError, match="no_such.fa: No such file"):
            ix.screen([str(tmp_path / "a.fa"), str(tmp_path / "no_such.fa")])
        with pytest.raises(F.FinchError, match="not a FASTA/FASTQ file"):
            ix.screen(b"ACGT\n")
        assert ix.screen(fa).tobytes() == base.tobytes()  # (a failed call leaves the index as it was)


def genomes(n, length, seed):
    return [SC.seq(length, seed + i) for i in range(n)]


def test_scaled_and_mash_libraries_over_the_same_genomes():
    gs = genomes(6, 20000, 300)
    sample = SC.fasta([gs[0][:6000], gs[2][3000:9000], gs[2][3000:5000], SC.seq(3000, 999)])
    ff = H.FilterParams(False)
    for params in (SketchParams.scaled(100000, SC.K, 0.01), SketchParams.mash(200, 200, False, SC.K)):
        refs = None
        for i, g in enumerate(gs):
            one = H.sketch_stream(SC.fasta([g]), "g%d" % i, params, ff)
            refs = one if refs is None else (refs.append(one) or refs)
        hashes = [[kc.hash for kc in refs.sketch(i).hashes] for i in range(len(refs))]
        rows, st = screen_both(refs, sample, sample, SC.K)
        want, wst = SM.screen(hashes, [sample], SC.K, 0)
        assert SM.rows_of(rows) == want and [st[f] for f in FIGURES] == [wst[f] for f in FIGURES]
        assert set(rows["reference"]) == {0, 2}
        with H.LibraryIndex(refs) as ix:  # (the parameters come from the library's sketches)
            assert ix.screen(sample).tobytes() == rows.tobytes()


def test_multiplicities_are_the_sketchers_counts():
    """mult of a library that holds every hash of the sample == the count column of a Mash sketch large enough to hold them all"""
    case = SC.case("repeats")
    text = case.texts[0]
    sk = H.sketch_stream(text, "s", SketchParams.mash(10 ** 6, 10 ** 6, True, case.k), H.FilterParams(False)).sketch(0)
    counts = {kc.hash: kc.count for kc in sk.hashes}
    assert counts == SC.mult_of(case.texts, case.k)
    hs = sorted(counts)
    single = SC.Case(case.texts, case.k, [SC.Ref([h]) for h in hs[:300]] + [SC.Ref(hs)])
    rows, _ = screen_both(SC.build(single), text, text, case.k)
    assert [int(x) for x in rows["sum_mult"][:300]] == [counts[h] for h in hs[:300]]
    assert int(rows["sum_mult"][300]) == sum(counts.values()) == sk.num_valid_kmers


def test_index_life():
    """after add and keep the screen is a fresh index's; two screens in a row; a search is the same bytes before and after"""
    t = SC._triple()
    text = t[0]
    hs = sorted(SC.mult_of(t, SC.K))
    first = SC.Case(t, SC.K, [SC.Ref(hs[:50]), SC.Ref(hs[40:200] + [9, 10]), SC.Ref([21, 22, 23])])
    more = SC.Case(t, SC.K, [SC.Ref(hs[100:400]), SC.Ref(hs[::7])])
    refs, extra = SC.build(first), SC.build(more)
    queries = SC.build(SC.Case(t, SC.K, [SC.Ref(hs[30:120]), SC.Ref(hs[::5])]))

    def fresh(sk):
        with H.LibraryIndex(sk) as other:
            return other.screen(text)

    with H.LibraryIndex(refs) as ix:
        before = ix.search(queries, 0.01)
        a = ix.screen(text)
        b = ix.screen(text)
        assert a.tobytes() == b.tobytes() == fresh(ix.refs).tobytes() and len(a) == 2
        after = ix.search(queries, 0.01)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        ix.add(extra)
        grown = ix.screen(text)
        assert len(ix.refs) == 5 and len(grown) == 4 and grown.tobytes() == fresh(ix.refs).tobytes()
        assert grown.tobytes() == H.screen_host(ix.refs, text, SC.K).tobytes()
        ix.keep([1, 2, 4])
        kept = ix.screen(text)
        assert kept.tobytes() == fresh(ix.refs).tobytes() == H.screen_host(ix.refs, text, SC.K).tobytes()
        assert [int(r) for r in kept["reference"]] == [0, 2] and kept[1]["ref_len"] == len(hs[::7])
        assert ix.search(queries, 0.01)[1].tobytes() == H.search(queries, ix.refs, 0.01)[1].tobytes()


@pytest.mark.parametrize("seed", (0, 42))
@pytest.mark.parametrize("k", range(1, 33))
def test_every_k_with_a_library_sketched_at_that_k(k, seed):
    """the sample of the k / seed cases against Mash sketches the device's own sketcher makes at that k and seed: of a genome the
    sample holds whole, and of an unrelated one; kmer_length and hash_seed come from the library"""
    case = SC.case("k%d_seed%d" % (k, seed))
    text = case.texts[0]
    params, ff = SketchParams.mash(100, 100, True, k, seed), H.FilterParams(False)
    refs = H.sketch_stream(SC.fasta([SC.S[:1500]]), "member", params, ff)
    refs.append(H.sketch_stream(SC.fasta([SC.seq(1500, 77)]), "other", params, ff))
    hashes = [[kc.hash for kc in refs.sketch(i).hashes] for i in range(2)]
    st = {}
    with H.LibraryIndex(refs) as ix:
        rows = ix.screen(text, stats=st)
    assert rows.tobytes() == H.screen_host(refs, text, k, seed).tobytes()
    want, wst = SM.screen(hashes, [text], k, seed)
    assert SM.rows_of(rows) == want and [st[f] for f in FIGURES] == [wst[f] for f in FIGURES]
    assert rows[0]["reference"] == 0 and rows[0]["shared"] == rows[0]["ref_len"] == len(hashes[0])
