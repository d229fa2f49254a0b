"""The host-side inflate (fh_inflate.h, fh_pargz.h) on the corpus of tests/deflate_writer.py: DEFLATE shapes zlib's encoder
never writes -- distances up to 32 768, long codes chosen on purpose, every header shape, the seams of the match copy --
must give zlib's text, and what zlib refuses must be refused here: through the BGZF batch reader, through the gzip
readers (the parallel one with chunks small enough for several, and the sequential one), and, under ASan + UBSan with
exact-size buffers, through the three decoders of tools/fuzz_inflate.cpp."""
import os
import shutil
import subprocess

import pytest

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError

import deflate_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READERS = [dict(pargz_chunk="4096", bgzf_threads="4"), dict(pargz="0")]


@pytest.fixture(scope="module")
def corpus():
    return W.corpus()


@pytest.fixture(autouse=True)
def options():
    yield
    F.debug_set(pargz_chunk=None, bgzf_threads=None, pargz=None)


def test_accepted_streams_as_bgzf_members(corpus):
    cases = [c for c in corpus.accepted if c.bgzf]
    assert len(cases) >= 13
    for c in cases:
        got, _, first = H.bgzf_batch_probe(W.bgzf_image([(c.raw, c.text)]), 1 << 20, 4096, 1 << 30, len(c.text) + 65536)
        assert got == c.text, c.id
        assert first == (c.text[0] if c.text else -1) or not c.text, c.id
    # all of them in one file, dealt out in small batches
    whole = b"".join(c.text for c in cases)
    img = W.bgzf_image([(c.raw, c.text) for c in cases])
    got, batches, _ = H.bgzf_batch_probe(img, 300_000, 3, 1 << 30, len(whole) + 65536)
    assert got == whole and batches > 1
    assert H.fastx_scan(img) == H.fastx_scan(whole)  # (the members of 1, 0 and 65 536 bytes among them, in that order)


@pytest.mark.parametrize("reader", range(len(READERS)))
def test_accepted_streams_as_gzip_files(corpus, reader):
    F.debug_set(**READERS[reader])
    for c in corpus.accepted + corpus.long:
        if not c.text:
            continue
        img = W.gzip_container(c.raw, c.text)
        assert H.source_probe(img, 1 << 20, len(c.text) + 4096) == c.text, c.id
        if c.fastq:
            assert H.fastx_scan(img) == H.fastx_scan(c.text), c.id
    want = H.fastx_scan(corpus.a9.text)
    for name, img in corpus.a9_images:
        assert H.fastx_scan(img) == want, name
        assert H.source_probe(img, 4096, len(corpus.a9.text) + 4096) == corpus.a9.text, name


def test_refused_streams_are_refused_by_every_reader(corpus):
    for cid, raw, text in corpus.refused:
        with pytest.raises(FinchError):
            H.bgzf_batch_probe(W.bgzf_image([(raw, text)]), 1 << 20, 4096, 1 << 30, len(text) + 65536)
        for opts in READERS:
            F.debug_set(**opts)
            with pytest.raises(FinchError):
                H.fastx_scan(W.gzip_container(raw, text))
            with pytest.raises(FinchError):
                H.source_probe(W.gzip_container(raw, text), 1 << 20, len(text) + 65536)
            F.debug_set(pargz_chunk=None, bgzf_threads=None, pargz=None)


def test_the_corpus_through_the_three_decoders_under_sanitizers(corpus, tmp_path):
    """tools/fuzz_inflate.cpp --corpus DIR: the one-shot, the streaming and the parallel decoder over NAME.deflate / NAME.txt
    pairs (text reproduced) and NAME.deflate alone (refused), every buffer at exactly its promised size"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_inflate")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "finch_rs_amd", "csrc"), os.path.join(ROOT, "tools", "fuzz_inflate.cpp"), "-lz", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-2000:]
    d = tmp_path / "corpus"
    d.mkdir()
    for c in corpus.accepted + corpus.long:
        (d / (c.id + ".deflate")).write_bytes(c.raw)
        (d / (c.id + ".txt")).write_bytes(c.text)
    for cid, raw, _ in corpus.refused:
        (d / (cid + ".deflate")).write_bytes(raw)
    r = subprocess.run([exe, "--corpus", str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "corpus: %d streams reproduced, %d refused, by all three decoders" % (len(corpus.accepted) + len(corpus.long), len(corpus.refused)) in r.stdout
