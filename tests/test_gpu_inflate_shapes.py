"""GPU tests of the device-side inflate (fh_bgzf.hip) on DEFLATE streams zlib's encoder never writes: the corpus of
tests/deflate_writer.py -- distances 32 507..32 768, codes of 9..15 bits chosen on purpose, every header shape, the seams of
copy_match, chains of matches that read the token before them, token groups around the size of the LDS ring, blocks of
every kind and size.  test_deflate_writer.py has zlib's verdict on each stream; here the text the kernels produce is
checked through its sketch against the oracle's sketch of zlib's text (the oracle never sees a stream), as BGZF members
(fh_push_bgzf_fastq) and as plain gzip (fh_push_gzip_fastq, finch_sketch_files), and what zlib refuses must be refused.
Run with -m gpu."""
import os
import subprocess
import sys
import zlib

import pytest

import finch_rs_amd as F

from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError, SketchParams
from oracle import oracle as O

import deflate_writer as W
from test_gpu_bgzf_device import assert_is_oracle_sketch, new_sketcher, push_members
from test_gpu_gzip_device import push_stream, sketch_of

pytestmark = pytest.mark.gpu

K, SIZE = 21, 500
ACCEPTED = ["A1", "A2", "A3", "A4", "A5a", "A5b", "A6", "A7", "A7e", "A7s", "A8", "A9"]  # (the ids with fastq=True, in order)
MEMBER_SIZES = ["A7m1", "A7m0", "A7m65536"]  # one FASTQ file together: members of 1, 0 and 65 536 bytes
_oracles = {}


@pytest.fixture(scope="module")
def corpus():
    c = W.corpus()
    assert [x.id for x in c.accepted if x.fastq] == ACCEPTED and [x.id for x in c.accepted if not x.fastq] == MEMBER_SIZES
    return c


@pytest.fixture
def chunk_env():
    yield
    F.debug_set(gz_chunk=None)


def oracle_of(key, text):
    """the oracle's sketch of a text, computed once"""
    if key not in _oracles:
        o = O.OracleSketcher(O.MASH, SIZE, K, 0, 0.001)
        assert o.sketch_stream(text) == 2  # (FASTQ)
        assert o.total_bases_and_kmers()[1] > 0
        _oracles[key] = o
    return _oracles[key]


def gzip_body(c):
    return c.raw + (zlib.crc32(c.text) & 0xFFFFFFFF).to_bytes(4, "little") + (len(c.text) & 0xFFFFFFFF).to_bytes(4, "little")


# ---------------------------------------------------------------------------------------------------------------------
# BGZF members: decoded from the first bit to the last, no design limit -- a refusal of an accepted stream is a bug
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ACCEPTED)
def test_bgzf_member_of_every_accepted_shape(corpus, cid):
    c = corpus.by_id[cid]
    sk = new_sketcher(SIZE, K)
    push_members(sk, [c.text], [c.raw], 1)
    assert_is_oracle_sketch(sk, oracle_of(cid, c.text))
    sk.close()


@pytest.mark.parametrize("batch", [1, 64])
def test_bgzf_members_of_all_shapes_in_one_file(corpus, batch):
    cases = [corpus.by_id[i] for i in ACCEPTED[:6] + MEMBER_SIZES + ACCEPTED[6:]]
    text = b"".join(c.text for c in cases)
    sk = new_sketcher(SIZE, K)
    push_members(sk, [c.text for c in cases], [c.raw for c in cases], batch)
    assert_is_oracle_sketch(sk, oracle_of("all", text))
    sk.close()


def serial_child(select):
    """option bgzf_serial (read once per process, hence the child): tests of this file through the A/B variant of the inflate
    kernel's symbol loop"""
    if "bgzf_serial" in os.environ.get("FH_DEBUG", ""):
        pytest.skip("this is the child")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", select],
                       env=F.debug_env(bgzf_serial="1"), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:]


def test_bgzf_members_under_the_one_symbol_at_a_time_loop():
    serial_child("test_bgzf_member_of or test_bgzf_members_of")


# ---------------------------------------------------------------------------------------------------------------------
# plain gzip: chunks, block starts found by search, marker windows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1024, 4096, None])
def test_gzip_stream_of_every_accepted_shape(corpus, chunk, chunk_env):
    F.debug_set(gz_chunk=None if chunk is None else str(chunk))
    for cid in ACCEPTED:
        c = corpus.by_id[cid]
        sk = new_sketcher(SIZE, K)
        done, trailing, _ = push_stream(sk, gzip_body(c))
        assert (done, trailing) == (1, 0), (cid, chunk)
        assert_is_oracle_sketch(sk, oracle_of(cid, c.text))
        sk.close()


@pytest.mark.parametrize("cid", ["L1", "L2"])
def test_a_byte_carried_through_many_chunk_windows(corpus, cid, chunk_env):
    """L1: the first 12 KiB of every period of 32 768 are matches at distance 32 768 -- a byte of period 0 reaches the text's
    end through seven copies, every one out of a chunk's unknown window (marker slots 0..12 287 among them); L2: a chain of
    1 200 matches, each reading the one before, across more than four chunks of 1 024 bytes"""
    c = corpus.by_id[cid]
    assert len(c.raw) >= 64 * 1024
    for chunk in ("1024", "4096", None):
        F.debug_set(gz_chunk=chunk)
        sk = new_sketcher(SIZE, K)
        done, trailing, _ = push_stream(sk, gzip_body(c))
        assert (done, trailing) == (1, 0), (cid, chunk)
        assert_is_oracle_sketch(sk, oracle_of(cid, c.text))
        sk.close()


def test_sketch_files_takes_the_far_distances_and_every_gzip_header_through_the_device(corpus, tmp_path, chunk_env):
    p = SketchParams.mash(SIZE, SIZE, True, K, 0)
    a1 = corpus.by_id["A1"]
    files = [("a1.fastq.gz", W.gzip_container(a1.raw, a1.text), a1)] + [("a9_%s.fastq.gz" % n, img, corpus.a9) for n, img in corpus.a9_images]
    for name, img, c in files:
        o = oracle_of(c.id, c.text)
        okc, okm = o.to_vec()
        want = (okc.tobytes(), okm.tobytes()) + o.total_bases_and_kmers()
        path = str(tmp_path / name)
        open(path, "wb").write(img)
        before = H.debug_device_gzip()
        got = sketch_of(path, p, n_threads=4)
        after = H.debug_device_gzip()
        assert got == want, name
        assert (after[0] - before[0], after[1] - before[1]) == (1, 0), name  # taken by the device, not read again
        assert sketch_of(path, p, device_gzip=False, n_threads=4) == want, name


# ---------------------------------------------------------------------------------------------------------------------
# what zlib refuses
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_as_bgzf_members_and_the_handle_lives_on(corpus):
    """Every refused stream is one valid fixed block and then one fault; none of them can index past a table before it is
    refused (read from the code before the first run):
      * read_dynamic_header: HLIT / HDIST come from 5-bit fields, so hlit + hdist <= 288 + 32 = 320 = sizeof L.lens even before
        the 286 / 30 test refuses the four oversize headers; a length is stored at L.lens[i] only while i < n, and a run only
        after `i + rep > n` has been tested (R_run_overruns, R_16_first: i == 0); cl_lens[sym] has sym < 32 = its size.
      * build_table: counts index cs.count[0..15] by a length <= 15 (3-bit / 4-bit sources); an over-subscribed or incomplete
        set returns before `sorted` or the table is written; otherwise offs[l] + rank < n <= 288 = sizeof sorted, and
        table indices are masked to the root's size.  decode_long reads sorted[offs[l] + idx] with idx < count[l] only.
      * block_symbols_parallel: table lookups are masked to 10 / 8 bits; an entry of an absent code (LIT_STOP / 0) ends the
        chain with BZ_BAD_CODE (symbols 286 / 287, distance symbols 30 / 31, the missing end-of-block); a distance is tested
        against the lane's output position before anything is queued (R_far_*), the output size before the queue is written;
        the stream is read at most 24 bytes past the member (mbits <= in_bits + 64 is tested every round), inside the
        staging buffer's padding like every member the existing tests push.
    Block type 3 and the stored length check are refused where the block header is read."""
    good = corpus.by_id["A9"]
    sk = new_sketcher(SIZE, K)
    for cid, raw, text in corpus.refused:
        with pytest.raises(_lib.FinchHipError) as ei:
            push_members(sk, [text], [raw], 1)
        assert ei.value.code == -1 and "BGZF member 0" in str(ei.value), cid  # FH_ERR_INVALID
        sk.reset()
    push_members(sk, [good.text], [good.raw], 1)
    assert_is_oracle_sketch(sk, oracle_of(good.id, good.text))
    sk.close()


def test_refused_under_the_one_symbol_at_a_time_loop():
    serial_child("test_refused_as_bgzf_members")


def test_refused_as_gzip_streams_and_the_handle_lives_on(corpus, chunk_env):
    good = corpus.by_id["A9"]
    F.debug_set(gz_chunk="4096")
    sk = new_sketcher(SIZE, K)
    for cid, raw, text in corpus.refused:
        body = raw + (zlib.crc32(text) & 0xFFFFFFFF).to_bytes(4, "little") + len(text).to_bytes(4, "little")
        with pytest.raises(_lib.FinchHipError):
            push_stream(sk, body)
        sk.reset()
    assert push_stream(sk, gzip_body(good))[:2] == (1, 0)
    assert_is_oracle_sketch(sk, oracle_of(good.id, good.text))
    sk.close()


def test_refused_files_get_the_same_error_with_the_device_pass_on_and_off(corpus, tmp_path):
    p = SketchParams.mash(SIZE, SIZE, True, K, 0)
    for cid, raw, text in corpus.refused:
        path = str(tmp_path / (cid + ".fastq.gz"))
        open(path, "wb").write(W.gzip_container(raw, text))
        errs = []
        for dev in (True, False):
            with pytest.raises(FinchError) as e:
                sketch_of(path, p, device_gzip=dev, n_threads=4)
            errs.append(str(e.value))
        assert errs[0] == errs[1], cid
