"""finch_minmer_matrix on the device against tests/matrix_model.py (distance.rs:345-364 as written): every matrix equal cell for
cell and int32, over the corners of the contract, the edges of the kernel's column blocks (256 lanes x 4 columns = 1024 per
workgroup), many LDS slices per sketch, many chunks over both result buffers and several device entries, random overlapping
sketches, and sketches the sketcher made."""
import ctypes

import numpy as np
import pytest

import finch_rs_amd as F
import matrix_inputs as I
import matrix_model as M
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import SketchParams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if F.device_count() < 1:
        pytest.skip("needs a GPU")


class options:
    """matrix_slice / matrix_chunk_rows for the calls inside, back to unset behind them"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            F.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            F.set_option(k, None)


def check(ref, sketches, want=None, refs_handle=None, sk_handle=None, **kw):
    """the library's matrix of `sketches` against reference `ref` == the model's"""
    want = M.minmer_matrix(ref[0], sketches) if want is None else want
    refs_handle = refs_handle or I.handle([ref], ["ref"])
    sk_handle = sk_handle or I.handle(sketches)
    got = H.minmer_matrix(refs_handle, 0, sk_handle, **kw)
    assert got.dtype == np.int32 and got.shape == (len(sketches), len(ref[0])) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    return got


def test_hand_made():
    assert np.array_equal(check(I.HAND_REF, I.HAND_SKETCHES), I.HAND_WANT)
    assert np.array_equal(check(I.HAND_REF_INNER, I.HAND_SKETCHES), I.HAND_WANT_INNER)
    # the reference is one of the sketches of the same handle: that row is its own counts
    both = [I.HAND_REF] + I.HAND_SKETCHES
    sk = I.handle(both)
    got = check(I.HAND_REF, both, refs_handle=sk, sk_handle=sk)
    assert np.array_equal(got[0], H.counts(sk, 0)) and got[0].tolist() == [7, 0, -(1 << 31), -1, 1]


@pytest.fixture(scope="module")
def pool_case():
    """a pool of 2600 hashes, four sketches drawn from it (one empty), and their handle"""
    rng = np.random.default_rng(77)
    pool = I.hash_pool(rng, 2600)
    sketches = I.pool_sketches(rng, pool, [0, 1, 700, 2600])
    return rng, pool, sketches, I.handle(sketches)


@pytest.mark.parametrize("n_ref", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_column_block_edges(pool_case, n_ref):
    rng, pool, sketches, sk = pool_case
    for ref_hashes in (pool[:n_ref], np.sort(rng.choice(pool, n_ref, replace=False))):
        stats = {}
        got = check((ref_hashes, np.ones(n_ref, np.uint32)), sketches, sk_handle=sk, stats=stats)
        assert stats["launches"] == 1 and stats["kernel_ms"] > 0
        assert np.count_nonzero(got[3]) >= n_ref - 1  # (the whole pool: every column matches, bar a count of 0)


@pytest.mark.parametrize("slice_", [1, 2, 3, 64, 128, 129, 130])
def test_slices(slice_):
    """a 130-hash sketch walked in slices of every size that changes the walk; the reference holds every one of its hashes (a match
    on the first and the last entry of every slice) with a stranger below, between every two and above"""
    hs = np.arange(130, dtype=np.uint64) * 10 + 5
    cs = np.arange(130, dtype=np.uint32) + 1
    cs[[0, 63, 64, 127, 128, 129]] = [1 << 31, I.U32_MAX, 0, 2, I.U32_MAX - 1, 3]
    ref = np.sort(np.concatenate([hs, hs - 3, [hs[-1] + 4]]).astype(np.uint64))
    sketches = [(hs, cs), (hs[::19], cs[::19]), ([], []), (hs[:129], cs[:129])]
    with options(matrix_slice=slice_):
        got = check((ref, np.ones(len(ref), np.uint32)), sketches)
    assert np.array_equal(got[0][1::2][:130].view(np.uint32), cs)
    # only some slices hold a match, among them the last entry of one and the first of the next
    few = (hs[[0, 63, 64, 129]], np.ones(4, np.uint32))
    with options(matrix_slice=slice_):
        check(few, sketches)


@pytest.mark.parametrize("devices", [(0,), (0, 0, 0)])
@pytest.mark.parametrize("chunk_rows", [1, 2, 5])
def test_chunks(chunk_rows, devices):
    rng = np.random.default_rng(5)
    pool = I.hash_pool(rng, 90)
    sketches = I.pool_sketches(rng, pool, [40, 0, 90, 1, 33])
    ref = (pool[::2], np.ones(45, np.uint32))
    stats = {}
    with options(matrix_chunk_rows=chunk_rows):
        check(ref, sketches, devices=devices, stats=stats)
    assert stats["launches"] == -(-5 // chunk_rows)


@pytest.fixture(scope="module", params=[1, 2, 3])
def random_case(request):
    """40 sketches of 0..300 hashes and a 200-hash reference out of one pool of 500: dense overlap; the model's matrix, once"""
    rng = np.random.default_rng(request.param)
    pool = I.hash_pool(rng, 500)
    sketches = I.pool_sketches(rng, pool, rng.integers(0, 301, 40))
    ref = I.pool_sketches(rng, pool, [200])[0]
    want = M.minmer_matrix(ref[0], sketches)
    want.setflags(write=False)
    assert np.count_nonzero(want) > 1000
    return ref, sketches, want, I.handle([ref]), I.handle(sketches)


@pytest.mark.parametrize("opts", [{}, {"matrix_slice": 7, "matrix_chunk_rows": 3}], ids=["defaults", "slice7_rows3"])
def test_random(random_case, opts):
    ref, sketches, want, rh, sh = random_case
    with options(**opts):
        a = check(ref, sketches, want, rh, sh)
        b = check(ref, sketches, want, rh, sh)
    assert np.array_equal(a, b)


def test_real_sketches():
    rng = np.random.default_rng(9)
    g = "".join("ACGT"[i] for i in rng.integers(0, 4, 3000))
    fa1 = (">one\n%s\n>again\n%s\n" % (g[:2000], g[300:900])).encode()  # a stretch seen twice: counts of 2
    fa2 = (">two\n%s\n" % g[1000:]).encode()
    p = SketchParams.mash(100, 100, False, 21, 0)
    sk = H.sketch_stream(fa1, "one", p, H.FilterParams(False))
    sk.append(H.sketch_stream(fa2, "two", p, H.FilterParams(False)))
    arrays = [sk.sketch(i).arrays[0] for i in range(2)]
    sketches = [(a["hash"], a["count"]) for a in arrays]
    assert [len(h) for h, _ in sketches] == [100, 100] and sketches[0][1].max() >= 2
    for ir in (0, 1):
        got = H.minmer_matrix(sk, ir, sk)
        assert got.dtype == np.int32 and np.array_equal(got, M.minmer_matrix(sketches[ir][0], sketches))
        assert np.array_equal(got[ir], H.counts(sk, ir)) and got[ir].min() >= 1
    assert 0 < np.count_nonzero(H.minmer_matrix(sk, 0, sk)[1]) < 100  # the two share some hashes, not all


def test_refusals_with_a_device_and_the_callers_device():
    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime the library is linked against: already loaded)

    def current_device():
        d = ctypes.c_int(-1)
        assert hip.hipGetDevice(ctypes.byref(d)) == 0
        return d.value
    mine = 1 if F.device_count() > 1 else 0
    assert hip.hipSetDevice(mine) == 0
    try:
        for what, args, words in I.refusals():
            rc, msg = I.raw_call(*args)
            assert rc == _lib.FH_ERR_INVALID, (what, rc, msg)
            assert msg.startswith(words[0]) and all(w in msg for w in words), (what, msg)
            assert current_device() == mine
        some = I.handle([([1, 5, 9], [1, 2, 3]), ([2, 9], [1, 7])])
        rc, msg = I.raw_call(some, 0, some, np.zeros(6, np.int32), 6, devices=(0, 4096))
        assert rc == _lib.FH_ERR_NO_DEVICE and "device 4096 requested" in msg and current_device() == mine
        with options(matrix_chunk_rows=1):
            assert H.minmer_matrix(some, 0, some, devices=(0, 0)).tolist() == [[1, 2, 3], [0, 0, 7]]
        assert current_device() == mine
    finally:
        assert hip.hipSetDevice(0) == 0
