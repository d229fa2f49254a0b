"""minmer_matrix (distance.rs:345-364): the model (tests/matrix_model.py) as written against the order-free predicate the
device computes, the corners of the contract, and everything finch_minmer_matrix decides before it looks for a device -- its
refusals, the matrices of zero cells, H.counts.  No device needed."""
import numpy as np
import pytest

import matrix_inputs as I
import matrix_model as M
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError

U64_MAX, U32_MAX = I.U64_MAX, I.U32_MAX


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as G
    G.build()
    return H.lib()


# ----------------------------------------------------------------------------------------------------------------------
# the model itself
# ----------------------------------------------------------------------------------------------------------------------

def test_cast_wraps():
    assert [M.as_i32(c) for c in (0, 1, (1 << 31) - 1, 1 << 31, U32_MAX)] == [0, 1, (1 << 31) - 1, -(1 << 31), -1]


def test_loop_equals_the_lookup_on_ascending_inputs():
    rng = np.random.default_rng(11)
    for n in range(300):
        pool = I.hash_pool(rng, int(rng.integers(2, 60)))
        ref = np.sort(rng.choice(pool, int(rng.integers(1, len(pool) + 1)), replace=False))
        sk = I.pool_sketches(rng, pool, rng.integers(0, len(pool) + 1, int(rng.integers(0, 6))))
        a, b = M.minmer_matrix(ref, sk), M.by_lookup(ref, sk)
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape == (len(sk), len(ref))
        assert np.array_equal(a, b), (n, ref, sk)


def test_hand_made_corners():
    assert np.array_equal(M.minmer_matrix(I.HAND_REF[0], I.HAND_SKETCHES), I.HAND_WANT)
    assert np.array_equal(M.by_lookup(I.HAND_REF[0], I.HAND_SKETCHES), I.HAND_WANT)
    assert np.array_equal(M.minmer_matrix(I.HAND_REF_INNER[0], I.HAND_SKETCHES), I.HAND_WANT_INNER)
    assert np.array_equal(M.by_lookup(I.HAND_REF_INNER[0], I.HAND_SKETCHES), I.HAND_WANT_INNER)
    # the reference among the sketches: its row is its own counts
    got = M.minmer_matrix(I.HAND_REF[0], [I.HAND_REF] + I.HAND_SKETCHES)
    assert got[0].tolist() == [M.as_i32(c) for c in I.HAND_REF[1]] and np.array_equal(got[1:], I.HAND_WANT)
    # a single reference hash: the cursor never moves
    assert M.minmer_matrix([7], [([1, 7, 9], [3, 4, 5]), ([8], [1])]).tolist() == [[4], [0]]


def test_empty_sides():
    assert M.minmer_matrix([1, 2], []).shape == (0, 2)
    assert M.minmer_matrix([], []).shape == (0, 0)
    assert M.minmer_matrix([], [([], []), ([], [])]).shape == (2, 0)  # no hash ever reads ref_sketch[0]
    assert M.minmer_matrix([1, 2], [([], [])]).tolist() == [[0, 0]]
    for f in (M.minmer_matrix, M.by_lookup):
        with pytest.raises(IndexError):
            f([], [([], []), ([5], [1])])


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI, up to where a device is needed
# ----------------------------------------------------------------------------------------------------------------------

def check_refusals():
    cases = I.refusals()
    assert len(cases) >= 14
    for what, args, words in cases:
        rc, msg = I.raw_call(*args)
        assert rc == _lib.FH_ERR_INVALID, (what, rc, msg)
        assert msg.startswith(words[0]) and all(w in msg for w in words), (what, msg)


def test_refusals_name_their_reason():
    check_refusals()


def test_refusals_through_python():
    bad = I.handle([([1, 5, 9], [1, 1, 1]), ([3, 2, 7], [1, 1, 1])], ["fine", "descends"])
    with pytest.raises(FinchError, match=r"^sketch 1 \(descends\): hashes not strictly ascending at 1"):
        H.minmer_matrix(bad, 0, bad)
    with pytest.raises(FinchError, match=r"^reference sketch 1 \(descends\)"):
        H.minmer_matrix(bad, 1, bad)
    with pytest.raises(FinchError, match="reference sketch 2 of 2"):
        H.minmer_matrix(bad, 2, bad)
    empty = I.handle([([], []), ([4], [1])], ["nothing", "one"])
    with pytest.raises(FinchError, match=r"reference sketch 0 \(nothing\) is empty"):
        H.minmer_matrix(empty, 0, empty)


def test_matrices_of_no_cells_need_no_device():
    some = I.handle([([1, 5, 9], [1, 2, 3]), ([2], [1])])
    empties = I.handle([([], []), ([], []), ([], [])])
    none = I.handle([])
    for refs, ir, sk, shape in [(empties, 1, empties, (3, 0)),  # R = 0 and every sketch empty
                                (some, 0, none, (0, 3)),         # S = 0
                                (empties, 0, none, (0, 0))]:
        stats = {}
        got = H.minmer_matrix(refs, ir, sk, stats=stats)
        assert got.shape == shape and got.dtype == np.int32 and got.flags["C_CONTIGUOUS"]
        assert stats == {"kernel_ms": 0.0, "launches": 0}
        assert np.array_equal(got, M.minmer_matrix([1, 5, 9] if refs is some else [], [([], [])] * shape[0]))
    # ... whatever the device list says, and with out == NULL
    assert I.raw_call(some, 0, none, None, 0, devices=(99,))[0] == 0
    assert I.raw_call(empties, 2, empties, None, 0)[0] == 0


def test_no_cpu_fallback():
    """a matrix with cells and no usable device: FH_ERR_NO_DEVICE, never a host computation"""
    if H.lib().fh_device_count() > 0:
        return  # (test_gpu_matrix.py has the other half: a device that is not there)
    some = I.handle([([1, 5, 9], [1, 2, 3]), ([2], [1])])
    rc, msg = I.raw_call(some, 0, some, np.zeros(6, np.int32), 6)
    assert rc == _lib.FH_ERR_NO_DEVICE and "no usable HIP device" in msg


def test_counts_are_the_u32_bits():
    hs = [3, 4, 5, 6, 7]
    cs = [0, 1, (1 << 31) - 1, 1 << 31, U32_MAX]
    sk = I.handle([(hs, cs), ([], [])])
    got = H.counts(sk, 0)
    assert got.dtype == np.int32 and got.tolist() == [0, 1, (1 << 31) - 1, -(1 << 31), -1]
    raw = np.zeros(5, np.uint32)
    assert H.lib().finch_sketch_copy(sk._p, 0, None, raw.ctypes.data, None, None) == 0
    assert raw.tolist() == cs and np.array_equal(got.view(np.uint32), raw)
    assert H.counts(sk, 1).shape == (0,) and H.counts(sk, 1).dtype == np.int32
    with pytest.raises(FinchError):
        H.counts(sk, 2)
