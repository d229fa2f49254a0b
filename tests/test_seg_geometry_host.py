"""The segment kernels' geometry, exhaustively and without a GPU: for every k in 1..64 and every stride the dispatcher can hand
k2_sketch_seg<k> / k2_sketch_ws<k>, one tile is walked lane by lane and round by round with the helpers the kernels themselves
compile (fh_core.h; tests/hostcore/fhcore_host.cpp fhcore_seg_check).  The kernels' contract -- the sketch is the oracle's
whatever the stride says -- needs every tile offset to be some lane's in exactly one round: a lost one is a k-mer not counted,
a doubled one a k-mer counted twice.  (The GPU cases of tests/test_gpu_segments.py are chosen by the same model.)"""
import pytest

from seg_model import FAILS, SegModel


@pytest.fixture(scope="module")
def model():
    return SegModel()


@pytest.mark.parametrize("k", list(range(1, 65)))
def test_every_offset_of_a_tile_is_taken_exactly_once(model, k):
    """every (k, stride) of the dispatcher, with the lanes per record it picks: no offset lost, none taken twice, every view
    inside the tile's strings and the strings inside their LDS blocks, every resume round c0 splits the tile in two"""
    s_max = model.max_stride if k > 32 else model.max_record
    bad, n = [], 0
    for S in range(model.min_stride, s_max + 1):
        if S <= k:
            continue
        sub = model.sub_for(k, S)
        if sub == 0:  # the tile kernel's: then launch_k2 takes it in no form either
            assert not any(model.launch_ok(k, S, s) for s in (0, 1, 2, 4)), (k, S)
            continue
        n += 1
        rc, lost = model.check(k, S, sub)
        if rc:
            bad.append((S, sub, FAILS[rc], lost))
    assert n > 0
    assert not bad, "k=%d: %d of %d strides fail, the first ones %r" % (k, len(bad), n, bad[:8])


@pytest.mark.parametrize("k", list(range(1, 65)))
def test_launch_k2_lets_through_only_what_the_sweep_has_walked(model, k):
    """whatever (stride, lanes per record) launch_k2's validation accepts covers its tile; what the dispatcher keeps off the
    segment kernels launch_k2 refuses, with any number of lanes"""
    for S in range(0, model.max_record + 40):
        want = model.sub_for(k, S)
        for sub in (0, 1, 2, 3, 4, 8, 0x100):
            ok = model.launch_ok(k, S, sub)
            assert ok == (want != 0 and (sub or 1) == want), (k, S, sub, want)
            if ok:
                assert model.check(k, S, sub or 1)[0] == 0, (k, S, sub)
    assert model.sub_for(k, model.min_stride - 1) == 0 and model.sub_for(k, k) == 0
    assert model.sub_for(k, (model.max_stride if k > 32 else model.max_record) + 1) == 0


def test_four_lanes_lose_offsets_at_k_1_and_2_only(model):
    """why k < 3 does not get the four-lane form: H = ceil((S - k) / 4), LAST = S - 3 H, LAST - H = k - pad with pad in 0..3, and
    the rounds go by LAST -- where pad > k the front lanes' offsets [LAST, H) are nobody's.  That is every second stride at k = 1
    and every fourth at k = 2 (3 x 16 x (H - LAST) offsets of a tile each), and no stride at any other k"""
    four = range(2 * model.max_stride + 1, model.max_record + 1)
    assert len(four) == 336
    for k in range(1, 33):
        failing = []
        for S in four:
            rc, lost = model.check(k, S, 4)
            _, H, LAST, _ = model.geom(k, S, 4)
            assert (rc != 0) == (LAST < H), (k, S, H, LAST)
            if rc:
                assert rc == 1 and lost == 3 * 16 * (H - LAST), (k, S, FAILS[rc], lost)
                failing.append(S)
        assert len(failing) == {1: 168, 2: 84}.get(k, 0), (k, len(failing))
        if failing:
            assert all(model.sub_for(k, S) == 0 for S in four), k  # ... so the dispatcher gives these k two lanes at most
        else:
            assert all(model.sub_for(k, S) == 4 for S in four), k
    assert model.check(1, 338, 4) == (1, 96) and model.geom(1, 338, 4)[1:3] == (85, 83)
    assert model.check(2, 339, 4) == (1, 48) and model.geom(2, 339, 4)[1:3] == (85, 84)
