"""Hashes that land exactly on a threshold, on the GPU: every path of the engine that takes the hash_mask test hook, on
crafted streams (tests/tie_inputs.py) in which max_hash, max_hash + 1, the n-th smallest hash and its successor are all
hashes of the input, and the tie hash stands for two distinct k-mers.  Held to the oracle bit for bit (assert_same of
tests/test_gpu_parity.py); tests/test_ties_model.py holds the oracle itself to a restatement of mash.rs / scaled.rs on the
same kind of input.  Every case first asserts, from the helper's statement of the stream, that the tie it is named after is
really there.  Needs a real MI355X: run with `-m gpu`.

Not reachable with a mask, and therefore NOT covered at equality here: the k <= 32 segment kernels
(fh_k2s.hip), the speculative first block, the sample pass, the batch sketcher, and the all-ones hash."""
import os
import subprocess
import sys

import numpy as np
import pytest

import finch_rs_amd as F
import tie_inputs as T
from oracle import oracle as O
from test_gpu_parity import assert_same
from ties_model import scaled_max_hash

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MASK12 = T.low_mask(12)
# (1/scale) as u64 = 2^53 -> max_hash 2047, inside the 12-bit range; 3 * 2^51 (not a power of two) -> 2730; 2^52 -> 4095, the
# mask's top value; 2^50 -> 16383, above every masked hash
SCALES = {"pow2": 2.0 ** -53, "nonpow2": 1.0 / (3 * 2.0 ** 51), "top": 2.0 ** -52, "above": 2.0 ** -50}


def params_of(kind, size, k, scale=0.001, seed=0):
    return F.SketchParams.mash(size, size, True, k, seed) if kind == O.MASH else F.SketchParams.scaled(size, k, scale, seed)


def oracle_of(kind, size, st, scale=0.001, data=None):
    ora = O.OracleSketcher(kind, size, st.k, 0, scale)
    ora.set_hash_mask(st.mask)
    ora.process_packed(st.data if data is None else data, 0)
    return ora


def record_len_for(k):
    """crafted records have stride k + 1; the segment kernels take strides 40..168: shorter records are padded with N"""
    return None if k + 1 >= 40 else 47


def hold(kind, size, st, scale=0.001, ctx="", how="block", max_launch=0, stride=0, pushes=1):
    """sketch the stream on the device by one of the routes into the engine and hold it to the oracle"""
    sk = params_of(kind, size, st.k, scale).create_sketcher(max_launch=max_launch, hash_mask=st.mask)
    bufs = []
    if stride:
        sk.set_record_stride(stride)
    cuts = [len(st) * i // pushes * st.stride for i in range(pushes + 1)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if how == "block":
            sk.push_block(st.data[a:b])
        else:  # resident in HBM (16-byte aligned: a fresh allocation per push)
            d = F.DeviceBuffer(b - a + 256)
            d.upload(st.data[a:b])
            bufs.append(d)
            sk.push_device(d.ptr, b - a)
    sk.sync()
    assert_same(sk, oracle_of(kind, size, st, scale), ctx)
    return sk, bufs


def scaled_stream(k, mask, scale, rng_seed, n_fill=300, order="shuffle", record_len=None):
    mh = scaled_max_hash(scale)
    c = T.Crafter(k, mask, rng_seed=rng_seed)
    x = T.floor_rank(mh, mask)
    st = c.around(min(x, c.n_ranks - 1), 30, 30).filler(n_fill).build(order=order, record_len=record_len)
    return st, mh, x


def assert_scaled_premise(st, mh, x, where):
    H, mask = st.H, st.mask
    if where in ("pow2", "nonpow2", "mixed"):
        assert T.value_of(x, mask) == mh and T.value_of(x + 1, mask) == mh + 1
        assert mh in H and mh + 1 in H and mh - 1 in H and mh in st.collided
    elif where == "top":
        assert mh == mask and mh in H and mh in st.collided and max(H) == mh
    elif where == "above":
        assert max(H) < mh
    elif where == "high":  # max_hash itself cannot be a masked hash; its successor 2^63 is, and so is the value below
        assert T.value_of(x + 1, mask) == mh + 1 and mh + 1 in H and T.value_of(x, mask) in H and T.value_of(x, mask) < mh
    n_le = sum(1 for h in H if h <= mh)
    assert 30 < n_le <= len(H)
    return n_le


@pytest.mark.parametrize("where", ["pow2", "nonpow2", "top", "above"])
@pytest.mark.parametrize("k", [21, 32, 33, 64])
def test_scaled_with_a_mask(k, where):
    """Scaled x mask: fh_k2.hip's MASKED branch (k <= 32) and fh_k2w.hip (k > 32) with max_hash a hash of the input"""
    scale = SCALES[where]
    iscale = int(1.0 / scale)
    assert (iscale & (iscale - 1) != 0) == (where == "nonpow2")
    st, mh, x = scaled_stream(k, MASK12, scale, 100 + k)
    assert oracle_of(O.SCALED, 1, st, scale).max_hash == mh
    n_le = assert_scaled_premise(st, mh, x, where)
    for size in (0, n_le - 7, n_le, n_le + 9):
        sk, _ = hold(O.SCALED, size, st, scale, "scaled k=%d %s size=%d" % (k, where, size))
        assert sk.finish()[0] == max(n_le, min(len(st.H), size))
        assert sk.debug_segments()[0] == 0


@pytest.mark.parametrize("k", [21, 40])
def test_scaled_with_the_mixed_and_the_high_mask(k):
    """mixed mask (top 8 and low 8 bits), max_hash = 127: equality needs the high word of the hash to be zero too.
    High-bit mask, scale 0.5: max_hash = 2^63 - 1 is no masked hash, but max_hash + 1 = 2^63 is one, and the largest masked
    hash below it shares its high word's top bits with tau"""
    st, mh, x = scaled_stream(k, T.MIXED_MASK, 2.0 ** -57, 200 + k)
    assert mh == 127
    n_le = assert_scaled_premise(st, mh, x, "mixed")
    for size in (0, n_le - 7, n_le, n_le + 9):
        hold(O.SCALED, size, st, 2.0 ** -57, "mixed k=%d size=%d" % (k, size))
    st, mh, x = scaled_stream(k, T.high_mask(12), 0.5, 300 + k)
    assert mh == 2**63 - 1
    n_le = assert_scaled_premise(st, mh, x, "high")
    for size in (0, n_le - 7, n_le, n_le + 1, n_le + 9):
        hold(O.SCALED, size, st, 0.5, "high k=%d size=%d" % (k, size))


def dense_mash_stream(n, k=21, bits=15, rng_seed=7, record_len=None, extra=2000):
    """a hash space whose lowest n + 50 values all occur, and `extra` ordinary ones above"""
    c = T.Crafter(k, T.low_mask(bits), rng_seed=rng_seed)
    multi = (0.6, 0.25, 0.15) if n <= 5000 else (0.8, 0.15, 0.05)
    c.dense(range(n + 50), multi=multi).filler(extra, n + 50)
    return c.build(record_len=record_len)


def assert_mash_premise(st, n):
    d = st.sorted_distinct()
    assert d[:n + 50] == [T.value_of(r, st.mask) for r in range(n + 50)]  # the lowest n + 50 values all occur
    t = d[n - 1]
    assert T.value_of(T.floor_rank(t, st.mask) + 1, st.mask) in st.H      # the successor of the n-th smallest is a hash
    assert any(h in st.collided for h in d[:n])                           # a kept hash stands for two distinct k-mers
    return t


@pytest.mark.parametrize("n", [1, 64, 1000, 3000, 3001, 4096, 4097, 12288, 12289, 20000])
def test_mash_on_a_dense_hash_space(n):
    """an off-by-one in any rank or cut is a wrong last row: 3000 is the fused small path's limit, 4096 / 12288 are
    SMALL_SORT_MAX / SMALL_MAX"""
    st = dense_mash_stream(max(n, 3))
    assert_mash_premise(st, max(n, 3))
    if n < 3:
        assert st.sorted_distinct()[n] == st.sorted_distinct()[n - 1] + 1
    sk, _ = hold(O.MASH, n, st, ctx="dense n=%d" % n)
    assert sk.to_arrays()[0]["hash"].tolist() == st.sorted_distinct()[:n]
    sk, _ = hold(O.MASH, n, st, ctx="dense n=%d, small launches" % n, max_launch=8192, pushes=3)
    # two-word k-mers, the same cut
    st = dense_mash_stream(max(n, 3), k=40, rng_seed=9)
    assert_mash_premise(st, max(n, 3))
    hold(O.MASH, n, st, ctx="dense k=40 n=%d" % n)


ROUTES_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import finch_rs_amd as F
import tie_inputs as T
import test_gpu_ties as G
from oracle import oracle as O
out = []
for kind, size, scale in G.ROUTE_CASES:
    st, _ = G.route_stream(kind, size, scale)
    sk, _ = G.hold(kind, size, st, scale, "routes %r" % ((kind, size),), max_launch=4096)
    kc, km, pos = sk.to_arrays()
    out.append((int(kc["hash"].sum(dtype=np.uint64)), int(kc["count"].sum()), int(kc["extra_count"].sum()), len(kc),
                int(km.astype(np.uint64).sum()), sk.debug_counters()["big_prunes"]))
print(repr(out))
'''

# 16-bit hash space, its 60 000 lowest values in the input: the live set passes half of the device-wide prune's target
# (65 536) while the stream runs.  Scaled: max_hash = 32767 ((1/scale) as u64 = 2^49) with `size` below the 32 768 hashes at
# or below it, and max_hash = 8191 (2^51) with `size` above the 8192 (a larger `size` would raise the prune's target beyond
# what a 16-bit hash space can fill)
ROUTE_CASES = [(O.MASH, 20000, 0.0), (O.SCALED, 1000, 2.0 ** -49), (O.SCALED, 12000, 2.0 ** -51)]


def route_stream(kind, size, scale):
    c = T.Crafter(21, T.low_mask(16), rng_seed=21)
    c.dense(range(60000), multi=(0.85, 0.1, 0.05))
    x = size - 1 if kind == O.MASH else scaled_max_hash(scale)
    st = c.around(x, 40, 40).build(max_reps=2)
    return st, x


def test_selection_routes_agree_at_a_tie():
    """the in-LDS prune, the device-wide sort and the radix select on dense input: the cut of the Mash selection and
    max_hash of the Scaled one both have their successor in the input.  Option no_select (read once: child processes)
    makes every device-wide prune the sort"""
    for kind, size, scale in ROUTE_CASES:
        st, x = route_stream(kind, size, scale)
        d = st.sorted_distinct()
        if kind == O.MASH:
            assert d[:size + 40] == list(range(size + 40)) and d[size - 1] in st.collided
        else:
            mh = scaled_max_hash(scale)
            assert mh in (32767, 8191) and mh in st.H and mh + 1 in st.H and mh in st.collided
            assert sum(1 for h in d if h <= mh) == mh + 1 and len(d) > 50000 and (size > mh + 1) == (mh == 8191)
    res = []
    for extra in ({}, {"no_select": "1"}):
        r = subprocess.run([sys.executable, "-c", ROUTES_CHILD], cwd=ROOT, env=F.debug_env(**extra), capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, (extra, r.stdout[-2000:], r.stderr[-3000:])
        res.append(eval(r.stdout.strip().splitlines()[-1]))
    assert res[0] == res[1], res
    assert all(x[5] >= 2 for x in res[0]) and all(x[5] >= 2 for x in res[1]), res  # the in-stream device-wide prune ran
    # the in-LDS prune on the same kind of input: a Mash sketch of 3000 with launches small enough to prune in between
    st = dense_mash_stream(3000, extra=9000)
    assert_mash_premise(st, 3000)
    sk, _ = hold(O.MASH, 3000, st, ctx="in-LDS prune", max_launch=4096)
    assert sk.debug_counters()["big_prunes"] == 0 and sk.debug_counters()["launches"] > 3


@pytest.mark.parametrize("k", [33, 40, 64])
def test_two_word_segment_kernel(k):
    """fh_k2ws.hip, the only segment kernel that runs under a mask: records of one length (padded with N where k + 1 is
    below the smallest stride), resident in HBM, the stride announced"""
    L = record_len_for(k)
    stride = (k if L is None else L) + 1
    for where in ("pow2", "top"):
        st, mh, x = scaled_stream(k, MASK12, SCALES[where], 400 + k, n_fill=1500, record_len=L)
        assert st.stride == stride and 40 <= stride <= 168
        n_le = assert_scaled_premise(st, mh, x, where)
        for size in (0, n_le, n_le + 9):
            sk, _ = hold(O.SCALED, size, st, SCALES[where], "k2ws scaled k=%d %s size=%d" % (k, where, size), how="device",
                         stride=stride)
            assert sk.debug_segments()[0] > 0
    for n in (64, 1000, 3001):
        st = dense_mash_stream(n, k=k, rng_seed=11, record_len=L)
        assert_mash_premise(st, n)
        sk, _ = hold(O.MASH, n, st, ctx="k2ws mash k=%d n=%d" % (k, n), how="device", stride=stride)
        assert sk.debug_segments()[0] > 0


@pytest.mark.parametrize("kind", [O.MASH, O.SCALED])
def test_routes_into_the_engine(kind):
    """push_block, a resident push_device, three pushes, small launches, reset and reuse of the handle"""
    if kind == O.MASH:
        size, scale = 500, 0.0
        st = dense_mash_stream(size, extra=3000)
        assert_mash_premise(st, size)
    else:
        scale = SCALES["pow2"]
        st, mh, x = scaled_stream(21, MASK12, scale, 55, n_fill=1500)
        size = assert_scaled_premise(st, mh, x, "pow2") + 9
    for how in ("block", "device"):
        for pushes in (1, 3):
            for max_launch in (0, 4096, 16384):
                sk, bufs = hold(kind, size, st, scale, "route %s pushes=%d max_launch=%d" % (how, pushes, max_launch), how=how,
                                max_launch=max_launch, pushes=pushes)
    first = sk.to_arrays()
    sk.reset()
    for b in bufs:
        sk.push_device(b.ptr, b.nbytes - 256)
    assert_same(sk, oracle_of(kind, size, st, scale), "after reset")
    assert all(np.array_equal(a, b) for a, b in zip(first, sk.to_arrays()))


@pytest.mark.parametrize("max_launch", [4096, 16384])
def test_loose_scaled_threshold_stops_and_relaunches(max_launch):
    """a Scaled threshold that lets half of a 16-bit hash space in: launches stop at the table's guarded size and are
    relaunched after a prune whose count of hashes at or below max_hash includes max_hash itself"""
    kind, size, scale = ROUTE_CASES[1]
    st, x = route_stream(kind, size, scale)
    mh = scaled_max_hash(scale)
    assert mh in st.H and mh + 1 in st.H and mh in st.collided
    sk, _ = hold(kind, size, st, scale, "loose scaled, max_launch=%d" % max_launch, max_launch=max_launch)
    c = sk.debug_counters()
    assert c["relaunches"] > 0, c


@pytest.mark.parametrize("kind", [O.MASH, O.SCALED])
def test_merge_of_two_handles_at_a_tie(kind):
    """fh_merge with stream offsets: the tie hash is in both shards, and its two colliding k-mers arrive first in
    different shards (the merged row takes the bytes of the smaller stream position, the counts of both)"""
    scale = SCALES["nonpow2"]
    found = None
    for seed in range(40):
        if kind == O.MASH:
            size = 300
            c = T.Crafter(21, MASK12, rng_seed=seed)
            st = c.dense(range(size - 60, size + 50)).dense(range(size - 60), multi=(1, 0, 0)).around(size - 1, 5, 5).filler(500, size + 50).build()
            t = st.sorted_distinct()[size - 1]
        else:
            st, mh, x = scaled_stream(21, MASK12, scale, seed, n_fill=500)
            size, t = sum(1 for h in st.H if h <= mh), mh
        half = len(st) // 2
        ia = [i for i in range(half) if st.hashes[i] == t]
        ib = [i for i in range(half, len(st)) if st.hashes[i] == t]
        if ia and ib and st.rows[ia[0]] != st.rows[ib[0]]:
            found = (st, size, t, half)
            break
    assert found, "no seed puts the tie hash's two k-mers first into different shards"
    st, size, t, half = found
    assert t in st.collided and T.value_of(T.floor_rank(t, st.mask) + 1, st.mask) in st.H
    cut = half * st.stride
    for size_ in (size, size - 1, size + 1):
        a = params_of(kind, size_, 21, scale).create_sketcher(hash_mask=st.mask)
        b = params_of(kind, size_, 21, scale).create_sketcher(hash_mask=st.mask)
        a.push_block(st.data[:cut])
        b.set_stream_offset(cut)
        b.push_block(st.data[cut:])
        a.finish()
        b.finish()
        assert t in a.to_arrays()[0]["hash"].tolist() and t in b.to_arrays()[0]["hash"].tolist()
        ia = a.to_arrays()[0]["hash"].tolist().index(t)
        ib = b.to_arrays()[0]["hash"].tolist().index(t)
        assert bytes(a.to_arrays()[1][ia]) != bytes(b.to_arrays()[1][ib])
        # both orders of the merge give the whole stream's sketch
        a.merge(b)
        assert_same(a, oracle_of(kind, size_, st, scale), "merge a <- b size=%d" % size_)
        a2 = params_of(kind, size_, 21, scale).create_sketcher(hash_mask=st.mask)
        a2.push_block(st.data[:cut])
        a2.finish()
        b.merge(a2)
        assert_same(b, oracle_of(kind, size_, st, scale), "merge b <- a size=%d" % size_)


HIST_CHILD = r'''
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_ties as G
G.hist_cases()
print("child ok")
'''


def hist_cases():
    """Mash sketches of the small fast path (size > 0: the quarter-octave histogram refreshes tau) whose n-th smallest hash
    is the LAST value of a histogram bucket and whose successor is the first of the next.  Low-bit mask: the hash sits
    exactly on qoct_upper_edge(q); high-bit mask: masked hashes span the whole u64 range, the bucket's last masked value is
    the largest one at or below the edge and edge + 1 is a masked hash."""
    edge, index = T.qoct_edges()
    n_cases = 0
    for mask in (T.low_mask(14), T.high_mask(14)):
        c = T.Crafter(21, mask, rng_seed=17)
        st = c.dense(range(1300)).filler(4000, 1300).build()
        d = st.sorted_distinct()
        assert d[:1300] == [T.value_of(r, mask) for r in range(1300)]
        # the ranks whose value ends a bucket
        ends = [r for r in range(200, 1250) if index(d[r]) != index(d[r + 1])]
        assert len(ends) >= 8, ends
        for r in ends[::2]:
            q = index(d[r])
            assert d[r] <= edge(q) < d[r + 1] and index(d[r + 1]) == q + 1
            if mask == T.low_mask(14):
                assert d[r] == edge(q) and d[r + 1] == edge(q) + 1   # exactly on the edge
            else:
                assert d[r + 1] == edge(q) + 1                       # the first hash of the next bucket
            for n in (r + 1, r + 2):  # the cut on the edge, and one past it
                for pushes, max_launch in ((1, 0), (3, 4096)):
                    hold(O.MASH, n, st, ctx="hist mask=%x n=%d pushes=%d" % (mask, n, pushes), pushes=pushes, max_launch=max_launch)
                    n_cases += 1
    return n_cases


def test_histogram_refresh_at_bucket_edges():
    """the default (histogram on) in this process, option no_hist in a child process: both are the oracle's sketch"""
    assert hist_cases() >= 32
    r = subprocess.run([sys.executable, "-c", HIST_CHILD], cwd=ROOT, env=F.debug_env(no_hist="1"), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
