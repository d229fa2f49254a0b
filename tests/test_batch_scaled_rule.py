"""The rule the batch path's Scaled sketches rest on (fh_batch.hip), held against the oracle's ScaledSketcher (scaled.rs) on
the CPU: with D = the distinct canonical-k-mer hashes of an input at or below max_hash, if D >= size (or size == 0) the
sketch is exactly those D hashes, ascending, with the exact (saturating) count and extra_count of each and the k-mer's bytes
-- whatever the order of the input.  The k-mers are counted here in plain Python, without the oracle's sketchers.

And the parameter checks of fh_batch_new, which come before its device check and so answer without a GPU."""
import ctypes as C

import numpy as np
import pytest

import finch_rs_amd as F
from finch_rs_amd import _lib
from finch_rs_amd._lib import FhParams, KIND_ALL_COUNTS, KIND_MASH, KIND_SCALED
from oracle import oracle as O

U64 = (1 << 64) - 1
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def max_hash_of(scale: float) -> int:
    """scaled.rs:23,31 (scales whose reciprocal is below 2^64: no saturating cast to restate)"""
    return U64 // int(1.0 / scale)


def count_kmers(seq: bytes, k: int, seed: int):
    """hash -> [count, extra_count, k-mer bytes] over the canonical k-mers of `seq` (upper case; any byte but ACGT breaks
    k-mers); the canonical form is the smaller of window and reverse complement, a tie counting as the reverse complement"""
    d = {}
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if w.strip(b"ACGT"):
            continue
        rc = w.translate(COMP)[::-1]
        canon, is_rc = (w, 0) if w < rc else (rc, 1)
        h = O.hash_f(canon, seed)
        e = d.setdefault(h, [0, 0, canon])
        assert e[2] == canon  # no 64-bit collision among a few hundred k-mers
        e[0] += 1
        e[1] += is_rc
    return d


def rule_sketch(d, max_hash):
    hs = sorted(h for h in d if h <= max_hash)
    return hs, [d[h][0] for h in hs], [d[h][1] for h in hs], [d[h][2] for h in hs]


def oracle_scaled(seq: bytes, size: int, k: int, seed: int, scale: float):
    o = O.OracleSketcher(O.SCALED, size, k, seed, scale)
    o.process(seq)
    return o


def check_rule(seq, size, k, seed, scale):
    d = count_kmers(seq, k, seed)
    mh = max_hash_of(scale)
    hs, cs, es, ks = rule_sketch(d, mh)
    assert size == 0 or len(hs) >= size
    o = oracle_scaled(seq, size, k, seed, scale)
    assert o.max_hash == mh
    kc, km = o.to_vec()
    assert [int(x) for x in kc["hash"]] == hs
    assert [int(x) for x in kc["count"]] == cs
    assert [int(x) for x in kc["extra_count"]] == es
    assert [bytes(r) for r in km] == ks
    assert o.total_bases_and_kmers()[1] == sum(v[0] for v in d.values())


def random_seq(rng, length, p_n=0.01):
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=length)
    s[rng.random(length) < p_n] = ord("N")
    return s.tobytes()


def test_rule_against_the_oracle_on_random_inputs():
    rng = np.random.default_rng(20261016)
    checked = exact = plus_one = zero = 0
    for case in range(600):
        k = int(rng.integers(4, 9))  # short k-mers: they repeat, and palindromes occur
        seq = random_seq(rng, int(rng.integers(60, 900)))
        scale = float(rng.choice([0.02, 0.05, 0.1, 0.2, 0.25, 0.5]))
        seed = int(rng.choice([0, 0, 42, 7]))
        D = len(rule_sketch(count_kmers(seq, k, seed), max_hash_of(scale))[0])
        mode = case % 4
        if mode == 0:
            size = D  # D == size exactly
            exact += 1
        elif mode == 1 and D >= 1:
            size = D - 1  # D == size + 1
            plus_one += 1
        elif mode == 2:
            size = 0
            zero += 1
        else:
            size = int(rng.integers(0, 60))
            if D < size:
                continue  # outside the rule: the sketch also holds hashes above max_hash (test below)
        check_rule(seq, size, k, seed, scale)
        checked += 1
    assert checked >= 400 and exact >= 100 and plus_one >= 100 and zero >= 100, (checked, exact, plus_one, zero)


def test_rule_at_scale_one():
    """max_hash = u64::MAX: every k-mer is a row, whatever the size"""
    rng = np.random.default_rng(3)
    for case in range(40):
        k = int(rng.integers(4, 8))
        seq = random_seq(rng, int(rng.integers(30, 400)))
        d = count_kmers(seq, k, 0)
        assert max_hash_of(1.0) == U64
        for size in (0, 1, len(d), max(len(d) - 1, 0)):
            check_rule(seq, size, k, 0, 1.0)


def test_below_size_the_sketch_is_not_the_rule_s():
    """D < size: the reference keeps hashes above max_hash too -- why such a file is 'not taken'"""
    rng = np.random.default_rng(4)
    seen = 0
    for case in range(50):
        seq = random_seq(rng, 300, 0.0)
        d = count_kmers(seq, 7, 0)
        D = len(rule_sketch(d, max_hash_of(0.05))[0])
        if D + 5 > len(d):
            continue
        kc, _ = oracle_scaled(seq, D + 5, 7, 0, 0.05).to_vec()
        assert len(kc) > D and int(kc["hash"][-1]) > max_hash_of(0.05)
        seen += 1
    assert seen >= 20


# --- fh_batch_new's parameter checks (they come before the device check) ---

def _batch_new(kind, k, size, scale, seed=0):
    L = _lib.load()
    p = FhParams(kind, k, size, seed, scale, 0, 0, 0)
    h = L.fh_batch_new(C.byref(p), 0, 4, 1 << 20)
    msg = "" if h else (L.fh_last_error() or b"").decode(errors="replace")
    if h:
        L.fh_batch_free(h)
    return bool(h), msg


def test_batch_new_accepts_scaled_parameters():
    L = _lib.load()
    for k, size, scale in ((21, 1000, 0.001), (1, 0, 1.0), (32, F.BatchSketcher.SCALED_MAX_ROWS, 0.5)):
        ok, msg = _batch_new(KIND_SCALED, k, size, scale)
        if L.fh_device_count() > 0:
            assert ok, msg
        else:
            assert not ok and "no usable HIP device" in msg, msg
    L.fh_release_cached()


def test_batch_new_still_refuses():
    ok, msg = _batch_new(KIND_ALL_COUNTS, 8, 0, 0.0)
    assert not ok and "serves Mash sketches only" in msg and "AllCounts" in msg
    # what fh_new refuses stays refused, by the same words
    for scale in (0.0, -0.5, 1.5, float("nan")):
        ok, msg = _batch_new(KIND_SCALED, 21, 1000, scale)
        assert not ok and msg == "scale must be in (0, 1]", (scale, msg)
        with pytest.raises(F.FinchHipError) as ei:
            F.SketchParams.scaled(1000, 21, scale).create_sketcher()
        assert "scale must be in (0, 1]" in str(ei.value)
    ok, msg = _batch_new(KIND_SCALED, 33, 1000, 0.001)
    assert not ok and "k = 1..32" in msg
    ok, msg = _batch_new(KIND_SCALED, 21, F.BatchSketcher.SCALED_MAX_ROWS + 1, 0.001)
    assert not ok and "Scaled sketches of size 0..%d" % F.BatchSketcher.SCALED_MAX_ROWS in msg
    ok, msg = _batch_new(KIND_MASH, 21, 3001, 0.0)
    assert not ok and "Mash sketches of 1..3000" in msg
    ok, msg = _batch_new(7, 21, 1000, 0.001)
    assert not ok and "unknown sketch kind" in msg
