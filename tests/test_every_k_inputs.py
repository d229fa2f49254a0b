"""The generator of the every-k sweep (tests/every_k_inputs.py) held to what tests/test_gpu_every_k.py relies on, for every k in
1..64 and through the CPU oracle with an unbounded sketch size: both strands and repeats are present, palindromes at even k, the
gap record yields exactly the windows its run lengths say -- and WHICH files the batch doors must take is predicted here, from a
restatement of bplan::tau and bplan::expected_below (finch_rs_amd/csrc/fh_batch_plan.h; it lives in tests/door_fuzz_inputs.py, and
tests/test_door_fuzz_inputs.py holds it to the header's host build), with a margin of 1.25 that makes the prediction independent
of whether a file's length counts its breakers.  The streamed record sketcher's three records (k <= 32) are held to the round
seams, the fold and the Scaled row bounds its sweep relies on.  No GPU."""
import numpy as np
import pytest

import every_k_inputs as E
from door_fuzz_inputs import EMPTY, expected_below, tau  # the restatement of bplan's rule (tests/door_fuzz_inputs.py)
from oracle import oracle as O

KS = list(range(1, 65))
UNBOUNDED = 1 << 22  # more hashes than any stream here has windows
SMALL_N, LARGE_N = 200, 3001          # the sketch sizes of the sweep's batch doors
SMALL_LIMIT, LARGE_LIMIT = 700, 11000  # ... and the positions of their `small` files
LARGE_WANT = 4


def oracle_all(block, k, seed=0):
    o = O.OracleSketcher(O.MASH, UNBOUNDED, k, seed)
    o.process_packed(np.ascontiguousarray(block), 0)
    kc, km = o.to_vec()
    return kc, km, o.total_bases_and_kmers()[1]


@pytest.mark.parametrize("k", KS)
def test_stream_is_what_the_module_says(k):
    records, packed = E.stream(k)
    again = [r for recs in E.parts.__wrapped__(k).values() for r in recs]
    assert len(again) == len(records) and all(np.array_equal(a, b) for a, b in zip(again, records))  # deterministic
    assert np.array_equal(packed, np.concatenate([np.concatenate([r, np.zeros(1, np.uint8)]) for r in records]))
    assert all(len(r) <= 8192 for r in records) and not any((r == 0).any() for r in records)
    p = E.parts(k)
    assert len(p["ragged"]) == 300 and [len(r) for r in p["exact"]] == [k - 1, k, k + 1]
    lens = [len(r) for r in p["ragged"] + p["filler"]]
    assert min(lens) >= max(1, k - 2) and max(lens) <= k + 70
    # breakers at every lane offset, and at several offsets of a tile
    breakers = np.flatnonzero(packed == 0)
    assert len(set(int(b) % 32 for b in breakers)) == 32 and len(set(int(b) % E.TILE for b in breakers)) > 200
    # the long record begins a tile of the stream, so its N sit on both sides of two tile edges
    at = E.long_offset(k)
    assert at % E.TILE == 0 and len(p["long"][0]) == 3 * E.TILE + k and np.array_equal(packed[at:-1], p["long"][0])
    assert [int(x) for x in np.flatnonzero(p["long"][0] == ord("N"))] == sorted(E.long_n_positions(k))
    assert 15_000 <= len(packed) <= 42_000
    for limit in (SMALL_LIMIT, LARGE_LIMIT):
        s = E.small(k, limit)
        assert 0 < len(s) <= limit and s[-1] == 0 and np.array_equal(s, packed[:len(s)])
        assert len(s) + len(records[int((s == 0).sum())]) + 1 > limit  # the next record would not fit
        assert oracle_all(s, k)[2] > 0  # a sketch, not an empty one
    # everything is admitted for the `small` files: at most E positions
    assert SMALL_LIMIT <= expected_below(SMALL_N) and LARGE_LIMIT <= LARGE_WANT * LARGE_N


@pytest.mark.parametrize("k", KS)
def test_repeats_strands_palindromes_and_gaps(k):
    _, packed = E.stream(k)
    kc, _, total = oracle_all(packed, k)
    assert 12_000 <= total <= 22_000, total  # (an oracle pass per case stays a matter of milliseconds)
    assert (kc["extra_count"] > 0).any()
    # A^k from 3k x A and, as a reverse complement, from 3k x T: 2k + 1 windows each
    assert int(kc["count"].max()) >= 2 * (2 * k + 1)
    p = E.parts(k)
    if k % 2 == 0:
        rec = p["palindromes"][0]
        pkc, pkm, _ = oracle_all(rec, k)
        assert int((pkc["extra_count"] > 0).sum()) >= 8
        rows = {bytes(r): int(e) for r, e in zip(pkm, pkc["extra_count"])}
        for b in range(8):  # each of the eight palindromes is there, and the tie went to the reverse complement
            pal = bytes(rec[b * (k + 3):b * (k + 3) + k])
            assert pal == bytes(E.revcomp(np.frombuffer(pal, dtype=np.uint8))) and rows[pal] > 0
    else:
        assert "palindromes" not in p
    # a run of L bases between two non-bases holds max(0, L - k + 1) windows: none below k, exactly one at k
    runs = E.gap_runs(k)
    assert runs[2:] == [k, k + 1, k + 2, k] and len(p["gaps"][0]) == sum(runs) + 6
    assert oracle_all(p["gaps"][0], k)[2] == sum(max(0, r - k + 1) for r in runs) == 7


@pytest.mark.parametrize("k", KS)
def test_which_files_the_batch_doors_take(k):
    """D = distinct hashes at or below the threshold `packed` is sketched at.  k >= 7: D >= 1.25 n, the file must be taken; k <= 6:
    D < n, it must not be (bplan::taken: inserted_total >= size); both batch sizes, both seeds of the sweep"""
    _, packed = E.stream(k)
    for seed in (0, 42):
        hashes = oracle_all(packed, k, seed)[0]["hash"]
        for n, want in ((SMALL_N, expected_below(SMALL_N)), (LARGE_N, LARGE_WANT * LARGE_N)):
            assert want == 4 * n
            t = tau(want, len(packed))
            assert t != EMPTY
            D = int((hashes <= np.uint64(t)).sum())
            if k >= 7:
                assert D >= 1.25 * n, (k, n, seed, D)
            else:
                assert D < n, (k, n, seed, D)


# --- the streamed record sketcher's records ---

K_ONE = list(range(1, 33))
STREAM_CAP = 1024  # hashes the streamed form keeps of a record (tests/test_gpu_records_stream.py holds the handle to it)


@pytest.mark.parametrize("k", K_ONE)
def test_stream_records_sit_on_the_round_seams(k):
    recs = E.stream_records(k)
    again = E.stream_records.__wrapped__(k)
    assert len(recs) == 3 and all(np.array_equal(a, b) for a, b in zip(recs, again))
    long = recs[0]
    assert [len(r) for r in recs] == [5 * 4096 + k + 37, 8193, k + 1] and not any((r == 0).any() for r in recs)
    assert len(long) % E.TILE != 0 and -(-len(long) // E.ROUND) == 6 and len(recs[1]) == 8192 + 1
    # N in front of the odd seams, k - 1 behind the even ones, and the one that closes the run of k bases: nowhere else
    want = sorted([4095, 2 * 4096 + k - 1, 3 * 4096 - 1, 4 * 4096 + k - 1, 5 * 4096 - 1, 4 * 4096 - 2])
    assert [int(x) for x in np.flatnonzero(long == ord("N"))] == want == E.stream_long_n_positions(k)
    upper = long & 0xDF
    assert set(np.unique(upper).tolist()) == {ord(c) for c in "ACGTN"} and 0.01 < float((long != upper).mean()) < 0.03
    # a run of exactly k bases between two N across the fourth seam: one valid window, which begins in one round and ends in the next
    s = E.stream_seam_window(k)
    assert long[s - 1] == ord("N") and long[s + k] == ord("N") and not (upper[s:s + k] == ord("N")).any()
    assert s == 4 * E.ROUND - 1 and (s + k - 1 >= 4 * E.ROUND or k == 1)
    assert oracle_all(long[s - 1:s + k + 1], k)[2] == 1  # ... valid in the oracle
    window = bytes(upper[s:s + k])
    rc = bytes(E.revcomp(np.frombuffer(window, dtype=np.uint8)))
    kc, km, total = oracle_all(long, k)
    assert min(window, rc) in {bytes(r) for r in km}
    # every window but those an N touches: six N, the first five k windows each, the pair around the seam window 2 k + 1 together
    touched = set()
    for n_at in want:
        touched |= set(range(max(0, n_at - k + 1), n_at + 1))
    assert total == len(long) - k + 1 - len(touched)
    # A^(3k) ends in front of the second seam's N: k - 1 of its windows span the seam
    at, run = E.stream_a_run(k)
    assert run == 3 * k and (upper[at:at + run] == ord("A")).all() and at < 2 * E.ROUND and at + run == 2 * E.ROUND + k - 1
    rows = {bytes(r): (int(c["count"]), int(c["extra_count"])) for r, c in zip(km, kc)}
    assert rows[b"A" * k][0] >= 2 * k + 1
    # the copied block: every k-mer of it was seen from both strands, first in round 1 and again, behind a fold, in round 4
    src, n, dst = E.COPIED
    assert src + n <= E.ROUND and 3 * E.ROUND <= dst and dst + n <= 4 * E.ROUND - 2
    assert np.array_equal(upper[dst:dst + n], E.revcomp(upper[src:src + n]))
    for p in range(src, src + n - k + 1):
        w = bytes(upper[p:p + k])
        r = bytes(E.revcomp(np.frombuffer(w, dtype=np.uint8)))
        count, extra = rows[w if w < r else r]
        assert count >= 2 and extra > 0, (k, p)


@pytest.mark.parametrize("k", K_ONE)
def test_stream_records_scaled_rows_are_within_the_cap(k):
    """the sweep's Scaled parameters (size 10, seed 7, STREAM_SCALE): the oracle's sketch of every record has between 1 and
    stream_cap rows, so the streamed door takes all three; and its Mash sizes fit the cap"""
    for r in E.stream_records(k):
        o = O.OracleSketcher(O.SCALED, 10, k, 7, E.STREAM_SCALE)
        o.process_packed(np.ascontiguousarray(r), 0)
        assert 1 <= len(o.to_vec()[0]) <= STREAM_CAP, (k, len(r))
    o = O.OracleSketcher(O.SCALED, 10, k, 7, E.STREAM_SCALE)
    o.process_packed(np.ascontiguousarray(E.stream_records(k)[0]), 0)
    if k >= 8:  # (4^k / 2 distinct k-mers below that) about 0.02 x 20 000 hashes at or below max_hash: more than `size`
        assert 300 <= len(o.to_vec()[0]) <= 520
    assert E.STREAM_SCALE == 0.02
