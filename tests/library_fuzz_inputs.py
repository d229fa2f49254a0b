"""The cases of the library fuzz (tests/test_gpu_fuzz_library.py): a randomised differential of the library calls -- dist, search,
gather, compare_counts, cluster, screen in their dense, indexed and host forms, minmer_matrix and merge -- over ONE index that
lives through a drawn sequence of finch_index_add / finch_index_keep, and, from the models alone (tests/*_model.py), what every
call must give at every state of that life.  Plain numpy, Python and the host library's constructors; no GPU.
tests/test_library_fuzz_inputs.py holds this module to what the GPU test relies on.

    case(seed0, i)      -> Case: the library (specs), the queries, the life, the settings, the sample; deterministic from
                           default_rng([seed0, i, redraw])
    states(c)           the library after 0, 1, ... steps of the life, as lists of Spec
    expect(c, s)        -> Expect: thresholds taken from the model's own realised values at state s, and the model's answer of
                           every call at them (computed once per case and state)
    build / model twins Sketches of a list of Spec; dist_model.Sk, gather_model.Sk, (hash, count) lists, merge records

A Spec is (name, hashes, counts): strictly ascending Python ints and u32 counts.  Every library is all Mash or all Scaled at one
scale; its sketches carry the case's k and hash seed, which are the screen's too.

What a case plants: hash 0, hash 2^64 - 1, a run of hashes that differ only in the low 32 bits and one that
differs only in the high 32 bits (a one-word compare or a truncated bound search breaks on them), ALL -- a hash every non-empty
reference holds, whose posting run is as long as the library -- and ONE, which exactly one reference holds; a duplicate of a
reference under another name, so that a containment and the gather's arg-max tie (the lowest index wins); counts from
moments_model.COUNTS and random u32, up to 2^32 - 1.

Sizes.  A pairwise call of n references is n^2 pairs for the models, which run in Python inside the test: libraries of 100 and
more sketches are drawn mostly from the short length edges and live three steps, and the literal cluster loop
(index_cluster_model.cluster) is run up to CLUSTER_LITERAL_MAX sketches -- above it the labels are index_cluster_model.labels_of
over index_dist_model's pairwise rows."""
import os
import struct
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import dist_model as M
import gather_model as GM
import index_cluster_model as ICM
import index_dist_model as IDM
import index_gather_model as IGM
import index_model as IM
import matrix_model as XM
import merge_model as MM
import moments_model as MOM
import screen_model as SM
import search_model as SRM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams

N_CASES = int(os.environ.get("FH_LIBRARY_FUZZ_CASES", "12"))
SEED0 = int(os.environ.get("FH_LIBRARY_FUZZ_SEED", "5300"))

U64_MAX = (1 << 64) - 1
Spec = namedtuple("Spec", "name hashes counts")

LIBRARY_SIZES = (1, 2, 63, 64, 65, 130)
LENGTH_EDGES = (0, 1, 63, 64, 65)
LONG_RANGE = (1000, 1100)
CLUSTER_LITERAL_MAX = 40
MAX_QUERY = 320                             # hashes of a query at most
GROWN = 60                                  # a library of this many sketches grows slowly (see the life)
CROWDED = 110                               # ... and one of this many is not added to
BANDS_MAX = 70                              # index_cluster_model.bands (what the device unites, drops, sends) up to here
MAX_SAMPLE_POSITIONS = 6000
SCALES = (0.001, 0.01, 0.3, 1.0, 2.0)       # 2.0: the reference divides by zero -- such a draw is redrawn
SCALE_P = (0.3, 0.3, 0.2, 0.16, 0.04)

# setting -> the values a case draws from (None: the library's default).  gather_pos_bytes' small value is worked out per state
# from the model (the bytes the largest query's candidates need): "fit" stands for it here.
OPTIONS = {
    "dist_slice": (1, 7, 64, None),
    "dist_chunk_pairs": (5, None),
    "matrix_slice": (3, None),
    "matrix_chunk_rows": (2, None),
    "cmpc_slice": (5, None),
    "cmpc_chunk_pairs": (7, None),
    "gather_slice": (3, None),
    "gather_pos_bytes": ("fit", None),
    "merge_tile": (3, None),
    "merge_chunk_records": (50, None),
    "index_chunk_queries": (1, None),
    "index_update_tile": (1, 64, None),
    "index_cluster_margin": (None, 0.25),        # (the default is 2^-20)
    "screen_piece": (2048, None),
    "screen_dir_bits": (1, None),
}
DEVICES = ((0,), (0, 0, 0))
TOP_N = (0, 1, 3)
DENSE_CHUNK_PAIRS = 4 << 20                 # dist_chunk_pairs' and cmpc_chunk_pairs' default
MERGE_RECORDS = 4 << 20                     # merge_chunk_records' default
CALL_KINDS = ("search", "dist", "pairwise", "gather", "compare_counts", "cluster", "screen")


class Case(SimpleNamespace):
    pass


class Expect(SimpleNamespace):
    pass


# --- drawing -------------------------------------------------------------------------------------------------------------

def _walk(values, seed0, i, salt):
    """value of a setting for case i: every block of eight cases holds every value at least once, in an order of its own per
    setting and block -- so any 24 consecutive cases hold every value, and two settings do not move in step"""
    rng = np.random.default_rng([seed0, 977, salt, i // 8])
    seq = rng.permutation(np.resize(np.arange(len(values)), 8))
    return values[int(seq[i % 8])]


def _universe(rng, n):
    """the small universe most hashes come from: random 64-bit values next to the two runs -> (sorted ints, low run, high run)"""
    base = int(rng.integers(1, 1 << 31))
    low = int(rng.integers(0, 1 << 31))
    low_run = [(base << 32) | (low + j) for j in range(6)]           # differ only in the low 32 bits
    high_run = [((base + 7 + j) << 32) | low for j in range(6)]      # differ only in the high 32 bits
    rnd = [int(x) for x in rng.integers(1, U64_MAX, n, dtype=np.uint64)]
    return sorted(set(rnd + low_run + high_run)), low_run, high_run


def _counts(rng, n):
    c = rng.choice(np.asarray(MOM.COUNTS, np.uint64), n)
    big = rng.random(n) < 0.25
    c[big] = rng.integers(0, 1 << 32, int(big.sum()), dtype=np.uint64)
    return [int(x) for x in c]


def _spec(rng, name, hashes):
    hs = sorted({int(h) for h in hashes})
    return Spec(name, hs, _counts(rng, len(hs)))


def _draw_hashes(rng, u, length, must=(), avoid=()):
    """`length` distinct hashes: those of `must`, then nine in ten from the universe and the rest from all 64 bits"""
    out = set(must)
    avoid = set(avoid)
    assert len(out) <= length or length == 0
    if length == 0:
        return []
    want_far = sum(rng.random(length - len(out)) < 0.1) if length > len(out) else 0
    pool = [h for h in u if h not in out and h not in avoid]
    take = min(len(pool), length - len(out) - want_far)
    out.update(int(x) for x in rng.choice(np.asarray(pool, np.uint64), take, replace=False))
    while len(out) < length:
        h = int(rng.integers(1, U64_MAX, dtype=np.uint64))
        if h not in avoid:
            out.add(h)
    return sorted(out)


def _length(rng, big_library):
    if rng.random() < (0.75 if big_library else 0.45):
        return int(rng.choice(LENGTH_EDGES))
    return int(rng.integers(100, 301))


def _sample(rng):
    """a short FASTA or FASTQ text of a few records, cut at random places (a record may be empty or shorter than k): mixed
    case, Ns and Us, in half of the draws a repeat of the first record's start, so that multiplicities pass 1"""
    n_rec = int(rng.integers(1, 6))
    total = int(rng.integers(200, MAX_SAMPLE_POSITIONS + 1))
    cuts = np.sort(rng.integers(0, total + 1, n_rec - 1)) if n_rec > 1 else np.zeros(0, np.int64)
    seqs, prev = [], 0
    for cut in list(cuts) + [total]:
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(cut) - prev)
        m = rng.random(len(s))
        s[m < 0.002] = ord("N")
        s[m > 0.995] = ord("U")
        low = rng.random(len(s)) < 0.1
        s[low] |= 0x20
        seqs.append(s.tobytes())
        prev = int(cut)
    if rng.random() < 0.5:  # a repeat: multiplicities above 1
        seqs.append(seqs[0][:min(len(seqs[0]), 300)].upper())
        seqs[0] = seqs[0][:len(seqs[0]) - len(seqs[-1])] if len(seqs[0]) > 2 * len(seqs[-1]) else seqs[0]
    while sum(len(s) for s in seqs) > MAX_SAMPLE_POSITIONS:
        seqs.pop()
    if rng.random() < 0.5:
        return b"".join(b"@q%d\n%s\n+\n%s\n" % (j, s, b"I" * len(s)) for j, s in enumerate(seqs))
    width = int(rng.choice([60, 70, 1 << 20]))
    out = []
    for j, s in enumerate(seqs):
        out.append(b">r%d words\n" % j)
        out += [s[o:o + width] + b"\n" for o in range(0, len(s), width)]
    return b"".join(out)


def _draw(seed0, i, redraw):
    rng = np.random.default_rng([seed0, i, redraw])
    c = Case(seed0=seed0, index=i, redraws=redraw)
    c.k = int(np.random.default_rng([seed0, 31]).permutation(np.arange(1, 33))[i % 32])
    c.hash_seed = int(rng.choice([0, 42]))
    c.kind = "scaled" if rng.random() < 0.5 else "mash"
    c.scale = float(rng.choice(SCALES, p=SCALE_P)) if c.kind == "scaled" else 0.0
    c.opts = {name: _walk(values, seed0, i, salt) for salt, (name, values) in enumerate(OPTIONS.items())}
    c.devices = _walk(DEVICES, seed0, i, 101)
    c.old_mode = bool(_walk((False, True), seed0, i, 102))
    c.top_n = int(_walk(TOP_N, seed0, i, 103))
    c.attach = i % 4 != 3          # one case in four never attaches the counts and asserts the refusal instead
    c.empty_sample = i % 10 == 7

    # the library
    n_refs = int(rng.choice(LIBRARY_SIZES)) if rng.random() < 0.7 else int(rng.integers(3, 201))
    big = n_refs >= 100
    u, low_run, high_run = _universe(rng, 150 if big else 400)
    c.ALL, c.ONE = u[len(u) // 3], u[2 * len(u) // 3]
    u = [h for h in u if h not in (c.ALL, c.ONE)]
    c.low_run, c.high_run = low_run, high_run
    c.sample = b"" if c.empty_sample else _sample(rng)
    own = sorted(SM.multiplicities((c.sample,), c.k, c.hash_seed)[0]) if c.sample else []
    c.planted_sample = [int(h) for h in rng.choice(np.asarray(own, np.uint64), min(len(own), 10), replace=False)] if own else []

    # (old mode refuses an empty query sketch beside a non-empty reference -- dist_model raises ReferencePanics -- and a pairwise
    # call takes every reference as a query: an old-mode case draws no empty reference)
    c.allow_empty = not c.old_mode
    specials = [0, U64_MAX] + low_run + high_run
    refs = []
    long_at = int(rng.integers(0, n_refs))
    for r in range(n_refs):
        if r == long_at:
            L = int(rng.integers(LONG_RANGE[0], LONG_RANGE[1] + 1))
            must = [c.ALL, c.ONE] + specials + c.planted_sample
        else:
            L = _length(rng, big)
            if L == 0 and not c.allow_empty:
                L = 1
            must = [c.ALL] if L else []
            if L >= 100 and rng.random() < 0.5:
                must += [h for h in specials if rng.random() < 0.5]
        refs.append(_spec(rng, "r%d" % r, _draw_hashes(rng, u, L, must, avoid=(c.ONE,))))
    # half of the sample's planted hashes into a second reference (two different shared counts), a duplicate (the tie), and the specials in one more than the long sketch
    if n_refs >= 2:
        other = (long_at + 1) % n_refs
        extra = set(refs[other].hashes) | set(c.planted_sample[:(len(c.planted_sample) + 1) // 2]) | {c.ALL, 0, U64_MAX} | set(low_run[:3]) | set(high_run[:3])
        refs[other] = _spec(rng, refs[other].name, extra)
    nonempty = [r for r in range(len(refs)) if len(refs[r].hashes) and r != long_at]
    c.dup_of = int(rng.choice(nonempty)) if nonempty else long_at
    if n_refs >= 2:
        refs.append(Spec("dup_of_r%d" % c.dup_of, list(refs[c.dup_of].hashes), list(refs[c.dup_of].counts)))
    c.refs0 = refs
    c.long_name = refs[long_at].name

    # the life: 3 .. 6 steps (three for a library that starts large).  What a step may bring follows the library as it is then,
    # so that no life grows a library the models need many seconds for: at GROWN sketches and more an add brings at most 12,
    # mostly from the short length edges, and at CROWDED and more the step is a keep
    n_steps = 3 if big else int(rng.integers(3, 7))
    special_step = int(rng.integers(0, n_steps - 1)) if i % 3 == 1 else -1   # once per three cases
    life, now, added = [], list(refs), 0
    follow = False
    for s in range(n_steps):
        grown = big or len(now) >= GROWN
        if s == special_step:
            empties = [j for j in range(len(now)) if not now[j].hashes]
            keep = empties if (empties and rng.random() < 0.5) else []       # drops every hash, or leaves an empty library
            life.append(("keep", keep))
            now = [now[j] for j in keep]
            follow = True                                                    # ... and an add follows it
            continue
        if follow or len(now) < 2:
            step = "add"
        elif len(now) >= CROWDED:
            step = "keep"
        else:
            step = "add" if rng.random() < 0.55 else "keep"
        follow = False
        if step == "add":
            n_new = int(rng.integers(1, 13 if grown else 41))
            lo, hi = (min(h for x in now for h in x.hashes), max(h for x in now for h in x.hashes)) if any(x.hashes for x in now) else (0, 0)
            more = []
            for j in range(n_new):
                name = "a%d_%d" % (added, j)
                if j == 0 and c.allow_empty:
                    more.append(Spec(name, [], []))
                elif j == 1 and any(x.hashes and c.ONE not in x.hashes for x in now):
                    src = now[int(rng.choice([t for t in range(len(now)) if now[t].hashes and c.ONE not in now[t].hashes]))]
                    more.append(Spec(name, list(src.hashes), list(src.counts)))   # a duplicate of a present reference
                else:
                    L = max(1, _length(rng, grown))
                    must = [c.ALL]
                    if j == 2:  # below, between and above the old postings
                        must += [h for h in (max(lo - 1, 0), min(hi + 1, U64_MAX), (lo + hi) // 2 | 1) if h != c.ONE]
                    more.append(_spec(rng, name, _draw_hashes(rng, u, max(L, len(set(must))), must, avoid=(c.ONE,))))
            life.append(("add", more))
            now = now + more
            added += 1
        else:
            m = int(rng.integers(1, len(now)))
            keep = sorted(int(x) for x in rng.choice(len(now), m, replace=False))
            life.append(("keep", keep))
            now = [now[j] for j in keep]
    c.life = life

    # the queries
    st0 = refs
    full = [x for x in st0 if x.hashes]
    qs = [Spec("q_empty", [], [])] if c.allow_empty else []
    qs.append(Spec("q_equal", list(st0[c.dup_of].hashes), list(st0[c.dup_of].counts)))
    stranger = [h for h in (int(x) for x in rng.integers(1, U64_MAX, 30, dtype=np.uint64)) if h not in set(u)]
    qs.append(_spec(rng, "q_stranger", stranger))
    long_h = st0[long_at].hashes
    qs.append(_spec(rng, "q_of_long", rng.choice(np.asarray(long_h, np.uint64), int(rng.integers(1, MAX_QUERY + 1)), replace=False)))
    for j in range(int(rng.integers(0, 9))):
        parts = [full[int(t)] for t in rng.choice(len(full), min(len(full), int(rng.integers(1, 4))), replace=False)] if full else []
        hs = {h for p in parts for h in p.hashes if rng.random() < 0.8}
        hs |= {int(x) for x in rng.integers(1, U64_MAX, int(rng.integers(0, 6)), dtype=np.uint64)}
        if j == 0:
            hs |= {0, U64_MAX, c.ONE} | set(low_run[1:4]) | set(high_run[1:4])
        if len(hs) > MAX_QUERY:  # (a union with the long sketch: the models walk every query against every reference)
            hs = {int(x) for x in rng.choice(np.asarray(sorted(hs), np.uint64), MAX_QUERY, replace=False)} | ({c.ONE, 0, U64_MAX} if j == 0 else set())
        qs.append(_spec(rng, "q_union%d" % j, hs))
    c.queries = qs
    c.order = [int(x) for x in rng.permutation(len(CALL_KINDS))]
    c.group_seed = int(rng.integers(0, 1 << 31))
    return c


_CASES = {}


def case(seed0, i):
    """case i of the list that starts at seed0; a draw for which the model raises ReferencePanics is redrawn.  A case and its
    expectations stay cached until forget() drops them"""
    if (seed0, i) not in _CASES:
        _CASES[(seed0, i)] = _case(seed0, i)
    return _CASES[(seed0, i)]


def forget(c):
    """drop a case and its expectations: a soak holds one case at a time"""
    _CASES.pop((c.seed0, c.index), None)
    for s in range(len(c.life) + 1):
        _EXPECT.pop((c.seed0, c.index, c.redraws, s), None)


def _case(seed0, i):
    for redraw in range(8):
        c = _draw(seed0, i, redraw)
        try:
            for s in range(len(c.life) + 1):
                expect(c, s)
        except M.ReferencePanics:
            for s in range(len(c.life) + 1):
                _EXPECT.pop((seed0, i, redraw, s), None)
            continue
        return c
    raise AssertionError("case %d of seed %d: eight draws in a row panic" % (i, seed0))


def cases(seed0=None, n=None):
    return [case(SEED0 if seed0 is None else seed0, i) for i in range(N_CASES if n is None else n)]


def states(c):
    """the library after 0, 1, ... steps of the life"""
    if not hasattr(c, "_states"):
        out, now = [list(c.refs0)], list(c.refs0)
        for what, arg in c.life:
            now = now + arg if what == "add" else [now[j] for j in arg]
            out.append(list(now))
        c._states = out
    return c._states


# --- the library's sketches and the models' twins --------------------------------------------------------------------------

def params_of(c):
    if c.kind == "scaled":
        return SketchParams.scaled(1000, c.k, c.scale, c.hash_seed)
    return SketchParams.mash(kmer_length=c.k, no_strict=True, hash_seed=c.hash_seed)


def kmer_of(c, name, h):
    """k bytes that say which sketch a record came from: the merge keeps the earliest member's"""
    return (b"%020d%s............" % (h % 10 ** 20, name.encode()))[:c.k].ljust(c.k, b".")


def seq_length_of(spec):
    return 100 + len(spec.hashes)


def mk(c, spec):
    kc = np.zeros(len(spec.hashes), KC_DTYPE)
    kc["hash"] = np.asarray(spec.hashes, np.uint64)
    kc["count"] = np.asarray(spec.counts, np.uint32)
    kc["extra_count"] = kc["count"] // 2
    km = (np.frombuffer(b"".join(kmer_of(c, spec.name, h) for h in spec.hashes), np.uint8).reshape(len(spec.hashes), c.k)
          if spec.hashes else np.zeros((0, c.k), np.uint8))
    return H.sketches_from_arrays(spec.name, seq_length_of(spec), 90, kc, km, params_of(c), H.FilterParams(False))


def build(c, specs):
    """the Sketches of a list of Spec; an empty list gives a collection of no sketches"""
    if not specs:
        return H.select(mk(c, Spec("none", [], [])), [])
    out = mk(c, specs[0])
    for s in specs[1:]:
        out.append(mk(c, s))
    return out


def dsk(c, spec):
    return M.Sk(spec.hashes, c.kind, c.scale, c.k)


def gsk(spec):
    return GM.Sk(spec.hashes, spec.counts)


def pairs_of(spec):
    return list(zip(spec.hashes, spec.counts))


def records_of(c, spec):
    return [(h, n, n // 2, kmer_of(c, spec.name, h)) for h, n in zip(spec.hashes, spec.counts)]


# --- what the models say ---------------------------------------------------------------------------------------------------

def bits(x):
    return struct.pack("<d", float(x))


def same_double(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or bits(a) == bits(b)


DIST_FIELDS = ("containment", "jaccard", "mash_distance", "common_hashes", "total_hashes")


def same_dist_row(row, q, r, d):
    """a DIST_DTYPE row (or finch_distance's dict with query / reference added) against the model's (q, r, dict)"""
    return (int(row["query"]) == q and int(row["reference"]) == r and int(row["common_hashes"]) == d["common_hashes"] and
            int(row["total_hashes"]) == d["total_hashes"] and all(same_double(row[f], d[f]) for f in DIST_FIELDS[:3]))


_EXPECT = {}


def expect(c, s):
    key = (c.seed0, c.index, c.redraws, s)
    if key not in _EXPECT:
        _EXPECT[key] = _expect(c, s)
    return _EXPECT[key]


def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def _expect(c, s):
    """the thresholds and the models' answers at state s.  Everything is drawn from default_rng([seed0, i, redraw, 7, s])"""
    rng = np.random.default_rng([c.seed0, c.index, c.redraws, 7, s])
    specs = states(c)[s]
    e = Expect(state=s, n_refs=len(specs), postings=sum(len(x.hashes) for x in specs))
    drefs, dqs = [dsk(c, x) for x in specs], [dsk(c, x) for x in c.queries]
    nq, nr = len(dqs), len(drefs)

    # -- search: the realised containments give the thresholds
    table = IM.postings(drefs)
    shared = [IM.shared(table, q) for q in dqs]
    e.touched = sum(len(x) for x in shared)                       # the pairs that share a hash
    conts = sorted({SRM.containment(*IM.closed_counts(dqs[q], drefs[r], n)[::2]) for q in range(nq) for r, n in shared[q].items()})
    if conts:
        on = _pick(rng, conts)
        if len(conts) >= 2:
            j = int(rng.integers(0, len(conts) - 1))
            between = float((conts[j] + conts[j + 1]) / 2)
            if not float(conts[j]) < between < float(conts[j + 1]):
                between = float(conts[j + 1])
        else:
            between = float(conts[0]) / 2
        e.min_containments = [float(on), between]
    else:
        e.min_containments = [0.5, 0.25]
    e.search = {}
    for t in e.min_containments:
        found, touched, passing = IM.search(dqs, drefs, t, c.top_n)
        assert found == SRM.search(dqs, drefs, t, c.top_n), "index_model and search_model disagree"
        on_threshold = sum(1 for q in range(nq) for r, n in shared[q].items()
                           if float(SRM.containment(*IM.closed_counts(dqs[q], drefs[r], n)[::2])) == t)
        e.search[t] = Expect(found=found, touched=touched, passing=passing, on_threshold=on_threshold)
    # best_match and filter_to_matches of every query, threshold 0 included
    e.best = [SRM.best_match(drefs, q) if drefs else None for q in dqs]
    # (filter_to_matches is the untruncated search back in library order: where top_n is 0 the rows are there already)
    e.matches = {t: [sorted(r for r, _ in found) for found in e.search[t].found] if c.top_n == 0 else
                 [SRM.filter_to_matches(drefs, q, t) for q in dqs] for t in e.min_containments}
    # ties: pairs of references with the same containment > 0 of one query (the search keeps the lower index first) ...
    e.containment_ties = 0
    for q in range(nq):
        seen = {}
        for r, n in shared[q].items():
            cont = SRM.containment(*IM.closed_counts(dqs[q], drefs[r], n)[::2])
            e.containment_ties += seen.get(cont, 0)
            seen[cont] = seen.get(cont, 0) + 1
    # ... and queries whose largest shared count is held by two references or more (the gather's arg-max takes the lower index)
    e.gather_ties = sum(1 for x in shared if x and sorted(x.values())[-2:].count(max(x.values())) == 2)

    # -- dist: one realised mash_distance below 1 is the bound
    full = M.calc_sketch_distances(dqs, drefs, c.old_mode, 1.0)
    below = sorted({d["mash_distance"] for _, _, d in full if d["mash_distance"] < 1.0})
    e.max_distance = _pick(rng, below) if below else 0.5
    e.dist_dense = [(q, r, d) for q, r, d in full if d["mash_distance"] <= e.max_distance]
    rows, touched, copied, _ = IDM.dist(dqs, drefs, c.old_mode, e.max_distance)
    assert rows == e.dist_dense, "index_dist_model and dist_model disagree"
    e.dist = Expect(rows=rows, touched=touched, copied=copied,
                    on_threshold=sum(1 for _, _, d in rows if d["mash_distance"] == e.max_distance))
    self_pair = lambda q, r: q == r   # (names are unique: a sketch equals only itself)
    rows, touched, copied, _ = IDM.dist(None, drefs, c.old_mode, e.max_distance, equal=self_pair)
    e.pairwise = Expect(rows=rows, touched=touched, copied=copied)

    # -- cluster
    if nr <= CLUSTER_LITERAL_MAX:
        labels, edges = ICM.cluster(drefs, c.old_mode, e.max_distance)
        assert labels == ICM.labels_of(nr, [(q, r) for q, r, _ in rows]) and edges == len(rows)
    else:
        labels, edges = ICM.labels_of(nr, [(q, r) for q, r, _ in rows]), len(rows)
    margin = c.opts["index_cluster_margin"]
    e.cluster = Expect(labels=labels, edges=edges, touched=touched,
                       bands=ICM.bands(drefs, c.old_mode, e.max_distance, margin or ICM.MARGIN_DEFAULT) if nr <= BANDS_MAX else None)

    # -- gather: one realised count, and that count plus 1
    grefs, gqs = [gsk(x) for x in specs], [gsk(x) for x in c.queries]
    commons = sorted({n for x in shared for n in x.values()})
    e.min_overlaps = [_pick(rng, commons) if commons else 1]
    e.min_overlaps.append(e.min_overlaps[0] + 1)
    gix = IGM.Index(grefs)
    e.gather = {}
    for mo in e.min_overlaps:
        want = GM.gather(gqs, grefs, mo, 0)
        assert want == IGM.gather(gqs, grefs, mo, 0, gix) or _nan_equal(want, IGM.gather(gqs, grefs, mo, 0, gix)), "the two gather models disagree"
        e.gather[mo] = Expect(rows=want, candidates=sum(1 for x in shared for n in x.values() if n >= mo),
                              on_threshold=sum(1 for x in shared for n in x.values() if n == mo))
    need = [4 * sum(n for n in x.values() if n >= min(e.min_overlaps)) for x in shared]
    e.gather_pos_fit = max([4] + need)   # the smallest budget the largest query's candidates fit

    # -- compare_counts: the pairs that share a hash, each walked once
    e.min_commons = list(e.min_overlaps)
    prefs, pqs = [pairs_of(x) for x in specs], [pairs_of(x) for x in c.queries]
    e.moments = {(q, r): MOM.compare_counts(prefs[r], pqs[q]) for q in range(nq) for r in sorted(shared[q])}
    for (q, r), t in e.moments.items():
        assert t[0] == shared[q][r]
    e.counts = {mc: [(q, r, t) for (q, r), t in sorted(e.moments.items()) if t[0] >= mc] for mc in e.min_commons}

    # -- the screen
    ref_hashes = [x.hashes for x in specs]
    rows1, figures = SM.screen(ref_hashes, [c.sample], c.k, c.hash_seed, 1)
    realised = sorted({row[1] for row in rows1})
    e.min_shareds = [_pick(rng, realised) if realised else 1]
    e.min_shareds.append(e.min_shareds[0] + 1)
    e.screen = {ms: SM.screen(ref_hashes, [c.sample], c.k, c.hash_seed, ms)[0] for ms in e.min_shareds}
    e.screen_figures = figures
    e.screen_on_threshold = sum(1 for row in rows1 if row[1] == e.min_shareds[0])

    # -- minmer_matrix and merge over random ordered groups of the current library
    grng = np.random.default_rng([c.group_seed, s])
    e.matrix = None
    nonempty = [r for r in range(nr) if specs[r].hashes]
    if nonempty:
        ir = int(grng.choice(nonempty))
        members = [int(x) for x in grng.integers(0, nr, int(grng.integers(1, 9)))] + [ir]
        sk = [(specs[m].hashes, specs[m].counts) for m in members]
        want = XM.minmer_matrix(specs[ir].hashes, sk)
        assert np.array_equal(want, XM.by_lookup(specs[ir].hashes, sk))
        e.matrix = Expect(ir=ir, members=members, want=want)
    e.merge_size = None if grng.random() < 0.5 else int(grng.choice([1, 5, 70]))
    e.merge_groups, e.merge = [], []
    scale = c.scale if c.kind == "scaled" else None
    for g in range(int(grng.integers(1, 4)) if nr else 0):
        members = [int(x) for x in grng.integers(0, nr, 1 if g == 0 else int(grng.integers(1, 5)))]
        e.merge_groups.append(members)
        e.merge.append(Expect(name=specs[members[0]].name, seq_length=MM.sums(seq_length_of(specs[m]) for m in members),
                              num_valid_kmers=MM.sums(90 for _ in members),
                              records=MM.fold([records_of(c, specs[m]) for m in members], e.merge_size, scale)))

    # -- launches, from the chunk sizes (fh_library.cpp's arithmetic restated; DENSE_CHUNK_PAIRS and MERGE_RECORDS are its defaults)
    chunk = c.opts["index_chunk_queries"]
    e.index_chunks = lambda n: 0 if n == 0 else (-(-n // chunk) if chunk else 1)
    n_dev = len(c.devices)

    def ref_chunks(option, n_queries):
        """launches of a dense call that deals the references in chunks of `option` pairs: at least one reference a launch"""
        if n_queries == 0 or nr == 0:
            return 0
        per = min(max(1, (c.opts[option] or DENSE_CHUNK_PAIRS) // n_queries), nr)
        return -(-nr // per)

    e.launches = Expect(dense_dist=ref_chunks("dist_chunk_pairs", nq), dense_search=ref_chunks("dist_chunk_pairs", nq),
                        dense_pairwise=ref_chunks("dist_chunk_pairs", nr), dense_counts=ref_chunks("cmpc_chunk_pairs", nq))
    # the dense gather: an entry takes the queries e, e + entries, ...; two kernels per chunk of references for the count, then two
    # per chunk of queries whose candidates' positions fit gather_pos_bytes (a chunk without a candidate launches nothing)
    e.launches.dense_gather = {}
    pos_bytes = e.gather_pos_fit if c.opts["gather_pos_bytes"] == "fit" else 1 << 30
    for mo in e.min_overlaps:
        total = 0
        n_entries = min(n_dev, nq) if nr else 0
        for ent in range(n_entries):
            mine = list(range(ent, nq, n_entries))
            total += 2 * ref_chunks("dist_chunk_pairs", len(mine))
            need = [4 * sum(n for n in shared[q].values() if n >= mo) for q in mine]
            q0 = 0
            while q0 < len(mine):
                q1, held = q0, 0
                while q1 < len(mine) and (q1 == q0 or held + need[q1] <= pos_bytes):
                    held += need[q1]
                    q1 += 1
                total += 2 * any(need[q0:q1])
                q0 = q1
        e.launches.dense_gather[mo] = total
    # the index: three kernels per chunk of queries for a gather; for compare_counts the count, the selection if a pair of the
    # chunk was touched, the walk if one passed
    e.launches.index_gather = 3 * e.index_chunks(nq) if e.postings else 0
    e.launches.index_counts = {}
    step = chunk or max(nq, 1)
    for mc in e.min_commons:
        total = 0
        for q0 in range(0, nq, step):
            group = range(q0, min(nq, q0 + step))
            total += 1 + any(shared[q] for q in group) + any(n >= mc for q in group for n in shared[q].values())
        e.launches.index_counts[mc] = total if e.postings else 0
    if e.matrix is not None:
        rows = len(e.matrix.members)
        e.matrix.launches = -(-rows // min(c.opts["matrix_chunk_rows"] or rows, rows))
    # the merge: the groups of two members and more, dealt over the entries; a launch takes groups while the bounds on their
    # accumulators (the members' lengths together; without a scale at most max(the first member's length, size)) fit the budget
    multi = [g for g in e.merge_groups if len(g) >= 2]
    budget = c.opts["merge_chunk_records"] or MERGE_RECORDS
    e.merge_launches = 0
    n_entries = min(n_dev, len(multi))
    for ent in range(n_entries):
        held = None
        for g in multi[ent::n_entries]:
            cap = sum(len(specs[m].hashes) for m in g)
            if e.merge_size is not None and scale is None:
                cap = min(cap, max(len(specs[g[0]].hashes), e.merge_size))
            if held is None or held + cap > budget:
                e.merge_launches += 1
                held = 0
            held += cap
    e.merge_records = sum(len(want.records) for g, want in zip(e.merge_groups, e.merge) if len(g) >= 2)
    return e


def _nan_equal(a, b):
    """two lists of lists of gather rows: integers by value, doubles as bit patterns, two NaNs being equal"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if len(ra) != len(rb):
            return False
        for x, y in zip(ra, rb):
            if any(x[f] != y[f] for f in GM.INTS) or not all(same_double(x[f], y[f]) for f in GM.DOUBLES):
                return False
    return True


def describe(c):
    return ("seed0=%d case=%d k=%d seed=%d %s scale=%g old_mode=%s devices=%r top_n=%d refs=%d queries=%d life=%s opts=%r" % (
        c.seed0, c.index, c.k, c.hash_seed, c.kind, c.scale, c.old_mode, c.devices, c.top_n, len(c.refs0), len(c.queries),
        [(w, len(a)) for w, a in c.life], {k: v for k, v in c.opts.items() if v is not None}))


# --- a call's rows against the model's -------------------------------------------------------------------------------------

def check_dist_rows(rows, want, ctx):
    """DIST_DTYPE rows against the model's [(q, r, dict)]"""
    assert len(rows) == len(want), (ctx, len(rows), len(want))
    for row, (q, r, d) in zip(rows, want):
        assert same_dist_row(row, q, r, d), (ctx, row, q, r, d)


def check_search(offsets, rows, found, ctx):
    assert [int(x) for x in offsets] == SRM.offsets(found), (ctx, offsets, SRM.offsets(found))
    check_dist_rows(rows, [(q, r, d) for q, per in enumerate(found) for r, d in per], ctx)


def check_gather(offsets, rows, want, ctx):
    assert [int(x) for x in offsets] == GM.offsets(want), (ctx, offsets)
    flat = [w for per in want for w in per]
    assert len(rows) == len(flat), (ctx, len(rows), len(flat))
    for row, w in zip(rows, flat):
        assert all(int(row[f]) == w[f] for f in GM.INTS) and all(same_double(row[f], w[f]) for f in GM.DOUBLES), (ctx, row, w)


COUNT_FIELDS = ("common", "ref_pos", "query_pos", "ref_count", "query_count", "var", "skew", "kurt")


def check_counts(rows, want, ctx):
    """COUNTS_DTYPE rows against the model's [(q, r, 8-tuple)]"""
    assert len(rows) == len(want), (ctx, len(rows), len(want))
    for row, (q, r, t) in zip(rows, want):
        assert (int(row["query"]), int(row["reference"])) == (q, r) and MOM.same(tuple(row[f] for f in COUNT_FIELDS), t), (ctx, row, q, r, t)


SCREEN_FIGURES = ("positions", "kmers", "hits", "distinct")


def check_screen(rows, st, want, figures, ctx):
    assert SM.rows_of(rows) == want, (ctx, SM.rows_of(rows)[:3], want[:3])
    for f in SCREEN_FIGURES:
        assert st[f] == figures[f], (ctx, f, st, figures)


def check_merged(got, want, ctx):
    """merge_cases.read()'s dict of a merged sketch against the model's: the first member's name, the sums, the fold's records"""
    assert (got["name"], got["seq_length"], got["num_valid_kmers"]) == (want.name, want.seq_length, want.num_valid_kmers), (ctx, got["name"])
    g, w = got["records"], want.records
    if g != w:
        at = next((j for j, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
        raise AssertionError("%r: records differ at %d of %d / %d: %r != %r" % (ctx, at, len(g), len(w), g[at:at + 2], w[at:at + 2]))
