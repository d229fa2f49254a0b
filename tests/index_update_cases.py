"""What the tests of finch_index_add / finch_index_keep share (include/finch_host.h): builders of sketches
from arrays, and THE CHECKER of the contract -- an updated index is indistinguishable from finch_index_new over the resulting
list of sketches, through every call that reads it.  A sketch is written (name, [(hash, count), ...]), hashes ascending; the
counts vary and are not all 1, so that compare_counts sees them."""
import math

import numpy as np

import finch_rs_amd as F
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, FinchError, SketchParams

TOP = 2 ** 64 - 1
TINY = 5e-324  # the smallest positive double: "any shared hash"
BELOW_ONE = math.nextafter(1.0, 0.0)


def count_of(h):
    """a count that follows from the hash: 1 .. 7, so that a sketch made twice is the same sketch"""
    return 1 + (int(h) * 2654435761 >> 7) % 7


def spec(name, hashes):
    """(name, [(hash, count)]) of these hashes, each once, sorted here"""
    return name, [(h, count_of(h)) for h in sorted({int(x) for x in hashes})]


def mk(name, entries, k=21):
    kc = np.zeros(len(entries), KC_DTYPE)
    kc["hash"] = np.asarray([h for h, _ in entries], np.uint64)
    kc["count"] = np.asarray([c for _, c in entries], np.uint32)
    km = np.zeros((len(entries), k), np.uint8)
    return H.sketches_from_arrays(name, 100, 100, kc, km, SketchParams.mash(kmer_length=k), H.FilterParams(False))


def collect(specs):
    """the Sketches of a list of (name, entries); an empty list gives a collection of no sketches"""
    if not specs:
        return H.select(mk("none", []), [])
    out = mk(*specs[0])
    for name, entries in specs[1:]:
        out.append(mk(name, entries))
    return out


def queries_for(specs, extra=()):
    """queries that meet the library in many ways: some of its own sketches, a union of two, half of one plus strangers, a
    sketch of strangers only, an empty one"""
    full = [s for s in specs if s[1]]
    qs = [("q_own%d" % i, list(s[1])) for i, s in enumerate(full[:: max(1, len(full) // 3)][:3])]
    if len(full) >= 2:
        qs.append(spec("q_union", {h for h, _ in full[0][1]} | {h for h, _ in full[-1][1]}))
        qs.append(spec("q_half", [h for h, _ in full[len(full) // 2][1][::2]] + [3, 5, TOP - 7]))
    qs.append(spec("q_strangers", [11, 13, TOP - 9]))
    qs.append(("q_empty", []))
    return qs + list(extra)


def index_built(refs, devices=(0,), chunk=None):
    """a LibraryIndex built with index_chunk_queries = chunk (read when the index is built)"""
    try:
        if chunk is not None:
            F.set_option("index_chunk_queries", chunk)
        return H.LibraryIndex(refs, devices=devices)
    finally:
        F.set_option("index_chunk_queries", None)


def _outcome(fn):
    """what a call gives: its arrays as bytes and its statistics without the times, or the refusal"""
    st = {}
    try:
        res = fn(st)
    except FinchError as e:
        return ("refused", type(e).__name__), {}
    parts = res if isinstance(res, tuple) else (res,)
    for key in ("kernel_ms", "upload_ms", "copy_ms", "gather_ms"):
        st.pop(key, None)
    return tuple(np.asarray(p).tobytes() for p in parts), st


def check_index(ix, specs, queries=None, devices=(0,), chunk=None, pairwise=True):
    """`ix` has been updated and should now be the index of the sketches `specs`: every reading call on it gives the bytes of
    the dense call on those sketches, and the bytes and the statistics of a fresh index over them (built with `devices` and
    `chunk`, as `ix` was).  -> the number of comparisons made"""
    refs = collect(specs)
    qs = collect(queries if queries is not None else queries_for(specs))
    assert len(ix.refs) == len(refs) and ix.refs.to_json() == refs.to_json()
    done = 0
    with index_built(refs, devices, chunk) as fresh:
        a, b = ix.stats(), fresh.stats()
        assert (a["n_refs"], a["postings"]) == (b["n_refs"], b["postings"]) == (len(specs), sum(len(e) for _, e in specs)), (a, b)
        assert a["device_bytes"] == b["device_bytes"], (a, b)
        calls = []
        for minc in (TINY, 0.1, 1.0):
            for top_n in (0, 3):
                calls.append((("search", minc, top_n), lambda st, x, m=minc, t=top_n: x.search(qs, m, t, stats=st),
                              lambda st, m=minc, t=top_n: H.search(qs, refs, m, t, devices=(0,), stats=st)))
        for maxd in (0.1, BELOW_ONE):
            for old in (False, True):
                calls.append((("dist", maxd, old), lambda st, x, d=maxd, o=old: x.dist(qs, d, o, stats=st),
                              lambda st, d=maxd, o=old: H.dist(qs, refs, d, o, devices=(0,), stats=st)))
                if pairwise:
                    calls.append((("pairwise", maxd, old), lambda st, x, d=maxd, o=old: x.dist(None, d, o, stats=st),
                                  lambda st, d=maxd, o=old: H.dist(refs, refs, d, o, devices=(0,), stats=st)))
        for min_overlap in (1, 3):
            calls.append((("gather", min_overlap), lambda st, x, m=min_overlap: x.gather(qs, m, stats=st),
                          lambda st, m=min_overlap: H.gather(qs, refs, m, devices=(0,), stats=st)))
        for min_common in (1, 2):
            calls.append((("compare_counts", min_common), lambda st, x, m=min_common: x.compare_counts(qs, m, stats=st),
                          lambda st, m=min_common: H.compare_counts(refs, qs, m, devices=(0,), stats=st)))
        for what, through, dense in calls:
            got, got_st = _outcome(lambda st: through(st, ix))
            want, want_st = _outcome(lambda st: through(st, fresh))
            direct, _ = _outcome(dense)
            # (old mode refuses an empty query beside a non-empty reference, in every form of the call; nothing else is refused)
            assert got[0] != "refused" or (what[0] in ("dist", "pairwise") and what[2]), what
            assert got == direct, ("the dense call", what)
            assert got == want, ("a fresh index", what)
            assert got_st == want_st, (what, got_st, want_st)
            done += 1
    return done
