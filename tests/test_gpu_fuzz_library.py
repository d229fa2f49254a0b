"""Randomised differential of the library calls over one index life: dist, search (best_match, filter_to_matches), gather,
compare_counts, cluster and screen in their dense, indexed and host forms, minmer_matrix and merge.  tests/library_fuzz_inputs.py
draws a case -- a library on the block-of-64 edges with sketch lengths on the lane step, hashes that break a one-word compare or a
bound search, a hash every reference holds and one that a single reference holds, a duplicate reference (ties), counts up to
2^32 - 1; queries; a life of finch_index_add / finch_index_keep steps; small slices, chunks and tiles; one or three device
entries on one device; old mode; a raw-read sample -- and says from the models alone (tests/*_model.py) what every call must
give at every state of that life, at thresholds that sit exactly on realised values (tests/test_library_fuzz_inputs.py holds
the generator, and the host contracts to the models on these very cases).

At the start and after every step, on the living index:
  * every call's dense form, indexed form and (where there is one) host form give the same bytes, and the model's rows;
  * a fresh index over ix.refs gives the same bytes, the same stats() and the same statistics (pairs_touched, launches, ...);
  * every indexed call runs twice in a row and gives the same bytes and statistics -- the second call is what sees a touched
    counter that a finish left at its value --, and the calls run in an order drawn per case and turned per state, so that each
    kind of finish runs behind each other kind;
  * the statistics the models can give: pairs_touched (the pairs that share a hash), pairs_copied, candidates, records_copied and
    pairs_walked (the rows), the cluster's bands, and the launches, which follow from the chunk sizes -- of every indexed call
    from index_chunk_queries, of every dense call from dist_chunk_pairs, cmpc_chunk_pairs, gather_pos_bytes, matrix_chunk_rows
    and merge_chunk_records, summed over the device entries: a call that ignored its chunk option fails here.  (The slice
    options -- dist_slice, matrix_slice, cmpc_slice, gather_slice, merge_tile -- change no count a call reports: they are held
    by the bytes alone);
  * the counts are attached once, at the first compare_counts, and never again: that they follow the updates is what is under
    test; one case in four never attaches them and asserts the refusal instead;
  * the refusals the contract names (a threshold <= 0, a bound >= 1, min_common 0, a `refs` of another size) come back as
    errors and leave the next call unchanged.

Old mode refuses an empty query sketch beside a non-empty reference (dist_model raises ReferencePanics), and a pairwise call or
a cluster takes every reference as a query: an old-mode case draws no empty query, no empty reference and no empty added sketch,
so the fuzz never exercises that refusal -- tests/test_gpu_index_update.py and tests/test_gpu_index_dist.py do.  best_match and
filter_to_matches are checked for every query, filter_to_matches at both thresholds; every compare_counts row is held to
H.compare_counts_pair.

soak runs: FH_LIBRARY_FUZZ_CASES=200 FH_LIBRARY_FUZZ_SEED=123456 python -m pytest tests/test_gpu_fuzz_library.py -m gpu
Needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import finch_rs_amd as F
import library_fuzz_inputs as L
import merge_cases as MC
from finch_rs_amd import _lib
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import FinchError

pytestmark = pytest.mark.gpu

TIMES = ("kernel_ms", "upload_ms", "copy_ms", "gather_ms", "table_ms", "build_kernel_ms")


@pytest.fixture(autouse=True)
def _release_parked_handles():
    """handles are parked by their parameters when freed: every case has its own"""
    yield
    F.load().fh_release_cached()


@pytest.mark.parametrize("i", range(L.N_CASES))
def test_random_case(i):
    run_case(L.SEED0, i)


def outcome(fn):
    """what a call gives: (its result, its arrays as bytes, its statistics without the times), or the refusal"""
    st = {}
    try:
        res = fn(st)
    except (FinchError, F.FinchHipError) as err:
        return None, ("refused", type(err).__name__), {}
    parts = res if isinstance(res, tuple) else (res,)
    return res, tuple(np.asarray(p).tobytes() for p in parts), {k: v for k, v in st.items() if k not in TIMES}


def names_of(sk):
    return [H.lib().finch_sketch_name(sk._p, j).decode() for j in range(len(sk))]


def raw_index_compare_counts(ix, qs, min_common):
    """finch_index_compare_counts itself, not the wrapper that attaches the counts -> (rc, rows or None, statistics)"""
    p, st = C.c_void_p(), {}
    rc = H.lib().finch_index_compare_counts(ix._handle(), qs._p, min_common, C.byref(p))
    return rc, (H._counts_rows(p, st, from_index=True) if rc == 0 else None), st


class Calls:
    """the calls of one state: (name, indexed form, dense form or None, check of the indexed result and its statistics against
    the model, check of the dense form's statistics against the model or None)"""

    def __init__(self, c, e, qs, specs, problems):
        self.c, self.e, self.qs, self.specs, self.problems = c, e, qs, specs, problems
        self.nq, self.nr = len(c.queries), len(specs)

    def soft(self, ok, *what):
        """a statistic the model gives: every disagreement of a case is reported, at its end"""
        if not ok:
            self.problems.append(("state %d" % self.e.state,) + what)

    def dense(self, ok, *what):
        self.soft(ok, "the dense call", *what)

    def launches(self, st, n, what):
        if self.e.postings and n:
            self.soft(st["launches"] == self.e.index_chunks(n), what, "launches", st["launches"], self.e.index_chunks(n))

    def of(self, kind):
        c, e, qs = self.c, self.e, self.qs
        dev = c.devices
        out = []
        if kind == "search":
            for t in e.min_containments:
                def check(res, st, t=t):
                    L.check_search(res[0], res[1], e.search[t].found, ("search", t))
                    self.soft(st["pairs_touched"] == e.search[t].touched, "search", t, st, e.search[t].touched)
                    self.launches(st, self.nq, "search")
                out.append((("search", t), lambda x, st, t=t: x.search(qs, t, c.top_n, stats=st),
                            lambda refs, st, t=t: H.search(qs, refs, t, c.top_n, devices=dev, stats=st), check,
                            lambda res, st: self.dense(st["launches"] == e.launches.dense_search, "search", st, e.launches.dense_search)))
        elif kind == "dist":
            def check(res, st):
                L.check_dist_rows(res, e.dist.rows, "dist")
                self.soft((st["pairs_touched"], st["pairs_copied"]) == (e.dist.touched, e.dist.copied), "dist", st, e.dist.touched, e.dist.copied)
                self.launches(st, self.nq, "dist")
            out.append((("dist",), lambda x, st: x.dist(qs, e.max_distance, c.old_mode, stats=st),
                        lambda refs, st: H.dist(qs, refs, e.max_distance, c.old_mode, devices=dev, stats=st), check,
                        lambda res, st: self.dense(st["launches"] == e.launches.dense_dist, "dist", st, e.launches.dense_dist)))
        elif kind == "pairwise":
            def check(res, st):
                L.check_dist_rows(res, e.pairwise.rows, "pairwise")
                self.soft((st["pairs_touched"], st["pairs_copied"]) == (e.pairwise.touched, e.pairwise.copied), "pairwise", st,
                          e.pairwise.touched, e.pairwise.copied)
                self.launches(st, self.nr, "pairwise")
            out.append((("pairwise",), lambda x, st: x.dist(None, e.max_distance, c.old_mode, stats=st),
                        lambda refs, st: H.dist(refs, refs, e.max_distance, c.old_mode, devices=dev, stats=st), check,
                        lambda res, st: self.dense(st["launches"] == e.launches.dense_pairwise, "pairwise", st, e.launches.dense_pairwise)))
        elif kind == "gather":
            for mo in e.min_overlaps:
                def check(res, st, mo=mo):
                    L.check_gather(res[0], res[1], e.gather[mo].rows, ("gather", mo))
                    self.soft(st["pairs_touched"] == e.touched, "gather", mo, "pairs_touched", st, e.touched)
                    self.soft(st["records_copied"] == len(res[1]), "gather", mo, "records_copied", st, len(res[1]))
                    self.soft(st["candidates"] == e.gather[mo].candidates, "gather", mo, "candidates", st, e.gather[mo].candidates)
                    self.soft(st["launches"] == e.launches.index_gather, "gather", mo, "launches", st, e.launches.index_gather)

                def dense_check(res, st, mo=mo):
                    want = dict(launches=e.launches.dense_gather[mo], candidates=e.gather[mo].candidates, records_copied=len(res[1]))
                    self.dense(st == want, "gather", mo, st, want)
                out.append((("gather", mo), lambda x, st, mo=mo: x.gather(qs, mo, 0, stats=st),
                            lambda refs, st, mo=mo: H.gather(qs, refs, mo, 0, devices=dev, stats=st), check, dense_check))
        elif kind == "compare_counts":
            for mc in e.min_commons:
                def check(res, st, mc=mc):
                    L.check_counts(res, e.counts[mc], ("compare_counts", mc))
                    self.soft((st["pairs_touched"], st["pairs_walked"], st["records_copied"]) == (e.touched, len(res), len(res)),
                              "compare_counts", mc, st, e.touched, len(res))
                    self.soft(st["launches"] == e.launches.index_counts[mc], "compare_counts", mc, "launches", st, e.launches.index_counts[mc])

                def dense_check(res, st, mc=mc):
                    want = dict(launches=e.launches.dense_counts, records_copied=len(res))
                    self.dense(st == want, "compare_counts", mc, st, want)
                out.append((("compare_counts", mc), lambda x, st, mc=mc: x.compare_counts(qs, mc, stats=st),
                            lambda refs, st, mc=mc: H.compare_counts(refs, qs, mc, devices=dev, stats=st), check, dense_check))
        elif kind == "cluster":
            def check(res, st):
                assert res.tolist() == e.cluster.labels, "cluster"
                self.soft((st["pairs_touched"], st["edges"], st["clusters"]) == (e.cluster.touched, e.cluster.edges, len(set(e.cluster.labels))),
                          "cluster", st, e.cluster.touched, e.cluster.edges)
                b = e.cluster.bands
                if b is not None:
                    self.soft((st["pairs_united"], st["pairs_copied"], st["pairs_kept_host"]) == (b["united"], b["copied"], b["kept_host"]),
                              "cluster bands", st, b)
                self.launches(st, self.nr, "cluster")
            out.append((("cluster",), lambda x, st: x.cluster(e.max_distance, c.old_mode, stats=st), None, check, None))
        else:
            assert kind == "screen"
            for ms in e.min_shareds:
                def check(res, st, ms=ms):
                    L.check_screen(res, st, e.screen[ms], e.screen_figures, ("screen", ms))
                    if e.screen_figures["distinct"]:  # one launch per staged piece of the sample (whole tiles of 2048 positions)
                        n_tiles = -(-(e.screen_figures["positions"] + len(L.SM.records(c.sample))) // 2048)
                        ok = st["launches"] >= n_tiles if c.opts["screen_piece"] else st["launches"] == 1
                        self.soft(ok, "screen", ms, "launches", st, n_tiles)
                    else:
                        self.soft(st["launches"] == 0, "screen", ms, "launches", st, 0)
                out.append((("screen", ms), lambda x, st, ms=ms: x.screen(c.sample, c.k, c.hash_seed, ms, stats=st), None, check, None))
        return out


def check_state(c, ix, s, qs, first, problems):
    e = L.expect(c, s)
    specs = L.states(c)[s]
    ctx = (L.describe(c), "state %d" % s)
    refs = ix.refs
    assert len(refs) == len(specs) and names_of(refs) == [x.name for x in specs], ctx
    if c.opts["gather_pos_bytes"] == "fit":
        F.set_option("gather_pos_bytes", e.gather_pos_fit)
    calls = Calls(c, e, qs, specs, problems)
    with H.LibraryIndex(refs, devices=c.devices) as fresh:
        a, b = ix.stats(), fresh.stats()
        assert (a["n_refs"], a["postings"]) == (b["n_refs"], b["postings"]) == (e.n_refs, e.postings), (ctx, a, b)
        assert a["device_bytes"] == b["device_bytes"], (ctx, a, b)
        order = c.order[s % len(c.order):] + c.order[:s % len(c.order)]
        again = None
        for kind in (L.CALL_KINDS[j] for j in order):
            for what, through, dense, check, dense_check in calls.of(kind):
                if what[0] == "compare_counts" and not c.attach:
                    # never attached: the index refuses, before and after every update; the dense call is held to the model
                    # (an index without a hash has no device entry and nothing to attach: it gives no rows)
                    rc, none, _ = raw_index_compare_counts(ix, qs, what[1])
                    assert (rc == _lib.FH_ERR_STATE) if e.postings else (rc == 0 and len(none) == 0), (ctx, what, rc)
                    res, _, st = outcome(lambda st: dense(refs, st))
                    L.check_counts(res, e.counts[what[1]], (ctx, what))
                    dense_check(res, st)
                    continue
                res, got, got_st = outcome(lambda st: through(ix, st))
                assert got[0] != "refused", (ctx, what, got)
                _, twice, twice_st = outcome(lambda st: through(ix, st))
                assert twice == got, (ctx, what, "the same call, a second time")
                assert twice_st == got_st, (ctx, what, "the same call, a second time", got_st, twice_st)
                try:
                    check(res, dict(got_st))
                except AssertionError as err:
                    raise AssertionError((ctx, what) + err.args)
                _, want, want_st = outcome(lambda st: through(fresh, st))
                assert got == want, (ctx, what, "a fresh index")
                assert got_st == want_st, (ctx, what, "a fresh index", got_st, want_st)
                if dense is not None:
                    dres, direct, dense_st = outcome(lambda st: dense(refs, st))
                    assert got == direct, (ctx, what, "the dense call")
                    dense_check(dres, dense_st)   # its chunks were its option's: launches, and what crossed to the host
                if what[0] == "cluster":
                    edges = []
                    assert res.tobytes() == H.cluster_host(refs, e.max_distance, c.old_mode, edges).tobytes() and edges == [e.cluster.edges], (ctx, what)
                if what[0] == "screen":
                    hst = {}
                    host = H.screen_host(refs, c.sample, c.k, c.hash_seed, what[1], stats=hst)
                    assert res.tobytes() == host.tobytes() and all(got_st[f] == hst[f] for f in L.SCREEN_FIGURES), (ctx, what, got_st, hst)
                if what[0] == "gather":
                    host = [H.gather_query(refs, qs, q, what[1], 0) for q in range(len(qs))]
                    assert res[1].tobytes() == np.concatenate(host).tobytes() or len(res[1]) == sum(len(h) for h in host) == 0, (ctx, what)
                if what[0] == "compare_counts":
                    for row in res:
                        t = H.compare_counts_pair(refs, int(row["reference"]), qs, int(row["query"]))
                        assert L.MOM.same(tuple(row[f] for f in L.COUNT_FIELDS), t), (ctx, what, row, t)
                if again is None and what[0] in ("search", "dist", "gather"):
                    again = (what, through, got)

        # best_match and filter_to_matches in both forms, of every query
        for q in range(len(c.queries)):
            if not specs:
                for fn in (lambda: H.best_match(refs, qs, q, devices=c.devices), lambda: ix.best_match(qs, q)):
                    with pytest.raises(FinchError):
                        fn()
                continue
            assert H.best_match(refs, qs, q, devices=c.devices) == ix.best_match(qs, q) == e.best[q], (ctx, "best_match", q)
            for t in e.min_containments:
                want = [specs[r].name for r in e.matches[t][q]]
                assert names_of(H.filter_to_matches(refs, qs, q, t, devices=c.devices)) == names_of(ix.filter_to_matches(qs, q, t)) == want, (ctx, "filter_to_matches", q, t)

        # minmer_matrix and merge over random ordered groups of the current library: no index form
        if e.matrix is not None:
            st = {}
            got = H.minmer_matrix(refs, e.matrix.ir, H.select(refs, e.matrix.members), devices=c.devices, stats=st)
            calls.dense(st["launches"] == e.matrix.launches, "minmer_matrix", st, e.matrix.launches)
            assert got.dtype == np.int32 and got.shape == e.matrix.want.shape and np.array_equal(got, e.matrix.want), (ctx, "minmer_matrix", e.matrix.ir, e.matrix.members)
        if e.merge_groups:
            st = {}
            merged = H.merge(refs, e.merge_groups, e.merge_size, devices=c.devices, stats=st)
            assert len(merged) == len(e.merge_groups)
            for g, want in enumerate(e.merge):
                L.check_merged(MC.read(merged, g), want, (ctx, "merge", e.merge_groups[g], e.merge_size))
            # (a group of one is that member: it launches nothing and nothing crosses)
            calls.dense((st["launches"], st["records_copied"]) == (e.merge_launches, e.merge_records), "merge", e.merge_groups, st,
                        e.merge_launches, e.merge_records)

        # the refusals the contract names come back as errors and leave the next call unchanged
        if specs and again is not None:
            with pytest.raises(FinchError):
                ix.search(qs, 0.0, c.top_n)
            with pytest.raises(FinchError):
                ix.search(qs, -0.5, c.top_n)
            with pytest.raises(FinchError):
                ix.dist(qs, 1.0, c.old_mode)
            with pytest.raises(FinchError):
                ix.compare_counts(qs, 0)
            rc, _, _ = raw_index_compare_counts(ix, qs, 0)   # (the C call itself: the wrapper above refuses in Python)
            assert rc == _lib.FH_ERR_INVALID, (ctx, "min_common 0", rc)
            other = H.select(refs, list(range(len(refs) - 1)))
            p = C.c_void_p()
            rc = H.lib().finch_index_dist(ix._handle(), other._p, qs._p, int(c.old_mode), e.max_distance, C.byref(p))
            assert rc == _lib.FH_ERR_INVALID, (ctx, "a refs of another size", rc)
            what, through, got = again
            _, after, _ = outcome(lambda st: through(ix, st))
            assert after == got, (ctx, what, "after the refusals")


def run_case(seed0, i):
    c = L.case(seed0, i)
    problems = []
    try:
        for name, value in c.opts.items():
            if value is not None and value != "fit":
                F.set_option(name, value)   # (index_chunk_queries is read when an index is built: the living one and the fresh ones)
        refs = L.build(c, L.states(c)[0])
        qs = L.build(c, c.queries)
        first = {"attached": False}
        with H.LibraryIndex(refs, devices=c.devices) as ix:
            check_state(c, ix, 0, qs, first, problems)
            for s, (what, arg) in enumerate(c.life, start=1):
                st = {}
                if what == "add":
                    ix.add(L.build(c, arg), stats=st)
                else:
                    ix.keep(arg, stats=st)
                check_state(c, ix, s, qs, first, problems)
    finally:
        for name in c.opts:
            F.set_option(name, None)
        L.forget(c)   # (a soak holds one case's expectations at a time)
    assert not problems, (L.describe(c), problems)
