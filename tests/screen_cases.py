"""What tests/test_screen_host.py and tests/test_gpu_index_screen.py share: the samples and libraries of the screen's cases,
built from a plain description the model (tests/screen_model.py) reads too, and the comparison of a call's rows and figures
with the model's."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import screen_model as SM
from finch_rs_amd import host as H
from finch_rs_amd.sketch_schemes import KC_DTYPE, SketchParams
from oracle import oracle as O

U64 = (1 << 64) - 1
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def seq(n, seed):
    return np.random.RandomState(seed).choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()


def revcomp(s):
    return s.translate(_COMP)[::-1]


def fasta(seqs, width=70):
    out = []
    for i, s in enumerate(seqs):
        out.append(b">r%d some words\n" % i)
        out += [s[o:o + width] + b"\n" for o in range(0, len(s), width)]
    return b"".join(out)


def fastq(seqs):
    return b"".join(b"@q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


@dataclass
class Ref:
    hashes: object
    kind: str = "mash"
    scale: float = 0.0


@dataclass
class Case:
    texts: list                 # the decompressed inputs, one sample
    k: int
    refs: list                  # of Ref
    seed: int = 0
    min_shared: int = 1
    opts: dict = field(default_factory=dict)  # library options in force for the device call
    whole: bool = False         # refs[0] holds every distinct hash of the sample: shared == distinct, sum_mult == kmers == hits


def build(case):
    """the case's library as one collection"""
    out = None
    for i, r in enumerate(case.refs):
        hs = np.asarray(sorted(int(h) for h in r.hashes), np.uint64)
        kc = np.zeros(len(hs), KC_DTYPE)
        kc["hash"], kc["count"], kc["extra_count"] = hs, 1, 0
        p = (SketchParams.scaled(1000, case.k, r.scale, case.seed) if r.kind == "scaled" else
             SketchParams.mash(kmer_length=case.k, no_strict=True, hash_seed=case.seed))
        one = H.sketches_from_arrays("ref%d" % i, 100, 100, kc, np.zeros((len(hs), case.k), np.uint8), p, H.FilterParams(False))
        if out is None:
            out = one
        else:
            out.append(one)
    return out


def mult_of(texts, k, seed=0):
    return SM.multiplicities(tuple(texts), k, seed)[0]


def whole(texts, k, seed=0):
    """a reference holding every distinct hash of the sample"""
    return Ref(sorted(mult_of(texts, k, seed)))


def hash_of(kmer, seed=0):
    return O.hash_f(min(kmer, revcomp(kmer)), seed)


def expect(case, min_shared=None):
    ms = case.min_shared if min_shared is None else min_shared
    return SM.screen([sorted(int(h) for h in r.hashes) for r in case.refs], case.texts, case.k, case.seed, ms)


def check(rows, st, case, min_shared=None):
    """a call's rows and figures against the model's"""
    want, wst = expect(case, min_shared)
    assert SM.rows_of(rows) == want
    for f in ("positions", "kmers", "hits", "distinct"):
        assert st[f] == wst[f], (f, st, wst)
    if case.whole and wst["kmers"]:
        r0 = rows[rows["reference"] == 0][0]
        assert int(r0["shared"]) == len(mult_of(case.texts, case.k, case.seed)) == int(r0["ref_len"])
        assert int(r0["sum_mult"]) == st["kmers"] == st["hits"]


S = seq(3000, 1)
K = 21


def _short_records():
    t = [fasta([S[:K - 1], S[100:100 + K], b"N" * 50, b"", S[200:700]])]
    return Case(t, K, [whole(t, K), Ref([5, 7])], whole=True)


def _lower_u():
    low = S[:1500].lower().replace(b"t", b"u", 200) + S[1500:2000].replace(b"T", b"U")
    return Case([fasta([low])], K, [whole([fasta([S[:2000]])], K)], whole=True)


def _no_valid_window():
    s = b"N".join(S[o:o + K - 1] for o in range(0, 2000, K - 1))
    return Case([fasta([s])], K, [whole([fasta([S])], K)])


def _junction():
    a, b = S[:300], S[300:600]
    t = [fasta([a, b])]
    return Case(t, K, [Ref([hash_of(a[-10:] + b[:11])]), whole(t, K)])


def _revcomp(forward):
    return Case([fasta([S if forward else revcomp(S)])], K, [whole([fasta([S])], K), Ref(sorted(mult_of([fasta([S])], K))[:100])], whole=True)


def _palindromes():
    s = b"ACGT" * 12 + S[:300] + b"AATT" * 10 + b"GAATTC" * 8 + S[300:400]
    t = [fasta([s])]
    return Case(t, 20, [whole(t, 20)], whole=True)


def _one_record(n, opts=None):
    t = [fasta([seq(n, 7)])]
    return Case(t, K, [whole(t, K)], opts=opts or {}, whole=True)


def _two_files():
    t = [fasta([S[:1200], S[1200:1300]]), fasta([S[1300:2500]])]
    return Case(t, K, [whole(t, K)], whole=True)


def _homopolymer():
    t = [fasta([b"A" * 5000])]
    return Case(t, K, [whole(t, K)], whole=True)


def _repeats(opts=None):
    m = seq(40, 99)
    s = bytearray(seq(12000, 5))
    # a 25-base motif twice within one lane's run of 32 window starts (its windows start at 96..100 and 121..125, lane 3 of
    # tile 0; the copies do not overlap) ...
    for at in (96, 121):
        s[at:at + 25] = m[:25]
    # ... and a 40-base one across lanes, across tiles and across pieces of 2048
    for at in (200, 200 + 64, 200 + 3000, 9000):
        s[at:at + 40] = m
    t = [fasta([bytes(s)])]
    mult = mult_of(t, K)
    assert all(mult[hash_of(m[i:i + K])] >= (6 if i < 5 else 4) for i in range(20))
    return Case(t, K, [whole(t, K)], opts=opts or {}, whole=True)


def _triple():
    """a sample whose k-mers occur once, twice and three times"""
    return [fasta([S[:1000], S[:500], S[:250]])]


def _medians():
    t = _triple()
    m = mult_of(t, K)
    by = {c: sorted(h for h, v in m.items() if v == c) for c in (1, 2, 3)}
    absent = [11, 13, 17]
    return Case(t, K, [Ref(by[1][:2] + by[3][:2] + absent),          # even: 1 1 3 3 -> 1
                       Ref(by[1][:1] + by[2][:1] + by[3][:3]),        # odd: 1 2 3 3 3 -> 3
                       Ref(by[2][:9]),                                # all equal
                       Ref(by[3][5:6] + absent),                      # shared == 1
                       Ref(by[1][:3] + by[2][:3]),                    # even: 1 1 1 2 2 2 -> 1
                       Ref(absent)])                                  # shares nothing: no row


def _few(n):
    t = [fasta([S])]
    return Case(t, K, [Ref(sorted(mult_of(t, K))[500:500 + n])])


def _extremes():
    t = [fasta([S])]
    hs = sorted(mult_of(t, K))
    return Case(t, K, [Ref([hs[0], hs[-1]]), Ref([hs[0]]), Ref([hs[-1], hs[len(hs) // 2]])])


def _neighbours(opts=None):
    t = [fasta([S])]
    m = mult_of(t, K)
    hs = [h for h in sorted(m)[::50][:50] if h - 1 not in m and h + 1 not in m and 0 < h < U64]
    return Case(t, K, [Ref(hs), Ref([h - 1 for h in hs] + [h + 1 for h in hs]), Ref([h + d for h in hs[:10] for d in (-1, 0, 1)])], opts=opts or {})


def _shared_by_200():
    t = _triple()
    hs = sorted(mult_of(t, K))
    return Case(t, K, [Ref([hs[3], 1000 + r]) for r in range(200)])


def _empty_reference():
    t = [fasta([S])]
    hs = sorted(mult_of(t, K))
    return Case(t, K, [Ref(hs[:10]), Ref([]), Ref(hs[5:20]), Ref([])])


def _long_scaled():
    t = _triple()
    hs = sorted(mult_of(t, K))
    fake = [(h * 0x9E3779B97F4A7C15 + 12345) & U64 for h in range(1, 9001)]
    m = set(hs)
    c = Case(t, K, [Ref(set(hs) | {f for f in fake if f not in m}, "scaled", 0.5), Ref(hs[:100], "scaled", 0.5)])
    # longer than any LDS-sized list, and its shared multiplicities are 1, 2 and 3: the median is not the trivial one
    assert len(c.refs[0].hashes) > 8192 and {mult_of(t, K)[h] for h in hs} == {1, 2, 3}
    return c


def _every_k(k, seed):
    t = [fasta([S[:1500], S[1400:2900].lower()])]
    hs = sorted(mult_of(t, k, seed))
    return Case(t, k, [whole(t, k, seed), Ref(hs[:100]), Ref(hs[1::2])], seed=seed, whole=True)


def _fastq():
    t = [fastq([S[o:o + 150] for o in range(0, 3000, 100)])]
    return Case(t, K, [whole(t, K)], whole=True)


def _empty_sample():
    return Case([b""], K, [Ref(sorted(mult_of([fasta([S])], K))[:10]), Ref([3, 4])])


def _empty_library():
    return Case([fasta([S])], K, [Ref([]), Ref([])])


CASES = {
    "short_records": _short_records,
    "lower_u": _lower_u,
    "no_valid_window": _no_valid_window,
    "junction": _junction,
    "forward": lambda: _revcomp(True),
    "revcomp": lambda: _revcomp(False),
    "palindromes": _palindromes,
    "record_2047": lambda: _one_record(2047),
    "record_2048": lambda: _one_record(2048),
    "record_2049": lambda: _one_record(2049),
    "record_2048_k": lambda: _one_record(2048 + K - 1),
    "record_20000_piece_2048": lambda: _one_record(20000, {"screen_piece": 2048}),
    "record_20000_piece_4096": lambda: _one_record(20000, {"screen_piece": 4096}),
    "two_files": _two_files,
    "homopolymer": _homopolymer,
    "repeats": _repeats,
    "repeats_piece_2048": lambda: _repeats({"screen_piece": 2048}),
    "medians": _medians,
    "one_hash": lambda: _few(1),
    "two_hashes": lambda: _few(2),
    "three_hashes": lambda: _few(3),
    "extremes": _extremes,
    "neighbours": _neighbours,
    "neighbours_dir_1": lambda: _neighbours({"screen_dir_bits": 1}),
    "neighbours_dir_4": lambda: _neighbours({"screen_dir_bits": 4}),
    "shared_by_200": _shared_by_200,
    "empty_reference": _empty_reference,
    "long_scaled": _long_scaled,
    "fastq": _fastq,
    "empty_library": _empty_library,
    "empty_sample": _empty_sample,
}
for _k in range(1, 33):
    for _seed in (0, 42):
        CASES["k%d_seed%d" % (_k, _seed)] = (lambda k=_k, seed=_seed: _every_k(k, seed))


@lru_cache(None)
def case(name):
    return CASES[name]()
