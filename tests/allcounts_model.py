"""An independent restatement of finch's AllCounts sketcher (lib/src/sketch_schemes/counts.rs driven by sketch_stream,
lib.rs:51-94) in Python and numpy, without the library: the yardstick of tests/test_gpu_allcounts.py.

  windows   seq.normalize(false).bit_kmers(k, false): the FORWARD k-mer of every start whose k normalised bytes are all
            A/C/G/T (oracle.normalize: acgt upper-cased, u/U -> T, whitespace dropped, every other byte -> N)
  index     the 2-bit word, A 0 C 1 G 2 T 3, first base most significant (needletail's BitKmer)
  counts    counts[ix] = counts[ix].saturating_add(1) per window = min(occurrences, u32::MAX)
  totals    seq_length = 0 (total_bases is never incremented); num_valid_kmers = the u64 sum of the saturated counts
  to_vec    counts.rs:43-64, both as the literal walk and as an order-free predicate; count + extra_count WRAPS (u32, a
            release build without overflow checks)
  filters   filter_counts (filtering.rs:60-87) through the oracle's filter_strands / guess_filter_threshold /
            filter_abundance; on by default for FASTQ only (lib.rs:70-76).  process_post_filter does nothing (mod.rs:115-128).
"""
import numpy as np

from oracle import oracle as O

U32 = 0xFFFFFFFF
KC_DTYPE = np.dtype([("hash", "<u8"), ("count", "<u4"), ("extra_count", "<u4")])
_CODE = np.full(256, 255, dtype=np.uint8)
for _b, _c in zip(b"ACGT", range(4)):
    _CODE[_b] = _c


def revcomp_ix(ix, k: int):
    """needletail bitkmer::reverse_complement on the index (scalar or numpy array)"""
    x = np.asarray(ix, dtype=np.uint64) ^ np.uint64(4 ** k - 1)
    r = np.zeros_like(x)
    for _ in range(k):
        r = (r << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return r if r.ndim else int(r)


def kmer_text(ix: int, k: int) -> bytes:
    """bitmer_to_bytes"""
    return bytes(b"ACGT"[(ix >> (2 * (k - 1 - i))) & 3] for i in range(k))


def window_indices(seq: bytes, k: int) -> np.ndarray:
    """the index of every forward window of one record's raw sequence bytes, in order"""
    codes = _CODE[np.frombuffer(O.normalize(bytes(seq)), dtype=np.uint8)]
    n = len(codes)
    if n < k:
        return np.zeros(0, dtype=np.uint64)
    good = (codes != 255).astype(np.int64)
    run = np.concatenate([[0], np.cumsum(good)])
    ok = (run[k:] - run[:-k]) == k  # window p: codes[p, p + k) all bases
    c = np.where(codes == 255, 0, codes).astype(np.uint64)
    ix = np.zeros(n - k + 1, dtype=np.uint64)
    for i in range(k):
        ix = (ix << np.uint64(2)) | c[i:n - k + 1 + i]
    return ix[ok]


def forward_counts(records, k: int) -> np.ndarray:
    """exact forward occurrences per index (uint64, unsaturated)"""
    tot = np.zeros(4 ** k, dtype=np.uint64)
    for r in records:
        w = window_indices(r, k)
        if len(w):
            tot += np.bincount(w.astype(np.int64), minlength=4 ** k).astype(np.uint64)
    return tot


def saturate(counts) -> np.ndarray:
    return np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(U32)).astype(np.uint32)


def to_vec_loop(c, k: int):
    """counts.rs:43-64 as written: a clone zeroed as it goes, the count + extra_count wrapping -> [(hash, kmer, count, extra)]"""
    c = [int(x) for x in c]
    clone = list(c)
    out = []
    for ix in range(len(c)):
        count = clone[ix]
        if count == 0:
            continue
        rc = revcomp_ix(ix, k)
        extra = c[rc]
        clone[rc] = 0
        out.append((ix, kmer_text(ix, k), (count + extra) & U32, extra))
    return out


def sparse_counts(records, k: int):
    """(ascending indices that occurred, their exact occurrences as uint64): the model for any k, without a 4^k array"""
    w = [window_indices(r, k) for r in records]
    w = np.concatenate(w) if w else np.zeros(0, dtype=np.uint64)
    ix, c = np.unique(w, return_counts=True)
    return ix.astype(np.uint64), c.astype(np.uint64)


def to_vec_sparse(ix, c, k: int):
    """to_vec as an order-free predicate over the bins that occurred (ix ascending, c their SATURATED counts): emit ix iff
    c[ix] > 0 and (rc >= ix or c[rc] == 0) -> (KC_DTYPE rows, kmers [n, k])"""
    ix = np.asarray(ix, dtype=np.uint64)
    c = np.asarray(c, dtype=np.uint32)
    rc = revcomp_ix(ix, k) if len(ix) else np.zeros(0, dtype=np.uint64)
    pos = np.searchsorted(ix, rc)
    found = pos < len(ix)
    found[found] = ix[pos[found]] == rc[found]
    crc = np.where(found, c[np.minimum(pos, max(len(ix) - 1, 0))] if len(ix) else 0, 0).astype(np.uint32)
    emit = (c > 0) & ((rc >= ix) | (crc == 0))
    kc = np.zeros(int(emit.sum()), dtype=KC_DTYPE)
    e = ix[emit]
    kc["hash"] = e
    kc["count"] = ((c[emit].astype(np.uint64) + crc[emit].astype(np.uint64)) & np.uint64(U32)).astype(np.uint32)
    kc["extra_count"] = crc[emit]
    km = np.zeros((len(e), k), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(k):
        km[:, i] = lut[((e >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.int64)]
    return kc, km


def to_vec_arrays(c, k: int):
    """the same over a dense count vector (index = position)"""
    c = np.asarray(c, dtype=np.uint32)
    nz = np.flatnonzero(c).astype(np.uint64)
    return to_vec_sparse(nz, c[nz.astype(np.int64)], k)


def filter_counts(kc, km, fastq: bool, filter_on=None, abun=(None, None), err_filter=1.0, strand_filter=0.1):
    """filtering.rs:60-87 with lib.rs:70-76's default -> (kc, km, abun_filter as it ends up)"""
    on = fastq if filter_on is None else filter_on
    lo, hi = abun
    if on and strand_filter > 0:
        kc, km = O.filter_strands(kc, km, strand_filter)
    if on and err_filter > 0:
        cutoff = O.guess_filter_threshold(kc, err_filter)
        if lo is None or cutoff > lo:
            lo = cutoff
    if on and (lo is not None or hi is not None):
        kc, km = O.filter_abundance(kc, km, lo, hi)
    return kc, km, (lo, hi)


def sketch(records, k: int, fastq: bool = False, **filters):
    """sketch_stream for AllCounts -> (kc, km, seq_length, num_valid_kmers)"""
    ix, c = sparse_counts(records, k)
    c = saturate(c)
    kc, km = to_vec_sparse(ix, c, k)
    kc, km, _ = filter_counts(kc, km, fastq, **filters)
    return kc, km, 0, int(c.astype(np.uint64).sum())
