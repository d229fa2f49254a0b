"""Python binding of the C++ host layer (include/finch_host.h): finch::sketch_files / sketch_stream,
FilterParams, the `.sk` (Mash-JSON) writer -- mirrors lib/src/lib.rs:29-94 of the reference."""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import FinchHipError
from .sketch_schemes import KC_DTYPE, FinchError, KmerCount, SketchParams


class CSketchParams(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("kmer_length", C.c_uint32), ("kmers_to_sketch", C.c_uint64),
                ("final_size", C.c_uint64), ("no_strict", C.c_uint32), ("pad", C.c_uint32),
                ("hash_seed", C.c_uint64), ("scale", C.c_double)]


class CFilterParams(C.Structure):
    _fields_ = [("filter_on", C.c_int32), ("has_abun_lo", C.c_uint32), ("abun_lo", C.c_uint32),
                ("has_abun_hi", C.c_uint32), ("abun_hi", C.c_uint32), ("pad", C.c_uint32),
                ("err_filter", C.c_double), ("strand_filter", C.c_double)]


@dataclass
class FilterParams:
    """filtering.rs:11-16"""
    filter_on: Optional[bool] = False
    abun_filter: Tuple[Optional[int], Optional[int]] = (None, None)
    err_filter: float = 0.0
    strand_filter: float = 0.0

    def to_c(self) -> CFilterParams:
        lo, hi = self.abun_filter
        return CFilterParams(-1 if self.filter_on is None else int(bool(self.filter_on)), lo is not None, lo or 0,
                             hi is not None, hi or 0, 0, self.err_filter, self.strand_filter)

    @staticmethod
    def from_c(c: CFilterParams) -> "FilterParams":
        return FilterParams(None if c.filter_on < 0 else bool(c.filter_on),
                            (c.abun_lo if c.has_abun_lo else None, c.abun_hi if c.has_abun_hi else None),
                            c.err_filter, c.strand_filter)


@dataclass
class Sketch:
    """serialization/mod.rs:46-55"""
    name: str
    seq_length: int
    num_valid_kmers: int
    comment: str
    hashes: List[KmerCount]
    filter_params: FilterParams
    sketch_params: SketchParams
    arrays: tuple = field(default=None, repr=False)  # (structured [hash,count,extra_count], kmers uint8[n,k])


_P = C.c_void_p
_SYMS = {
    "finch_last_error": (C.c_char_p, []),
    "finch_default_sketch_params": (None, [C.POINTER(CSketchParams)]),
    "finch_default_filter_params": (None, [C.POINTER(CFilterParams)]),
    "finch_sketch_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(CSketchParams), C.POINTER(CFilterParams),
                                     C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "finch_sketch_buffer": (C.c_int, [_P, C.c_uint64, C.c_char_p, C.POINTER(CSketchParams), C.POINTER(CFilterParams),
                                      C.c_int, C.POINTER(_P)]),
    "finch_sketch_records": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(CSketchParams), C.POINTER(CFilterParams),
                                       C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "finch_sketch_records_buffer": (C.c_int, [_P, C.c_uint64, C.POINTER(CSketchParams), C.POINTER(CFilterParams),
                                              C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "finch_sketch_records_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                             C.POINTER(C.c_uint64)]),
    "finch_sketch_records_stream_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "finch_sketch_file_sharded": (C.c_int, [C.c_char_p, C.POINTER(CSketchParams), C.POINTER(CFilterParams), C.POINTER(C.c_int),
                                            C.c_uint32, C.c_uint64, C.POINTER(_P)]),
    "finch_sketch_buffer_sharded": (C.c_int, [_P, C.c_uint64, C.c_char_p, C.POINTER(CSketchParams), C.POINTER(CFilterParams),
                                              C.POINTER(C.c_int), C.c_uint32, C.c_uint64, C.POINTER(_P)]),
    "finch_shard_probe": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "finch_sketches_to_bsk": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "finch_sketches_to_msh": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "finch_free_bytes": (None, [_P]),
    "finch_sketches_from_bsk": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "finch_sketches_from_msh": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "finch_sketches_from_json": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "finch_open_sketch_file": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "finch_write_sketch_file": (C.c_int, [_P, C.c_char_p]),
    "finch_sketch_params_of": (C.c_int, [_P, C.c_uint32, C.POINTER(CSketchParams)]),
    "finch_sketch_comment": (C.c_char_p, [_P, C.c_uint32]),
    "finch_sketch_set_comment": (C.c_int, [_P, C.c_uint32, C.c_char_p]),
    "finch_sketches_append": (C.c_int, [_P, _P]),
    "finch_filter_sketch": (C.c_int, [_P, C.c_uint32, C.POINTER(CFilterParams)]),
    "finch_sketch_cardinality": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64)]),
    "finch_sketch_hist": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "finch_sketch_from_sketcher": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.c_int, C.POINTER(CSketchParams), C.POINTER(CFilterParams),
                                             C.POINTER(_P)]),
    "finch_sketches_free": (None, [_P]),
    "finch_sketches_len": (C.c_uint32, [_P]),
    "finch_sketch_name": (C.c_char_p, [_P, C.c_uint32]),
    "finch_sketch_seq_length": (C.c_uint64, [_P, C.c_uint32]),
    "finch_sketch_num_valid_kmers": (C.c_uint64, [_P, C.c_uint32]),
    "finch_sketch_n_hashes": (C.c_uint64, [_P, C.c_uint32]),
    "finch_sketch_filter_params": (C.c_int, [_P, C.c_uint32, C.POINTER(CFilterParams)]),
    "finch_sketch_copy": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P]),
    "finch_sketches_to_json": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "finch_free_string": (None, [_P]),
    "finch_sketches_from_arrays": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P, _P,
                                             C.POINTER(CSketchParams), C.POINTER(CFilterParams), C.POINTER(_P)]),
    "finch_apply_filters": (C.c_int, [_P, C.c_uint32, C.POINTER(CFilterParams)]),
    "finch_guess_filter_threshold": (C.c_uint32, [_P, C.c_uint64, C.c_double]),
    "finch_fastx_scan": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "finch_fasta_count_chunked": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "finch_read_file_probe": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "finch_source_probe": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "finch_debug_device_inflate": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "finch_debug_device_gzip": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "finch_debug_kernel_times": (None, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "finch_debug_file_batch": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "finch_debug_fastq_host_strip": (C.c_uint64, []),
    "finch_fastq_strip_probe": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "finch_fasta_two_bit_probe": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    "finch_gzip_probe": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint32)]),
    "finch_bgzf_batch_probe": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
}
class CDistance(C.Structure):
    _fields_ = [("containment", C.c_double), ("jaccard", C.c_double), ("mash_distance", C.c_double),
                ("common_hashes", C.c_uint64), ("total_hashes", C.c_uint64)]


_SYMS["finch_distance"] = (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.c_int, C.POINTER(CDistance)])
_SYMS["finch_raw_distance"] = (C.c_int, [_P, C.c_uint64, _P, C.c_uint64, C.c_double, C.POINTER(CDistance)])
_SYMS["finch_dist"] = (C.c_int, [_P, _P, C.c_int, C.c_double, C.POINTER(C.c_int), C.c_uint32, C.POINTER(_P)])
_SYMS["finch_dist_len"] = (C.c_uint64, [_P])
_SYMS["finch_dist_copy"] = (C.c_int, [_P, _P, _P, _P])
_SYMS["finch_dist_to_json"] = (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)])
_SYMS["finch_dist_stats"] = (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)])
_SYMS["finch_dist_free"] = (None, [_P])
_SYMS["finch_sketches_select"] = (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)])
_SYMS["finch_minmer_matrix"] = (C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_int), C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_double),
                                          C.POINTER(C.c_uint64)])
_SYMS["finch_search"] = (C.c_int, [_P, _P, C.c_double, C.c_uint32, C.POINTER(C.c_int), C.c_uint32, C.POINTER(_P)])
_SYMS["finch_search_len"] = (C.c_uint64, [_P])
_SYMS["finch_search_offsets"] = (C.c_int, [_P, _P])
_SYMS["finch_search_copy"] = (C.c_int, [_P, _P, _P, _P])
_SYMS["finch_search_stats"] = (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_SYMS["finch_search_free"] = (None, [_P])
_SYMS["finch_index_new"] = (C.c_int, [_P, C.POINTER(C.c_int), C.c_uint32, C.POINTER(_P)])
_SYMS["finch_index_search"] = (C.c_int, [_P, _P, C.c_double, C.c_uint32, C.POINTER(_P)])
_SYMS["finch_index_stats"] = (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)])
_SYMS["finch_index_search_stats"] = (C.c_int, [_P, C.POINTER(C.c_uint64)])
_SYMS["finch_index_free"] = (None, [_P])
_SYMS["finch_index_dist"] = (C.c_int, [_P, _P, _P, C.c_int, C.c_double, C.POINTER(_P)])
_SYMS["finch_index_dist_stats"] = (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])


class CClusterStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double)] + [(f, C.c_uint64) for f in ("launches", "pairs_touched", "pairs_united", "pairs_copied",
                                                                       "pairs_kept_host", "edges", "clusters")]


_SYMS["finch_index_cluster"] = (C.c_int, [_P, _P, C.c_int, C.c_double, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(CClusterStats)])
_SYMS["finch_cluster_host"] = (C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64)])


class CScreenRow(C.Structure):
    _fields_ = [("reference", C.c_uint32), ("shared", C.c_uint32), ("ref_len", C.c_uint32), ("reserved", C.c_uint32),
                ("median_mult", C.c_uint64), ("sum_mult", C.c_uint64), ("containment", C.c_double)]


_SYMS["finch_index_screen"] = (C.c_int, [_P, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_P)])
_SYMS["finch_index_screen_buffer"] = (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_P)])
_SYMS["finch_screen_host"] = (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(_P)])
_SYMS["finch_screen_len"] = (C.c_uint64, [_P])
_SYMS["finch_screen_copy"] = (C.c_int, [_P, _P])
_SYMS["finch_screen_stats"] = (C.c_int, [_P] + [C.POINTER(C.c_uint64)] * 5 + [C.POINTER(C.c_double)] * 2 + [C.POINTER(C.c_uint64)])
_SYMS["finch_screen_free"] = (None, [_P])
_SYMS["finch_gather_query"] = (C.c_int, [_P, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64)])
_SYMS["finch_gather"] = (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.c_uint32, C.POINTER(_P)])
_SYMS["finch_gather_len"] = (C.c_uint64, [_P])
_SYMS["finch_gather_offsets"] = (C.c_int, [_P, _P])
_SYMS["finch_gather_copy"] = (C.c_int, [_P, _P, _P, _P])
_SYMS["finch_gather_stats"] = (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_SYMS["finch_gather_free"] = (None, [_P])
_SYMS["finch_index_gather"] = (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.POINTER(_P)])
_SYMS["finch_index_gather_stats"] = (C.c_int, [_P, C.POINTER(C.c_uint64)])


class CCountMoments(C.Structure):
    _fields_ = [("common", C.c_uint64), ("ref_pos", C.c_uint64), ("query_pos", C.c_uint64), ("ref_count", C.c_uint64),
                ("query_count", C.c_uint64), ("var", C.c_double), ("skew", C.c_double), ("kurt", C.c_double)]


_SYMS["finch_compare_counts_pair"] = (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(CCountMoments)])
_SYMS["finch_compare_counts"] = (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_int), C.c_uint32, C.POINTER(_P)])
_SYMS["finch_compare_counts_len"] = (C.c_uint64, [_P])
_SYMS["finch_compare_counts_copy"] = (C.c_int, [_P, _P, _P, _P])
_SYMS["finch_compare_counts_stats"] = (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_SYMS["finch_compare_counts_free"] = (None, [_P])
_SYMS["finch_index_attach_counts"] = (C.c_int, [_P, _P, C.POINTER(C.c_uint64)])
_SYMS["finch_index_compare_counts"] = (C.c_int, [_P, _P, C.c_uint64, C.POINTER(_P)])
_SYMS["finch_index_compare_counts_stats"] = (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_SYMS["finch_index_add"] = (C.c_int, [_P, _P, C.POINTER(C.c_double)])
_SYMS["finch_index_keep"] = (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_double)])
_SYMS["finch_merge_pair"] = (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(_P)])
_SYMS["finch_merge_groups"] = (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_uint32, C.POINTER(_P),
                                         C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)])
_bound = None


def lib():
    global _bound
    if _bound is None:
        L = _lib.load()
        for name, (res, args) in _SYMS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _bound = L
    return _bound


def _check(rc):
    if rc != 0:
        msg = (lib().finch_last_error() or b"").decode(errors="replace")
        if rc == _lib.FH_ERR_INVALID:
            raise FinchError(msg)
        raise FinchHipError(rc, msg)


def _params_c(p: SketchParams) -> CSketchParams:
    kind = {"mash": 0, "scaled": 1, "allcounts": 2}[p.kind]
    return CSketchParams(kind, p.kmer_length, p.kmers_to_sketch, p.final_size, int(p.no_strict), 0, p.hash_seed, p.scale)


class Sketches:
    """owning wrapper of a finch_sketches*"""

    def __init__(self, ptr, params: SketchParams):
        self._p, self.params = ptr, params

    def __del__(self):
        if getattr(self, "_p", None) and lib is not None:  # module globals are gone at interpreter shutdown
            lib().finch_sketches_free(self._p)
            self._p = None

    def __len__(self):
        return lib().finch_sketches_len(self._p)

    def params_of(self, i: int) -> SketchParams:
        c = CSketchParams()
        _check(lib().finch_sketch_params_of(self._p, i, C.byref(c)))
        kind = {0: "mash", 1: "scaled", 2: "allcounts"}[c.kind]
        # (only the Scaled variant has a scale; the dataclass default stands in elsewhere so that equal variants compare equal)
        return SketchParams(kind, c.kmers_to_sketch, c.final_size, bool(c.no_strict), c.kmer_length, c.hash_seed,
                            c.scale if kind == "scaled" else SketchParams().scale)

    def sketch(self, i: int) -> Sketch:
        L = lib()
        n = L.finch_sketch_n_hashes(self._p, i)
        if self.params is None:
            return self._sketch_loaded(i)
        k = self.params.kmer_length
        hs, cs, es = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        km = np.zeros((n, k), np.uint8)
        _check(L.finch_sketch_copy(self._p, i, hs.ctypes.data, cs.ctypes.data, es.ctypes.data, km.ctypes.data))
        fp = CFilterParams()
        _check(L.finch_sketch_filter_params(self._p, i, C.byref(fp)))
        kc = np.zeros(n, dtype=KC_DTYPE)
        kc["hash"], kc["count"], kc["extra_count"] = hs, cs, es
        hashes = [KmerCount(int(hs[j]), bytes(km[j]), int(cs[j]), int(es[j])) for j in range(n)]
        return Sketch(L.finch_sketch_name(self._p, i).decode(), L.finch_sketch_seq_length(self._p, i),
                      L.finch_sketch_num_valid_kmers(self._p, i), "", hashes, FilterParams.from_c(fp), self.params,
                      (kc, km))

    def _sketch_loaded(self, i: int) -> Sketch:
        """a sketch that came out of a file: k-mers may be absent (.msh) or of any length"""
        L = lib()
        n = L.finch_sketch_n_hashes(self._p, i)
        p = self.params_of(i)
        hs, cs, es = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        km = np.zeros((n, p.kmer_length), np.uint8)
        _check(L.finch_sketch_copy(self._p, i, hs.ctypes.data, cs.ctypes.data, es.ctypes.data, km.ctypes.data))
        fp = CFilterParams()
        _check(L.finch_sketch_filter_params(self._p, i, C.byref(fp)))
        kc = np.zeros(n, dtype=KC_DTYPE)
        kc["hash"], kc["count"], kc["extra_count"] = hs, cs, es
        has_kmers = bool(km.any())
        hashes = [KmerCount(int(hs[j]), bytes(km[j]) if has_kmers else b"", int(cs[j]), int(es[j])) for j in range(n)]
        return Sketch(L.finch_sketch_name(self._p, i).decode(), L.finch_sketch_seq_length(self._p, i),
                      L.finch_sketch_num_valid_kmers(self._p, i), L.finch_sketch_comment(self._p, i).decode(), hashes,
                      FilterParams.from_c(fp), p, (kc, km))

    def _bytes(self, fn) -> bytes:
        out, n = _P(), C.c_uint64()
        _check(fn(self._p, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out.value, n.value)
        finally:
            lib().finch_free_bytes(out)

    def to_bsk(self) -> bytes:
        """write_finch_file (serialization/mod.rs:123-166)"""
        return self._bytes(lib().finch_sketches_to_bsk)

    def to_msh(self) -> bytes:
        """write_mash_file (serialization/mash.rs:12-58)"""
        return self._bytes(lib().finch_sketches_to_msh)

    def write(self, path: str) -> None:
        """.sk / .json, .bsk or .msh by file name (cli/src/main.rs:53-70)"""
        _check(lib().finch_write_sketch_file(self._p, path.encode()))

    def append(self, other: "Sketches") -> None:
        _check(lib().finch_sketches_append(self._p, other._p))

    def comment(self, i: int) -> str:
        """sketch i's comment (sketch_records: the rest of the record's header line behind its name)"""
        return lib().finch_sketch_comment(self._p, i).decode(errors="replace")

    def set_comment(self, i: int, comment: str) -> None:
        _check(lib().finch_sketch_set_comment(self._p, i, comment.encode()))

    def filter_sketch(self, i: int, filters: FilterParams) -> None:
        """FilterParams::filter_sketch (filtering.rs:20-54)"""
        c = filters.to_c()
        _check(lib().finch_filter_sketch(self._p, i, C.byref(c)))

    def cardinality(self, i: int) -> int:
        """statistics.rs:8-23"""
        out = C.c_uint64()
        _check(lib().finch_sketch_cardinality(self._p, i, C.byref(out)))
        return out.value

    def hist(self, i: int) -> np.ndarray:
        """statistics.rs:30-47"""
        n = C.c_uint64()
        _check(lib().finch_sketch_hist(self._p, i, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint64)
        _check(lib().finch_sketch_hist(self._p, i, out.ctypes.data, n.value, C.byref(n)))
        return out

    def to_list(self) -> List[Sketch]:
        return [self.sketch(i) for i in range(len(self))]

    def to_json(self) -> str:
        out, n = _P(), C.c_uint64()
        _check(lib().finch_sketches_to_json(self._p, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out.value, n.value).decode()
        finally:
            lib().finch_free_string(out)

    def apply_filters(self, i: int, filters: FilterParams) -> FilterParams:
        c = filters.to_c()
        _check(lib().finch_apply_filters(self._p, i, C.byref(c)))
        return FilterParams.from_c(c)


def sketch_files(filenames: Sequence[str], sketch_params: SketchParams, filters: FilterParams,
                 devices: Optional[Sequence[int]] = None, n_threads: int = 0) -> Sketches:
    """finch::sketch_files (lib.rs:29-49)"""
    arr = (C.c_char_p * len(filenames))(*[f.encode() for f in filenames])
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    _check(lib().finch_sketch_files(arr, len(filenames), C.byref(sp), C.byref(fp), darr, len(devs), n_threads, C.byref(out)))
    return Sketches(out, sketch_params)


def sketch_records(inputs, sketch_params: SketchParams, filters: Optional[FilterParams] = None, devices: Sequence[int] = (0,),
                   n_threads: int = 0, stats: Optional[dict] = None) -> Sketches:
    """one Sketch per record of FASTA inputs (finch_sketch_records): `inputs` is a path, a sequence of paths, or the bytes of
    one input; `stats`, if given, receives records / in_lds / one_by_one / kernel_ms / launches / streamed of this call"""
    if filters is None:
        dflt = CFilterParams()
        lib().finch_default_filter_params(C.byref(dflt))
        filters = FilterParams.from_c(dflt)
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    if isinstance(inputs, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(inputs, dtype=np.uint8)
        _check(lib().finch_sketch_records_buffer(buf.ctypes.data, len(buf), C.byref(sp), C.byref(fp), darr, len(devs), n_threads, C.byref(out)))
    else:
        paths = [inputs] if isinstance(inputs, str) else list(inputs)
        arr = (C.c_char_p * len(paths))(*[f.encode() for f in paths])
        _check(lib().finch_sketch_records(arr, len(paths), C.byref(sp), C.byref(fp), darr, len(devs), n_threads, C.byref(out)))
    res = Sketches(out, sketch_params)
    if stats is not None:
        a, b, c, ms, nl = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double(), C.c_uint64()
        _check(lib().finch_sketch_records_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(ms), C.byref(nl)))
        stats.update(records=a.value, in_lds=b.value, one_by_one=c.value, kernel_ms=ms.value, launches=nl.value)
        stats.update(streamed=records_stream_stats()[0])
    return res


def records_stream_stats():
    """(streamed records, the streamed kernel's milliseconds, its launches) of this thread's last sketch_records call
    (finch_sketch_records_stream_stats)"""
    a, ms, nl = C.c_uint64(), C.c_double(), C.c_uint64()
    _check(lib().finch_sketch_records_stream_stats(C.byref(a), C.byref(ms), C.byref(nl)))
    return a.value, ms.value, nl.value


def sketch_stream(data: bytes, name: str, sketch_params: SketchParams, filters: FilterParams, device: int = 0) -> Sketches:
    """finch::sketch_stream (lib.rs:51-94) over an in-memory file image"""
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    buf = np.frombuffer(data, dtype=np.uint8)
    _check(lib().finch_sketch_buffer(buf.ctypes.data, len(data), name.encode(), C.byref(sp), C.byref(fp), device, C.byref(out)))
    return Sketches(out, sketch_params)


def sketch_file_sharded(filename: str, sketch_params: SketchParams, filters: FilterParams, devices: Sequence[int],
                        chunk_bytes: int = 0) -> Sketches:
    """ONE input partitioned over the handles in `devices` (an entry per handle; entries may repeat), partial sketches
    merged on the host: the north_star's single-large-input path (include/finch_host.h)"""
    devs = list(devices)
    darr = (C.c_int * len(devs))(*devs)
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    _check(lib().finch_sketch_file_sharded(filename.encode(), C.byref(sp), C.byref(fp), darr, len(devs), chunk_bytes, C.byref(out)))
    return Sketches(out, sketch_params)


def sketch_stream_sharded(data: bytes, name: str, sketch_params: SketchParams, filters: FilterParams, devices: Sequence[int],
                          chunk_bytes: int = 0) -> Sketches:
    devs = list(devices)
    darr = (C.c_int * len(devs))(*devs)
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    buf = np.frombuffer(data, dtype=np.uint8)
    _check(lib().finch_sketch_buffer_sharded(buf.ctypes.data, len(data), name.encode(), C.byref(sp), C.byref(fp), darr, len(devs),
                                             chunk_bytes, C.byref(out)))
    return Sketches(out, sketch_params)


def shard_probe(data: bytes, k: int, chunk_bytes: int):
    """chunks the sharded reader deals out (test hook, no device): [(text_off, length, start_state, halo bytes)], records, total_bases"""
    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(data) // max(1, chunk_bytes // 4) + 64
    meta, halos = np.zeros(4 * cap, np.uint64), np.zeros(64 * cap, np.uint8)
    n, nr, tb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib().finch_shard_probe(src.ctypes.data, len(data), k, chunk_bytes, cap, meta.ctypes.data, halos.ctypes.data,
                                   C.byref(n), C.byref(nr), C.byref(tb)))
    assert n.value <= cap
    out = []
    for i in range(n.value):
        off, ln, st, hl = (int(x) for x in meta[4 * i:4 * i + 4])
        out.append((off, ln, st, halos[64 * i:64 * i + hl].tobytes()))
    return out, nr.value, tb.value


def _loaded(fn, *args) -> Sketches:
    out = _P()
    _check(fn(*args, C.byref(out)))
    return Sketches(out, None)  # parameters live per sketch (Sketches.params_of)


def sketches_from_bsk(data: bytes) -> Sketches:
    """read_finch_file (serialization/mod.rs:168-222)"""
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return _loaded(lib().finch_sketches_from_bsk, buf.ctypes.data, len(data))


def sketches_from_msh(data: bytes) -> Sketches:
    """read_mash_file (serialization/mash.rs:60-135)"""
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return _loaded(lib().finch_sketches_from_msh, buf.ctypes.data, len(data))


def sketches_from_json(text) -> Sketches:
    """MultiSketch::to_sketches (serialization/json.rs:244-262)"""
    data = text.encode() if isinstance(text, str) else bytes(text)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return _loaded(lib().finch_sketches_from_json, buf.ctypes.data, len(data))


def open_sketch_file(path: str) -> Sketches:
    """finch::open_sketch_file (lib.rs:96-118)"""
    return _loaded(lib().finch_open_sketch_file, path.encode())


def sketch_from_sketcher(sketcher, name: str, seq_length: int, fmt: int, sketch_params: SketchParams, filters: FilterParams) -> Sketches:
    """the tail of sketch_stream (lib.rs:70-93) on a HipSketcher the caller fed itself: to_vec -> filters -> post filter"""
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    _check(lib().finch_sketch_from_sketcher(sketcher._h, name.encode(), seq_length, fmt, C.byref(sp), C.byref(fp), C.byref(out)))
    return Sketches(out, sketch_params)


def sketches_from_arrays(name, seq_length, num_valid_kmers, kc, km, sketch_params: SketchParams, filters: FilterParams) -> Sketches:
    hs = np.ascontiguousarray(kc["hash"], np.uint64)
    cs = np.ascontiguousarray(kc["count"], np.uint32)
    es = np.ascontiguousarray(kc["extra_count"], np.uint32)
    km = np.ascontiguousarray(km, np.uint8)
    sp, fp = _params_c(sketch_params), filters.to_c()
    out = _P()
    _check(lib().finch_sketches_from_arrays(name.encode(), seq_length, num_valid_kmers, len(hs), hs.ctypes.data, cs.ctypes.data,
                                            es.ctypes.data, km.ctypes.data if km.size else None, C.byref(sp), C.byref(fp),
                                            C.byref(out)))
    return Sketches(out, sketch_params)


def guess_filter_threshold(counts, level: float) -> int:
    a = np.ascontiguousarray(counts, np.uint32)
    return lib().finch_guess_filter_threshold(a.ctypes.data, len(a), level)


def fastx_scan(data: bytes):
    n, tb, fmt = C.c_uint64(), C.c_uint64(), C.c_int()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    _check(lib().finch_fastx_scan(buf.ctypes.data, len(data), C.byref(n), C.byref(tb), C.byref(fmt)))
    return n.value, tb.value, fmt.value


def fasta_count_chunked(data: bytes, chunk: int):
    """(records, total_bases) as the device-side FASTA path counts them, text fed in `chunk`-byte pieces"""
    n, tb = C.c_uint64(), C.c_uint64()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    _check(lib().finch_fasta_count_chunked(buf.ctypes.data, len(data), chunk, C.byref(n), C.byref(tb)))
    return n.value, tb.value


def bgzf_batch_probe(data: bytes, buf_bytes: int, max_members: int, text_budget: int, cap: int):
    """(text, batches, first byte) as the device-inflate reader would deal a BGZF image out, inflated on the host (test hook)"""
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = np.zeros(max(cap, 1), np.uint8)
    n, nb, fb = C.c_uint64(), C.c_uint64(), C.c_int()
    _check(lib().finch_bgzf_batch_probe(src.ctypes.data, len(data), buf_bytes, max_members, text_budget, out.ctypes.data, cap,
                                        C.byref(n), C.byref(nb), C.byref(fb)))
    return out[:n.value].tobytes(), nb.value, fb.value


def debug_device_inflate():
    """(inputs sketched with the BGZF inflate on the device, inputs re-read through the host inflate) -- test hook"""
    a, b = C.c_uint64(), C.c_uint64()
    lib().finch_debug_device_inflate(C.byref(a), C.byref(b))
    return a.value, b.value


def gzip_probe(data: bytes, piece_bytes: int = 1 << 20):
    """(header length, first text byte or -1, DEFLATE bytes the reader hands over, their CRC-32) of a gzip image -- test hook, no device"""
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    h, fb, n, crc = C.c_uint64(), C.c_int(), C.c_uint64(), C.c_uint32()
    _check(lib().finch_gzip_probe(src.ctypes.data, len(data), piece_bytes, C.byref(h), C.byref(fb), C.byref(n), C.byref(crc)))
    return h.value, fb.value, n.value, crc.value


def debug_device_gzip():
    """(inputs sketched with plain gzip inflated on the device, inputs re-read through the host inflate) -- test hook"""
    a, b = C.c_uint64(), C.c_uint64()
    lib().finch_debug_device_gzip(C.byref(a), C.byref(b))
    return a.value, b.value


def fastq_strip_probe(text: bytes, threads: int):
    """-> (packed stream, records, total_bases) of plain 4-line FASTQ text through the host-side strip; FinchError if it is not"""
    src = np.frombuffer(text, dtype=np.uint8)
    out = np.zeros(len(text) // 2 + 64, dtype=np.uint8)
    m, nr, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib().finch_fastq_strip_probe(src.ctypes.data, len(text), threads, out.ctypes.data, len(out), C.byref(m), C.byref(nr), C.byref(nb)))
    return out[:m.value].tobytes(), nr.value, nb.value


def fasta_two_bit_probe(text: bytes, piece: int):
    """-> (region, positions, records, total_bases): FASTA text through the workers' piecewise walk into the two-bit form"""
    src = np.frombuffer(text, dtype=np.uint8)
    cap = ((len(text) + 2047) // 2048 + 1) * 768
    region = np.full(cap + 64, 0xA5, dtype=np.uint8)
    m, nr, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib().finch_fasta_two_bit_probe(src.ctypes.data, len(text), piece, region.ctypes.data, cap, C.byref(m), C.byref(nr), C.byref(nb)))
    assert np.all(region[cap:] == 0xA5)
    return region[:((m.value + 2047) // 2048 + 1) * 768], m.value, nr.value, nb.value


def debug_fastq_host_strip() -> int:
    return lib().finch_debug_fastq_host_strip()


def debug_file_batch():
    """(files sketched many-per-launch, files the batch path handed to a sketcher of their own) by this process so far"""
    a, b = C.c_uint64(), C.c_uint64()
    lib().finch_debug_file_batch(C.byref(a), C.byref(b))
    return a.value, b.value


def debug_kernel_times(enable: int = -1):
    """(sketch-kernel ms, launches, positions) over the inputs sketched since the hook was switched on; then enable = 1 switches
    it on and zeroes the sums, 0 off, -1 leaves it -- measurement hook"""
    ms, nl, npos = C.c_double(), C.c_uint64(), C.c_uint64()
    lib().finch_debug_kernel_times(enable, C.byref(ms), C.byref(nl), C.byref(npos))
    return ms.value, nl.value, npos.value


def source_probe(data: bytes, chunk: int, cap: int) -> bytes:
    """the (decompressed) byte stream the parsers see for an input image, read `chunk` bytes at a time (test hook)"""
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    buf = np.zeros(max(cap, 1), np.uint8)
    got = C.c_uint64()
    _check(lib().finch_source_probe(src.ctypes.data, len(data), chunk, buf.ctypes.data, cap, C.byref(got)))
    return buf[:got.value].tobytes()


def read_file_probe(path: str, chunk: int, read_threads: int, cap: int) -> bytes:
    """the bytes the text paths get from a plain file read in `chunk`-byte requests (test hook)"""
    buf = np.zeros(max(cap, 1), np.uint8)
    got = C.c_uint64()
    _check(lib().finch_read_file_probe(path.encode(), chunk, read_threads, buf.ctypes.data, cap, C.byref(got)))
    return buf[:got.value].tobytes()


def raw_distance(query_hashes, ref_hashes, scale: float = 0.0):
    """distance.rs:66-126 -> (containment, jaccard, common, total)"""
    q = np.ascontiguousarray(query_hashes, np.uint64)
    r = np.ascontiguousarray(ref_hashes, np.uint64)
    d = CDistance()
    _check(lib().finch_raw_distance(q.ctypes.data if len(q) else None, len(q), r.ctypes.data if len(r) else None, len(r), scale, C.byref(d)))
    return d.containment, d.jaccard, d.common_hashes, d.total_hashes


def distance(a: Sketches, ia: int, b: Sketches, ib: int, old_mode: bool = False):
    """distance.rs:9-47 -> dict(containment, jaccard, mash_distance, common_hashes, total_hashes)"""
    d = CDistance()
    _check(lib().finch_distance(a._p, ia, b._p, ib, int(old_mode), C.byref(d)))
    return {"containment": d.containment, "jaccard": d.jaccard, "mash_distance": d.mash_distance,
            "common_hashes": d.common_hashes, "total_hashes": d.total_hashes}


# one row of finch_dist: the indices of the pair, then finch_distance_out's fields
DIST_DTYPE = np.dtype([("query", np.uint32), ("reference", np.uint32), ("containment", np.float64), ("jaccard", np.float64),
                       ("mash_distance", np.float64), ("common_hashes", np.uint64), ("total_hashes", np.uint64)])
_CDIST_DTYPE = np.dtype([("containment", np.float64), ("jaccard", np.float64), ("mash_distance", np.float64),
                         ("common_hashes", np.uint64), ("total_hashes", np.uint64)])


def _dist_result(queries: Sketches, refs: Sketches, max_distance: float, old_mode: bool, devices: Sequence[int]):
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    out = _P()
    _check(lib().finch_dist(queries._p, refs._p, int(old_mode), float(max_distance), darr, len(devs), C.byref(out)))
    return out


def _dist_rows(p, stats: Optional[dict], from_index: bool = False) -> np.ndarray:
    """the rows of a finch_dist_result, which is freed"""
    L = lib()
    try:
        n = L.finch_dist_len(p)
        qi, ri, d = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, _CDIST_DTYPE)
        _check(L.finch_dist_copy(p, qi.ctypes.data, ri.ctypes.data, d.ctypes.data))
        if stats is not None:
            ms, nl = C.c_double(), C.c_uint64()
            _check(L.finch_dist_stats(p, C.byref(ms), C.byref(nl)))
            stats.update(kernel_ms=ms.value, launches=nl.value)
            if from_index:
                nt, nc = C.c_uint64(), C.c_uint64()
                _check(L.finch_index_dist_stats(p, C.byref(nt), C.byref(nc)))
                stats.update(pairs_touched=nt.value, pairs_copied=nc.value)
    finally:
        L.finch_dist_free(p)
    rows = np.empty(n, DIST_DTYPE)
    rows["query"], rows["reference"] = qi, ri
    for f in _CDIST_DTYPE.names:
        rows[f] = d[f]
    return rows


def _dist_text(p) -> str:
    """the JSON text of a finch_dist_result, which is freed"""
    L = lib()
    try:
        s, n = _P(), C.c_uint64()
        _check(L.finch_dist_to_json(p, C.byref(s), C.byref(n)))
        try:
            return C.string_at(s, n.value).decode()
        finally:
            L.finch_free_string(s)
    finally:
        L.finch_dist_free(p)


def dist(queries: Sketches, refs: Sketches, max_distance: float = 1.0, old_mode: bool = False, devices: Sequence[int] = (0,),
         stats: Optional[dict] = None) -> np.ndarray:
    """calc_sketch_distances (cli/src/main.rs:315-333) on the GPU: one DIST_DTYPE row per (query, reference) pair kept, in the
    reference's order (for each reference, for each query); `stats`, if given, receives the kernels' time and launches"""
    return _dist_rows(_dist_result(queries, refs, max_distance, old_mode, devices), stats)


def dist_json(queries: Sketches, refs: Sketches, max_distance: float = 1.0, old_mode: bool = False,
              devices: Sequence[int] = (0,)) -> str:
    """the same rows as serde_json::to_writer(&Vec<SketchDistance>) writes them (main.rs:117-121)"""
    return _dist_text(_dist_result(queries, refs, max_distance, old_mode, devices))


def select(sketches: Sketches, idx: Sequence[int]) -> Sketches:
    """the sketches idx, in that order, as a collection of their own"""
    a = np.ascontiguousarray(idx, np.uint32)
    out = _P()
    _check(lib().finch_sketches_select(sketches._p, a.ctypes.data if len(a) else None, len(a), C.byref(out)))
    return Sketches(out, sketches.params)


def minmer_matrix(refs: Sketches, ir: int, sketches: Sketches, devices: Sequence[int] = (0,), stats: Optional[dict] = None) -> np.ndarray:
    """minmer_matrix (distance.rs:345-364) on the GPU: the (len(sketches), hashes of refs[ir]) int32 matrix whose cell (i, p) is
    the count sketches[i] holds for the reference's p-th hash (a count >= 2^31 wraps negative, as `as i32` does), 0 where it
    does not have that hash; `stats`, if given, receives the kernels' time and launches"""
    L = lib()
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    out = np.empty((len(sketches), L.finch_sketch_n_hashes(refs._p, ir)), np.int32)
    ms, nl = C.c_double(), C.c_uint64()
    _check(L.finch_minmer_matrix(refs._p, ir, sketches._p, darr, len(devs), out.ctypes.data if out.size else None, out.size,
                                 C.byref(ms), C.byref(nl)))
    if stats is not None:
        stats.update(kernel_ms=ms.value, launches=nl.value)
    return out


def _search_rows(p, n_queries: int, stats: Optional[dict], from_index: bool = False):
    """(offsets, rows) of a finch_search_result, which is freed here"""
    L = lib()
    try:
        n = L.finch_search_len(p)
        offsets = np.zeros(n_queries + 1, np.uint64)
        _check(L.finch_search_offsets(p, offsets.ctypes.data))
        qi, ri, d = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, _CDIST_DTYPE)
        _check(L.finch_search_copy(p, qi.ctypes.data, ri.ctypes.data, d.ctypes.data))
        if stats is not None:
            ms, nl, nc = C.c_double(), C.c_uint64(), C.c_uint64()
            _check(L.finch_search_stats(p, C.byref(ms), C.byref(nl), C.byref(nc)))
            stats.update(kernel_ms=ms.value, launches=nl.value, candidates_copied=nc.value)
            if from_index:
                nt = C.c_uint64()
                _check(L.finch_index_search_stats(p, C.byref(nt)))
                stats.update(pairs_touched=nt.value)
    finally:
        L.finch_search_free(p)
    rows = np.empty(n, DIST_DTYPE)
    rows["query"], rows["reference"] = qi, ri
    for f in _CDIST_DTYPE.names:
        rows[f] = d[f]
    return offsets, rows


def search(queries: Sketches, refs: Sketches, min_containment: float = 0.0, top_n: int = 0, devices: Sequence[int] = (0,),
           stats: Optional[dict] = None):
    """per query the references with containment >= min_containment, best first (containment descending, then reference index
    ascending), at most top_n of them if top_n > 0 -> (offsets, rows): the DIST_DTYPE rows grouped by query in query order,
    query q's being rows[offsets[q]:offsets[q + 1]]; each row is what distance() gives for the pair.  The selection runs on the
    GPU; `stats`, if given, receives the kernels' time, the launches and the candidates that crossed to the host"""
    L = lib()
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    p = _P()
    _check(L.finch_search(queries._p, refs._p, float(min_containment), int(top_n), darr, len(devs), C.byref(p)))
    return _search_rows(p, len(queries), stats)


def best_match(refs: Sketches, queries: Sketches, iq: int = 0, devices: Sequence[int] = (0,)) -> int:
    """Multisketch.best_match (python.rs:202-216) of sketch iq of `queries` in the library `refs`: the index of the first
    reference with the largest containment, 0 if no containment is above 0; FinchError on an empty library (the reference
    indexes sketches[0] and panics)"""
    if len(refs) == 0:
        raise FinchError("best_match: the library has no sketches")
    _, rows = search(select(queries, [iq]), refs, 0.0, 1, devices)
    return int(rows["reference"][0])


def filter_to_matches(refs: Sketches, queries: Sketches, iq: int, threshold: float, devices: Sequence[int] = (0,)) -> Sketches:
    """Multisketch.filter_to_matches (python.rs:223-234): the references whose containment of sketch iq of `queries` is
    >= threshold, in library order, as a collection of their own"""
    _, rows = search(select(queries, [iq]), refs, threshold, 0, devices)
    return select(refs, np.sort(rows["reference"]))


SMALLEST_POSITIVE = 5e-324  # the smallest positive double: the threshold "any shared hash that counts"


class LibraryIndex:
    """an inverted index of the library `refs` on the GPU (finch_index_new): built once, searched many times.  For
    min_containment > 0, .search(queries, min_containment, top_n) == search(queries, refs, min_containment, top_n), byte for
    byte, at a cost that follows the pairs that share a hash instead of len(queries) x len(refs).  The index keeps its own copy
    of what it needs on the device (`refs` itself for filter_to_matches' result and for dist's rows); a context manager, or
    .close().  .refs is the library of the index at any time: .add() appends to the object it holds -- the caller's, until the
    first .keep() --, .keep() and what is built on it put a new collection there and leave the caller's object as it was.  Read
    the library from .refs after an update, not from the object the index was made from"""

    def __init__(self, refs: Sketches, devices: Sequence[int] = (0,)):
        devs = list(devices) if devices else [0]
        darr = (C.c_int * len(devs))(*devs)
        self._p, self.refs = _P(), refs
        _check(lib().finch_index_new(refs._p, darr, len(devs), C.byref(self._p)))

    def close(self) -> None:
        if getattr(self, "_p", None) and lib is not None:  # module globals are gone at interpreter shutdown
            lib().finch_index_free(self._p)
        self._p = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if not self._p:
            raise FinchError("the index is closed")
        return self._p

    def stats(self) -> dict:
        nr, np_, nb, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _check(lib().finch_index_stats(self._handle(), C.byref(nr), C.byref(np_), C.byref(nb), C.byref(ms)))
        return dict(n_refs=nr.value, postings=np_.value, device_bytes=nb.value, build_kernel_ms=ms.value)

    def search(self, queries: Sketches, min_containment: float, top_n: int = 0, stats: Optional[dict] = None):
        """search()'s (offsets, rows) for a threshold above 0 (FinchError for one <= 0: the index cannot see the pairs that share
        nothing); `stats` receives search()'s figures and pairs_touched, the pairs the device counted"""
        p = _P()
        _check(lib().finch_index_search(self._handle(), queries._p, float(min_containment), int(top_n), C.byref(p)))
        return _search_rows(p, len(queries), stats, from_index=True)

    def _dist_result(self, queries: Optional[Sketches], max_distance: float, old_mode: bool):
        p = _P()
        _check(lib().finch_index_dist(self._handle(), self.refs._p, queries._p if queries is not None else None, int(old_mode),
                                      float(max_distance), C.byref(p)))
        return p

    def dist(self, queries: Optional[Sketches] = None, max_distance: float = 0.1, old_mode: bool = False,
             stats: Optional[dict] = None) -> np.ndarray:
        """dist(queries, refs, max_distance, old_mode)'s rows, byte for byte, for a bound below 1 (FinchError for one >= 1: the
        index cannot see the pairs that share nothing); queries=None is pairwise, dist(refs, refs, ...), read from the index's own
        copy of the library.  `stats` receives dist()'s figures, pairs_touched (the pairs the device counted) and pairs_copied
        (those that passed the device's pre-filter)"""
        return _dist_rows(self._dist_result(queries, max_distance, old_mode), stats, from_index=True)

    def dist_json(self, queries: Optional[Sketches] = None, max_distance: float = 0.1, old_mode: bool = False) -> str:
        """dist_json(queries, refs, max_distance, old_mode)'s text for a bound below 1"""
        return _dist_text(self._dist_result(queries, max_distance, old_mode))

    def cluster(self, max_distance: float = 0.1, old_mode: bool = False, stats: Optional[dict] = None) -> np.ndarray:
        """single-linkage clusters of the library at `max_distance` (finch_index_cluster): a uint32 array over self.refs,
        labels[v] = the smallest index of v's component, where a and b are linked when dist(refs, refs, max_distance, old_mode)
        has the row (a, b) or (b, a) -- cluster_host()'s answer for a bound below 1 (FinchError for one >= 1).  The device unites
        the pairs that are surely within the bound and only a narrow band crosses to the host's exact test.  `stats` receives
        finch_cluster_stats' fields"""
        labels = np.empty(len(self.refs), np.uint32)
        st = CClusterStats()
        _check(lib().finch_index_cluster(self._handle(), self.refs._p, int(old_mode), float(max_distance),
                                         labels.ctypes.data_as(C.POINTER(C.c_uint32)), len(labels), C.byref(st)))
        if stats is not None:
            stats.update({f: getattr(st, f) for f, _ in CClusterStats._fields_})
        return labels

    def dereplicate(self, max_distance: float = 0.1, old_mode: bool = False) -> np.ndarray:
        """cluster(), then keep(np.unique(labels)): self.refs is afterwards one sketch per cluster, its lowest-indexed member, in
        library order -> the labels as they were before the keep.  Single linkage: a cluster's members are chained to its
        survivor, not each within the bound of it"""
        labels = self.cluster(max_distance, old_mode)
        self.keep(np.unique(labels))
        return labels

    def gather(self, queries: Sketches, min_overlap: int = 1, max_rounds: int = 0, stats: Optional[dict] = None):
        """gather(queries, refs, min_overlap, max_rounds)'s (offsets, rows), byte for byte, the rounds over the index's live
        counters (finch_index_gather); `stats` receives gather()'s figures and pairs_touched, the pairs the device counted"""
        p = _P()
        _check(lib().finch_index_gather(self._handle(), queries._p, int(min_overlap), int(max_rounds), C.byref(p)))
        return _gather_rows(p, len(queries), stats, from_index=True)

    def attach_counts(self) -> int:
        """the `count` column of the library to every device entry of the index (finch_index_attach_counts), which holds only the
        hashes until then; calling it again replaces what is there -> the bytes the attachment holds"""
        nb = C.c_uint64()
        _check(lib().finch_index_attach_counts(self._handle(), self.refs._p, C.byref(nb)))
        self._counts_attached = True
        return nb.value

    def compare_counts(self, queries: Sketches, min_common: int = 1, stats: Optional[dict] = None) -> np.ndarray:
        """compare_counts(refs, queries, min_common)'s rows, byte for byte, for min_common >= 1 (FinchError below that: the index
        cannot see the pairs that share nothing); only the pairs that pass are walked (finch_index_compare_counts).  The
        library's counts are attached on first use.  `stats` receives compare_counts()'s figures, pairs_touched (the pairs the
        device counted) and pairs_walked (the pairs whose moments it computed)"""
        if int(min_common) < 1:
            raise FinchError("LibraryIndex.compare_counts: min_common %d keeps pairs that share nothing, which an index cannot "
                             "enumerate -- use compare_counts" % int(min_common))
        h = self._handle()
        if not getattr(self, "_counts_attached", False):
            self.attach_counts()
        p = _P()
        _check(lib().finch_index_compare_counts(h, queries._p, min(int(min_common), 2 ** 64 - 1), C.byref(p)))
        return _counts_rows(p, stats, from_index=True)

    def screen(self, inputs, kmer_length: Optional[int] = None, hash_seed: Optional[int] = None, min_shared: int = 1,
               n_threads: int = 0, stats: Optional[dict] = None) -> np.ndarray:
        """containment of every reference in RAW READS (finch_index_screen; what `mash screen` is reached for): `inputs` -- a
        path, a sequence of paths, or the bytes of one input; FASTA or FASTQ, plain or compressed -- is read as one sample, every
        k-mer of it is hashed and looked up among the library's hashes -> SCREEN_DTYPE rows, one per reference that holds at
        least max(1, min_shared) hashes of the sample, in library order: shared, sum_mult, median_mult (the lower median of the
        shared hashes' multiplicities), ref_len, containment = shared / ref_len; == screen_host(self.refs, data, ...), byte for
        byte.  mash screen's identity is rows["containment"] ** (1 / kmer_length).  kmer_length / hash_seed default to those
        of the library's sketches, which must then agree among themselves (FinchError).  `stats` receives finch_screen_stats'
        figures"""
        if kmer_length is None or hash_seed is None:
            ps = {(q.kmer_length, q.hash_seed) for q in (self.refs.params_of(i) for i in range(len(self.refs)))}
            if not ps:
                raise FinchError("LibraryIndex.screen: the library has no sketches to take kmer_length and hash_seed from; name them")
            if len(ps) != 1:
                raise FinchError("LibraryIndex.screen: the library's sketches have %d different (kmer_length, hash_seed); name the "
                                 "sample's" % len(ps))
            k0, s0 = next(iter(ps))
            kmer_length = k0 if kmer_length is None else kmer_length
            hash_seed = s0 if hash_seed is None else hash_seed
        p = _P()
        if isinstance(inputs, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(inputs, dtype=np.uint8)
            _check(lib().finch_index_screen_buffer(self._handle(), buf.ctypes.data if len(buf) else None, len(buf), int(kmer_length),
                                                   int(hash_seed), int(min_shared), int(n_threads), C.byref(p)))
        else:
            paths = [inputs] if isinstance(inputs, str) else list(inputs)
            arr = (C.c_char_p * len(paths))(*[f.encode() for f in paths])
            _check(lib().finch_index_screen(self._handle(), arr, len(paths), int(kmer_length), int(hash_seed), int(min_shared),
                                            int(n_threads), C.byref(p)))
        return _screen_rows(p, stats)

    def add(self, more: Sketches, stats: Optional[dict] = None) -> None:
        """Multisketch.add (python.rs:191-194): the sketches of `more` after the library's last one, in the index
        (finch_index_add: a merge on the device, nothing of the old library crosses the link) and in self.refs, which grows
        as the Multisketch does: self.refs is appended to in place, and that is the caller's own object as long as no keep()
        has replaced it.  `more` must be another object than self.refs (FinchError).  Attached counts are extended.  `stats`
        receives kernel_ms, the update kernels' time"""
        if more is self.refs:
            raise FinchError("LibraryIndex.add: `more` is the library itself; add a copy (select(refs, range(len(refs))))")
        ms = C.c_double()
        _check(lib().finch_index_add(self._handle(), more._p, C.byref(ms)))
        self.refs.append(more)
        if stats is not None:
            stats.update(kernel_ms=ms.value)

    def keep(self, idx, stats: Optional[dict] = None) -> None:
        """the library becomes select(refs, idx), idx strictly ascending (FinchError otherwise: the order of a library is
        kept, as Multisketch.__delitem__, filter_to_matches and filter_to_names keep it), in the index (finch_index_keep: a
        compaction on the device) and in self.refs, which becomes a NEW collection: an object the index was made from, or
        that add() grew, stays as it is and no longer follows the index.  Attached counts are compacted.  `stats` receives
        kernel_ms"""
        idx = np.ascontiguousarray(idx, np.int64).ravel()
        if len(idx) and (idx.min() < 0 or idx.max() >= 2 ** 32):
            raise FinchError("LibraryIndex.keep: index %d out of range" % (idx.min() if idx.min() < 0 else idx.max()))
        arr = idx.astype(np.uint32)
        ms = C.c_double()
        _check(lib().finch_index_keep(self._handle(), arr.ctypes.data_as(C.POINTER(C.c_uint32)) if len(arr) else None, len(arr), C.byref(ms)))
        self.refs = select(self.refs, arr)
        if stats is not None:
            stats.update(kernel_ms=ms.value)

    def filter_to_names(self, names, stats: Optional[dict] = None) -> None:
        """Multisketch.filter_to_names (python.rs:242-248): keep the sketches whose name is listed, in library order"""
        wanted, L = set(names), lib()
        self.keep([i for i in range(len(self.refs)) if L.finch_sketch_name(self.refs._p, i).decode() in wanted], stats)

    def delete(self, i: int, stats: Optional[dict] = None) -> None:
        """Multisketch.__delitem__ (python.rs:158-164): keep every sketch but sketch i (a negative i counts from the end)"""
        n = len(self.refs)
        if not -n <= i < n:
            raise FinchError("LibraryIndex.delete: index %d out of range for %d sketches" % (i, n))
        self.keep([j for j in range(n) if j != i % n], stats)

    def best_match(self, queries: Sketches, iq: int = 0) -> int:
        """best_match(refs, queries, iq): a top-1 search at the smallest positive threshold; a query that shares nothing with
        the library has no row and gets index 0, as the tie rule gives it there"""
        if len(self.refs) == 0:
            raise FinchError("best_match: the library has no sketches")
        _, rows = self.search(select(queries, [iq]), SMALLEST_POSITIVE, 1)
        return int(rows["reference"][0]) if len(rows) else 0

    def filter_to_matches(self, queries: Sketches, iq: int, threshold: float) -> Sketches:
        """filter_to_matches(refs, queries, iq, threshold); a threshold <= 0 keeps every reference and needs no device"""
        if threshold <= 0:
            self._handle()
            return select(self.refs, np.arange(len(self.refs)))
        _, rows = self.search(select(queries, [iq]), threshold, 0)
        return select(self.refs, np.sort(rows["reference"]))


# one row of finch_gather / finch_gather_query: finch_gather_row's nine integers and five doubles
GATHER_DTYPE = np.dtype([(f, np.uint64) for f in ("query", "reference", "round", "overlap", "common", "ref_len", "query_len", "abund",
                                                   "remaining")] +
                        [(f, np.float64) for f in ("f_unique_to_query", "f_orig_query", "f_match", "average_abund", "f_unique_weighted")])


# one row of finch_index_screen / finch_screen_host: finch_screen_row
SCREEN_DTYPE = np.dtype([("reference", np.uint32), ("shared", np.uint32), ("ref_len", np.uint32), ("reserved", np.uint32),
                         ("median_mult", np.uint64), ("sum_mult", np.uint64), ("containment", np.float64)])
assert SCREEN_DTYPE.itemsize == C.sizeof(CScreenRow)


def _screen_rows(p, stats: Optional[dict]) -> np.ndarray:
    L = lib()
    try:
        rows = np.zeros(L.finch_screen_len(p), SCREEN_DTYPE)
        _check(L.finch_screen_copy(p, rows.ctypes.data if len(rows) else None))
        if stats is not None:
            u = [C.c_uint64() for _ in range(6)]
            d = [C.c_double(), C.c_double()]
            _check(L.finch_screen_stats(p, *[C.byref(x) for x in u[:5]], C.byref(d[0]), C.byref(d[1]), C.byref(u[5])))
            stats.update(positions=u[0].value, kmers=u[1].value, hits=u[2].value, distinct=u[3].value, table_bytes=u[4].value,
                         table_ms=d[0].value, kernel_ms=d[1].value, launches=u[5].value)
        return rows
    finally:
        L.finch_screen_free(p)


def screen_host(refs: Sketches, data: bytes, kmer_length: int, hash_seed: int = 0, min_shared: int = 1,
                stats: Optional[dict] = None) -> np.ndarray:
    """finch_screen_host: the screen's contract on the host with a hash map, no device -> SCREEN_DTYPE rows; `data` is the
    image of one input, container included"""
    buf = np.frombuffer(data, dtype=np.uint8)
    p = _P()
    _check(lib().finch_screen_host(refs._p, buf.ctypes.data if len(buf) else None, len(buf), int(kmer_length), int(hash_seed),
                                   int(min_shared), C.byref(p)))
    return _screen_rows(p, stats)


def cluster_host(sketches: Sketches, max_distance: float, old_mode: bool = False, edges: Optional[list] = None) -> np.ndarray:
    """finch_cluster_host: the clustering contract on the host, every ordered pair -> labels (uint32, labels[v] = the smallest
    index of v's component); `edges`, a list, is appended the number of ordered pairs q != r within the bound"""
    labels = np.empty(len(sketches), np.uint32)
    n = C.c_uint64()
    _check(lib().finch_cluster_host(sketches._p, int(old_mode), float(max_distance), labels.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    len(labels), C.byref(n)))
    if edges is not None:
        edges.append(n.value)
    return labels


def gather_query(refs: Sketches, queries: Sketches, iq: int, min_overlap: int = 1, max_rounds: int = 0) -> np.ndarray:
    """the greedy decomposition of sketch iq of `queries` over the library `refs` on the host, the loop as the contract
    (include/finch_host.h) reads -> GATHER_DTYPE rows in round order: round t takes the reference that shares the most hashes
    with what is left of the query (ties: the lowest index), at least min_overlap (below 1: 1) of them, and removes its hashes
    from the query; at most max_rounds rounds if max_rounds > 0"""
    rows = np.zeros(len(refs), GATHER_DTYPE)  # (a reference is never taken twice)
    n = C.c_uint64()
    _check(lib().finch_gather_query(refs._p, queries._p, int(iq), int(min_overlap), int(max_rounds), rows.ctypes.data if len(rows) else None,
                                    len(rows), C.byref(n)))
    return rows[:n.value]


def _gather_rows(p, n_queries: int, stats: Optional[dict], from_index: bool = False):
    """(offsets, rows) of a finch_gather_result, which is freed here"""
    L = lib()
    try:
        n = L.finch_gather_len(p)
        offsets = np.zeros(n_queries + 1, np.uint64)
        _check(L.finch_gather_offsets(p, offsets.ctypes.data))
        rows = np.empty(n, GATHER_DTYPE)
        _check(L.finch_gather_copy(p, None, None, rows.ctypes.data))
        if stats is not None:
            ms, nl, nc, nrec = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            _check(L.finch_gather_stats(p, C.byref(ms), C.byref(nl), C.byref(nc), C.byref(nrec)))
            stats.update(kernel_ms=ms.value, launches=nl.value, candidates=nc.value, records_copied=nrec.value)
            if from_index:
                nt = C.c_uint64()
                _check(L.finch_index_gather_stats(p, C.byref(nt)))
                stats.update(pairs_touched=nt.value)
    finally:
        L.finch_gather_free(p)
    return offsets, rows


def gather(queries: Sketches, refs: Sketches, min_overlap: int = 1, max_rounds: int = 0, devices: Sequence[int] = (0,),
           stats: Optional[dict] = None):
    """gather_query for every query, the loop on the GPU -> (offsets, rows): the GATHER_DTYPE rows grouped by query in query order,
    query q's being rows[offsets[q]:offsets[q + 1]] in round order; every field is what gather_query gives.  `stats`, if given,
    receives the kernels' time, the kernel launches, the candidates (pairs that share at least min_overlap hashes) and the records
    that crossed to the host (exactly the rows)"""
    L = lib()
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    p = _P()
    _check(L.finch_gather(queries._p, refs._p, int(min_overlap), int(max_rounds), darr, len(devs), C.byref(p)))
    return _gather_rows(p, len(queries), stats)


# one row of finch_compare_counts: the indices of the pair, then finch_count_moments' fields
_CMOMENTS_DTYPE = np.dtype([("common", np.uint64), ("ref_pos", np.uint64), ("query_pos", np.uint64), ("ref_count", np.uint64),
                            ("query_count", np.uint64), ("var", np.float64), ("skew", np.float64), ("kurt", np.float64)])
COUNTS_DTYPE = np.dtype([("query", np.uint32), ("reference", np.uint32)] + _CMOMENTS_DTYPE.descr)


def compare_counts_pair(refs: Sketches, ir: int, queries: Sketches, iq: int):
    """Sketch.compare_counts (python.rs:496-559) of one pair on the host, the reference's loop as written ->
    (common, ref_pos, query_pos, ref_count, query_count, var, skew, kurt)"""
    m = CCountMoments()
    _check(lib().finch_compare_counts_pair(refs._p, ir, queries._p, iq, C.byref(m)))
    return (m.common, m.ref_pos, m.query_pos, m.ref_count, m.query_count, m.var, m.skew, m.kurt)


def _counts_rows(p, stats: Optional[dict], from_index: bool = False) -> np.ndarray:
    """the COUNTS_DTYPE rows of a finch_compare_counts_result, which is freed here"""
    L = lib()
    try:
        n = L.finch_compare_counts_len(p)
        qi, ri, m = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, _CMOMENTS_DTYPE)
        _check(L.finch_compare_counts_copy(p, ri.ctypes.data, qi.ctypes.data, m.ctypes.data))
        if stats is not None:
            ms, nl, nc = C.c_double(), C.c_uint64(), C.c_uint64()
            _check(L.finch_compare_counts_stats(p, C.byref(ms), C.byref(nl), C.byref(nc)))
            stats.update(kernel_ms=ms.value, launches=nl.value, records_copied=nc.value)
            if from_index:
                nt, nw = C.c_uint64(), C.c_uint64()
                _check(L.finch_index_compare_counts_stats(p, C.byref(nt), C.byref(nw)))
                stats.update(pairs_touched=nt.value, pairs_walked=nw.value)
    finally:
        L.finch_compare_counts_free(p)
    rows = np.empty(n, COUNTS_DTYPE)
    rows["query"], rows["reference"] = qi, ri
    for f in _CMOMENTS_DTYPE.names:
        rows[f] = m[f]
    return rows


def compare_counts(refs: Sketches, queries: Sketches, min_common: int = 0, devices: Sequence[int] = (0,),
                   stats: Optional[dict] = None) -> np.ndarray:
    """Sketch.compare_counts for every (query, reference) pair with common >= min_common, on the GPU: COUNTS_DTYPE rows ordered by
    query, then by reference index; each row's values are what compare_counts_pair gives for the pair.  `stats`, if given,
    receives the kernels' time, the launches and the records that crossed to the host"""
    L = lib()
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    p = _P()
    _check(L.finch_compare_counts(refs._p, queries._p, int(min_common), darr, len(devs), C.byref(p)))
    return _counts_rows(p, stats)


def merge_pair(a: Sketches, ia: int, b: Sketches, ib: int, size: Optional[int] = None) -> Sketches:
    """Sketch.merge (merge_sketches, python.rs:24-100) of one pair on the host, the reference's loop as written: a one-sketch
    collection holding sketch ia of `a` merged with sketch ib of `b` and clipped by (size, the first sketch's scale)"""
    out = _P()
    sz = C.c_uint64(size) if size is not None else None
    _check(lib().finch_merge_pair(a._p, ia, b._p, ib, C.byref(sz) if sz is not None else None, C.byref(out)))
    return Sketches(out, a.params)


def merge(sketches: Sketches, groups: Sequence[Sequence[int]], size: Optional[int] = None, devices: Sequence[int] = (0,),
          stats: Optional[dict] = None) -> Sketches:
    """Sketch.merge folded over groups of sketches on the GPU: result g is sketches[groups[g][0]] merged with groups[g][1], then
    with groups[g][2], ..., each merge with the same `size` -- what folding merge_pair gives, field by field; a group of one
    member is that member.  `stats`, if given, receives the kernels' time, the launches, the records that crossed to the host
    and the wall times of the upload, the copies back and the k-mer gather"""
    offsets = np.zeros(len(groups) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64) if len(groups) else []
    flat = [int(i) for g in groups for i in g]
    if any(not 0 <= i < 2 ** 32 for i in flat):
        raise FinchError("merge: a member index is not a u32")
    mem = np.asarray(flat, np.uint32) if flat else np.zeros(1, np.uint32)
    devs = list(devices) if devices else [0]
    darr = (C.c_int * len(devs))(*devs)
    sz = C.c_uint64(size) if size is not None else None
    out, ms, nl, nc, ph = _P(), C.c_double(), C.c_uint64(), C.c_uint64(), (C.c_double * 3)()
    _check(lib().finch_merge_groups(sketches._p, offsets.ctypes.data, mem.ctypes.data, len(groups), C.byref(sz) if sz is not None else None,
                                    darr, len(devs), C.byref(out), C.byref(ms), C.byref(nl), C.byref(nc), ph))
    if stats is not None:
        stats.update(kernel_ms=ms.value, launches=nl.value, records_copied=nc.value, upload_ms=ph[0], copy_ms=ph[1], gather_ms=ph[2])
    return Sketches(out, sketches.params)


def counts(sk: Sketches, i: int) -> np.ndarray:
    """Sketch.counts (python.rs:579-583): the counts of sketch i, each u32 as i32"""
    L = lib()
    if not 0 <= i < len(sk):
        raise FinchError("sketch %d of %d" % (i, len(sk)))
    cs = np.zeros(L.finch_sketch_n_hashes(sk._p, i), np.uint32)
    _check(L.finch_sketch_copy(sk._p, i, None, cs.ctypes.data, None, None))
    return cs.view(np.int32)


def dist_queries(names: Sequence[str], pairwise: bool = False, queries=None) -> Optional[List[int]]:
    """the query selection of the `dist` subcommand (main.rs:90-113): None = every sketch (--pairwise), else the indices of
    the sketches whose name is in `queries` (--queries), else the first sketch"""
    if pairwise:
        return None
    if queries is not None:
        wanted = set(queries)
        return [i for i, n in enumerate(names) if n in wanted]
    if not names:
        raise FinchError("No sketches present!")
    return [0]


def dist_command(sketches: Sketches, pairwise: bool = False, queries=None, max_distance: float = 1.0, old_mode: bool = False,
                 devices: Sequence[int] = (0,)) -> np.ndarray:
    """`finch dist` over already opened sketches (main.rs:85-125): DIST_DTYPE rows whose query and reference both index
    `sketches`"""
    names = [lib().finch_sketch_name(sketches._p, i).decode(errors="surrogateescape") for i in range(len(sketches))]
    idx = dist_queries(names, pairwise, queries)
    if idx is None:
        return dist(sketches, sketches, max_distance, old_mode, devices)
    rows = dist(select(sketches, idx), sketches, max_distance, old_mode, devices)
    rows["query"] = np.asarray(idx, np.uint32)[rows["query"]] if len(idx) else rows["query"]
    return rows
