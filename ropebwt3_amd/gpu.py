"""ctypes binding of the C ABI in include/rb3gpu.h (librb3gpu.so).

This module mirrors the reference's call surface for the merge path: `Rb3Gpu` stands where
an `mrope_t*` stands in build.c, with `from_plain` = rb3_enc_plain2fmr (fm-index.c:114),
`merge_plain` = rb3_fmi_merge_plain (fm-index.c:279), `get_acc` = rb3_fmi_get_acc and
`export_runs` = the leaf iteration of rb3_enc_fmr2fmd (fm-index.c:31-54).

There is NO CPU fallback: importing works anywhere, but creating a handle raises when the
shared object or a HIP device is missing.
"""
import ctypes
import os

import numpy as np

from . import _build

ASIZE = 6

_ERR = {0: "OK", -1: "ENODEV", -2: "ENOMEM", -3: "EINVAL", -4: "ESYMBOL", -5: "ESTATE", -6: "EINTERNAL", -7: "EUNSUP"}


class Rb3GpuError(RuntimeError):
    def __init__(self, code, what):
        RuntimeError.__init__(self, "%s failed: %s (%d)" % (what, _ERR.get(code, "?"), code))
        self.code = code


class Opt(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("split_log2", ctypes.c_int32), ("verbose", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Stats(ctypes.Structure):
    _fields_ = [("ms_h2d", ctypes.c_double), ("ms_lf", ctypes.c_double), ("ms_rank", ctypes.c_double),
                ("ms_build", ctypes.c_double), ("ms_export", ctypes.c_double), ("ms_chain", ctypes.c_double),
                ("n_rank_launches", ctypes.c_int64), ("n_lf_steps", ctypes.c_int64), ("n_symbols_merged", ctypes.c_int64),
                ("n_rounds", ctypes.c_int64), ("n_fallbacks", ctypes.c_int64), ("bytes_index", ctypes.c_int64), ("bytes_peak", ctypes.c_int64),
                ("ms_ssa", ctypes.c_double), ("ms_ssa_walk", ctypes.c_double), ("ms_sort", ctypes.c_double), ("n_sort_rounds", ctypes.c_int64),
                ("n_reb_groups", ctypes.c_int64), ("n_reb_groups_window", ctypes.c_int64), ("n_lf_checked", ctypes.c_int64), ("n_long_settles", ctypes.c_int64), ("ms_alloc", ctypes.c_double), ("n_allocs", ctypes.c_int64), ("n_reb_again", ctypes.c_int64), ("bytes_rebuild", ctypes.c_int64), ("n_thinned", ctypes.c_int64), ("tent_mask_bits", ctypes.c_int64), ("n_junctions_checked", ctypes.c_int64), ("n_peer_rounds", ctypes.c_int64), ("n_reb_groups_tier2", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


EMIT_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64)
EMITW_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64)
EMIT_WORDS_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64)
EMIT_BYTES_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint8))


class BreStats(ctypes.Structure):
    """rb3gpu_bre_stats_t"""
    _fields_ = [("n_rec", ctypes.c_int64), ("n_sym", ctypes.c_int64), ("n_run", ctypes.c_int64), ("n_pieces", ctypes.c_int64),
                ("ms_scan", ctypes.c_double), ("ms_pack", ctypes.c_double), ("ms_fill", ctypes.c_double)]


KOUNT_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64))


class KountStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_expand", ctypes.c_double), ("n_nodes", ctypes.c_int64), ("n_out", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

MEM_REC = np.dtype([("query", "<i8"), ("x0", "<i8"), ("size", "<i8"), ("st", "<i4"), ("en", "<i4")])  # rb3gpu_mem_rec_t
MEM_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)


class MemStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_walk", ctypes.c_double), ("n_steps", ctypes.c_int64), ("n_walkers", ctypes.c_int64), ("n_records", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

HAPDIV_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p)
SW_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
SW_HIT = np.dtype([("lo", "<i8"), ("hi", "<i8"), ("score", "<i4"), ("qlen", "<i4"), ("rlen", "<i4"), ("n_steps", "<i4"), ("step_off", "<i8"), ("pos_off", "<i8"),
                   ("n_pos", "<i8")])  # rb3gpu_sw_hit_t
SW_OPS = b"=XID"   # the operation of a step byte is its high nibble, the base of the index (1..5) its low one


class SwOpt(ctypes.Structure):
    _fields_ = [("n_best", ctypes.c_int32), ("min_sc", ctypes.c_int32), ("match", ctypes.c_int32), ("mis", ctypes.c_int32), ("gap_open", ctypes.c_int32),
                ("gap_ext", ctypes.c_int32), ("e2e_drop", ctypes.c_int32), ("end_len", ctypes.c_int32), ("max_pos", ctypes.c_int64)]


class SwStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_dp", ctypes.c_double), ("ms_backtrack", ctypes.c_double), ("n_ext", ctypes.c_int64), ("n_hits", ctypes.c_int64),
                ("n_steps", ctypes.c_int64), ("n_tier2", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SwlStats(ctypes.Structure):
    _fields_ = [("sw", SwStats), ("n_nodes", ctypes.c_int64), ("n_edges", ctypes.c_int64)]

    def as_dict(self):
        d = self.sw.as_dict()
        d.update(n_nodes=self.n_nodes, n_edges=self.n_edges)
        return d


class HapdivOpt(ctypes.Structure):
    _fields_ = [("n_best", ctypes.c_int32), ("min_sc", ctypes.c_int32), ("match", ctypes.c_int32), ("mis", ctypes.c_int32), ("gap_open", ctypes.c_int32),
                ("gap_ext", ctypes.c_int32), ("e2e_drop", ctypes.c_int32)]


class HapdivStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_dp", ctypes.c_double), ("n_ext", ctypes.c_int64), ("n_windows", ctypes.c_int64), ("n_tier2", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

POS = np.dtype([("sid", "<i8"), ("pos", "<i8")])  # rb3gpu_pos_t
LOCATE_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)
MEM_POS_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)


class LocateStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_locate", ctypes.c_double), ("n_pops", ctypes.c_int64), ("n_intervals", ctypes.c_int64), ("n_tier2", ctypes.c_int64),
                ("max_heap", ctypes.c_int64), ("n_pairs", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

SUFFIX_REC = np.dtype([("start", "<i8"), ("size", "<i8")])  # rb3gpu_suffix_rec_t
SUFFIX_OUT = np.dtype([("query", "<i8"), ("start", "<i8"), ("length", "<i8"), ("size", "<i8")])  # what Rb3Gpu.suffix returns
RETRIEVE_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)


class SuffixStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_walk", ctypes.c_double), ("n_queries", ctypes.c_int64), ("n_symbols", ctypes.c_int64), ("n_steps", ctypes.c_int64),
                ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SeedStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_walk", ctypes.c_double), ("n_queries", ctypes.c_int64), ("n_present", ctypes.c_int64), ("n_walkers", ctypes.c_int64),
                ("n_steps", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RetrieveStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_count", ctypes.c_double), ("ms_emit", ctypes.c_double), ("n_rows", ctypes.c_int64), ("n_symbols", ctypes.c_int64),
                ("n_steps", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

class PiecesStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_pieces", ctypes.c_double), ("ms_join", ctypes.c_double), ("ms_sort", ctypes.c_double), ("ms_emit", ctypes.c_double),
                ("n_rows", ctypes.c_int64), ("n_symbols", ctypes.c_int64), ("n_slices", ctypes.c_int64), ("n_pieces", ctypes.c_int64), ("n_steps", ctypes.c_int64),
                ("max_piece_steps", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RemoveStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_mark", ctypes.c_double), ("ms_build", ctypes.c_double), ("n_strings", ctypes.c_int64), ("n_rows", ctypes.c_int64),
                ("n_steps", ctypes.c_int64), ("n_pieces", ctypes.c_int64), ("max_piece_steps", ctypes.c_int64), ("removed", ctypes.c_int64 * 6)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "removed" else getattr(self, k)) for k, _ in self._fields_}


DEDUP_REC = np.dtype([("occ", "<i8"), ("copies", "<i8"), ("cls", "<i8")])  # rb3gpu_dedup_rec_t


class DedupStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_walk", ctypes.c_double), ("n_strings", ctypes.c_int64), ("n_steps", ctypes.c_int64), ("n_early", ctypes.c_int64),
                ("n_dup", ctypes.c_int64), ("n_contained", ctypes.c_int64), ("n_classes", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


OVERLAP_REC = np.dtype([("a", "<i4"), ("b", "<i4"), ("len", "<i4"), ("len_b", "<i4")])  # rb3gpu_overlap_rec_t
OVERLAP_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)


class OverlapStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_count", ctypes.c_double), ("ms_who", ctypes.c_double), ("ms_emit", ctypes.c_double), ("n_strings", ctypes.c_int64),
                ("n_steps_count", ctypes.c_int64), ("n_steps_emit", ctypes.c_int64), ("n_early", ctypes.c_int64), ("n_hits", ctypes.c_int64), ("n_groups", ctypes.c_int64),
                ("n_capped_groups", ctypes.c_int64), ("n_capped_hits", ctypes.c_int64), ("n_emitters", ctypes.c_int64), ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReduceStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_count", ctypes.c_double), ("ms_who", ctypes.c_double), ("ms_emit", ctypes.c_double), ("ms_reduce", ctypes.c_double),
                ("ms_compact", ctypes.c_double), ("n_strings", ctypes.c_int64), ("n_hits", ctypes.c_int64), ("n_kept", ctypes.c_int64), ("n_groups", ctypes.c_int64),
                ("n_capped_groups", ctypes.c_int64), ("n_capped_hits", ctypes.c_int64), ("n_emitters", ctypes.c_int64), ("n_slices", ctypes.c_int64),
                ("resident_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


UNITIG_REC = np.dtype([("head", "<i4"), ("tail", "<i4"), ("members", "<i4"), ("circ", "<i4"), ("len", "<i8")])  # rb3gpu_unitig_t
UNITIG_MEMBER = np.dtype([("row", "<i4"), ("o_in", "<i4"), ("off", "<i8")])  # rb3gpu_unitig_member_t
UNITIG_LINK = np.dtype([("from", "<i4"), ("to", "<i4"), ("len", "<i4"), ("from_rev", "u1"), ("to_rev", "u1"), ("pad", "u1", (2,))])  # rb3gpu_unitig_link_t
UNITIG_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
UNITIG_LINK_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)


class UnitigStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_reduce", ctypes.c_double), ("ms_graph", ctypes.c_double), ("ms_rank", ctypes.c_double), ("ms_emit", ctypes.c_double),
                ("n_strings", ctypes.c_int64), ("n_kept", ctypes.c_int64), ("n_simple", ctypes.c_int64), ("n_unitigs", ctypes.c_int64), ("n_members", ctypes.c_int64),
                ("n_symbols", ctypes.c_int64), ("n_steps_emit", ctypes.c_int64), ("n_cycles", ctypes.c_int64), ("n_asym", ctypes.c_int64), ("n_links", ctypes.c_int64),
                ("n_rounds", ctypes.c_int64), ("max_members", ctypes.c_int64), ("n_slices", ctypes.c_int64), ("resident_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FetchStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_table", ctypes.c_double), ("ms_plan", ctypes.c_double), ("ms_walk", ctypes.c_double), ("n_regions", ctypes.c_int64),
                ("n_symbols", ctypes.c_int64), ("n_walkers", ctypes.c_int64), ("n_measured", ctypes.c_int64), ("n_steps", ctypes.c_int64), ("max_walk_steps", ctypes.c_int64),
                ("n_slices", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


FETCH_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)

# name -> (restype, argtypes); every symbol declared in include/rb3gpu.h
SYMBOLS = {
    "rb3gpu_opt_init": (None, [ctypes.POINTER(Opt)]),
    "rb3gpu_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "rb3gpu_create": (ctypes.c_void_p, [ctypes.POINTER(Opt)]),
    "rb3gpu_destroy": (None, [ctypes.c_void_p]),
    "rb3gpu_from_plain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_merge_plain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_from_plain_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_merge_plain_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_merge_plain_walkers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_merge_plain_dev_walkers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_mg_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_mg_walk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_mg_pos_ptr": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]),
    "rb3gpu_mg_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_mg_rank_plain_walkers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_mg_rank_plain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_rank1a_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_get_acc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_get_tot": (ctypes.c_int64, [ctypes.c_void_p]),
    "rb3gpu_export_runs": (ctypes.c_int, [ctypes.c_void_p, EMIT_F, ctypes.c_void_p]),
    "rb3gpu_export_run_words": (ctypes.c_int, [ctypes.c_void_p, EMIT_WORDS_F, ctypes.c_void_p]),
    "rb3gpu_export_fmd_words": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]),
    "rb3gpu_host_free": (None, [ctypes.c_void_p]),
    "rb3gpu_export_plain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_export_plain_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_ssa_dims": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    "rb3gpu_ssa_gen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_bwt_from_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_sort_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_merge_text_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_merge_text_sa_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_sort_text_sa": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_sorter_sort_uploaded_sa": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "rb3gpu_sorter_sort_sa": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "rb3gpu_mg_rank_text_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_sorter_sort": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "rb3gpu_sorter_create": (ctypes.c_void_p, [ctypes.c_int]),
    "rb3gpu_sorter_destroy": (None, [ctypes.c_void_p]),
    "rb3gpu_sorter_bwt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_sorter_release": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_sorter_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_sorter_upload_fwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_sorter_upload_fwd_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_sorter_upload_end": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_sorter_sort_uploaded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "rb3gpu_pinned_alloc": (ctypes.c_void_p, [ctypes.c_int64]),
    "rb3gpu_pinned_free": (None, [ctypes.c_void_p]),
    "rb3gpu_walker_step": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]),
    "rb3gpu_sorter_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "rb3gpu_from_runs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_from_fmd_words": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_merge_fmd_words": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_export_bre": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, EMIT_BYTES_F, ctypes.c_void_p, ctypes.POINTER(BreStats)]),
    "rb3gpu_from_bre": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(BreStats)]),
    "rb3gpu_merge_bre": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(BreStats)]),
    "rb3gpu_merge_index": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_tune": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "rb3gpu_test_settle": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "rb3gpu_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Stats)]),
    "rb3gpu_buffer_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64)]),
    "rb3gpu_stats_reset": (None, [ctypes.c_void_p]),
    "rb3gpu_dev_alloc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    "rb3gpu_dev_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "rb3gpu_dev_download": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "rb3gpu_dev_free": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_dev_copy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "rb3gpu_dev_memset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "rb3gpu_sh_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_sh_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "rb3gpu_device_count": (ctypes.c_int, []),
    "rb3gpu_sh_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rb3gpu_group_create": (ctypes.c_void_p, [ctypes.c_int]),
    "rb3gpu_group_comm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_group_abort": (None, [ctypes.c_void_p]),
    "rb3gpu_group_destroy": (None, [ctypes.c_void_p]),
    "rb3gpu_rccl_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_rccl_comm_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_rccl_comm_destroy": (None, [ctypes.c_void_p]),
    "rb3gpu_stream_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_ipc_peer_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_ipc_peer_disable": (None, [ctypes.c_void_p]),
    "rb3gpu_merge_text_step_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "rb3gpu_set_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_get_order": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_sorter_set_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_sorter_order_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "rb3gpu_order_strings_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_sentinel_ranks_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_walkers_step_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_shard_split": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_shard_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_shard_gather": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_shard_destroy": (None, [ctypes.c_void_p]),
    "rb3gpu_shard_rebalance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_shard_get_acc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_shard_export_runs": (ctypes.c_int, [ctypes.c_void_p, EMIT_F, ctypes.c_void_p]),
    "rb3gpu_shard_export_run_words": (ctypes.c_int, [ctypes.c_void_p, EMITW_F, ctypes.c_void_p]),
    "rb3gpu_sh_merge_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rb3gpu_tprev_from_tw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_balanced_bounds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rb3gpu_export_plain_range_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "rb3gpu_shard_handle": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_shard_bounds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_device_of": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_kount": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, KOUNT_F, ctypes.c_void_p, ctypes.POINTER(KountStats)]),
    "rb3gpu_stream_of": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rb3gpu_ssa_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rb3gpu_ssa_keep": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rb3gpu_ssa_drop": (ctypes.c_int, [ctypes.c_void_p]),
    "rb3gpu_ssa_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)]),
    "rb3gpu_locate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, LOCATE_F, ctypes.c_void_p, ctypes.POINTER(LocateStats)]),
    "rb3gpu_mem_pos": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, MEM_POS_F, ctypes.c_void_p,
                                      ctypes.POINTER(MemStats), ctypes.POINTER(LocateStats)]),
    "rb3gpu_hapdiv": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(HapdivOpt), HAPDIV_F, ctypes.c_void_p,
                                     ctypes.POINTER(HapdivStats)]),
    "rb3gpu_sw_e2e": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SwOpt), SW_F, ctypes.c_void_p, ctypes.POINTER(SwStats),
                                     ctypes.POINTER(LocateStats)]),
    "rb3gpu_sw_local": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(SwOpt), SW_F, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SwlStats), ctypes.POINTER(LocateStats)]),
    "rb3gpu_mem": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, MEM_F, ctypes.c_void_p, ctypes.POINTER(MemStats)]),
    "rb3gpu_suffix": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SuffixStats)]),
    "rb3gpu_seed_present": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(SeedStats)]),
    "rb3gpu_retrieve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, RETRIEVE_F, ctypes.c_void_p, ctypes.POINTER(RetrieveStats)]),
    "rb3gpu_retrieve_pieces": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, RETRIEVE_F, ctypes.c_void_p, ctypes.POINTER(PiecesStats)]),
    "rb3gpu_remove": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RemoveStats)]),
    "rb3gpu_dedup": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(DedupStats)]),
    "rb3gpu_overlap": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, OVERLAP_F, ctypes.c_void_p, ctypes.POINTER(OverlapStats)]),
    "rb3gpu_overlap_reduced": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, OVERLAP_F, ctypes.c_void_p, ctypes.POINTER(ReduceStats)]),
    "rb3gpu_unitigs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, UNITIG_F, ctypes.c_void_p, UNITIG_LINK_F, ctypes.POINTER(UnitigStats)]),
    "rb3gpu_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), FETCH_F, ctypes.c_void_p, ctypes.POINTER(FetchStats)]),
}

# rb3gpu_comm_t (include/rb3gpu.h): the two collectives of the interval-sharded merge
ALL_GATHER_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int64))
ALL_TO_ALL_F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)
ABORT_F = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


class CommStruct(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("rank", ctypes.c_int), ("world", ctypes.c_int),
                ("all_gather", ctypes.c_void_p), ("all_to_all", ctypes.c_void_p), ("abort", ctypes.c_void_p), ("stream_barrier", ctypes.c_void_p),
                ("peer_export", ctypes.c_void_p), ("peer_import", ctypes.c_void_p)]

_libs = {}


# string orders of an index (include/rb3gpu.h RB3GPU_SO_*; mrope.h MR_SO_*): input order, reverse lexicographic (build -s), reverse
# complement lexicographic (build -r)
SO_IO, SO_RLO, SO_RCLO = 0, 1, 2


def load_library(hooks=False, path=None):
    """Load librb3gpu.so (the in-tree build) and declare every prototype.  Raises if absent.
    hooks=True: the test build (librb3gpu_hooks.so, -DRB3GPU_TEST_HOOKS), whose rb3gpu_tune also knows the keys that
    make a merge pretend a failure; only tests load it."""
    if path is None:
        path = _build.LIB_GPU_HOOKS if hooks else os.environ.get("RB3GPU_LIB", _build.LIB_GPU)  # override for kernel experiments only
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the engine is HIP-only; there is no CPU fallback)" % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        f = getattr(lib, name)  # AttributeError if the header and the library disagree
        f.restype, f.argtypes = res, args
    _libs[path] = lib
    return lib


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


def walker_step(device, length, n_strings, lib=None):
    """rb3gpu_walker_step: the text distance between the LF walkers of a batch (as many walkers as the walker kernel keeps resident)"""
    r = load_library(False, lib).rb3gpu_walker_step(int(device), int(length), int(n_strings))
    if r < 0:
        raise Rb3GpuError(int(r), "rb3gpu_walker_step")
    return int(r)


class PinnedArray:
    """a uint8 numpy array in page-locked host memory (rb3gpu_pinned_alloc): a batch built here goes to HBM with one DMA"""

    def __init__(self, nbytes, lib=None):
        self._lib = load_library(False, lib)
        self._p = self._lib.rb3gpu_pinned_alloc(int(max(nbytes, 1)))
        if not self._p:
            raise MemoryError("rb3gpu_pinned_alloc(%d) failed" % nbytes)
        self.array = np.ctypeslib.as_array(ctypes.cast(self._p, ctypes.POINTER(ctypes.c_uint8)), shape=(int(max(nbytes, 1)),))[:nbytes]

    def free(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.rb3gpu_pinned_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Sorter:
    """rb3gpu_sorter_t: the GPU suffix sorter as an object of its own (own HIP stream, scratch, two output buffers): what the
    CLI's sorter thread runs while the batch before is being merged (rb3_build_sais, sais-ss.c:50-56, build.c:55-83)"""

    def __init__(self, device=0, lib=None):
        self._lib = load_library(False, lib)
        self._s = self._lib.rb3gpu_sorter_create(int(device))
        if not self._s:
            raise RuntimeError("rb3gpu_sorter_create failed on device %d (no HIP device: there is no CPU fallback)" % device)

    def _chk(self, r, what):
        if r < 0:
            raise Rb3GpuError(r, what)

    def upload(self, text):
        """the text of a batch host -> HBM (the H2D copy of the merge path); returns when the copy is complete"""
        assert text.dtype == np.uint8 and text.flags["C_CONTIGUOUS"]
        self._chk(self._lib.rb3gpu_sorter_upload(self._s, text.size, text.ctypes.data), "rb3gpu_sorter_upload")

    def upload_fwd(self, text, pair_start):
        """upload of a batch of a few long records on both strands: forward strands only, reverse complements made on the device"""
        assert text.dtype == np.uint8 and text.flags["C_CONTIGUOUS"]
        ps = np.ascontiguousarray(pair_start, dtype=np.int64)
        self._chk(self._lib.rb3gpu_sorter_upload_fwd(self._s, text.size, text.ctypes.data, ps.size, ps.ctypes.data), "rb3gpu_sorter_upload_fwd")

    def upload_fwd_begin(self, text, pair_start):
        """upload_fwd without waiting: the copies are queued on the sorter's stream (page-locked text) and run beside whatever the
        caller does next; the text must not change until upload_end() or sort_uploaded() has returned"""
        assert text.dtype == np.uint8 and text.flags["C_CONTIGUOUS"]
        ps = np.ascontiguousarray(pair_start, dtype=np.int64)
        self._chk(self._lib.rb3gpu_sorter_upload_fwd_begin(self._s, text.size, text.ctypes.data, ps.size, ps.ctypes.data), "rb3gpu_sorter_upload_fwd_begin")

    def upload_end(self):
        self._chk(self._lib.rb3gpu_sorter_upload_end(self._s), "rb3gpu_sorter_upload_end")

    def sort_uploaded_sa(self, length):
        """sort_uploaded with the suffix array: (d_bwt, d_tw, d_sa), all released by release(d_bwt)"""
        p, q, r = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_sorter_sort_uploaded_sa(self._s, int(length), ctypes.byref(p), ctypes.byref(q), ctypes.byref(r)), "rb3gpu_sorter_sort_uploaded_sa")
        return p, q, r

    def sort_uploaded(self, length):
        """suffix-sort the text uploaded last: (d_bwt, d_tw) device pointers, valid until release(d_bwt)"""
        p, q = ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_sorter_sort_uploaded(self._s, int(length), ctypes.byref(p), ctypes.byref(q)), "rb3gpu_sorter_sort_uploaded")
        return p, q

    def sort(self, text):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        p, q = ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_sorter_sort(self._s, text.size, text.ctypes.data, ctypes.byref(p), ctypes.byref(q)), "rb3gpu_sorter_sort")
        return p, q

    def release(self, d_bwt):
        self._chk(self._lib.rb3gpu_sorter_release(self._s, d_bwt), "rb3gpu_sorter_release")

    def set_order(self, so):
        """every batch sorted from now on is first put into string order so (SO_IO, SO_RLO, SO_RCLO) on the device"""
        self._chk(self._lib.rb3gpu_sorter_set_order(self._s, int(so)), "rb3gpu_sorter_set_order")

    def order_ms(self):
        """cumulative milliseconds spent putting batches into order (not part of stats()["ms_sort"])"""
        ms = ctypes.c_double()
        self._chk(self._lib.rb3gpu_sorter_order_stats(self._s, ctypes.byref(ms)), "rb3gpu_sorter_order_stats")
        return ms.value

    def stats(self):
        up, so, nb, ns = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        self._chk(self._lib.rb3gpu_sorter_stats(self._s, ctypes.byref(up), ctypes.byref(so), ctypes.byref(nb), ctypes.byref(ns)), "rb3gpu_sorter_stats")
        return {"ms_upload": up.value, "ms_sort": so.value, "n_batches": nb.value, "n_symbols": ns.value}

    def close(self):
        if getattr(self, "_s", None):
            self._lib.rb3gpu_sorter_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Rb3Gpu:
    """One accumulated BWT resident in the HBM of one MI355X."""

    def __init__(self, device=0, split_log2=0, verbose=1, hooks=False, lib=None):
        self._lib = load_library(hooks, lib)   # lib: another build of the library (kernel experiments, tools/probe_*.py)
        n = self._lib.rb3gpu_device_count()
        if n <= 0:
            raise RuntimeError("no HIP device visible (rb3gpu_device_count=%d); the engine has no CPU fallback" % n)
        opt = Opt()
        self._lib.rb3gpu_opt_init(ctypes.byref(opt))
        opt.device, opt.split_log2, opt.verbose = device, split_log2, verbose
        self._h = self._lib.rb3gpu_create(ctypes.byref(opt))
        if not self._h:
            raise RuntimeError("rb3gpu_create failed on device %d" % device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rb3gpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tune(self, key, value):
        """rb3gpu_tune: a diagnostic switch of this handle (see include/rb3gpu.h)"""
        self._chk(self._lib.rb3gpu_tune(self._h, key.encode(), int(value)), "rb3gpu_tune(%s)" % key)

    def test_settle(self, ids, records, n_a, n_b, q=1, maxhops=64, engine=0, phase=1, masks=None, chunk_ctr=None):
        """rb3gpu_test_settle (test build only): the merge's settle phase on a hand-made stretch table.  ids: ascending stretch ids;
        records: uint32 array (len(ids), 16), the 64-byte records; masks: for q > 1, uint32 (len(ids), 8q).  Returns a dict: sfin
        (int32 per id), masks (uint32 (len(ids), 8q)), bad (the three validation counters), second_chance (bool)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(ids.size, 16)
        m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32).reshape(ids.size, 8 * q)
        cc = None if chunk_ctr is None else np.ascontiguousarray(chunk_ctr, dtype=np.uint32).reshape(64)
        sfin = np.zeros(ids.size, dtype=np.int32)
        mout = np.zeros((ids.size, 8 * q), dtype=np.uint32)
        bad = np.zeros(3, dtype=np.uint64)
        sc = ctypes.c_int(0)
        self._chk(self._lib.rb3gpu_test_settle(self._h, ids.size, ids.ctypes.data, rec.ctypes.data, None if m is None else m.ctypes.data, int(n_a), int(n_b),
                                               None if cc is None else cc.ctypes.data, int(q), int(maxhops), int(engine), int(phase),
                                               sfin.ctypes.data, mout.ctypes.data, bad.ctypes.data, ctypes.byref(sc)), "rb3gpu_test_settle")
        return {"sfin": sfin, "masks": mout, "bad": bad, "second_chance": bool(sc.value)}

    def _chk(self, r, what):
        if r < 0:
            raise Rb3GpuError(r, what)
        return r

    # -- the reference's entry points -------------------------------------------------------
    def from_plain(self, bwt):
        bwt = _u8(bwt)
        self._chk(self._lib.rb3gpu_from_plain(self._h, bwt.size, bwt.ctypes.data), "rb3gpu_from_plain")

    def merge_plain(self, bwt):
        bwt = _u8(bwt)
        self._chk(self._lib.rb3gpu_merge_plain(self._h, bwt.size, bwt.ctypes.data), "rb3gpu_merge_plain")

    @staticmethod
    def _walkers(w):
        w = np.ascontiguousarray(w, dtype=np.int64)
        assert w.ndim == 2 and w.shape[1] == 4, "walkers: (n, 4) int64 rows of (row, ka0, nsteps, flags)"
        return w

    def merge_plain_walkers(self, bwt, walkers):
        bwt, w = _u8(bwt), self._walkers(walkers)
        self._chk(self._lib.rb3gpu_merge_plain_walkers(self._h, bwt.size, bwt.ctypes.data, w.shape[0], w.ctypes.data), "rb3gpu_merge_plain_walkers")

    def merge_plain_dev_walkers(self, d_bwt, length, walkers, commit=True):
        if isinstance(walkers, (int, np.integer)):  # the number of strings: one walker per string, made on the device
            self._chk(self._lib.rb3gpu_merge_plain_dev_walkers(self._h, length, d_bwt, int(walkers), None, 1 if commit else 0), "rb3gpu_merge_plain_dev_walkers")
            return
        w = self._walkers(walkers)
        self._chk(self._lib.rb3gpu_merge_plain_dev_walkers(self._h, length, d_bwt, w.shape[0], w.ctypes.data, 1 if commit else 0), "rb3gpu_merge_plain_dev_walkers")

    # staged merge (multi-GPU): begin -> walk (repeatable) -> [collective on pos] -> finish
    def mg_begin(self, d_bwt, length, d_pos_ext=None):
        acc2 = np.zeros(7, dtype=np.int64)
        self._chk(self._lib.rb3gpu_mg_begin(self._h, length, d_bwt, d_pos_ext, acc2.ctypes.data), "rb3gpu_mg_begin")
        return acc2

    def mg_walk(self, walkers=None, stop_row=-1):
        """run walkers; returns the exact value a walker arrived at stop_row with, or -1"""
        if walkers is None:
            self._chk(self._lib.rb3gpu_mg_walk(self._h, 0, None, -1, None), "rb3gpu_mg_walk")
            return -1
        w = self._walkers(walkers)
        arr = np.full(1, -1, dtype=np.int64)
        self._chk(self._lib.rb3gpu_mg_walk(self._h, w.shape[0], w.ctypes.data, stop_row, arr.ctypes.data), "rb3gpu_mg_walk")
        return int(arr[0])

    def mg_pos_ptr(self):
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._chk(self._lib.rb3gpu_mg_pos_ptr(self._h, ctypes.byref(p), ctypes.byref(n)), "rb3gpu_mg_pos_ptr")
        return p.value, n.value

    def mg_finish(self, commit=True):
        self._chk(self._lib.rb3gpu_mg_finish(self._h, 1 if commit else 0), "rb3gpu_mg_finish")

    def mg_rank_plain(self, bwt):
        bwt = _u8(bwt)
        pos = np.empty(bwt.size, dtype=np.int64)
        acc2 = np.zeros(7, dtype=np.int64)
        self._chk(self._lib.rb3gpu_mg_rank_plain(self._h, bwt.size, bwt.ctypes.data, pos.ctypes.data, acc2.ctypes.data), "rb3gpu_mg_rank_plain")
        return pos, acc2

    def mg_rank_plain_walkers(self, bwt, walkers):
        bwt, w = _u8(bwt), self._walkers(walkers)
        pos = np.empty(bwt.size, dtype=np.int64)
        acc2 = np.zeros(7, dtype=np.int64)
        self._chk(self._lib.rb3gpu_mg_rank_plain_walkers(self._h, bwt.size, bwt.ctypes.data, w.shape[0], w.ctypes.data, pos.ctypes.data, acc2.ctypes.data), "rb3gpu_mg_rank_plain_walkers")
        return pos, acc2

    def rank1a(self, k):
        k = np.ascontiguousarray(k, dtype=np.int64)
        ok = np.empty((k.size, 6), dtype=np.int64)
        self._chk(self._lib.rb3gpu_rank1a_batch(self._h, k.size, k.ctypes.data, ok.ctypes.data), "rb3gpu_rank1a_batch")
        return ok

    def get_acc(self):
        acc = np.zeros(7, dtype=np.int64)
        self._chk(self._lib.rb3gpu_get_acc(self._h, acc.ctypes.data), "rb3gpu_get_acc")
        return acc

    def get_tot(self):
        return int(self._lib.rb3gpu_get_tot(self._h))

    def export_plain(self):
        out = np.empty(self.get_tot(), dtype=np.uint8)
        self._chk(self._lib.rb3gpu_export_plain(self._h, out.ctypes.data), "rb3gpu_export_plain")
        return out

    def export_fmd_words(self):
        """the data section of the index's .fmd, packed on the GPU (rb3_enc_fmr2fmd + rld_enc, fm-index.c:31-52): uint64 array"""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._chk(self._lib.rb3gpu_export_fmd_words(self._h, ctypes.byref(p), ctypes.byref(n)), "rb3gpu_export_fmd_words")
        out = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n.value,)).copy()
        self._lib.rb3gpu_host_free(p)
        return out

    def export_bre(self, b_per_run=2, stats=None):
        """the records of the index's BRE file (`build -e` without header and footer), packed on the GPU: bytes.  stats: a dict that
        receives n_rec, n_sym, n_run (the footer's counts), n_pieces, ms_scan and ms_pack"""
        parts = []

        def emit(_data, n, p):
            parts.append(ctypes.string_at(p, n))
            return 0
        st = BreStats()
        self._chk(self._lib.rb3gpu_export_bre(self._h, int(b_per_run), EMIT_BYTES_F(emit), None, ctypes.byref(st)), "rb3gpu_export_bre")
        if stats is not None:
            stats.update({k: getattr(st, k) for k, _ in BreStats._fields_})
        return b"".join(parts)

    def _bre_call(self, fn, name, records, b_per_run, stats):
        rec = np.frombuffer(bytes(records), dtype=np.uint8)
        rs = 1 + int(b_per_run)
        if rec.size % rs != 0:
            raise ValueError("%d bytes are not whole records of %d bytes" % (rec.size, rs))
        st = BreStats()
        self._chk(fn(self._h, int(b_per_run), rec.size // rs, rec.ctypes.data if rec.size else None, ctypes.byref(st)), name)
        if stats is not None:
            stats.update({k: getattr(st, k) for k, _ in BreStats._fields_})

    def from_bre(self, records, b_per_run=2, stats=None):
        """index the records of a BRE file (read_bre), unpacked on the device; stats: the counts the device found, ms_scan, ms_fill, n_pieces"""
        self._bre_call(self._lib.rb3gpu_from_bre, "rb3gpu_from_bre", records, b_per_run, stats)

    def merge_bre(self, records, b_per_run=2, stats=None):
        """merge the records of a BRE file into the index as one batch (rb3gpu_merge_bre)"""
        self._bre_call(self._lib.rb3gpu_merge_bre, "rb3gpu_merge_bre", records, b_per_run, stats)

    def merge_index(self, other):
        """merge the whole index of another handle (any GPU of the node) into this one (rb3_fmi_merge, fm-index.c:251-277)"""
        self._chk(self._lib.rb3gpu_merge_index(self._h, other._h), "rb3gpu_merge_index")

    def set_order(self, so):
        """the string order of the index (SO_IO, SO_RLO, SO_RCLO): batches sorted by this handle are put into it first, merged batches
        must be in it (their sentinels go among the index's strings, not behind them)"""
        self._chk(self._lib.rb3gpu_set_order(self._h, int(so)), "rb3gpu_set_order")

    def get_order(self):
        return int(self._lib.rb3gpu_get_order(self._h))

    def order_strings_dev(self, d_text, length, so):
        """rb3gpu_order_strings_dev: a batch text in device memory reordered in place into string order so (SO_RLO or SO_RCLO)"""
        self._chk(self._lib.rb3gpu_order_strings_dev(self._h, int(length), d_text, int(so)), "rb3gpu_order_strings_dev")

    def order_strings(self, text, so):
        """a batch text (host) put into string order so on the device: the reordered text"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        d = self.dev_upload(text)
        try:
            self.order_strings_dev(d, text.size, so)
            return self.dev_download(d, text.size)
        finally:
            self.dev_free(d)

    def sentinel_ranks_dev(self, d_bwt, d_tw, length, n_strings):
        """rb3gpu_sentinel_ranks_dev: p0 of the next merge of an ordered batch (n_strings strings) in the handle's order, as an int64 array;
        d_tw None: the strings are read through the batch's BWT"""
        p0 = np.empty(int(n_strings), dtype=np.int64)
        self._chk(self._lib.rb3gpu_sentinel_ranks_dev(self._h, int(length), d_bwt, d_tw, int(n_strings), p0.ctypes.data), "rb3gpu_sentinel_ranks_dev")
        return p0

    def export_plain_dev(self, d_out):
        self._chk(self._lib.rb3gpu_export_plain_dev(self._h, d_out), "rb3gpu_export_plain_dev")

    def bwt_from_text(self, text, step=0):
        """suffix-sort a batch text on the GPU (rb3_build_sais, sais-ss.c:10-56): returns (device pointer of the
        BWT -- free it with dev_free --, ckrow or None)"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        p = ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, text.size + 16, ctypes.byref(p)), "rb3gpu_dev_alloc")
        ck = np.empty((text.size + step - 1) // step, dtype=np.int64) if step > 0 else None
        self._chk(self._lib.rb3gpu_bwt_from_text(self._h, text.size, text.ctypes.data, p, step, ck.ctypes.data if ck is not None else None), "rb3gpu_bwt_from_text")
        return p, ck

    def sort_text(self, text):
        """suffix-sort a batch text on the GPU: returns device pointers (BWT, text-order words) for merge_text_dev;
        free both with dev_free"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        p, q = ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, text.size + 16, ctypes.byref(p)), "rb3gpu_dev_alloc")
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, text.size * 8, ctypes.byref(q)), "rb3gpu_dev_alloc")
        self._chk(self._lib.rb3gpu_sort_text(self._h, text.size, text.ctypes.data, p, q), "rb3gpu_sort_text")
        return p, q

    def sort_text_sa(self, text):
        """sort_text with the suffix array: (BWT, text-order words, suffix array) device pointers; free all three with dev_free"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        p, q, r = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, text.size + 16, ctypes.byref(p)), "rb3gpu_dev_alloc")
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, text.size * 8, ctypes.byref(q)), "rb3gpu_dev_alloc")
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, text.size * 4, ctypes.byref(r)), "rb3gpu_dev_alloc")
        self._chk(self._lib.rb3gpu_sort_text_sa(self._h, text.size, text.ctypes.data, p, q, r), "rb3gpu_sort_text_sa")
        return p, q, r

    def merge_text_dev(self, d_bwt, d_tw, length, walkers, commit=True, d_sa=None):
        """merge a batch given by its BWT and text-order words (walkers by text position: host.walkers_text); d_sa: the batch's
        suffix array if the caller has it (rb3gpu_merge_text_sa_dev)"""
        if isinstance(walkers, (int, np.integer)):  # the number of strings: one walker per string, made on the device
            self._chk(self._lib.rb3gpu_merge_text_sa_dev(self._h, length, d_bwt, d_tw, d_sa, int(walkers), None, 1 if commit else 0), "rb3gpu_merge_text_sa_dev")
            return
        w = self._walkers(walkers)
        self._chk(self._lib.rb3gpu_merge_text_sa_dev(self._h, length, d_bwt, d_tw, d_sa, w.shape[0], w.ctypes.data, 1 if commit else 0), "rb3gpu_merge_text_sa_dev")

    def merge_text_step_dev(self, d_bwt, d_tw, length, n_strings, step, commit=True, d_sa=None):
        """rb3gpu_merge_text_step_dev: the walker list made on the device (a walker per string and one every `step` text positions)"""
        self._chk(self._lib.rb3gpu_merge_text_step_dev(self._h, int(length), d_bwt, d_tw, d_sa, int(n_strings), int(step), 1 if commit else 0), "rb3gpu_merge_text_step_dev")

    def walkers_step_dev(self, d_tw, length, n_strings, step):
        """the walker list rb3gpu_merge_text_step_dev makes on the device, as an (n, 4) int64 array (row = text position, ka0, nsteps, flags)"""
        n, p = ctypes.c_int64(0), ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_walkers_step_dev(self._h, int(length), d_tw, int(n_strings), int(step), ctypes.byref(n), ctypes.byref(p)), "rb3gpu_walkers_step_dev")
        w = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int64)), shape=(n.value, 4)).copy()
        self._lib.rb3gpu_host_free(p)
        return w

    def mg_rank_text_dev(self, d_bwt, d_tw, length, walkers):
        pos = np.empty(length, dtype=np.int64)
        acc2 = np.zeros(7, dtype=np.int64)
        if isinstance(walkers, (int, np.integer)):
            self._chk(self._lib.rb3gpu_mg_rank_text_dev(self._h, length, d_bwt, d_tw, int(walkers), None, pos.ctypes.data, acc2.ctypes.data), "rb3gpu_mg_rank_text_dev")
            return pos, acc2
        w = self._walkers(walkers)
        self._chk(self._lib.rb3gpu_mg_rank_text_dev(self._h, length, d_bwt, d_tw, w.shape[0], w.ctypes.data, pos.ctypes.data, acc2.ctypes.data), "rb3gpu_mg_rank_text_dev")
        return pos, acc2

    def dev_download(self, p, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        self._chk(self._lib.rb3gpu_dev_download(self._h, out.ctypes.data, p, nbytes), "rb3gpu_dev_download")
        return out

    def dev_download_i64(self, p, n):
        return self.dev_download(p, int(n) * 8).view(np.int64)

    def ssa_gen(self, ssa_shift):
        """sampled suffix array of the index (rb3_ssa_gen, ssa.c:54-81): (ms, r2i[m], ssa[n_ssa]) as uint64"""
        m, n_ssa, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        self._chk(self._lib.rb3gpu_ssa_dims(self._h, ssa_shift, ctypes.byref(m), ctypes.byref(n_ssa), ctypes.byref(ms)), "rb3gpu_ssa_dims")
        r2i = np.empty(m.value, dtype=np.uint64)
        ssa = np.empty(max(n_ssa.value, 1), dtype=np.uint64)
        self._chk(self._lib.rb3gpu_ssa_gen(self._h, ssa_shift, r2i.ctypes.data, ssa.ctypes.data), "rb3gpu_ssa_gen")
        return ms.value, r2i, ssa[:n_ssa.value]

    def export_runs(self):
        runs = []

        def emit(_data, c, l):
            runs.append((c, l))
            return 0
        cb = EMIT_F(emit)
        self._chk(self._lib.rb3gpu_export_runs(self._h, cb, None), "rb3gpu_export_runs")
        return runs

    def from_runs(self, runs):
        arr = np.array([(l << 3) | c for c, l in runs], dtype=np.uint64)
        self._chk(self._lib.rb3gpu_from_runs(self._h, arr.size, arr.ctypes.data), "rb3gpu_from_runs")

    # -- device-resident variants ------------------------------------------------------------
    def from_fmd_file(self, path):
        """load an .fmd file, decoding it on the device (rb3gpu_from_fmd_words)"""
        raw = np.fromfile(path, dtype=np.uint8)
        assert raw[:4].tobytes() == b"RLD\x03", "not an FMD file"
        hdr = raw[8:32].view(np.uint64)
        mc = raw[32:80].view(np.uint64).astype(np.int64)
        n_words = int(hdr[1]) // 8
        words = np.ascontiguousarray(raw[80:80 + n_words * 8]).view(np.uint64)
        self._chk(self._lib.rb3gpu_from_fmd_words(self._h, n_words, words.ctypes.data, mc.ctypes.data), "rb3gpu_from_fmd_words")

    def dev_upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, arr.nbytes + 16, ctypes.byref(p)), "rb3gpu_dev_alloc")
        self._chk(self._lib.rb3gpu_dev_upload(self._h, p, arr.ctypes.data, arr.nbytes), "rb3gpu_dev_upload")
        return p

    def dev_free(self, p):
        self._chk(self._lib.rb3gpu_dev_free(self._h, p), "rb3gpu_dev_free")

    def from_plain_dev(self, d_bwt, length):
        self._chk(self._lib.rb3gpu_from_plain_dev(self._h, length, d_bwt), "rb3gpu_from_plain_dev")

    def merge_plain_dev(self, d_bwt, length, commit=True):
        self._chk(self._lib.rb3gpu_merge_plain_dev(self._h, length, d_bwt, 1 if commit else 0), "rb3gpu_merge_plain_dev")

    # -- interval-sharded index (multi-GPU; ropebwt3_amd/multi.py) ------------------------------
    def dev_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._chk(self._lib.rb3gpu_dev_alloc(self._h, int(nbytes), ctypes.byref(p)), "rb3gpu_dev_alloc")
        return p.value

    def dev_copy(self, d_dst, d_src, nbytes):
        self._chk(self._lib.rb3gpu_dev_copy(self._h, d_dst, d_src, int(nbytes)), "rb3gpu_dev_copy")

    def dev_memset(self, d_dst, byte, nbytes):
        self._chk(self._lib.rb3gpu_dev_memset(self._h, d_dst, int(byte), int(nbytes)), "rb3gpu_dev_memset")

    def dev_upload_to(self, d_dst, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self._lib.rb3gpu_dev_upload(self._h, d_dst, arr.ctypes.data, arr.nbytes), "rb3gpu_dev_upload")

    def sh_step(self, n_states, d_in, d_tw, d_ka, adj, bounds, my_iv, d_send):
        """one LF step of the states resident on this rank; returns counts[n_iv + 1] (see include/rb3gpu.h)"""
        adj = np.ascontiguousarray(adj, dtype=np.int64)
        bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        counts = np.zeros(bounds.size, dtype=np.int64)
        self._chk(self._lib.rb3gpu_sh_step(self._h, int(n_states), d_in, d_tw, d_ka, adj.ctypes.data, bounds.size - 1, bounds.ctypes.data, int(my_iv), d_send, counts.ctypes.data), "rb3gpu_sh_step")
        return counts

    def sh_finish(self, jlo, n_rows, d_bwt, d_ka, iv_start, commit=True):
        self._chk(self._lib.rb3gpu_sh_finish(self._h, int(jlo), int(n_rows), d_bwt, d_ka, int(iv_start), 1 if commit else 0), "rb3gpu_sh_finish")

    def sh_merge(self, comm, bounds, d_bwt, d_tw, n2, sent_tp, commit=True):
        """rb3gpu_sh_merge: one batch merged into the interval-sharded index, the lock-step loop inside the library.  comm: a
        GroupComm / RcclComm / CallbackComm of this rank.  Returns (bounds after the merge, lock-step rounds)."""
        b = np.array(bounds, dtype=np.int64)
        tp = np.ascontiguousarray(sent_tp, dtype=np.int64)
        rounds = ctypes.c_int64(0)
        self._chk(self._lib.rb3gpu_sh_merge(self._h, ctypes.addressof(comm.struct), b.ctypes.data, int(n2), d_bwt, d_tw, tp.size, tp.ctypes.data, 1 if commit else 0, ctypes.addressof(rounds)), "rb3gpu_sh_merge")
        return b, int(rounds.value)

    def sh_merge_text(self, comm, bounds, d_tprev, d_tw_slice, n2, sent_tp, commit=True):
        """rb3gpu_sh_merge_text: the same with the BATCH sharded -- d_tprev: the symbol before every text position (1 byte each, whole),
        d_tw_slice: the text-order words of this rank's text range only; the rows come from the owners of the text ranges at the end"""
        b = np.array(bounds, dtype=np.int64)
        tp = np.ascontiguousarray(sent_tp, dtype=np.int64)
        rounds = ctypes.c_int64(0)
        self._chk(self._lib.rb3gpu_sh_merge_text(self._h, ctypes.addressof(comm.struct), b.ctypes.data, int(n2), d_tprev, d_tw_slice, tp.size, tp.ctypes.data, 1 if commit else 0, ctypes.addressof(rounds)), "rb3gpu_sh_merge_text")
        return b, int(rounds.value)

    def tprev_from_tw(self, d_tw, n2):
        """device array of n2 bytes: the symbol before every text position (rb3gpu_tprev_from_tw); free it with dev_free"""
        d = self.dev_alloc(int(n2) + 64)
        self._chk(self._lib.rb3gpu_tprev_from_tw(self._h, int(n2), d_tw, d), "rb3gpu_tprev_from_tw")
        return d

    def balanced_bounds(self, n):
        b = np.zeros(n + 1, dtype=np.int64)
        self._chk(self._lib.rb3gpu_balanced_bounds(self._h, int(n), b.ctypes.data), "rb3gpu_balanced_bounds")
        return b

    def kount(self, k, min_occ, others=(), max_level_nodes=0, stats=None):
        """rb3gpu_kount: the k-mers that occur at least min_occ times in this index or one of `others` (handles on the same device; all 4^k
        for min_occ <= 0), in the reference's output order: (kmers, counts), uint8 (N, k) with symbols 1..4 = A C G T and int64 (N, 1 + len(others)).
        max_level_nodes: the cap of one depth's frontier (0: by the free device memory); stats: a dict that receives rb3gpu_kount_stats_t"""
        hs = [self] + list(others)
        arr = (ctypes.c_void_p * len(hs))(*[x._h for x in hs])
        kms, cts = [], []

        def cb(_ud, n, n_idx, kk, kmers, counts):
            kms.append(np.ctypeslib.as_array(kmers, shape=(n * kk,)).reshape(n, kk).copy())
            cts.append(np.ctypeslib.as_array(counts, shape=(n * n_idx,)).reshape(n, n_idx).copy())
            return 0
        st = KountStats()
        self._chk(self._lib.rb3gpu_kount(arr, len(hs), int(k), int(min_occ), int(max_level_nodes), KOUNT_F(cb), None, ctypes.byref(st)), "rb3gpu_kount")
        if stats is not None:
            stats.update(st.as_dict())
        if not kms:
            return np.zeros((0, int(k)), dtype=np.uint8), np.zeros((0, len(hs)), dtype=np.int64)
        return np.concatenate(kms), np.concatenate(cts)

    def set_ssa(self, ssa_shift, ms, r2i, ssa):
        """rb3gpu_ssa_set: the sampled suffix array of the index as a .ssa file holds it (read_ssa), uploaded and kept on the device"""
        r2i = np.ascontiguousarray(r2i, dtype=np.uint64)
        ssa = np.ascontiguousarray(ssa, dtype=np.uint64)
        self._chk(self._lib.rb3gpu_ssa_set(self._h, int(ssa_shift), int(ms), r2i.size, ssa.size, r2i.ctypes.data if r2i.size else None, ssa.ctypes.data if ssa.size else None), "rb3gpu_ssa_set")

    def keep_ssa(self, ssa_shift):
        """rb3gpu_ssa_keep: the sampled suffix array built on the device and kept there"""
        self._chk(self._lib.rb3gpu_ssa_keep(self._h, int(ssa_shift)), "rb3gpu_ssa_keep")

    def drop_ssa(self):
        self._chk(self._lib.rb3gpu_ssa_drop(self._h), "rb3gpu_ssa_drop")

    def ssa_info(self):
        """(ssa_shift, n_ssa) of the sampled suffix array on the handle, None without one"""
        ss, n = ctypes.c_int(), ctypes.c_int64()
        return (ss.value, n.value) if self._lib.rb3gpu_ssa_info(self._h, ctypes.byref(ss), ctypes.byref(n)) == 0 else None

    def locate(self, lo, hi, max_pos, stats=None):
        """rb3gpu_locate: up to max_pos positions of the rows of every interval [lo[i], hi[i]), the reference's pairs in the reference's order:
        (off, pos) with the pairs of interval i at pos[off[i]:off[i + 1]] (POS: sid, pos); stats: a dict that receives rb3gpu_locate_stats_t"""
        lo = np.ascontiguousarray(lo, dtype=np.int64)
        hi = np.ascontiguousarray(hi, dtype=np.int64)
        if lo.shape != hi.shape or lo.ndim != 1:
            raise ValueError("lo and hi must be one-dimensional and of one length")
        offs, got = [np.zeros(1, dtype=np.int64)], []
        base = [0]

        def cb(_ud, _i0, n, off, pos):
            o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
            got.append(np.frombuffer(ctypes.string_at(pos, int(o[n]) * POS.itemsize), dtype=POS).copy())
            offs.append(o[1:] + base[0])
            base[0] += int(o[n])
            return 0
        st = LocateStats()
        self._chk(self._lib.rb3gpu_locate(self._h, lo.size, lo.ctypes.data if lo.size else None, hi.ctypes.data if hi.size else None, int(max_pos), LOCATE_F(cb), None, ctypes.byref(st)),
                  "rb3gpu_locate")
        if stats is not None:
            stats.update(st.as_dict())
        return np.concatenate(offs), (np.concatenate(got) if got else np.zeros(0, dtype=POS))

    def mem(self, queries, min_len=19, min_occ=1, chunk=None, stats=None, max_pos=0, locate_stats=None):
        """rb3gpu_mem: the super-maximal exact matches of the queries (each a uint8 array of nt6 codes 0..5, or bytes / str of characters) of at
        least min_len symbols and min_occ occurrences, as the reference's `mem` finds them: a structured array (MEM_REC: query, x0, size, st, en)
        in the reference's output order.  chunk: query symbols per walker (None: the engine's default; the result does not depend on it);
        stats: a dict that receives rb3gpu_mem_stats_t.  max_pos > 0 (rb3gpu_mem_pos; the handle needs set_ssa / keep_ssa): returns (records, off, pos)
        with up to max_pos positions per record, those of record i at pos[off[i]:off[i + 1]] (POS), as Rb3Gpu.locate gives them for [x0, x0 + size);
        locate_stats: a dict that receives rb3gpu_locate_stats_t"""
        qs = [nt6_of(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.int64)
        if qs:
            off[1:] = np.cumsum([q.size for q in qs])
        sym = np.concatenate(qs) if qs else np.zeros(0, dtype=np.uint8)
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        got = []

        def cb(_ud, n, recs):
            got.append(np.frombuffer(ctypes.string_at(recs, n * MEM_REC.itemsize), dtype=MEM_REC).copy())
            return 0
        st = MemStats()
        if max_pos > 0:
            offs, pairs, base = [np.zeros(1, dtype=np.int64)], [], [0]

            def cbp(_ud, n, recs, poff, pos):
                o = np.ctypeslib.as_array(poff, shape=(n + 1,)).copy()
                got.append(np.frombuffer(ctypes.string_at(recs, n * MEM_REC.itemsize), dtype=MEM_REC).copy())
                pairs.append(np.frombuffer(ctypes.string_at(pos, int(o[n]) * POS.itemsize), dtype=POS).copy())
                offs.append(o[1:] + base[0])
                base[0] += int(o[n])
                return 0
            lst = LocateStats()
            self._chk(self._lib.rb3gpu_mem_pos(self._h, len(qs), off.ctypes.data, sym.ctypes.data if sym.size else None, int(min_len), int(min_occ), 0 if chunk is None else int(chunk),
                                               int(max_pos), MEM_POS_F(cbp), None, ctypes.byref(st), ctypes.byref(lst)), "rb3gpu_mem_pos")
            if stats is not None:
                stats.update(st.as_dict())
            if locate_stats is not None:
                locate_stats.update(lst.as_dict())
            return (np.concatenate(got) if got else np.zeros(0, dtype=MEM_REC)), np.concatenate(offs), (np.concatenate(pairs) if pairs else np.zeros(0, dtype=POS))
        self._chk(self._lib.rb3gpu_mem(self._h, len(qs), off.ctypes.data, sym.ctypes.data if sym.size else None, int(min_len), int(min_occ), 0 if chunk is None else int(chunk),
                                       MEM_F(cb), None, ctypes.byref(st)), "rb3gpu_mem")
        if stats is not None:
            stats.update(st.as_dict())
        return np.concatenate(got) if got else np.zeros(0, dtype=MEM_REC)

    def suffix(self, queries, stats=None):
        """rb3gpu_suffix: per query (forms as for mem) the longest suffix that occurs in the index, as the reference's `suffix` finds it: a structured
        array (SUFFIX_OUT), one entry per query in input order -- query, start (where the suffix begins in the query), length (of the query), size
        (the occurrences of the suffix; 0 where start == length).  stats: a dict that receives rb3gpu_suffix_stats_t"""
        qs = [nt6_of(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.int64)
        if qs:
            off[1:] = np.cumsum([q.size for q in qs])
        sym = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        rec = np.zeros(len(qs), dtype=SUFFIX_REC)
        st = SuffixStats()
        self._chk(self._lib.rb3gpu_suffix(self._h, len(qs), off.ctypes.data, sym.ctypes.data if sym.size else None, rec.ctypes.data if rec.size else None, ctypes.byref(st)),
                  "rb3gpu_suffix")
        if stats is not None:
            stats.update(st.as_dict())
        out = np.zeros(len(qs), dtype=SUFFIX_OUT)
        out["query"], out["start"], out["length"], out["size"] = np.arange(len(qs)), rec["start"], off[1:] - off[:-1], rec["size"]
        return out

    def seed_present(self, queries, min_len, chunk=None, stats=None):
        """rb3gpu_seed_present: per query (forms as for suffix) whether a stretch of at least min_len symbols of it occurs in the index, the test behind the
        reference's `sw -j` (rb3_fmd_smem_present): a bool array, one entry per query in input order; False for a query shorter than min_len.  chunk: window
        starts per walker (None: the engine's default; the answer does not depend on it); stats: a dict that receives rb3gpu_seed_stats_t"""
        qs = [nt6_of(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.int64)
        if qs:
            off[1:] = np.cumsum([q.size for q in qs])
        sym = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        flag = np.zeros(len(qs), dtype=np.uint8)
        st = SeedStats()
        self._chk(self._lib.rb3gpu_seed_present(self._h, len(qs), off.ctypes.data, sym.ctypes.data if sym.size else None, int(min_len), 0 if chunk is None else int(chunk),
                                                flag.ctypes.data if flag.size else None, ctypes.byref(st)), "rb3gpu_seed_present")
        if stats is not None:
            stats.update(st.as_dict())
        return flag != 0

    def retrieve(self, rows, stats=None, pieces=False):
        """rb3gpu_retrieve: for every row asked for, in the order asked, the string in front of the suffix of that row (for a sentinel's row k < acc[1]
        the whole of indexed string k) as the reference's `get` spells it: (end_rows, seqs) -- end_rows an int64 array, the row each walk met the
        sentinel at (-1 for a row outside the index), seqs a list of uint8 arrays of nt6 codes in text order (empty for such a row).  stats: a dict
        that receives rb3gpu_retrieve_stats_t.  pieces=True: the same answers through rb3gpu_retrieve_pieces (the whole index walked once in pieces,
        for long strings or much of the index; stats then receives rb3gpu_pieces_stats_t)"""
        rows = np.ascontiguousarray(list(rows) if not isinstance(rows, np.ndarray) else rows, dtype=np.int64).reshape(-1)
        return self._retrieve(rows.size, rows.ctypes.data if rows.size else None, stats, pieces)

    def retrieve_all(self, stats=None):
        """rb3gpu_retrieve_pieces for all the strings of the index: what retrieve(range(acc[1]), pieces=True) returns, without the list of rows"""
        return self._retrieve(-1, None, stats, True)

    def _retrieve(self, n, rows_ptr, stats, pieces):
        ends, seqs = [], []

        def cb(_ud, _i0, n, end_row, off, symbols):
            o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
            ends.append(np.ctypeslib.as_array(end_row, shape=(n,)).copy())
            buf = np.frombuffer(ctypes.string_at(symbols, int(o[n])), dtype=np.uint8) if o[n] > 0 else np.zeros(0, dtype=np.uint8)
            seqs.extend(buf[int(o[i]):int(o[i + 1])].copy() for i in range(n))
            return 0
        if pieces:
            st = PiecesStats()
            self._chk(self._lib.rb3gpu_retrieve_pieces(self._h, n, rows_ptr, RETRIEVE_F(cb), None, ctypes.byref(st)), "rb3gpu_retrieve_pieces")
        else:
            st = RetrieveStats()
            self._chk(self._lib.rb3gpu_retrieve(self._h, n, rows_ptr, RETRIEVE_F(cb), None, ctypes.byref(st)), "rb3gpu_retrieve")
        if stats is not None:
            stats.update(st.as_dict())
        return (np.concatenate(ends) if ends else np.zeros(0, dtype=np.int64)), seqs

    def remove(self, rows, pieces=False, stats=None):
        """rb3gpu_remove: the strings rows (numbers in [0, acc[1]); duplicates collapse) taken out of the index on the handle; the strings that stay keep their
        order.  pieces=True marks the rows through the walk in pieces (for long strings).  An empty list changes nothing; a row outside the range, or a request
        that would leave no string, raises with RB3GPU_EINVAL and the index as it was.  stats: a dict that receives rb3gpu_remove_stats_t"""
        rows = np.ascontiguousarray(list(rows) if not isinstance(rows, np.ndarray) else rows, dtype=np.int64).reshape(-1)
        st = RemoveStats()
        self._chk(self._lib.rb3gpu_remove(self._h, rows.size, rows.ctypes.data if rows.size else None, 1 if pieces else 0, ctypes.byref(st)), "rb3gpu_remove")
        if stats is not None:
            stats.update(st.as_dict())

    def dedup(self, pair=False, dup_only=False, records=False, stats=None):
        """rb3gpu_dedup: which strings of the index are copies of another one ('D') or lie inside a longer one ('C'; never with dup_only), and which stay ('K'):
        (kind, keeper) -- a uint8 array of the letters and an int64 array of the smallest unit of each unit's class, one entry per unit.  A unit is a row; with
        pair=True sequence u, rows 2u and 2u + 1 of an index of both strands in input order.  records=True: (kind, keeper, rec), rec a structured array
        (DEDUP_REC) of occ, copies and cls per ROW -- (1, 1, -1) where the walk ended early.  stats: a dict that receives rb3gpu_dedup_stats_t"""
        m = int(self.get_acc()[1])
        nu = m >> 1 if pair else m
        kind, keeper = np.zeros(max(nu, 1), dtype=np.uint8), np.zeros(max(nu, 1), dtype=np.int64)
        rec = np.zeros(max(m, 1), dtype=DEDUP_REC) if records else None
        st = DedupStats()
        self._chk(self._lib.rb3gpu_dedup(self._h, 1 if pair else 0, 1 if dup_only else 0, kind.ctypes.data, keeper.ctypes.data, rec.ctypes.data if records else None,
                                         ctypes.byref(st)), "rb3gpu_dedup")
        if stats is not None:
            stats.update(st.as_dict())
        return (kind[:nu], keeper[:nu], rec[:m]) if records else (kind[:nu], keeper[:nu])

    def overlap(self, min_len, max_hits=0, stats=None, lengths=False, reduce=False):
        """rb3gpu_overlap: the suffix-prefix overlaps of all the strings of the index: one structured array (OVERLAP_REC) of the records (a, b, len, len_b) -- the last
        len symbols of string a are the first len of string b, min_len <= len < the length of a, len_b the length of b -- ordered by a, then longest first, then in
        the index's order of the partners.  max_hits > 0 leaves out every group of more than max_hits partners of one (a, len).  lengths=True: (records, the length of
        every string, int64).  stats: a dict that receives rb3gpu_overlap_stats_t.  reduce=True: rb3gpu_overlap_reduced, only the irreducible records -- those that no
        two longer ones imply -- in the same order; stats then receives rb3gpu_reduce_stats_t"""
        got = []

        def cb(_ud, n, recs):
            got.append(np.frombuffer(ctypes.string_at(recs, int(n) * OVERLAP_REC.itemsize), dtype=OVERLAP_REC))
            return 0
        m = int(self.get_acc()[1])
        ln = np.zeros(max(m, 1), dtype=np.int64) if lengths else None
        st, name = (ReduceStats(), "rb3gpu_overlap_reduced") if reduce else (OverlapStats(), "rb3gpu_overlap")
        self._chk(getattr(self._lib, name)(self._h, int(min_len), int(max_hits), ln.ctypes.data if lengths else None, OVERLAP_F(cb), None, ctypes.byref(st)), name)
        if stats is not None:
            stats.update(st.as_dict())
        rec = np.concatenate(got) if got else np.zeros(0, dtype=OVERLAP_REC)
        return (rec, ln[:m]) if lengths else rec

    def unitigs(self, min_len, max_hits=0, pair=False, links=False, stats=None):
        """rb3gpu_unitigs: the unambiguous paths of the string graph of the irreducible overlaps (those of overlap(reduce=True) for the same min_len and max_hits), each
        spelled: (unitigs, members, sequences) -- a structured array (UNITIG_REC: head, tail, members, circ, len) by ascending head, one (UNITIG_MEMBER: row, o_in, off)
        of their members, unitig after unitig by rank, and a list of uint8 arrays of nt6 codes in text order.  links=True: a fourth item, the structured array
        (UNITIG_LINK) of the kept overlaps between unitigs.  pair=True: the index holds both strands in input order and one of every two mirror chains is returned; a
        graph that is not strand-symmetric raises with RB3GPU_EUNSUP (stats still receives n_asym).  stats: a dict that receives rb3gpu_unitig_stats_t"""
        utg, mem, seqs, lnk = [], [], [], []

        def cb(_ud, _u0, n, u, mb, off, symbols):
            n = int(n)
            us = np.frombuffer(ctypes.string_at(u, n * UNITIG_REC.itemsize), dtype=UNITIG_REC)
            o = np.frombuffer(ctypes.string_at(off, (n + 1) * 8), dtype=np.int64)
            sym = np.frombuffer(ctypes.string_at(symbols, int(o[n])), dtype=np.uint8)
            utg.append(us)
            mem.append(np.frombuffer(ctypes.string_at(mb, int(us["members"].sum()) * UNITIG_MEMBER.itemsize), dtype=UNITIG_MEMBER))
            seqs.extend(sym[int(o[i]):int(o[i + 1])].copy() for i in range(n))
            return 0

        def lcb(_ud, n, ls):
            lnk.append(np.frombuffer(ctypes.string_at(ls, int(n) * UNITIG_LINK.itemsize), dtype=UNITIG_LINK))
            return 0
        st = UnitigStats()
        code = self._lib.rb3gpu_unitigs(self._h, int(min_len), int(max_hits), 1 if pair else 0, UNITIG_F(cb), None, UNITIG_LINK_F(lcb) if links else UNITIG_LINK_F(),
                                        ctypes.byref(st))
        if stats is not None:
            stats.update(st.as_dict())
        self._chk(code, "rb3gpu_unitigs")
        out = (np.concatenate(utg) if utg else np.zeros(0, dtype=UNITIG_REC), np.concatenate(mem) if mem else np.zeros(0, dtype=UNITIG_MEMBER), seqs)
        return out + (np.concatenate(lnk) if lnk else np.zeros(0, dtype=UNITIG_LINK),) if links else out

    def fetch(self, rows, begs, ends, stats=False):
        """rb3gpu_fetch: the symbols [begs[i], ends[i]) of string rows[i] (0-based, end exclusive; string r is what retrieve([r]) spells), read through the
        sampled suffix array on the handle (ssa_keep / ssa_set): a list of uint8 arrays of nt6 codes in text order, in the order asked.  stats=True: (that list,
        rb3gpu_fetch_stats_t as a dict).  An invalid region raises with RB3GPU_EINVAL, the index of the first one in the message and in the error's `bad`"""
        reg = np.empty((len(rows), 3), dtype=np.int64)
        if len(rows) != len(begs) or len(rows) != len(ends):
            raise ValueError("rows, begs and ends must be of one length")
        reg[:, 0], reg[:, 1], reg[:, 2] = rows, begs, ends
        seqs = []

        def cb(_ud, _i0, n, off, symbols):
            o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
            buf = np.frombuffer(ctypes.string_at(symbols, int(o[n])), dtype=np.uint8) if o[n] > 0 else np.zeros(0, dtype=np.uint8)
            seqs.extend(buf[int(o[i]):int(o[i + 1])].copy() for i in range(n))
            return 0
        st, bad = FetchStats(), ctypes.c_int64(-1)
        r = self._lib.rb3gpu_fetch(self._h, reg.shape[0], reg.ctypes.data if reg.size else None, ctypes.byref(bad), FETCH_F(cb), None, ctypes.byref(st))
        if r < 0:
            e = Rb3GpuError(r, "rb3gpu_fetch" if bad.value < 0 else "rb3gpu_fetch (region %d)" % bad.value)
            e.bad = bad.value
            raise e
        return (seqs, st.as_dict()) if stats else seqs

    def hapdiv(self, queries, k=101, w=50, n_best=25, min_sc=30, match=1, mis=3, gap_open=5, gap_ext=2, e2e_drop=-1, stats=None):
        """rb3gpu_hapdiv on the windows of the queries (k symbols every w, as the reference's `hapdiv` cuts them; queries as for mem): an (n, 9) int32
        array, a row of n_al, max_ed, n_hap[0..6] per window in query order, and -- second value -- the (query, offset) of every window as an (n, 2)
        int64 array.  stats: a dict that receives rb3gpu_hapdiv_stats_t"""
        if k < 1 or w < 1:
            raise ValueError("k and w must be at least 1")
        qs = [nt6_of(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.int64)
        if qs:
            off[1:] = np.cumsum([q.size for q in qs])
        sym = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        where = [(i, x) for i, q in enumerate(qs) for x in range(0, q.size - k + 1, w)]
        where = np.array(where, dtype=np.int64).reshape(-1, 2)
        win = np.ascontiguousarray(off[where[:, 0]] + where[:, 1], dtype=np.int64)
        out = np.zeros((win.size, 9), dtype=np.int32)

        def cb(_ud, i0, n, recs):
            out[i0:i0 + n] = np.frombuffer(ctypes.string_at(recs, n * 36), dtype=np.int32).reshape(n, 9)
            return 0
        st = HapdivStats()
        opt = HapdivOpt(int(n_best), int(min_sc), int(match), int(mis), int(gap_open), int(gap_ext), int(e2e_drop))
        self._chk(self._lib.rb3gpu_hapdiv(self._h, win.size, win.ctypes.data if win.size else None, sym.ctypes.data if sym.size else None, int(k), ctypes.byref(opt),
                                          HAPDIV_F(cb), None, ctypes.byref(st)), "rb3gpu_hapdiv")
        if stats is not None:
            stats.update(st.as_dict())
        return out, where

    def sw_e2e(self, queries, n_best=25, min_sc=30, match=1, mis=3, gap_open=5, gap_ext=2, e2e_drop=-1, end_len=1, max_pos=None, stats=None, locate_stats=None):
        """rb3gpu_sw_e2e: the end-to-end alignments of the queries (as for mem) as the reference's `sw -e` finds them (end_len: its -k).  Returns a
        list with one entry per query: the list of its hits in the reference's order, each a dict of lo, hi, score, qlen, rlen, steps (bytes, one
        per step from query position 0 on: SW_OPS[b >> 4] and the base b & 15) and pos (a POS array; empty without positions).  max_pos None: no
        positions; 0 or more (the handle needs set_ssa / keep_ssa): what `sw -p max_pos` gives every hit, one position each at 0.
        stats / locate_stats: dicts that receive rb3gpu_sw_stats_t / rb3gpu_locate_stats_t"""
        qs = [nt6_of(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.int64)
        if qs:
            off[1:] = np.cumsum([q.size for q in qs])
        sym = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        out = [None] * len(qs)

        def cb(_ud, q0, nq, n_hit, hits, steps, pos):
            nh = np.frombuffer(ctypes.string_at(n_hit, nq * 4), dtype=np.int32)
            tot = int(nh.sum())
            hs = np.frombuffer(ctypes.string_at(hits, tot * SW_HIT.itemsize), dtype=SW_HIT) if tot else np.zeros(0, dtype=SW_HIT)
            at = 0
            for i in range(nq):
                mine = []
                for r in hs[at:at + int(nh[i])]:
                    st_b = ctypes.string_at(steps + int(r["step_off"]), int(r["n_steps"])) if r["n_steps"] else b""
                    n_pos = int(r["n_pos"])
                    pp = np.frombuffer(ctypes.string_at(pos + int(r["pos_off"]) * POS.itemsize, n_pos * POS.itemsize), dtype=POS).copy() if n_pos else np.zeros(0, dtype=POS)
                    mine.append(dict(lo=int(r["lo"]), hi=int(r["hi"]), score=int(r["score"]), qlen=int(r["qlen"]), rlen=int(r["rlen"]), steps=st_b, pos=pp))
                out[q0 + i] = mine
                at += int(nh[i])
            return 0
        st, lst = SwStats(), LocateStats()
        opt = SwOpt(int(n_best), int(min_sc), int(match), int(mis), int(gap_open), int(gap_ext), int(e2e_drop), int(end_len), -1 if max_pos is None else int(max_pos))
        self._chk(self._lib.rb3gpu_sw_e2e(self._h, len(qs), off.ctypes.data, sym.ctypes.data if sym.size else None, ctypes.byref(opt), SW_F(cb), None, ctypes.byref(st),
                                          ctypes.byref(lst)), "rb3gpu_sw_e2e")
        if stats is not None:
            stats.update(st.as_dict())
        if locate_stats is not None:
            locate_stats.update(lst.as_dict())
        return out

    def sw_local(self, queries, n_best=25, min_sc=30, match=1, mis=3, gap_open=5, gap_ext=2, end_len=11, max_pos=None, stats=None, locate_stats=None, dawg=None):
        """rb3gpu_sw_local: the best local hit of every query (as for mem) as the reference's `sw` finds it in its default mode (end_len: its -k), aligned
        over the query's DAWG, which the host library builds (host.dawg_batch; dawg: one built before, for the same queries).  Returns a list with one
        entry per query: the list of its hits, none or one, each a dict as of sw_e2e plus qoff0 (where the hit starts on the query), n_qoff (in how
        many places of the query the aligned part occurs: the qh tag) and node (the node of the graph it ends at).  qlen is the part of the query it
        spans.  max_pos as for sw_e2e.  stats receives rb3gpu_swl_stats_t (flat) and dawg_ms, the host's time for the graphs"""
        import time
        from . import host
        qs = [nt6_of(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.int64)
        if qs:
            off[1:] = np.cumsum([q.size for q in qs])
        sym = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        t0 = time.time()
        g = dawg if dawg is not None else host.dawg_batch(off, sym)
        dawg_ms = (time.time() - t0) * 1e3
        node_off = np.ascontiguousarray(g["node_off"], dtype=np.int64)
        nsym = np.ascontiguousarray(g["sym"], dtype=np.uint8)
        pre_off = np.ascontiguousarray(g["pre_off"], dtype=np.int64)
        pre = np.ascontiguousarray(g["pre"], dtype=np.int32)
        if node_off.size != len(qs) + 1 or (node_off.size and (pre_off.size != int(node_off[-1]) + 1 or nsym.size != int(node_off[-1]) or pre.size != int(pre_off[-1]))):
            raise ValueError("the graphs do not belong to these queries")
        hit_node = np.full(max(len(qs), 1), -1, dtype=np.int32)
        out = [None] * len(qs)

        def cb(_ud, q0, nq, n_hit, hits, steps, pos):
            nh = np.frombuffer(ctypes.string_at(n_hit, nq * 4), dtype=np.int32)
            tot = int(nh.sum())
            hs = np.frombuffer(ctypes.string_at(hits, tot * SW_HIT.itemsize), dtype=SW_HIT) if tot else np.zeros(0, dtype=SW_HIT)
            at = 0
            for i in range(nq):
                mine = []
                for r in hs[at:at + int(nh[i])]:
                    st_b = ctypes.string_at(steps + int(r["step_off"]), int(r["n_steps"])) if r["n_steps"] else b""
                    n_pos = int(r["n_pos"])
                    pp = np.frombuffer(ctypes.string_at(pos + int(r["pos_off"]) * POS.itemsize, n_pos * POS.itemsize), dtype=POS).copy() if n_pos else np.zeros(0, dtype=POS)
                    node = int(hit_node[q0 + i])
                    gi = int(node_off[q0 + i]) + node
                    mine.append(dict(lo=int(r["lo"]), hi=int(r["hi"]), score=int(r["score"]), qlen=int(r["qlen"]), rlen=int(r["rlen"]), steps=st_b, pos=pp,
                                     node=node, qoff0=int(g["qoff0"][gi]), n_qoff=int(g["n_qoff"][gi])))
                out[q0 + i] = mine
                at += int(nh[i])
            return 0
        st, lst = SwlStats(), LocateStats()
        opt = SwOpt(int(n_best), int(min_sc), int(match), int(mis), int(gap_open), int(gap_ext), -1, int(end_len), -1 if max_pos is None else int(max_pos))
        self._chk(self._lib.rb3gpu_sw_local(self._h, len(qs), off.ctypes.data, sym.ctypes.data if sym.size else None, node_off.ctypes.data, nsym.ctypes.data if nsym.size else None,
                                            pre_off.ctypes.data if pre_off.size else None, pre.ctypes.data if pre.size else None, ctypes.byref(opt), SW_F(cb), None,
                                            hit_node.ctypes.data, ctypes.byref(st), ctypes.byref(lst)), "rb3gpu_sw_local")
        if stats is not None:
            stats.update(st.as_dict())
            stats["dawg_ms"] = dawg_ms
        if locate_stats is not None:
            locate_stats.update(lst.as_dict())
        return out

    def sync(self):
        self._chk(self._lib.rb3gpu_sync(self._h), "rb3gpu_sync")

    def stats(self):
        st = Stats()
        self._chk(self._lib.rb3gpu_stats(self._h, ctypes.byref(st)), "rb3gpu_stats")
        return st.as_dict()

    def stats_reset(self):
        self._lib.rb3gpu_stats_reset(self._h)

    def buffers(self):
        """{name: bytes} of every device buffer the handle holds right now (rb3gpu_buffer_bytes)"""
        out, i = {}, 0
        name, nb = ctypes.c_char_p(), ctypes.c_int64()
        while self._lib.rb3gpu_buffer_bytes(self._h, i, ctypes.byref(name), ctypes.byref(nb)) == 0:
            if nb.value:
                out[name.value.decode()] = int(nb.value)
            i += 1
        return out


class CommGroup:
    """rb3gpu_group_*: the ranks of an interval-sharded index as THREADS of this process, one handle each (barriers + peer copies)"""

    def __init__(self, world, lib=None, hooks=False):
        self._lib = load_library(hooks, lib)
        self.world = int(world)
        self._g = self._lib.rb3gpu_group_create(self.world)
        if not self._g:
            raise Rb3GpuError(-3, "rb3gpu_group_create")

    def comm(self, rank, engine):
        c = GroupComm()
        c.struct = CommStruct()
        r = self._lib.rb3gpu_group_comm(self._g, int(rank), engine._h, ctypes.addressof(c.struct))
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_group_comm")
        c.group = self   # keeps the group alive
        return c

    def abort(self):
        self._lib.rb3gpu_group_abort(self._g)

    def close(self):
        if self._g:
            self._lib.rb3gpu_group_destroy(self._g)
            self._g = None


class GroupComm:
    struct = None


def ipc_peer_enable(engine, comm):
    """rb3gpu_ipc_peer_enable: PEER ROUNDS for ranks that are processes of one node (HIP IPC memory and event handles, a spin barrier in shared memory) on top
    of any communicator of world > 1.  COLLECTIVE: every rank calls it.  True: enabled on every rank; False: not available (the communicator is as it was)."""
    r = engine._lib.rb3gpu_ipc_peer_enable(engine._h, ctypes.addressof(comm.struct))
    if r == 0:
        return True
    if r == -7:
        return False
    raise Rb3GpuError(int(r), "rb3gpu_ipc_peer_enable")


def ipc_peer_disable(engine, comm):
    engine._lib.rb3gpu_ipc_peer_disable(ctypes.addressof(comm.struct))


class RcclComm:
    """rb3gpu_rccl_*: one process per GPU; grouped ncclSend/ncclRecv on the engine's stream.  `uid`: the 128 bytes rank 0 got
    from RcclComm.unique_id() and sent to the other ranks."""

    @staticmethod
    def unique_id(lib=None):
        l = load_library(False, lib)
        buf = ctypes.create_string_buffer(128)
        r = l.rb3gpu_rccl_unique_id(buf)
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_rccl_unique_id")
        return buf.raw

    def __init__(self, engine, rank, world, uid):
        self._lib = engine._lib
        self.struct = CommStruct()
        self.rank, self.world = int(rank), int(world)
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        r = self._lib.rb3gpu_rccl_comm_create(engine._h, self.rank, self.world, buf, ctypes.addressof(self.struct))
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_rccl_comm_create")
        self._open = True

    def close(self):
        if self._open:
            self._lib.rb3gpu_rccl_comm_destroy(ctypes.addressof(self.struct))
            self._open = False


class CallbackComm:
    """a communicator whose two collectives are Python callables (tests: gloo, threads):
    all_gather(vec int64[n]) -> array [world, n];  exchange(d_send, stride, send_counts, d_recv, recv_counts) with device pointers
    as ints (states of 16 bytes; region d of the send buffer starts at d_send + d * stride * 16)."""

    def __init__(self, rank, world, all_gather, exchange, abort=None):
        self.rank, self.world = int(rank), int(world)
        self.error = None

        def _ag(ctx, send, n, recv):
            try:
                out = np.asarray(all_gather(np.ctypeslib.as_array(send, shape=(n,)).copy()), dtype=np.int64).reshape(self.world * n)
                np.ctypeslib.as_array(recv, shape=(self.world * n,))[:] = out
                return 0
            except BaseException as e:   # (an exception must not unwind through the C frames)
                self.error = e
                return -6

        def _a2a(ctx, d_send, stride, send_cnt, d_recv, recv_cnt, stream):
            try:
                sc = np.ctypeslib.as_array(send_cnt, shape=(self.world,)).copy()
                rc = np.ctypeslib.as_array(recv_cnt, shape=(self.world,)).copy()
                # The send regions are complete ON THE ENGINE'S STREAM (include/rb3gpu.h): a callable that reads them with the runtime's synchronous copies -- the null
                # stream, which does not wait for a non-blocking stream -- must not start before that stream is done.  (The merge's last phase, the exchange with the owners
                # of the text ranges, calls this right behind the kernel that fills the regions: eight processes lost rows there, four got away with it.)
                if stream:
                    load_library().rb3gpu_stream_sync(stream)
                exchange(int(d_send or 0), int(stride), sc, int(d_recv or 0), rc)
                return 0
            except BaseException as e:
                self.error = e
                return -6

        def _ab(ctx):
            if abort is not None:
                try:
                    abort()
                except BaseException:
                    pass

        self._keep = (ALL_GATHER_F(_ag), ALL_TO_ALL_F(_a2a), ABORT_F(_ab))   # the C side holds raw pointers to these
        self.struct = CommStruct(None, self.rank, self.world, ctypes.cast(self._keep[0], ctypes.c_void_p), ctypes.cast(self._keep[1], ctypes.c_void_p), ctypes.cast(self._keep[2], ctypes.c_void_p))


class Shard:
    """rb3gpu_shard_*: the index of `engine` cut into n intervals (one handle per device of `devices`), batches merged by n threads
    inside the library, put back together by gather()"""

    def __init__(self, engine, devices):
        self._e, self._lib = engine, engine._lib
        dev = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        opt = Opt()
        self._lib.rb3gpu_opt_init(ctypes.byref(opt))
        opt.verbose = 1
        self._s = self._lib.rb3gpu_shard_split(engine._h, len(devices), dev, ctypes.addressof(opt))
        if not self._s:
            raise Rb3GpuError(-1, "rb3gpu_shard_split")
        self.n = len(devices)

    def bounds(self):
        b = np.zeros(self.n + 1, dtype=np.int64)
        self._lib.rb3gpu_shard_bounds(self._s, b.ctypes.data)
        return b

    def merge(self, d_bwt, d_tw, n2, sent_tp):
        tp = np.ascontiguousarray(sent_tp, dtype=np.int64)
        rounds = ctypes.c_int64(0)
        r = self._lib.rb3gpu_shard_merge(self._s, int(n2), d_bwt, d_tw, tp.size, tp.ctypes.data, ctypes.addressof(rounds))
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_shard_merge")
        return int(rounds.value)

    def get_acc(self):
        a = np.zeros(7, dtype=np.int64)
        r = self._lib.rb3gpu_shard_get_acc(self._s, a.ctypes.data)
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_shard_get_acc")
        return a

    def export_plain(self):
        """the whole index as one byte per symbol, straight from the intervals in rank order (rb3gpu_shard_export_runs: no gather)"""
        out = []
        runs = []

        def emit(_d, c, l):
            runs.append((int(c), int(l)))
            return 0
        cb = EMIT_F(emit)
        r = self._lib.rb3gpu_shard_export_runs(self._s, cb, None)
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_shard_export_runs")
        assert all(runs[i][0] != runs[i + 1][0] for i in range(len(runs) - 1)), "runs that meet at a seam must be joined"
        for c, l in runs:
            out.append(np.full(l, c, dtype=np.uint8))
        return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)

    def export_run_words(self):
        """(starts, symbols) of the maximal runs of the whole index and its length, from rb3gpu_shard_export_run_words"""
        words, end = [], [-1]

        def emit(_d, n, w, e):
            if n > 0:
                words.append(np.ctypeslib.as_array(w, shape=(n,)).copy())
            if e >= 0:
                end[0] = int(e)
            return 0
        cb = EMITW_F(emit)
        r = self._lib.rb3gpu_shard_export_run_words(self._s, cb, None)
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_shard_export_run_words")
        w = np.concatenate(words) if words else np.zeros(0, dtype=np.uint64)
        return (w >> np.uint64(3)).astype(np.int64), (w & np.uint64(7)).astype(np.uint8), end[0]

    def rebalance(self, pct=25):
        r = self._lib.rb3gpu_shard_rebalance(self._s, int(pct))
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_shard_rebalance")
        return int(r)

    def handle_stats(self, i):
        st = Stats()
        self._lib.rb3gpu_stats(self._lib.rb3gpu_shard_handle(self._s, int(i)), ctypes.byref(st))
        return st.as_dict()

    def destroy(self):
        s, self._s = self._s, None
        if s:
            self._lib.rb3gpu_shard_destroy(s)

    def gather(self):
        s, self._s = self._s, None
        r = self._lib.rb3gpu_shard_gather(s)
        if r < 0:
            raise Rb3GpuError(int(r), "rb3gpu_shard_gather")


def read_bre(path):
    """a BRE file (bre.h of the reference) -> (b_per_run, records, (n_rec, n_sym, n_run)): the raw records in front of the all-zero
    record and the footer's three counts.  ValueError for anything the host library's reader refuses as well"""
    raw = open(path, "rb").read()
    if raw[:4] != b"BRE\x01" or len(raw) < 24:
        raise ValueError("not a BRE file")
    bps, bpr = raw[4], raw[5]
    asize, l_aux = int.from_bytes(raw[8:16], "little"), int.from_bytes(raw[16:24], "little")
    if bps != 1 or asize != 6 or not 1 <= bpr <= 8:
        raise ValueError("BRE header: b_per_sym %d, b_per_run %d, asize %d" % (bps, bpr, asize))
    body, rs = raw[24 + l_aux:], 1 + bpr
    a = np.frombuffer(body[:len(body) // rs * rs], dtype=np.uint8).reshape(-1, rs)
    zero = np.flatnonzero(~a.any(axis=1))
    if zero.size == 0:
        raise ValueError("BRE file without an all-zero record")
    n_rec = int(zero[0])
    if n_rec == 0 or int(a[:n_rec, 0].max()) > 5 or not a[:n_rec, 1:].any(axis=1).all():
        raise ValueError("BRE file with no records, a symbol above 5 or a record of no symbols")
    ftr = body[(n_rec + 1) * rs:]
    if len(ftr) < 24:
        raise ValueError("BRE file without a footer")
    counts = tuple(int.from_bytes(ftr[8 * i:8 * i + 8], "little") for i in range(3))
    if counts[0] != n_rec:
        raise ValueError("BRE footer: %d records, the file holds %d" % (counts[0], n_rec))
    return bpr, body[:n_rec * rs], counts


def write_bre(path, records, b_per_run, counts):
    """header, records, all-zero record and the three counts (n_rec, n_sym, n_run) as a BRE file"""
    with open(path, "wb") as fp:
        fp.write(b"BRE\x01" + bytes([1, int(b_per_run), 2, 0]) + (6).to_bytes(8, "little") + (0).to_bytes(8, "little"))
        fp.write(bytes(records))
        fp.write(bytes(1 + int(b_per_run)) + b"".join(int(c).to_bytes(8, "little") for c in counts))


def kount_lines(kmers, counts):
    """the reference's `kount` output for (kmers, counts) of Rb3Gpu.kount: the k-mer, then a tab and the count per index, per line (bytes)"""
    kmers = np.asarray(kmers, dtype=np.uint8)
    counts = np.asarray(counts, dtype=np.int64)
    lut = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    out = []
    for s, c in zip(lut[kmers], counts):
        out.append(s.tobytes() + b"".join(b"\t%d" % x for x in c) + b"\n")
    return b"".join(out)


_NT6 = np.full(256, 5, dtype=np.uint8)
_NT6[:5] = np.arange(5)
for _i, _c in enumerate(b"ACGT"):
    _NT6[_c] = _NT6[_c + 32] = _i + 1


def nt6_of(q):
    """a query as nt6 codes: characters (bytes / str) through the reference's table (A C G T in either case 1..4, anything else 5); arrays as they are"""
    if isinstance(q, str):
        q = q.encode()
    if isinstance(q, (bytes, bytearray)):
        return _NT6[np.frombuffer(bytes(q), dtype=np.uint8)]
    return np.ascontiguousarray(q, dtype=np.uint8)


def read_ssa(path):
    """a .ssa file (rb3_ssa_dump, ssa.c:198-213): (ssa_shift, ms, r2i, ssa), the arrays uint64"""
    with open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"SSA\1" or len(b) < 28:
        raise ValueError("not a sampled suffix array: %s" % path)
    ss, ms = np.frombuffer(b, dtype="<u4", count=2, offset=4)
    m, n = np.frombuffer(b, dtype="<i8", count=2, offset=12)
    if len(b) < 28 + 8 * (int(m) + int(n)):
        raise ValueError("truncated sampled suffix array: %s" % path)
    return int(ss), int(ms), np.frombuffer(b, dtype="<u8", count=int(m), offset=28).copy(), np.frombuffer(b, dtype="<u8", count=int(n), offset=28 + 8 * int(m)).copy()


def mem_lines(recs, names=None, first_id=0, positions=None, seq_names=None, lengths=None):
    """the reference's `mem` output for the records of Rb3Gpu.mem: name, start, end, occurrences per match (bytes); names[q] is the name of
    query q (None, or a None entry: seq<first_id + q + 1>, as for queries without a name).  positions = (off, pos) of Rb3Gpu.mem(max_pos=...)
    with the names and lengths of the indexed sequences (seq_names, lengths: what <index>.len.gz holds) adds the `-p` columns"""
    out = []
    if positions is not None:
        off, pos = positions
        for i, r in enumerate(recs):
            q = int(r["query"])
            nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
            if isinstance(nm, str):
                nm = nm.encode()
            line = b"%s\t%d\t%d\t%d" % (nm, r["st"], r["en"], r["size"])
            a, b = int(off[i]), int(off[i + 1])
            if b > a:
                line += b"\t%d" % (b - a)
                for p in pos[a:b]:
                    s = int(p["sid"]) >> 1
                    sn = seq_names[s].encode() if isinstance(seq_names[s], str) else seq_names[s]
                    x = int(lengths[s]) - (int(p["pos"]) + int(r["en"]) - int(r["st"])) if int(p["sid"]) & 1 else int(p["pos"])
                    line += b"\t%s:%s:%d" % (sn, b"-" if int(p["sid"]) & 1 else b"+", x)
            out.append(line + b"\n")
        return b"".join(out)
    for r in recs:
        q = int(r["query"])
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        if isinstance(nm, str):
            nm = nm.encode()
        out.append(b"%s\t%d\t%d\t%d\n" % (nm, r["st"], r["en"], r["size"]))
    return b"".join(out)


def suffix_lines(recs, names=None, first_id=0):
    """the reference's `suffix` output for the records of Rb3Gpu.suffix: name, start, length of the query, occurrences per query (bytes); names as
    for mem_lines -- a query without a name is seq<first_id + q + 1>, the running number of the record"""
    out = []
    for r in recs:
        q = int(r["query"])
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        if isinstance(nm, str):
            nm = nm.encode()
        out.append(b"%s\t%d\t%d\t%d\n" % (nm, r["start"], r["length"], r["size"]))
    return b"".join(out)


def get_lines(rows, end_rows, seqs):
    """the reference's `get` output for (end_rows, seqs) of Rb3Gpu.retrieve(rows): `>row end_row` and the string in $ACGTN letters, two lines per row;
    nothing for a row outside the index (end row -1)"""
    lut = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    out = []
    for k, e, s in zip(rows, end_rows, seqs):
        if int(e) >= 0:
            out.append(b">%d %d\n" % (int(k), int(e)) + lut[np.minimum(np.asarray(s, dtype=np.uint8), 5)].tobytes() + b"\n")
    return b"".join(out)


def hapdiv_lines(recs, where, k, names=None, first_id=0):
    """the reference's `hapdiv` output for the windows of Rb3Gpu.hapdiv (recs, where as it returns them): consecutive windows of one query with the
    same nine numbers make one line -- name, first offset, last offset + k, n_al, max_ed, n_hap[0..6] (bytes); names as for mem_lines"""
    out, i, n = [], 0, len(recs)
    while i < n:
        j = i + 1
        while j < n and where[j][0] == where[i][0] and np.array_equal(recs[j], recs[i]):
            j += 1
        q = int(where[i][0])
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        if isinstance(nm, str):
            nm = nm.encode()
        out.append(nm + b"\t%d\t%d" % (int(where[i][1]), int(where[j - 1][1]) + k) + b"".join(b"\t%d" % int(x) for x in recs[i]) + b"\n")
        i = j
    return b"".join(out)


def sw_cigar(steps):
    """(cigar string, matching length, block length) of the step bytes of a hit"""
    runs = []
    for b in steps:
        if runs and runs[-1][1] == b >> 4:
            runs[-1][0] += 1
        else:
            runs.append([1, b >> 4])
    return "".join("%d%s" % (n, "=XID"[op]) for n, op in runs), sum(n for n, op in runs if op == 0), len(steps)


def sw_cs(steps, query):
    """the cs string of a hit: query is the nt6 codes that were aligned"""
    out, y, i, n = [], 0, 0, len(steps)
    while i < n:
        j, op = i, steps[i] >> 4
        while j < n and steps[j] >> 4 == op:
            j += 1
        if op == 0:
            out.append(":%d" % (j - i))
        elif op == 1:
            out.extend("*%s%s" % ("$acgtn"[min(int(query[y + t - i]), 5)], "$acgtn"[steps[t] & 15]) for t in range(i, j))
        elif op == 2:
            out.append("+" + "".join("$acgtn"[min(int(query[y + t]), 5)] for t in range(j - i)))
        else:
            out.append("-" + "".join("$acgtn"[steps[t] & 15] for t in range(i, j)))
        if op != 3:
            y += j - i
        i = j
    return "".join(out)


def sw_rs(steps):
    """the aligned symbols of the index (the rs tag of --seq)"""
    return "".join("$ACGTN"[b & 15] for b in steps if b >> 4 != 2)


def sw_lines(queries, hits, names=None, first_id=0, seq_names=None, lengths=None, unmapped=False, with_rs=False):
    """the reference's PAF (`sw -e`, `sw`) for the hits of Rb3Gpu.sw_e2e or Rb3Gpu.sw_local (bytes).  queries: what was aligned; names as for mem_lines; seq_names and lengths
    (what <index>.len.gz holds) name the positions -- without them a position is written as string number and offset, and a hit without a position
    has stars.  unmapped: the -u lines; with_rs: the rs tag of --seq"""
    out = []
    for q, (query, mine) in enumerate(zip(queries, hits)):
        query = nt6_of(query)
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        if isinstance(nm, bytes):
            nm = nm.decode()
        if not mine and unmapped:
            out.append("%s\t%d\t*\t*\t*\t*\t*\t*\t*\t0\t0\t0\n" % (nm, query.size))
        for h in mine:
            rlen, pos = h["rlen"], h["pos"]
            cg, mlen, blen = sw_cigar(h["steps"])

            def stranded(p):
                clen, x = int(lengths[int(p["sid"]) >> 1]), int(p["pos"])
                return (clen, x, x + rlen) if int(p["sid"]) & 1 == 0 else (clen, clen - (x + rlen), clen - x)
            q0 = h.get("qoff0", 0)         # (a local hit starts where its node does; an end-to-end one at 0)
            f = [nm, str(query.size), str(q0), str(q0 + h["qlen"])]
            if len(pos) > 0:
                sid = int(pos[0]["sid"])
                if seq_names is not None:
                    clen, st, en = stranded(pos[0])
                    f += ["+-"[sid & 1], seq_names[sid >> 1], str(clen), str(st), str(en)]
                else:
                    f += ["+", str(sid), "*", str(int(pos[0]["pos"])), str(int(pos[0]["pos"]) + rlen)]
            else:
                f += ["*", "*", str(rlen), "*", "*"]
            f += [str(mlen), str(blen), "0", "AS:i:%d" % h["score"], "qh:i:%d" % h.get("n_qoff", 1), "rh:i:%d" % (h["hi"] - h["lo"]), "cg:Z:" + cg, "cs:Z:" + sw_cs(h["steps"], query[q0:])]
            if with_rs:
                f.append("rs:Z:" + sw_rs(h["steps"]))
            if len(pos) > 1:
                if seq_names is not None:
                    f.append("ap:Z:" + "".join("%s,%s,%d;" % (seq_names[int(p["sid"]) >> 1], "+-"[int(p["sid"]) & 1], stranded(p)[1]) for p in pos[1:]))
                else:
                    f.append("aq:Z:" + "".join("%d,%d;" % (int(p["sid"]), int(p["pos"])) for p in pos[1:]))
            out.append("\t".join(f) + "\n")
    return "".join(out).encode()


SW_ALL_HEADER = b"CC\tQS  queryName  queryLen  numHap\nCC\tQH  refCount   score     editDist   cs   strand   nOut   totAln\nCC\n"


def sw_all_lines(queries, hits, names=None, first_id=0, max_out=0, hits_rev=None):
    """the reference's compact format (`sw --all-e2e`, `-g max_out`) without its three header lines (SW_ALL_HEADER): a QS line, the QH lines and // per
    query; hits_rev: the hits of the reverse-complemented queries (-b), written as the `-` block behind each `+` block"""
    out = []
    cap = max_out if max_out > 0 else 1 << 62
    for q, query in enumerate(queries):
        query = nt6_of(query)
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        if isinstance(nm, bytes):
            nm = nm.decode()
        for strand, mine in (("+", hits[q]),) + ((("-", hits_rev[q]),) if hits_rev is not None else ()):
            seq = query if strand == "+" else revcomp6(query)
            tot = sum(h["hi"] - h["lo"] for h in mine)
            n_out = 0
            for h in mine:
                n_out += h["hi"] - h["lo"]
                if n_out >= cap:
                    break
            out.append("QS\t%s\t%d\t%d\t%s\t%d\t%d\n" % (nm, query.size, len(mine), strand, n_out, tot))
            n_out = 0
            for h in mine:
                _, mlen, blen = sw_cigar(h["steps"])
                out.append("QH\t%d\t%d\t%d\t%s\n" % (h["hi"] - h["lo"], h["score"], blen - mlen, sw_cs(h["steps"], seq)))
                n_out += h["hi"] - h["lo"]
                if n_out >= cap:
                    break
            out.append("//\n")
    return "".join(out).encode()


def revcomp6(q):
    """the reverse complement of nt6 codes (rb3_revcomp6: 1..4 are complemented, everything else stays)"""
    q = np.asarray(q, dtype=np.uint8)[::-1].copy()
    m = (q >= 1) & (q <= 4)
    q[m] = 5 - q[m]
    return q
