"""ribbit_amd -- MI355X-native implementation of ribbit's shift-XOR tandem-repeat scan.

This module is only the Python face of the C ABI in include/ribbit_hip.h (ctypes, no torch
types cross the boundary).  All compute happens in ribbit_amd/libribbit_hip.so (hand-written
gfx950 kernels + C++ host logic).  There is no CPU fallback: importing works anywhere, but
opening a scanner without the built library or without a gfx950 GPU raises.

How the module is laid out: _signatures() is the one table of the C signatures (ABI_SYMBOLS is its keys, load_library() applies
it); _ok, _ptr, _bytes, _name, _records, _call, _array and _text are what every wrapper is made of; every row output is
marshalled once, in a _record_*(call, ...) function that its host_record_* twin and its Scanner.record_* method both call.
An array's address does not keep the array alive: whatever _ptr() is given is bound to a local name of the calling frame.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

__all__ = ["RibbitHipError", "ScanParams", "Scanner", "library_path", "load_library", "host_replay_calls", "pack_planes", "pack_bit_planes",
           "RUN_DT", "CALL_DT", "SEED_DT", "JOB_DT", "ENDS_DT", "RANK", "TERM", "RefineParams", "host_refine_jobs", "host_refine_bed", "host_merge_chunks", "host_perfect_runs_from_events", "pair_halves", "ssw_align", "ssw_align_periodic", "merge_chunk_runs", "join_run_halves",
           "RUN_NOT_OWNED", "RUN_HALF_START", "RUN_HALF_END",
           "MASK_MODES", "host_mask_record", "bed_intervals", "host_repeat_sequences",
           "LOCUS_DT", "host_record_loci", "host_record_density", "bed_loci_text",
           "OverlapTotals", "OVERLAP_TOTALS", "host_record_overlap", "bed_overlap_text",
           "host_record_best", "bed_rows_text",
           "MOTIF_CLASS_DT", "bed_motifs", "host_record_classes", "bed_class_text", "class_summary_text",
           "COMPOUND_DT", "host_record_compounds", "class_labels", "compound_text",
           "INTERRUPTION_DT", "ROW_PURITY_DT", "bed_cigars", "host_record_interruptions", "interruption_text", "bed_purity_text",
           "Nearest", "NEAREST_DT", "host_record_nearest", "bed_nearest_text", "nearest_other_text",
           "COMPOSITION_DT", "BASE_COUNTS_DT", "host_record_composition", "host_record_base_windows", "bed_composition_text", "base_windows_text",
           "PRIMERS_DT", "PrimerParams", "primer_params", "host_record_primers", "bed_primers_text",
           "PRIMER_PAIRS_DT", "PrimerPairParams", "primer_pair_params", "host_record_primer_pairs", "bed_primer_pairs_text", "oligo_duplex", "oligo_hairpin",
           "PRIMER_PRODUCTS_DT", "OLIGO_SITES_DT", "ProductParams", "product_params", "host_record_oligo_sites", "host_record_primer_products",
           "bed_primer_products_text",
           "PRIMER_SPECIFIC_DT", "host_record_specific_primer_pairs", "bed_primer_specific_text",
           "PRIMER_SHORTLISTS_DT", "PRIMER_VERDICTS_DT", "host_record_primer_shortlists", "host_record_shortlist_verdicts", "primer_verdicts_merge",
           "primer_shortlists_choose",
           "PAIR_AMPLICONS_DT", "host_record_pair_amplicons", "pair_amplicons_merge", "bed_marker_text",
           "PANEL_DT", "PanelParams", "panel_params", "host_panel_pools", "bed_panel_text",
           "ALLELES_DT", "pair_amplicon_sizes", "host_marker_alleles", "bed_alleles_text", "allele_matrix_text"]

_HERE = os.path.dirname(os.path.abspath(__file__))

RANK = {"P": 5, "Q": 4, "S": 3, "F": 2, "C": 1, "A": 0, "N": -1}     # global_variables.cpp:28-34
TERM = {"ZERO": 0, "N": 1, "EOS": 2}

JOB_DT = np.dtype([("seed_index", "<i4"), ("seed_type", "<i4"), ("motif_length", "<i4"), ("atomicity", "<i4"),
                   ("query_start", "<i4"), ("query_length", "<i4"), ("ppr_length", "<i4"), ("small", "<i4"),
                   ("motif_offset", "<i4")])
ENDS_DT = np.dtype([(n, "<i4") for n in ("score", "ref_end", "query_end", "score2", "ref_end2", "ref_begin", "query_begin", "flag")])
RUN_DT = np.dtype([("start", "<i4"), ("end", "<i4"), ("mlen", "<i4"), ("term", "<i4")])
CALL_DT = np.dtype([("pos", "<i4"), ("mlen", "<i4"), ("start", "<i4"), ("end", "<i4")])
SEED_DT = np.dtype([("start", "<i4"), ("end", "<i4"), ("mlen", "<i4"), ("type", "<i4")])
LOCUS_DT = np.dtype([(n, "<i4") for n in ("start", "end", "rows", "covered", "best_row")])      # RibbitLocus
MOTIF_CLASS_DT = np.dtype([("bases", "<i8")] + [(n, "<i4") for n in ("length", "rows", "first_row", "longest_row")])      # RibbitMotifClass
COMPOUND_DT = np.dtype([("bases", "<i8")] + [(n, "<i4") for n in ("start", "end", "rows", "classes", "switches", "overlaps", "first", "pad")])      # RibbitCompound
INTERRUPTION_DT = np.dtype([(n, "<i4") for n in ("row", "start", "end", "x", "ins", "del", "cigar_at", "cigar_len")])      # RibbitInterruption
ROW_PURITY_DT = np.dtype([(n, "<i4") for n in ("first", "count", "x", "ins", "del", "query", "pure_start", "pure_end")])      # RibbitRowPurity
NEAREST_DT = np.dtype([(n, "<i4") for n in ("kind", "hit", "left", "left_dist", "right", "right_dist")])      # RibbitNearest

COMPOSITION_DT = np.dtype([(n, "<i4") for n in ("a", "c", "g", "t", "other", "left", "left_gc", "left_other", "left_covered",
                                                 "right", "right_gc", "right_other", "right_covered")])      # RibbitRowComposition
BASE_COUNTS_DT = np.dtype([(n, "<i4") for n in ("a", "c", "g", "t", "other")])      # RibbitBaseCounts
PRIMERS_DT = np.dtype([(f"{side}_{n}", "<i4") for side in ("left", "right") for n in ("start", "length", "tm", "penalty", "bases_lo", "bases_hi")]
                      + [("left_candidates", "<i4"), ("right_candidates", "<i4")])      # RibbitRowPrimers
PRIMER_PAIRS_DT = np.dtype([(f"{side}_{n}", "<i4") for side in ("left", "right") for n in ("start", "length", "tm", "penalty", "bases_lo", "bases_hi")]
                           + [(n, "<i4") for n in ("pair_penalty", "tm_difference", "product", "left_rank", "right_rank", "left_self_any", "left_self_end", "left_hairpin",
                                                   "right_self_any", "right_self_end", "right_hairpin", "pair_any", "pair_end", "left_candidates", "right_candidates",
                                                   "left_passed", "right_passed", "pairs_tried", "pairs_admissible", "reserved")])      # RibbitRowPrimerPair
PRIMER_PRODUCTS_DT = np.dtype([(n, "<i4") for n in ("left_forward", "left_reverse", "right_forward", "right_reverse", "products", "own", "shortest_other",
                                                     "reserved")])      # RibbitRowProducts
PRIMER_SPECIFIC_DT = np.dtype([(n, "<i4") for n in ("place", "pairs_admissible", "pairs_specific", "pairs_over", "pairs_other", "first_products", "reserved0",
                                                     "reserved1")])      # RibbitRowSpecific
_PRIMER_DT = np.dtype([(n, "<i4") for n in ("start", "length", "tm", "penalty", "bases_lo", "bases_hi")])      # RibbitPrimer
PRIMER_SHORTLISTS_DT = np.dtype([("left", _PRIMER_DT, (8,)), ("right", _PRIMER_DT, (8,))]
                                + [(n, "<i4") for n in ("left_candidates", "right_candidates", "left_passed", "right_passed")])      # RibbitTargetShortlists
PRIMER_VERDICTS_DT = np.dtype([(n, "<u8") for n in ("admissible", "over", "other", "own")] + [("forward", "<i4", (16,)), ("reverse", "<i4", (16,))]
                              + [(n, "<i4") for n in ("first_others", "records", "home_records", "reserved")])      # RibbitTargetVerdicts
PAIR_AMPLICONS_DT = np.dtype([(n, "<i4") for n in ("left_forward", "left_reverse", "right_forward", "right_reverse", "products", "record", "start", "end",
                                                    "forward_of", "reverse_of", "inner_start", "inner_end", "tract_start", "tract_end", "tract_strand",
                                                    "reserved")])      # RibbitRowAmplicon
ALLELES_DT = np.dtype([(n, "<i4") for n in ("typed", "absent", "several", "over", "alleles", "min_size", "max_size", "major_size", "major_count", "same", "off_step",
                                             "reserved")] + [("het_num", "<i8"), ("pic_num", "<i8")])      # RibbitRowAlleles
PANEL_DT = np.dtype([(n, "<i4") for n in ("pool", "conflicts", "dimer", "size", "near", "reserved0", "reserved1", "reserved2")])      # RibbitPanelRow
OLIGO_SITES_DT = np.dtype([(n, "<i4") for n in ("forward", "reverse", "forward_at", "reverse_at")])      # RibbitOligoSites
_OLIGO_DT = np.dtype([(n, "<i4") for n in ("length", "bases_lo", "bases_hi")])      # RibbitOligo
_I4 = np.dtype("<i4")

MASK_MODES = {"soft": 0, "hard": 1}     # RIBBIT_MASK_SOFT / RIBBIT_MASK_HARD


class RibbitHipError(RuntimeError):
    pass


class ScanParams(C.Structure):
    """RibbitScanParams (ribbit.cpp:191,240-243; fasta_utils.cpp:165)."""
    _fields_ = [("min_motif", C.c_int32), ("max_motif", C.c_int32), ("window_length", C.c_int32),
                ("subst_threshold", C.c_int32), ("anchor_threshold", C.c_int32), ("anchor_length", C.c_int32)]


class OverlapTotals(C.Structure):
    """RibbitOverlapTotals: what record_overlap counts over all rows and all OTHER intervals (include/ribbit_hip.h)."""
    _fields_ = [("rows_bases", C.c_int64), ("other_bases", C.c_int64), ("both_bases", C.c_int64),
                ("rows", C.c_int32), ("rows_hit", C.c_int32), ("other", C.c_int32), ("other_hit", C.c_int32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in OVERLAP_TOTALS}


# the totals in the order of ribbit-hip --overlap-summary's columns (behind name and length)
OVERLAP_TOTALS = ("rows", "rows_hit", "other", "other_hit", "rows_bases", "other_bases", "both_bases")


class Nearest(C.Structure):
    """RibbitNearest: what record_nearest finds for one query (include/ribbit_hip.h; kind 0: apart, 1: over, 2: inside); NEAREST_DT is
    the same record for numpy."""
    _fields_ = [(n, C.c_int32) for n in ("kind", "hit", "left", "left_dist", "right", "right_dist")]


class PrimerParams(C.Structure):
    """RibbitPrimerParams: what record_primers takes for a primer (include/ribbit_hip.h; Tm in tenths of a degree); primer_params()
    fills one."""
    _fields_ = [(n, C.c_int32) for n in ("flank", "min_length", "max_length", "opt_length", "tm_min", "tm_opt", "tm_max", "gc_min_percent", "gc_max_percent",
                                         "max_run", "gc_clamp")]


class PrimerPairParams(C.Structure):
    """RibbitPrimerPairParams: the shortlist and the limits record_primer_pairs holds a pair to (include/ribbit_hip.h; the Tm
    difference in tenths of a degree); primer_pair_params() fills one."""
    _fields_ = [(n, C.c_int32) for n in ("shortlist", "max_self_any", "max_self_end", "max_hairpin", "max_pair_any", "max_pair_end", "max_tm_difference")]


class ProductParams(C.Structure):
    """RibbitProductParams: the exact 3' seed, the mismatches outside it, the longest product and the longest list of sites
    that record_oligo_sites and record_primer_products work with (include/ribbit_hip.h); product_params() fills one."""
    _fields_ = [(n, C.c_int32) for n in ("seed", "max_mismatches", "max_product", "max_sites")]


class PanelParams(C.Structure):
    """RibbitPanelParams: the cross-dimer limits, the least distance of two product sizes, the longest product two pairs of one
    record may make between them and the members of a pool that panel_pools works with (include/ribbit_hip.h); panel_params()
    fills one."""
    _fields_ = [(n, C.c_int32) for n in ("max_cross_any", "max_cross_end", "size_gap", "max_cross_product", "pool_size")]


class DebugPairing(C.Structure):
    """RibbitDebugPairing: the caller's buffers and the words ribbit_hip_debug_pair_events_sharded fills (include/ribbit_hip.h)."""
    _fields_ = [("runs", C.c_void_p), ("runs_cap", C.c_size_t), ("halves", C.c_void_p), ("halves_cap", C.c_size_t),
                ("dense", C.c_void_p), ("dense_cap", C.c_size_t), ("table", C.c_void_p), ("table_cap", C.c_size_t),
                ("status", C.c_uint32 * 3), ("published", C.c_uint32 * 64),
                ("summary", C.c_uint32), ("overflow", C.c_uint32), ("table_status", C.c_uint32)]


class SeedLists(C.Structure):
    """RibbitSeedLists (malloc'ed arrays returned by ribbit_host_replay_calls)."""
    _fields_ = [("perfect", C.c_void_p), ("n_perfect", C.c_size_t), ("subst", C.c_void_p), ("n_subst", C.c_size_t),
                ("anchored", C.c_void_p), ("n_anchored", C.c_size_t), ("dispatch", C.c_void_p), ("n_dispatch", C.c_size_t),
                ("guard_hits", C.c_int64)]


class DebugMergeKnobs(C.Structure):
    """RibbitDebugMergeKnobs: where and how ribbit_hip_debug_merge_ranges runs the first pass (include/ribbit_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("where", "full", "calls_per_range", "resident_waves", "max_passes", "head_cap")] + \
               [(n, C.c_int64) for n in ("log_cap", "device_limit", "only_range")]


class DebugMergeRanges(C.Structure):
    """RibbitDebugMergeRanges: what ribbit_hip_debug_merge_ranges fills (include/ribbit_hip.h)."""
    _fields_ = [("ran", C.c_int32), ("reserved", C.c_int32), ("caps", C.c_int32 * 16), ("n_ranges", C.c_size_t),
                ("cuts", C.c_void_p), ("first", C.c_void_p), ("cursors0", C.c_void_p), ("range", C.c_void_p),
                ("own", C.c_void_p), ("n_own", C.c_size_t), ("undo", C.c_void_p), ("n_undo", C.c_size_t),
                ("reads", C.c_void_p), ("n_reads", C.c_size_t), ("heads", C.c_void_p), ("n_heads", C.c_size_t),
                ("lists", SeedLists), ("device_merge", C.c_int32 * 5)]


class RefineParams(C.Structure):
    """RibbitRefineParams (MINIMUM_LENGTH / PERFECT_UNITS tables, purity, cones threshold)."""
    _fields_ = [("min_length", C.c_int32 * 1024), ("perfect_units", C.c_int32 * 1024),
                ("purity_threshold", C.c_float), ("continuous_ones_threshold", C.c_int32)]


class Alignment(C.Structure):
    """RibbitAlignment (StripedSmithWaterman::Alignment without the strings)."""
    _fields_ = [(n, C.c_int32) for n in ("sw_score", "sw_score_next_best", "ref_begin", "ref_end", "query_begin",
                                         "query_end", "ref_end_next_best", "mismatches", "flag", "cigar_len")]


class ChunkCalls(C.Structure):
    """RibbitChunkCalls: what one window stage of one chunk of a longer record keeps (ribbit_hip_stage_calls_chunk)."""
    _fields_ = [("calls", C.c_void_p), ("n", C.c_size_t), ("pend", C.c_void_p), ("tail_pend", C.c_int32), ("inexact", C.c_int32),
                ("flush", C.c_void_p), ("n_flush", C.c_size_t), ("dev_calls", C.c_void_p), ("dev_pend", C.c_void_p), ("streaks", C.c_int64)]


class DebugWindowStage(C.Structure):
    """RibbitDebugWindowStage: the caller-made streaks and the chunk window of ribbit_hip_debug_window_calls (include/ribbit_hip.h)."""
    _fields_ = [("streaks", C.c_void_p), ("n_streaks", C.c_size_t), ("min_span", C.c_void_p), ("dropped_ends", C.c_void_p),
                ("n_dropped", C.c_size_t), ("own_lo", C.c_int64), ("own_hi", C.c_int64), ("z_lo", C.c_int64), ("pos_offset", C.c_int64),
                ("first_edge_cap", C.c_size_t), ("full", C.c_int32), ("keep_flush", C.c_int32)]


class ChunkPart(C.Structure):
    """RibbitChunkPart: one chunk's contribution to ribbit_host_merge_chunks."""
    _fields_ = [("runs", C.c_void_p), ("n_runs", C.c_size_t), ("halves", C.c_void_p), ("n_halves", C.c_size_t),
                ("subst", ChunkCalls), ("anchored", ChunkCalls)]


STAGE_PERFECT, STAGE_SUBST, STAGE_ANCHORED = 0, 1, 2
# scan kernels of Scanner.debug_set_scan_split (RIBBIT_SCAN_* of include/ribbit_hip.h)
SCAN_PERFECT, SCAN_SUBST, SCAN_ANCHORED, SCAN_XA_WINDOW, SCAN_ALL = 0, 1, 2, 3, 4


def _signatures() -> dict:
    """{symbol: (restype, argtypes)} of every symbol include/ribbit_hip.h declares (tests/test_abi.py holds the keys to the header).
    c_char_p takes bytes, c_void_p an integer address or a byref(): they are not interchangeable."""
    P, vp, cp, sz, ci, i32, i64 = C.POINTER, C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int32, C.c_int64
    st = C.c_int                                     # a status: 0, or an error that ribbit_hip_last_error() explains
    pvp, psz, pi32 = P(vp), P(sz), P(i32)
    scan, refine = P(ScanParams), P(RefineParams)
    planes = [i64, vp, vp, vp, sz, vp, sz]           # length, hi, lo, brk, their words, xa, its stride
    t = {
        "ribbit_scan_params_default": (None, [scan, i32, i32]),
        "ribbit_hip_last_error": (cp, []),
        "ribbit_hip_abi_version": (ci, []),
        "ribbit_hip_device_count": (ci, []),
        "ribbit_hip_open": (st, [scan, ci, pvp]),
        "ribbit_hip_close": (st, [vp]),
        "ribbit_hip_set_stream": (st, [vp, vp]),
        "ribbit_hip_load_record": (st, [vp, cp, i64]),
        "ribbit_hip_load_record_device": (st, [vp, vp, i64]),
        "ribbit_hip_load_record_pinned": (st, [vp, vp, i64]),
        "ribbit_hip_host_alloc": (st, [sz, pvp]),
        "ribbit_hip_host_free": (st, [vp]),
        "ribbit_fasta_open": (st, [cp, ci, pvp]),
        "ribbit_fasta_next": (ci, [vp, P(cp), pvp, P(i64), P(ci)]),
        "ribbit_fasta_release": (st, [vp, vp]),
        "ribbit_fasta_close": (st, [vp]),
        "ribbit_fasta_last_error": (cp, []),
        "ribbit_hip_seeds_substitutions": (st, [vp, pvp, psz, pvp, psz]),
        "ribbit_hip_seeds_anchored": (st, [vp] + [pvp, psz] * 3),
        "ribbit_hip_guard_hits": (i64, [vp]),
        "ribbit_host_replay_calls": (st, [scan] + planes + [vp, sz, vp, sz, vp, sz, P(SeedLists)]),
        "ribbit_seed_lists_free": (None, [P(SeedLists)]),
        "ribbit_debug_last_merge": (None, [ci, P(i32 * 5)]),
        "ribbit_debug_last_device_merge": (None, [P(i32 * 5)]),
        "ribbit_debug_last_dispatch_ranges": (i32, []),
        "ribbit_host_debug_thread_faults": (i64, [i32, i32]),
        "ribbit_debug_alignment_counters": (None, [P(i64 * 3)]),
        "ribbit_debug_level_counters": (None, [P(i64 * 3)]),
        "ribbit_debug_small_motif_counters": (None, [P(i64 * 2)]),
        "ribbit_debug_set_merge_min_range": (None, [sz]),
        "ribbit_hip_device_pci_bus_id": (st, [ci, cp, sz]),
        "ribbit_hip_adopt_dispatch": (st, [vp, vp, sz]),
        "ribbit_hip_refine_met_empty_query": (ci, [vp]),
        "ribbit_hip_small_motifs": (st, [vp] * 6),
        "ribbit_hip_seed_best_rows": (st, [vp] * 4),
        "ribbit_host_longest_runs": (st, [scan] + planes[:5] + [vp, sz, vp]),
        "ribbit_hip_plane_bits": (st, [vp, i32, i64, i64, vp]),
        "ribbit_hip_range_popcount": (st, [vp, i32, i64, i64, pi32]),
        "ribbit_hip_plane_words": (i64, [vp]),
        "ribbit_hip_packed_plane": (st, [vp, ci, vp]),
        "ribbit_hip_last_timing_ms": (st, [vp, ci, P(C.c_double)]),
        "ribbit_hip_last_event_count": (i64, [vp]),
        "ribbit_refine_params_default": (None, [refine, i32, i32]),
        "ribbit_hip_refine_jobs": (st, [vp, refine, pvp, psz, pvp]),
        "ribbit_host_refine_jobs": (st, [scan, refine] + planes + [vp, sz, pvp, psz, pvp, psz]),
        "ribbit_refine_jobs_free": (None, [vp, vp]),
        "ribbit_hip_refine_bed": (st, [vp, refine, cp, pvp, psz]),
        "ribbit_host_refine_bed": (st, [scan, refine, cp] + planes + [vp, sz, cp, pvp, psz]),
        "ribbit_hip_xa_words": (st, [vp, i64, i64, vp]),
        "ribbit_hip_xa_words_strided": (st, [vp, i64, i64, vp, i64]),
        "ribbit_hip_perfect_runs_partial": (st, [vp, i64, i64, i64, pvp, psz, pvp, psz]),
        "ribbit_hip_scan_perfect_chunk": (st, [vp, i64, i64, i64, vp, sz, vp, sz, pvp, psz, pvp, psz]),
        "ribbit_hip_scan_perfect_begin": (st, [vp, i64, i64, i64]),
        "ribbit_hip_scan_perfect_end": (st, [vp, vp, sz, vp, sz, ci, pvp, psz, pvp, psz]),
        "ribbit_hip_scan_perfect_wait": (st, [vp]),
        "ribbit_hip_scan_perfect_end_device": (st, [vp, pvp, psz, pvp, psz]),
        "ribbit_hip_stage_calls_chunk": (st, [vp, ci, i64, i64, i64, i64, P(ChunkCalls)]),
        "ribbit_host_merge_chunks": (st, [scan] + planes + [P(ChunkPart), sz, P(SeedLists)]),
        "ribbit_host_perfect_runs_from_events": (st, [scan, sz, vp, vp, pvp, psz]),
        "ribbit_hip_host_register": (st, [vp, sz]),
        "ribbit_hip_host_unregister": (st, [vp]),
        "ribbit_hip_set_host_threads": (st, [vp, i32]),
        "ribbit_hip_set_timing": (st, [vp, i32]),
        "ribbit_hip_debug_set_scan_split": (st, [vp, i32, i32]),
        "ribbit_hip_debug_last_scan_split": (st, [vp, i32, pi32, pi32]),
        "ribbit_hip_debug_pair_events": (st, [vp, vp, sz, i64, vp, sz, psz, P(C.c_uint32)]),
        "ribbit_hip_debug_pair_events_sharded": (st, [vp, vp, vp, sz, i64, i64, i64, i64, P(DebugPairing)]),
        "ribbit_hip_debug_window_calls": (st, [vp, ci, P(DebugWindowStage), P(ChunkCalls), P(C.c_uint32)]),
        "ribbit_hip_debug_stream_read": (st, [vp, i64, P(i64)]),
        "ribbit_hip_debug_merge_ranges": (st, [vp, scan, i64, vp, sz, vp, sz, vp, sz, vp, sz, P(DebugMergeKnobs), P(DebugMergeRanges)]),
        "ribbit_debug_merge_ranges_free": (None, [P(DebugMergeRanges)]),
        "ribbit_hip_ssw_passes": (st, [vp, vp, sz, cp, sz, i32, vp]),
        "ribbit_hip_ssw_align_jobs": (st, [vp, vp, sz, cp, sz, i32, vp, vp, sz, vp, vp]),
        "ribbit_ssw_align": (st, [cp, i32, cp, i32, i32, P(Alignment), cp, sz]),
        "ribbit_debug_ssw_align_periodic": (st, [cp, i32, cp, i32, i32, i32, P(Alignment), cp, sz]),
        "ribbit_hip_repeat_sequences": (st, [vp, cp, vp, sz, i32, pvp, psz, psz]),
        "ribbit_host_repeat_sequences": (st, [cp, cp, i64, vp, sz, i32, pvp, psz]),
        "ribbit_bed_intervals": (st, [cp, sz, pvp, psz]),
        "ribbit_bed_motifs": (st, [cp, sz, pvp, pvp, psz]),
        "ribbit_bed_cigars": (st, [cp, sz, pvp, pvp, psz]),
        "ribbit_class_labels": (st, [vp, vp, sz, vp, sz, pvp]),
        "ribbit_debug_composition_prefix_builds": (i64, []),
        "ribbit_primer_params_default": (None, [P(PrimerParams)]),
        "ribbit_primer_pair_params_default": (None, [P(PrimerPairParams)]),
        "ribbit_product_params_default": (None, [P(ProductParams)]),
        "ribbit_host_oligo_duplex": (st, [cp, cp, pi32, pi32]),
        "ribbit_host_oligo_hairpin": (st, [cp, pi32]),
        # the text writers: malloc'ed text and its length come last (interruption_text: and the rows left out)
        "ribbit_bed_loci_text": (st, [cp, cp, sz, vp, sz, pvp, psz]),
        "ribbit_bed_class_text": (st, [cp, sz, vp, vp, vp, sz, pvp, psz]),
        "ribbit_class_summary_text": (st, [cp, vp, sz, vp, vp, vp, sz, pvp, psz]),
        "ribbit_compound_text": (st, [cp, cp, sz, i64, vp, sz, vp, sz, vp, sz, pvp, psz]),
        "ribbit_interruption_text": (st, [cp, cp, sz, vp, sz, vp, vp, sz, cp, cp, vp, pvp, psz, psz]),
        "ribbit_bed_purity_text": (st, [cp, sz, vp, vp, vp, sz, pvp, psz]),
        "ribbit_bed_nearest_text": (st, [cp, sz, vp, sz, vp, cp, vp, sz, pvp, psz]),
        "ribbit_nearest_other_text": (st, [cp, vp, cp, vp, sz, vp, vp, cp, vp, sz, pvp, psz]),
        "ribbit_base_windows_text": (st, [cp, i64, i32, vp, sz, pvp, psz]),
        "ribbit_bed_primer_products_text": (st, [cp, sz, vp, vp, sz, pvp, psz]),
        "ribbit_bed_primer_specific_text": (st, [cp, sz, vp, vp, vp, sz, pvp, psz]),
        "ribbit_primer_verdicts_merge": (st, [vp, vp, sz]),
        "ribbit_primer_shortlists_choose": (st, [vp, vp, sz, P(PrimerPairParams), pvp, pvp, pvp]),
        "ribbit_pair_amplicons_merge": (st, [vp, vp, sz]),
        "ribbit_bed_marker_text": (st, [cp, sz, vp, vp, cp, vp, sz, sz, pvp, psz]),
        "ribbit_panel_params_default": (None, [P(PanelParams)]),
        "ribbit_hip_panel_pools": (st, [vp, vp, vp, sz, P(PanelParams), pvp, pi32]),
        "ribbit_host_panel_pools": (st, [vp, vp, sz, P(PanelParams), pvp, pi32]),
        "ribbit_hip_debug_panel_conflicts": (st, [vp, vp, vp, sz, P(PanelParams), vp]),
        "ribbit_bed_panel_text": (st, [cp, sz, vp, sz, pvp, psz]),
        "ribbit_pair_amplicon_sizes": (st, [vp, sz, vp]),
        "ribbit_hip_marker_alleles": (st, [vp, vp, sz, sz, vp, vp, pvp]),
        "ribbit_host_marker_alleles": (st, [vp, sz, sz, vp, vp, pvp]),
        "ribbit_bed_alleles_text": (st, [cp, sz, vp, vp, sz, sz, pvp, psz]),
        "ribbit_allele_matrix_text": (st, [cp, sz, vp, sz, sz, vp, cp, vp, pvp, psz]),
    }
    for name in ("ribbit_hip_scan_perfect_runs", "ribbit_hip_perfect_calls", "ribbit_hip_seeds_perfect", "ribbit_hip_subst_calls",
                 "ribbit_hip_anchored_calls", "ribbit_hip_dispatch_seeds", "ribbit_hip_seed_longest_runs"):
        t[name] = (st, [vp, pvp, psz])                       # a list of the handle's and its length
    for name in ("ribbit_hip_debug_set_event_capacity", "ribbit_hip_debug_set_repeat_text_budget", "ribbit_hip_debug_set_small_record_capacity",
                 "ribbit_hip_debug_set_specific_batch"):
        t[name] = (st, [vp, sz])
    for name in ("ribbit_bed_overlap_text", "ribbit_bed_rows_text", "ribbit_bed_composition_text", "ribbit_bed_primers_text",
                 "ribbit_bed_primer_pairs_text"):
        t[name] = (st, [cp, sz, vp, sz, pvp, psz])           # BED text, an array with a record per row
    for name in ("ribbit_text_free", "ribbit_runs_free", "ribbit_intervals_free", "ribbit_loci_free", "ribbit_motif_classes_free",
                 "ribbit_compounds_free", "ribbit_row_purity_free", "ribbit_interruptions_free", "ribbit_nearest_free", "ribbit_composition_free",
                 "ribbit_primers_free", "ribbit_primer_pairs_free", "ribbit_products_free", "ribbit_primer_specific_free",
                 "ribbit_primer_genome_free", "ribbit_pair_amplicons_free", "ribbit_panel_free", "ribbit_alleles_free"):
        t[name] = (None, [vp])
    # the row outputs: the device form takes the handle, the host form the record's length, or its bases and their number
    length, bases = [i64], [cp, i64]
    for name, lead, rest in (("mask_record", bases, [vp, sz, i32, i32, pvp, psz]),
                             ("record_loci", length, [vp, sz, i32, pvp, psz]),
                             ("record_density", length, [vp, sz, i32, pvp, psz]),
                             ("record_overlap", length, [vp, sz, vp, sz, pvp, P(OverlapTotals)]),
                             ("record_nearest", length, [vp, sz, vp, sz, pvp]),
                             ("record_composition", bases, [vp, sz, i32, pvp]),
                             ("record_base_windows", bases, [i32, pvp, psz]),
                             ("record_primers", bases, [vp, sz, vp, sz, P(PrimerParams), pvp]),
                             ("record_primer_pairs", bases, [vp, sz, vp, sz, P(PrimerParams), P(PrimerPairParams), pvp]),
                             ("record_oligo_sites", bases, [vp, sz, P(ProductParams), pvp, pvp, psz]),
                             ("record_primer_products", bases, [vp, sz, P(ProductParams), pvp]),
                             ("record_specific_primer_pairs", bases, [vp, sz, vp, sz, P(PrimerParams), P(PrimerPairParams), P(ProductParams), pvp, pvp, pvp]),
                             ("record_primer_shortlists", bases, [vp, sz, vp, sz, P(PrimerParams), P(PrimerPairParams), pvp]),
                             ("record_shortlist_verdicts", bases, [vp, sz, i32, P(PrimerPairParams), P(ProductParams), pvp]),
                             ("record_pair_amplicons", bases, [vp, sz, cp, vp, i32, P(ProductParams), pvp]),
                             ("record_best", length, [vp, sz, pvp, psz, P(i64)]),
                             ("record_classes", length, [vp, sz, vp, vp, pvp, pvp, pvp, psz]),
                             ("record_compounds", length, [vp, vp, sz, i32, pvp, psz, pvp, psz]),
                             ("record_interruptions", bases, [vp, vp, sz, cp, vp, pvp, pvp, psz, pvp, pvp])):
        t[f"ribbit_hip_{name}"], t[f"ribbit_host_{name}"] = (st, [vp] + rest), (st, lead + rest)
    return t


_ABI = _signatures()
ABI_SYMBOLS = list(_ABI)


def library_path() -> str:
    # RIBBIT_HIP_LIBRARY: another build of the same library (the sanitizer build of the CPU tests)
    return os.environ.get("RIBBIT_HIP_LIBRARY") or os.path.join(_HERE, "libribbit_hip.so")


_lib = None
loaded_before_torch = False      # libribbit_hip.so entered the process before torch did: torch.cuda will not work in it


def _share_torchs_hip_runtime() -> bool:
    """One HIP runtime per process, whichever of torch and this library comes first (round 4; until then the multi-GPU bench
    leg depended on `import torch` coming first).  The torch wheel bundles its own runtime (torch/lib/libamdhip64.so, SONAME
    libamdhip64.so.7) and asks for it by FILE name; libribbit_hip.so needs "libamdhip64.so.7" and would otherwise pull in
    /opt/rocm's copy -- two runtimes, and the second one (torch's) finds the device taken.  If a torch is installed and not yet
    imported, its bundled runtime is loaded HERE first (by path, globally): the library's NEEDED entry is then satisfied by it
    (same SONAME), and a later `import torch` finds the very file it asks for already in the process.  Without torch installed
    nothing happens and the library runs on /opt/rocm's runtime, as the command-line front end does.  torch itself is not
    imported.  -> True if torch's runtime is now the process's (or already was)."""
    if "torch" in sys.modules:
        return True
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return False
    if spec is None or not spec.submodule_search_locations:
        return False
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return False
    try:
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        return False
    return True


def load_library():
    """Load libribbit_hip.so; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RibbitHipError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(make -C ribbit_amd/csrc). ribbit_amd has no CPU fallback.")
    global loaded_before_torch
    loaded_before_torch = "torch" not in sys.modules and not _share_torchs_hip_runtime()      # see ribbit_amd.distributed.device_bytes
    L = C.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


# what every wrapper below is made of ------------------------------------------------------------
def _ok(label: str, rc: int) -> None:
    """the status check: label is the symbol's name for a module-level function, ribbit_hip for a Scanner method"""
    if rc != 0:
        raise RibbitHipError(f"{label} error {rc}: {load_library().ribbit_hip_last_error().decode()}")


def _ptr(a):
    """the address of an array, or None when it is empty.  The address does not keep the array alive: `a` is a local name of
    the caller's, bound until the C call has returned."""
    return a.ctypes.data if len(a) else None


def _bytes(text) -> bytes:
    return text.encode() if isinstance(text, str) else bytes(text)


def _name(name) -> bytes:
    raw = _bytes(name)
    if b"\0" in raw:
        raise ValueError("a record name cannot hold a NUL byte")
    return raw


def _records(a, dt) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=dt).reshape(-1))


def _pairs(intervals) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(intervals, dtype=np.int32).reshape(-1, 2))


def _int32(value, what: str) -> int:
    value = int(value)
    if not -(1 << 31) <= value < (1 << 31):
        raise ValueError(f"{what} {value} is not an int32")
    return value


def _all_int32(a, message: str) -> None:
    if len(a) and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise ValueError(message)


def _copy(ptr, n, dt):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dt)
    buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dt).copy()


def _view(ptr, n, dt):
    """read-only numpy view of n records at ptr (no copy)"""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dt)
    v = np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(ptr), dtype=dt)
    v.flags.writeable = False
    return v


def _host(symbol: str, *lead) -> tuple:
    """a call of a module-level function: the entry point, its leading arguments, its name as the error label, and that the
    results are malloc'ed and the caller's to free.  Scanner._dev makes the device form's: the handle leads, the label is
    ribbit_hip, the results are the handle's."""
    return symbol, lead, symbol, True


def _host_bases(symbol: str, sequence) -> tuple:
    seq = bytes(sequence)
    return _host(symbol, seq, len(seq))


def _call(call, *args) -> bool:
    """make the call (a symbol's name, or what _host / Scanner._dev return) with args behind its leading arguments and check
    its status -> whether the results are the caller's to free"""
    symbol, lead, label, owned = _host(call) if isinstance(call, str) else call
    _ok(label, getattr(load_library(), symbol)(*lead, *args))
    return owned


def _free(owned: bool, free: str, *pointers) -> None:
    if owned:
        for p in pointers:
            getattr(load_library(), free)(p)


def _array(call, *args, dt, free: str, count=None, tail=()) -> np.ndarray:
    """a call whose result is one array of dt records: `count` of them, or as many as the call says behind the pointer; copied,
    and freed where it is the caller's"""
    out, n = C.c_void_p(), C.c_size_t()
    owned = _call(call, *args, C.byref(out), *(() if count is not None else (C.byref(n),)), *tail)
    try:
        return _copy(out.value, n.value if count is None else count, dt)
    finally:
        _free(owned, free, out)


def _text(call, *args, tail=()) -> bytes:
    """a call whose result is text and its length: copied, and freed where it is the caller's"""
    text, n = C.c_void_p(), C.c_size_t()
    owned = _call(call, *args, C.byref(text), C.byref(n), *tail)
    try:
        return C.string_at(text.value, n.value) if n.value else b""
    finally:
        _free(owned, "ribbit_text_free", text)


def _params(struct, default: str, c_name: str, fields: dict):
    p = struct()
    getattr(load_library(), default)(C.byref(p))
    names = {n for n, _ in struct._fields_}
    for name, value in fields.items():
        if name not in names:
            raise TypeError(f"{c_name} has no field {name!r}")
        if not -2**31 <= int(value) < 2**31:
            raise ValueError(f"{name} {value} does not fit int32")
        setattr(p, name, int(value))
    return p


def _params_arg(params, builder, struct, what: str = "params"):
    if params is None:
        params = builder()
    if not isinstance(params, struct):
        raise TypeError(f"{what}: a {struct.__name__} ({builder.__name__}())")
    return params


def _scan_params(min_motif: int, max_motif: int) -> ScanParams:
    params = ScanParams()
    load_library().ribbit_scan_params_default(C.byref(params), min_motif, max_motif)
    return params


def _refine_params(refine_params, min_motif: int, max_motif: int) -> RefineParams:
    if refine_params is None:
        refine_params = RefineParams()
        load_library().ribbit_refine_params_default(C.byref(refine_params), min_motif, max_motif)
    return refine_params


def _seed_lists(out: SeedLists) -> dict:
    """a filled RibbitSeedLists -> dict of copies; the lists are freed"""
    try:
        return {"perfect": _copy(out.perfect, out.n_perfect, SEED_DT), "subst": _copy(out.subst, out.n_subst, SEED_DT),
                "anchored": _copy(out.anchored, out.n_anchored, SEED_DT), "dispatch": _copy(out.dispatch, out.n_dispatch, SEED_DT),
                "guard_hits": int(out.guard_hits)}
    finally:
        load_library().ribbit_seed_lists_free(C.byref(out))


def _pool(texts, offsets):
    """a pool of texts and its offsets as given, or made of a list of strings (offsets None)"""
    if offsets is None:
        parts = [_bytes(t) for t in texts]
        offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts], dtype=np.int64)])
        texts = b"".join(parts)
    return _bytes(texts), np.asarray(offsets)


def pack_planes(sequence: bytes, max_motif: int):
    """numpy packing of a record into (hi, lo, brk) uint32 planes with the padding
    ribbit_host_replay_calls needs.  Host-side helper for replaying call lists that came from
    another rank; scans never use it (the GPU packs its own planes)."""
    n = len(sequence)
    raw = np.frombuffer(sequence, dtype=np.uint8)
    up = raw | 0x20
    valid = (up == ord("a")) | (up == ord("c")) | (up == ord("g")) | (up == ord("t"))
    code = np.where(valid, ((raw >> 1) & 3) ^ ((raw >> 2) & 1), 0).astype(np.uint8)
    nwords = n // 32 + 1 + (max_motif + 2) // 32 + 4
    def pack(bits):
        buf = np.zeros(nwords * 32, dtype=np.uint8)
        buf[:n] = bits
        return np.packbits(buf, bitorder="little").view("<u4").copy()
    brk_bits = np.ones(nwords * 32, dtype=np.uint8)
    brk_bits[:n] = ~valid
    brk = np.packbits(brk_bits, bitorder="little").view("<u4").copy()
    return pack(code >> 1), pack(code & 1), brk


def pack_bit_planes(planes_bits, length: int):
    """list of byte-per-base 0/1 arrays -> (uint32 words motif-major, stride): the xa argument of
    ribbit_host_replay_calls."""
    stride = (length // 32 + 1 + 7) // 8 * 8 + 16
    out = np.zeros((len(planes_bits), stride), dtype="<u4")
    for i, bits in enumerate(planes_bits):
        buf = np.zeros(stride * 32, dtype=np.uint8)
        buf[:length] = bits
        out[i] = np.packbits(buf, bitorder="little").view("<u4")
    return np.ascontiguousarray(out), stride


def host_replay_calls(min_motif: int, max_motif: int, sequence: bytes, perfect_calls, subst_calls=None,
                      anchored_calls=None, xa=None, xa_stride: int = 0):
    """ribbit_host_replay_calls: call lists -> dict(perfect, subst, anchored, dispatch, guard_hits). No GPU needed."""
    params = _scan_params(min_motif, max_motif)
    hi, lo, brk = pack_planes(sequence, max_motif)
    empty = np.zeros(0, CALL_DT)
    pc = np.ascontiguousarray(perfect_calls, dtype=CALL_DT)
    sc = np.ascontiguousarray(subst_calls if subst_calls is not None else empty, dtype=CALL_DT)
    ac = np.ascontiguousarray(anchored_calls if anchored_calls is not None else empty, dtype=CALL_DT)
    out = SeedLists()
    _call("ribbit_host_replay_calls", C.byref(params), len(sequence), hi.ctypes.data, lo.ctypes.data, brk.ctypes.data, len(hi),
          xa.ctypes.data if xa is not None else None, xa_stride, pc.ctypes.data, len(pc), sc.ctypes.data, len(sc),
          ac.ctypes.data if anchored_calls is not None else None, len(ac), C.byref(out))
    return _seed_lists(out)


def host_merge_chunks(min_motif: int, max_motif: int, length: int, hi, lo, brk, xa, xa_stride: int, parts):
    """ribbit_host_merge_chunks: the merging rank's half of the chunk-sharded path.  parts (chunk order) = dicts with
    RUN_DT arrays `runs`, `halves` and, per window stage s in ("subst", "anchored"), `<s>_calls` (CALL_DT), `<s>_pend`
    (int32 per call, or None), `<s>_tail_pend` (int), `<s>_flush` (CALL_DT).  -> dict of the record's seed lists."""
    params = _scan_params(min_motif, max_motif)
    hi, lo, brk = (np.ascontiguousarray(a, dtype="<u4") for a in (hi, lo, brk))
    keep = []                                        # arrays the C structs point into

    def arr(a, dt):
        a = np.ascontiguousarray(a if a is not None else np.zeros(0, dt), dtype=dt)
        keep.append(a)
        return a

    cparts = (ChunkPart * max(len(parts), 1))()
    for k, p in enumerate(parts):
        runs, halves = arr(p["runs"], RUN_DT), arr(p["halves"], RUN_DT)
        cparts[k].runs, cparts[k].n_runs = runs.ctypes.data, len(runs)
        cparts[k].halves, cparts[k].n_halves = halves.ctypes.data, len(halves)
        for stage in ("subst", "anchored"):
            cc = getattr(cparts[k], stage)
            calls, flush = arr(p[f"{stage}_calls"], CALL_DT), arr(p[f"{stage}_flush"], CALL_DT)
            cc.calls, cc.n = calls.ctypes.data, len(calls)
            cc.flush, cc.n_flush = flush.ctypes.data, len(flush)
            pend = p.get(f"{stage}_pend")
            if pend is not None and len(calls):
                pend = arr(pend, "<i4")
                assert len(pend) == len(calls)
                cc.pend = pend.ctypes.data
            cc.tail_pend = int(p[f"{stage}_tail_pend"])
            cc.inexact = int(p.get(f"{stage}_inexact", 0))
    out = SeedLists()
    _call("ribbit_host_merge_chunks", C.byref(params), length, hi.ctypes.data, lo.ctypes.data, brk.ctypes.data, len(hi),
          xa.ctypes.data if xa is not None else None, xa_stride, cparts, len(parts), C.byref(out))
    return _seed_lists(out)


def _alignment(symbol: str, cap: int, *args):
    """-> (dict of alignment fields, cigar string) of a call that ends in an alignment, a text buffer and its capacity"""
    out, buf = Alignment(), C.create_string_buffer(cap)
    _call(symbol, *args, C.byref(out), buf, cap)
    return {n: getattr(out, n) for n, _ in Alignment._fields_}, buf.value.decode()


def ssw_align(query: bytes, ref: bytes, ref_len: int | None = None, mask_len: int = 15):
    """ribbit_ssw_align -> (dict of alignment fields, cigar string)"""
    return _alignment("ribbit_ssw_align", 16 * (len(query) + len(ref)) + 64,
                      query, len(query), ref, len(ref) if ref_len is None else ref_len, mask_len)


def ssw_align_periodic(query: bytes, motif: bytes, ref_len: int, mask_len: int = 15):
    """ribbit_debug_ssw_align_periodic (test hook): the alignment against `motif` repeated past ref_len, finished the way
    refinement finishes an alignment whose path is known -> (dict of alignment fields, cigar string)"""
    return _alignment("ribbit_debug_ssw_align_periodic", 16 * (len(query) + ref_len + len(motif)) + 64,
                      query, len(query), motif, len(motif), ref_len, mask_len)


def _jobs_with_motifs(jobs, pool: bytes):
    """-> list of (job record, motif string)"""
    return [(j, pool[int(j["motif_offset"]):int(j["motif_offset"]) + int(j["atomicity"])].decode()) for j in jobs]


def _counters(symbol: str, ctype, n: int) -> tuple:
    out = (ctype * n)()
    getattr(load_library(), symbol)(C.byref(out))
    return tuple(int(v) for v in out)


def alignment_counters():
    """(alignments refinement made, of them with GPU passes, with GPU paths), cumulative"""
    return _counters("ribbit_debug_alignment_counters", C.c_int64, 3)


def level_counters():
    """(levels run, nodes put off, alignments of those nodes) of the level-by-level GPU refinement of long-motif seeds'
    recursion trees, cumulative"""
    return _counters("ribbit_debug_level_counters", C.c_int64, 3)


def last_device_merge():
    """(ranges the GPU merged, ranges it was given but left to the host threads, ranges the host threads merged while its kernel
    ran, ranges of the stage, ranges merged again by the validation walk) of the calling thread's last anchored-stage merge; the
    first three are zero when the merge ran on the host threads alone"""
    return _counters("ribbit_debug_last_device_merge", C.c_int32, 5)


MERGE_ON_LANES, MERGE_ON_HOST = 0, 1      # RIBBIT_MERGE_ON_LANES / RIBBIT_MERGE_ON_HOST
MERGE_CAPS = ("ps_cap", "cand_cap", "ps_spill", "cand_spill", "child_cap", "cov_cap", "resident_waves", "max_passes",
              "scratch_full", "log_full", "bad_plane", "runaway", "too_slow")


def debug_merge_ranges(scanner, min_motif: int, max_motif: int, length: int, perfect, subst, calls, xa, xa_stride: int, *, where: int,
                       full: bool = False, calls_per_range: int = 1, resident_waves: int = 0, max_passes: int = 0, head_cap: int = 0,
                       log_cap: int = 0, device_limit: int = -1, only_range: int = -1) -> dict:
    """ribbit_hip_debug_merge_ranges (test hook): the first parallel pass of the anchored stage's merge on lists, planes (the
    words and stride of pack_bit_planes) and calls made by the caller, on the lanes of `scanner` (MERGE_ON_LANES) or on the host
    workers (MERGE_ON_HOST; scanner may be None).  -> dict: ran, caps (by the names of MERGE_CAPS), cuts, first, cursors0, and
    raw (full False): ranges = one dict per range (status, own, guard_hits, cursor, head_reads, undo, reads, heads: the logs as
    sorted lists of tuples without the range); full: lists (as host_replay_calls returns them) and device_merge."""
    params = _scan_params(min_motif, max_motif)
    p, s = _records(perfect, SEED_DT), _records(subst, SEED_DT)
    c, words = _records(calls, CALL_DT), np.ascontiguousarray(xa, dtype="<u4")
    knobs = DebugMergeKnobs(int(where), int(bool(full)), int(calls_per_range), int(resident_waves), int(max_passes), int(head_cap),
                            int(log_cap), int(device_limit), int(only_range))
    out = DebugMergeRanges()
    if words.size < (max_motif - min_motif + 1) * xa_stride:
        raise ValueError("xa holds fewer words than a plane per motif size")
    _ok("ribbit_hip_debug_merge_ranges", load_library().ribbit_hip_debug_merge_ranges(
        scanner._h if scanner is not None else None, C.byref(params), int(length), _ptr(p), len(p), _ptr(s), len(s), _ptr(c), len(c),
        words.ctypes.data, int(xa_stride), C.byref(knobs), C.byref(out)))
    try:
        nr = int(out.n_ranges)
        res = {"ran": bool(out.ran), "caps": dict(zip(MERGE_CAPS, (int(v) for v in out.caps))),
               "cuts": _copy(out.cuts, nr, _I4), "first": _copy(out.first, nr + 1, _I4), "cursors0": _copy(out.cursors0, 2 * nr, _I4).reshape(-1, 2)}
        if full:
            lists = out.lists
            res["lists"] = {"perfect": _copy(lists.perfect, lists.n_perfect, SEED_DT), "subst": _copy(lists.subst, lists.n_subst, SEED_DT),
                            "anchored": _copy(lists.anchored, lists.n_anchored, SEED_DT), "guard_hits": int(lists.guard_hits)}
            res["device_merge"] = tuple(int(v) for v in out.device_merge)
            return res
        res["ranges"] = []
        if not out.ran or not out.own:
            return res
        rng = _copy(out.range, 12 * nr, _I4).reshape(-1, 12)
        own = _copy(out.own, out.n_own, SEED_DT)
        logs = {}
        for name, ptr, n, width in (("undo", out.undo, out.n_undo, 4), ("reads", out.reads, out.n_reads, 4), ("heads", out.heads, out.n_heads, 8)):
            rows = _copy(ptr, width * n, _I4).reshape(-1, width)
            logs[name] = [sorted(tuple(int(v) for v in r[1:]) for r in rows[rows[:, 0] == k]) for k in range(nr)]
        u64 = lambda lo, hi: (int(lo) & 0xFFFFFFFF) | ((int(hi) & 0xFFFFFFFF) << 32)
        for k in range(nr):
            r = rng[k]
            guards = u64(r[3], r[4])
            res["ranges"].append({"status": int(r[0]) & 0xFFFFFFFF, "own": own[int(r[1]):int(r[1]) + int(r[2])],
                                  "guard_hits": guards - (1 << 64) if guards >> 63 else guards, "cursor": (int(r[5]), int(r[6])),
                                  "head_reads": (u64(r[7], r[8]), u64(r[9], r[10])),
                                  "undo": logs["undo"][k], "reads": logs["reads"][k], "heads": logs["heads"][k]})
        return res
    finally:
        load_library().ribbit_debug_merge_ranges_free(C.byref(out))


def small_motif_counters():
    """(seeds refinement took from the GPU's possibleMotifs table, seeds it computed on the host), cumulative"""
    return _counters("ribbit_debug_small_motif_counters", C.c_int64, 2)


def host_longest_runs(min_motif: int, max_motif: int, sequence: bytes, seeds):
    """ribbit_host_longest_runs: longestContinuousMatches of seeds on the composed planes, recomputed on the host. No GPU."""
    params = _scan_params(min_motif, max_motif)
    hi, lo, brk = pack_planes(sequence, max_motif)
    s = np.ascontiguousarray(seeds, dtype=SEED_DT)
    out = np.zeros(len(s), dtype="<i4")
    _call("ribbit_host_longest_runs", C.byref(params), len(sequence), hi.ctypes.data, lo.ctypes.data, brk.ctypes.data, len(hi),
          s.ctypes.data, len(s), out.ctypes.data)
    return out


def host_refine_jobs(min_motif: int, max_motif: int, sequence: bytes, xa, xa_stride: int, dispatch, refine_params=None):
    """ribbit_host_refine_jobs: dispatch seeds + planes -> (jobs array, motif pool bytes). No GPU needed."""
    params, rp = _scan_params(min_motif, max_motif), _refine_params(refine_params, min_motif, max_motif)
    hi, lo, brk = pack_planes(sequence, max_motif)
    d = np.ascontiguousarray(dispatch, dtype=SEED_DT)
    jobs, nj, pool, npool = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
    _call("ribbit_host_refine_jobs", C.byref(params), C.byref(rp), len(sequence), hi.ctypes.data, lo.ctypes.data, brk.ctypes.data,
          len(hi), xa.ctypes.data if xa is not None else None, xa_stride, d.ctypes.data, len(d),
          C.byref(jobs), C.byref(nj), C.byref(pool), C.byref(npool))
    try:
        return _copy(jobs.value, nj.value, JOB_DT), C.string_at(pool.value, npool.value)
    finally:
        load_library().ribbit_refine_jobs_free(jobs, pool)


def host_refine_bed(min_motif: int, max_motif: int, sequence: bytes, xa, xa_stride: int, dispatch, sequence_id: str = "seq",
                    refine_params=None) -> str:
    """ribbit_host_refine_bed: dispatch seeds + planes -> BED text.  No GPU needed."""
    params, rp = _scan_params(min_motif, max_motif), _refine_params(refine_params, min_motif, max_motif)
    hi, lo, brk = pack_planes(sequence, max_motif)
    d = np.ascontiguousarray(dispatch, dtype=SEED_DT)
    return _text("ribbit_host_refine_bed", C.byref(params), C.byref(rp), sequence, len(sequence), hi.ctypes.data, lo.ctypes.data,
                 brk.ctypes.data, len(hi), xa.ctypes.data if xa is not None else None, xa_stride, d.ctypes.data, len(d),
                 sequence_id.encode()).decode()


# the row outputs: each marshalled once, for its host twin and its Scanner method ------------------------------
def _mask_record(call, intervals, mode: str, line_width: int) -> bytes:
    if mode not in MASK_MODES:
        raise ValueError(f"mask mode must be one of {sorted(MASK_MODES)}, got {mode!r}")
    iv = _pairs(intervals)
    return _text(call, _ptr(iv), len(iv), MASK_MODES[mode], int(line_width))


def host_mask_record(sequence: bytes, intervals, mode: str = "soft", line_width: int = 60) -> bytes:
    """ribbit_host_mask_record: the masked, line-wrapped FASTA body of `sequence` (no header) under the union of the
    half-open (start, end) rows of `intervals`.  No GPU needed."""
    return _mask_record(_host_bases("ribbit_host_mask_record", sequence), intervals, mode, line_width)


def _repeat_args(name, intervals, flank: int):
    raw = _name(name)
    flank = int(flank)
    if flank > 0x7FFFFFFF:
        raise ValueError(f"flank {flank} is larger than INT32_MAX")
    return raw, _pairs(intervals), max(flank, -(1 << 31))


def host_repeat_sequences(name, sequence: bytes, intervals, flank: int = 100) -> bytes:
    """ribbit_host_repeat_sequences: one FASTA entry per (start, end) row, in order: ">name:s-e flank=left,right" and the
    row's bases with `flank` bases on either side, clipped to the record (include/ribbit_hip.h).  No GPU needed."""
    raw, iv, f = _repeat_args(name, intervals, flank)
    seq = bytes(sequence)
    return _text("ribbit_host_repeat_sequences", raw, seq, len(seq), _ptr(iv), len(iv), f)


def _rows_arg(intervals, value: int, what: str):
    value = _int32(value, what)
    return _pairs(intervals), value


def _record_loci(call, intervals, gap: int) -> np.ndarray:
    iv, gap = _rows_arg(intervals, gap, "gap")
    return _array(call, _ptr(iv), len(iv), gap, dt=LOCUS_DT, free="ribbit_loci_free")


def host_record_loci(length: int, intervals, gap: int = 0) -> np.ndarray:
    """ribbit_host_record_loci: the rows of a record of `length` bases merged into loci (runs of covered positions, joined
    while they lie at most `gap` apart), by ascending start: a LOCUS_DT array (include/ribbit_hip.h).  No GPU needed."""
    return _record_loci(_host("ribbit_host_record_loci", int(length)), intervals, gap)


def _record_density(call, intervals, window: int) -> np.ndarray:
    iv, window = _rows_arg(intervals, window, "window")
    return _array(call, _ptr(iv), len(iv), window, dt=_I4, free="ribbit_intervals_free")


def host_record_density(length: int, intervals, window: int) -> np.ndarray:
    """ribbit_host_record_density: covered bases per window of `window` bases (the last one may be short), int32.  No GPU needed."""
    return _record_density(_host("ribbit_host_record_density", int(length)), intervals, window)


def _record_overlap(call, rows, other):
    iv, ot, totals = _pairs(rows), _pairs(other), OverlapTotals()
    per_row = _array(call, _ptr(iv), len(iv), _ptr(ot), len(ot), dt=_I4, free="ribbit_intervals_free", count=2 * len(iv), tail=(C.byref(totals),))
    return per_row.reshape(-1, 2), totals.as_dict()


def host_record_overlap(length: int, rows, other):
    """ribbit_host_record_overlap: the rows of a record of `length` bases against the intervals `other` -> ((n, 2) int32 array:
    per row the number of OTHER intervals it overlaps and the number of its bases that OTHER covers; the totals as a dict with
    the keys OVERLAP_TOTALS).  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_overlap(_host("ribbit_host_record_overlap", int(length)), rows, other)


def _record_nearest(call, queries, targets) -> np.ndarray:
    q, t = _pairs(queries), _pairs(targets)
    return _array(call, _ptr(q), len(q), _ptr(t), len(t), dt=NEAREST_DT, free="ribbit_nearest_free", count=len(q))


def host_record_nearest(length: int, queries, targets) -> np.ndarray:
    """ribbit_host_record_nearest: for every query interval on a record of `length` bases, the target it lies in or overlaps and its
    neighbours to either side -> a NEAREST_DT array, one record per query.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_nearest(_host("ribbit_host_record_nearest", int(length)), queries, targets)


def _record_composition(call, intervals, flank: int) -> np.ndarray:
    iv, flank = _rows_arg(intervals, flank, "flank")
    return _array(call, _ptr(iv), len(iv), flank, dt=COMPOSITION_DT, free="ribbit_composition_free", count=len(iv))


def host_record_composition(sequence: bytes, intervals, flank: int = 100) -> np.ndarray:
    """ribbit_host_record_composition: the A, C, G, T and other bases of every (start, end) row of `sequence`, and of the `flank` bases on
    either side of it the length, the C + G, the other bases and the positions that rows cover -> a COMPOSITION_DT array, one record
    per row.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_composition(_host_bases("ribbit_host_record_composition", sequence), intervals, flank)


def _record_base_windows(call, window: int) -> np.ndarray:
    return _array(call, _int32(window, "window"), dt=BASE_COUNTS_DT, free="ribbit_composition_free")


def host_record_base_windows(sequence: bytes, window: int) -> np.ndarray:
    """ribbit_host_record_base_windows: the A, C, G, T and other bases of every window of `window` bases of `sequence` (the last one may
    be short) -> a BASE_COUNTS_DT array.  No GPU needed."""
    return _record_base_windows(_host_bases("ribbit_host_record_base_windows", sequence), window)


def primer_params(**fields) -> PrimerParams:
    """ribbit_primer_params_default with the given fields replaced, e.g. primer_params(flank=100, gc_clamp=0); the ranges are
    checked by the calls that take it (include/ribbit_hip.h)"""
    return _params(PrimerParams, "ribbit_primer_params_default", "RibbitPrimerParams", fields)


def primer_pair_params(**fields) -> PrimerPairParams:
    """ribbit_primer_pair_params_default with the given fields replaced, e.g. primer_pair_params(shortlist=4, max_hairpin=2); the
    ranges are checked by the calls that take it (include/ribbit_hip.h)"""
    return _params(PrimerPairParams, "ribbit_primer_pair_params_default", "RibbitPrimerPairParams", fields)


def product_params(**fields) -> ProductParams:
    """ribbit_product_params_default with the given fields replaced, e.g. product_params(seed=12, max_sites=256); the ranges are
    checked by the calls that take it (include/ribbit_hip.h)"""
    return _params(ProductParams, "ribbit_product_params_default", "RibbitProductParams", fields)


def _record_primers(call, intervals, targets, params) -> np.ndarray:
    iv, tg = _pairs(intervals), _pairs(targets)
    params = _params_arg(params, primer_params, PrimerParams)
    return _array(call, _ptr(iv), len(iv), _ptr(tg), len(tg), C.byref(params), dt=PRIMERS_DT, free="ribbit_primers_free", count=len(tg))


def host_record_primers(sequence: bytes, intervals, targets, params: PrimerParams | None = None) -> np.ndarray:
    """ribbit_host_record_primers: for every (start, end) target a forward primer in the flank to its left and a reverse primer in
    the flank to its right, clear of every base that the rows `intervals` cover or that is not A, C, G or T -> a PRIMERS_DT array,
    one record per target.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_primers(_host_bases("ribbit_host_record_primers", sequence), intervals, targets, params)


def _record_primer_pairs(call, intervals, targets, params, pair_params) -> np.ndarray:
    iv, tg = _pairs(intervals), _pairs(targets)
    params = _params_arg(params, primer_params, PrimerParams)
    pair_params = _params_arg(pair_params, primer_pair_params, PrimerPairParams, "pair_params")
    return _array(call, _ptr(iv), len(iv), _ptr(tg), len(tg), C.byref(params), C.byref(pair_params), dt=PRIMER_PAIRS_DT, free="ribbit_primer_pairs_free",
                  count=len(tg))


def host_record_primer_pairs(sequence: bytes, intervals, targets, params: PrimerParams | None = None, pair_params: PrimerPairParams | None = None) -> np.ndarray:
    """ribbit_host_record_primer_pairs: for every (start, end) target the forward and the reverse primer of host_record_primers'
    candidates chosen as one pair: each oligo within the limits on self-dimers and hairpins, the two within the limits on
    cross-dimers and on their Tm difference, the pair with the least penalty -> a PRIMER_PAIRS_DT array, one record per target.
    The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_primer_pairs(_host_bases("ribbit_host_record_primer_pairs", sequence), intervals, targets, params, pair_params)


def _oligos(oligos) -> np.ndarray:
    """oligos as text, 5' to 3', letters of ACGT in either case -> RibbitOligo records (a text of no or of more than 32 letters keeps
    its length, for the call to refuse)"""
    out = np.zeros(len(oligos), dtype=_OLIGO_DT)
    for i, text in enumerate(oligos):
        letters = _bytes(text).upper()
        if any(ch not in b"ACGT" for ch in letters):
            raise ValueError(f"oligo {i}: {letters!r} has letters other than ACGT")
        bases = sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(letters[:32]))
        out[i] = (len(letters), np.uint32(bases & 0xffffffff).astype(np.int32), np.uint32(bases >> 32).astype(np.int32))
    return out


def _record_oligo_sites(call, oligos, params):
    """-> an OLIGO_SITES_DT array and the flat positions"""
    og, params = _oligos(oligos), _params_arg(params, product_params, ProductParams)
    sites, positions, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    owned = _call(call, _ptr(og), len(og), C.byref(params), C.byref(sites), C.byref(positions), C.byref(n))
    try:
        return _copy(sites.value, len(og), OLIGO_SITES_DT), _copy(positions.value, n.value, _I4)
    finally:
        _free(owned, "ribbit_products_free", sites, positions)


def host_record_oligo_sites(sequence: bytes, oligos, params: ProductParams | None = None):
    """ribbit_host_record_oligo_sites: where every oligo (text, 5' to 3') primes on either strand of the record: its last `seed`
    bases match exactly, at most max_mismatches of the others differ -> (an OLIGO_SITES_DT array, one record per oligo, and the
    int32 window starts of the kept lists one behind the other: list = positions[forward_at : forward_at + forward]; a list longer
    than max_sites has forward_at -1).  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_oligo_sites(_host_bases("ribbit_host_record_oligo_sites", sequence), oligos, params)


def _record_primer_products(call, pairs, params) -> np.ndarray:
    rw, params = _records(pairs, PRIMER_PAIRS_DT), _params_arg(params, product_params, ProductParams)
    return _array(call, _ptr(rw), len(rw), C.byref(params), dt=PRIMER_PRODUCTS_DT, free="ribbit_products_free", count=len(rw))


def host_record_primer_products(sequence: bytes, pairs, params: ProductParams | None = None) -> np.ndarray:
    """ribbit_host_record_primer_products: an in-silico PCR of every pair of `pairs` (a PRIMER_PAIRS_DT array: record_primer_pairs'
    rows, or hand-made ones) on the record: the sites of both primers on both strands, the products between a forward and a reverse
    site of either, whether the pair's own product is among them and the shortest of the others -> a PRIMER_PRODUCTS_DT array.  A
    pair is specific in this record when products - own == 0.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_primer_products(_host_bases("ribbit_host_record_primer_products", sequence), pairs, params)


def _record_specific_primer_pairs(call, intervals, targets, params, pair_params, product_params):
    """-> a PRIMER_PAIRS_DT, a PRIMER_PRODUCTS_DT and a PRIMER_SPECIFIC_DT array, one record per target each"""
    iv, tg = _pairs(intervals), _pairs(targets)
    params = _params_arg(params, primer_params, PrimerParams)
    pair_params = _params_arg(pair_params, primer_pair_params, PrimerPairParams, "pair_params")
    product_params = _params_arg(product_params, globals()["product_params"], ProductParams, "product_params")
    pairs, products, specific = C.c_void_p(), C.c_void_p(), C.c_void_p()
    owned = _call(call, _ptr(iv), len(iv), _ptr(tg), len(tg), C.byref(params), C.byref(pair_params), C.byref(product_params), C.byref(pairs), C.byref(products),
                  C.byref(specific))
    try:
        return _copy(pairs.value, len(tg), PRIMER_PAIRS_DT), _copy(products.value, len(tg), PRIMER_PRODUCTS_DT), _copy(specific.value, len(tg), PRIMER_SPECIFIC_DT)
    finally:
        _free(owned, "ribbit_primer_specific_free", pairs, products, specific)


def host_record_specific_primer_pairs(sequence: bytes, intervals, targets, params: PrimerParams | None = None, pair_params: PrimerPairParams | None = None,
                                      product_params: ProductParams | None = None):
    """ribbit_host_record_specific_primer_pairs: for every (start, end) target the best admissible pair of host_record_primer_pairs'
    two shortlists that amplifies nothing else in the record: the admissible pairs in the order of that choice, each judged by
    host_record_primer_products' in-silico PCR, the first one with products - own == 0 taken; no fallback -> (a PRIMER_PAIRS_DT array
    of the chosen pairs, a PRIMER_PRODUCTS_DT array of their products, a PRIMER_SPECIFIC_DT array: the chosen pair's place in that
    order, the admissible pairs by outcome and what the pair in place 0 amplifies besides its own product).  The contract is in
    include/ribbit_hip.h.  No GPU needed."""
    return _record_specific_primer_pairs(_host_bases("ribbit_host_record_specific_primer_pairs", sequence), intervals, targets, params, pair_params, product_params)


def _record_primer_shortlists(call, intervals, targets, params, pair_params) -> np.ndarray:
    iv, tg = _pairs(intervals), _pairs(targets)
    params = _params_arg(params, primer_params, PrimerParams)
    pair_params = _params_arg(pair_params, primer_pair_params, PrimerPairParams, "pair_params")
    return _array(call, _ptr(iv), len(iv), _ptr(tg), len(tg), C.byref(params), C.byref(pair_params), dt=PRIMER_SHORTLISTS_DT, free="ribbit_primer_genome_free",
                  count=len(tg))


def host_record_primer_shortlists(sequence: bytes, intervals, targets, params: PrimerParams | None = None, pair_params: PrimerPairParams | None = None) -> np.ndarray:
    """ribbit_host_record_primer_shortlists: for every (start, end) target the two shortlists that host_record_specific_primer_pairs
    makes internally, in a form that leaves the record: up to 8 primers a side by rank (an empty place has start -1) and the side
    counts -> a PRIMER_SHORTLISTS_DT array, one record per target.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_primer_shortlists(_host_bases("ribbit_host_record_primer_shortlists", sequence), intervals, targets, params, pair_params)


def _record_shortlist_verdicts(call, lists, home, pair_params, product_params) -> np.ndarray:
    ls = _records(lists, PRIMER_SHORTLISTS_DT)
    pair_params = _params_arg(pair_params, primer_pair_params, PrimerPairParams, "pair_params")
    product_params = _params_arg(product_params, globals()["product_params"], ProductParams, "product_params")
    return _array(call, _ptr(ls), len(ls), _int32(home, "home"), C.byref(pair_params), C.byref(product_params), dt=PRIMER_VERDICTS_DT,
                  free="ribbit_primer_genome_free", count=len(ls))


def host_record_shortlist_verdicts(sequence: bytes, lists, home, pair_params: PrimerPairParams | None = None, product_params: ProductParams | None = None) -> np.ndarray:
    """ribbit_host_record_shortlist_verdicts: every admissible pair of every target's shortlists (a PRIMER_SHORTLISTS_DT array) judged
    by the in-silico PCR on `sequence`, which may be any record; home (0 or 1): whether it is the record the lists were made on, where
    alone a pair's own product exists -> a PRIMER_VERDICTS_DT array: the admissible, over, other and own pairs as masks (bit 8 l + r),
    the sites of the 16 places, what the pair in place 0 amplifies besides its own product.  Sum them over the records of a genome with
    primer_verdicts_merge and choose with primer_shortlists_choose.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_shortlist_verdicts(_host_bases("ribbit_host_record_shortlist_verdicts", sequence), lists, home, pair_params, product_params)


def primer_verdicts_merge(into, other) -> np.ndarray:
    """ribbit_primer_verdicts_merge: the verdicts of two sets of records together -> a new PRIMER_VERDICTS_DT array (neither argument
    is changed): the masks OR-ed, the counts added; `admissible` must be equal target by target"""
    a, b = _records(into, PRIMER_VERDICTS_DT).copy(), _records(other, PRIMER_VERDICTS_DT)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} and {len(b)} verdicts")
    _call("ribbit_primer_verdicts_merge", _ptr(a), _ptr(b), len(a))
    return a


def primer_shortlists_choose(lists, verdicts, pair_params: PrimerPairParams | None = None):
    """ribbit_primer_shortlists_choose: per target the first admissible pair of its lists, in the order of the choice, that is neither
    over nor other in the summed verdicts -> (a PRIMER_PAIRS_DT, a PRIMER_PRODUCTS_DT and a PRIMER_SPECIFIC_DT array) as
    host_record_specific_primer_pairs gives them, every count and verdict over all judged records; bed_primer_specific_text prints them"""
    ls, vd = _records(lists, PRIMER_SHORTLISTS_DT), _records(verdicts, PRIMER_VERDICTS_DT)
    if len(ls) != len(vd):
        raise ValueError(f"{len(ls)} lists and {len(vd)} verdicts")
    pair_params = _params_arg(pair_params, primer_pair_params, PrimerPairParams, "pair_params")
    pairs, products, specific = C.c_void_p(), C.c_void_p(), C.c_void_p()
    owned = _call("ribbit_primer_shortlists_choose", _ptr(ls), _ptr(vd), len(ls), C.byref(pair_params), C.byref(pairs), C.byref(products), C.byref(specific))
    try:
        return _copy(pairs.value, len(ls), PRIMER_PAIRS_DT), _copy(products.value, len(ls), PRIMER_PRODUCTS_DT), _copy(specific.value, len(ls), PRIMER_SPECIFIC_DT)
    finally:
        _free(owned, "ribbit_primer_genome_free", pairs, products, specific)


def _record_pair_amplicons(call, pairs, motifs, record, params) -> np.ndarray:
    rw, params = _records(pairs, PRIMER_PAIRS_DT), _params_arg(params, product_params, ProductParams)
    offsets = None
    if isinstance(motifs, tuple):
        motifs, offsets = motifs
    pool, off = _pool(motifs, offsets)
    if off.ndim != 1 or len(off) != len(rw) + 1:
        raise ValueError(f"{len(rw)} pairs want {len(rw) + 1} offsets")
    _all_int32(off, "an offset is not an int32")
    off = np.ascontiguousarray(off, dtype=np.int32)
    return _array(call, _ptr(rw), len(rw), pool, off.ctypes.data, _int32(record, "record"), C.byref(params), dt=PAIR_AMPLICONS_DT,
                  free="ribbit_pair_amplicons_free", count=len(rw))


def host_record_pair_amplicons(sequence: bytes, pairs, motifs, record: int = 0, params: ProductParams | None = None) -> np.ndarray:
    """ribbit_host_record_pair_amplicons: every pair of `pairs` (a PRIMER_PAIRS_DT array) typed on the record, which may be any
    record: the sites of both primers, the products, where the first product lies and the longest tract of the pair's motif inside
    it -> a PAIR_AMPLICONS_DT array with `record` as the label of every pair that has a product.  motifs: a list of strings, one per
    pair, or (pool, offsets) as bed_motifs returns them.  Sum over the records of an assembly with pair_amplicons_merge.  The
    contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_pair_amplicons(_host_bases("ribbit_host_record_pair_amplicons", sequence), pairs, motifs, record, params)


def pair_amplicons_merge(into, other) -> np.ndarray:
    """ribbit_pair_amplicons_merge: the amplicons of two sets of records together -> a new PAIR_AMPLICONS_DT array (neither argument
    is changed): the counts added, products -1 if either is, the product of `into` kept where it has one"""
    a, b = _records(into, PAIR_AMPLICONS_DT).copy(), _records(other, PAIR_AMPLICONS_DT)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} and {len(b)} amplicons")
    _call("ribbit_pair_amplicons_merge", _ptr(a), _ptr(b), len(a))
    return a


def bed_marker_text(bed, pairs, amplicons, names) -> bytes:
    """ribbit_bed_marker_text: the lines of `bed` (the targets' BED rows, target i on line i), each with 20 more columns: the eight
    primer columns and the designed product of row i of `pairs`, the products of row i of `amplicons` (record_pair_amplicons, summed
    over the other assembly's records) and, where that is exactly one, the record's name out of `names` (a list, by the amplicon's
    `record`), where the product lies, its orientation, its size, the size's difference from the designed product and the tract."""
    text_in, rw, am = _bytes(bed), _records(pairs, PRIMER_PAIRS_DT), _records(amplicons, PAIR_AMPLICONS_DT)
    if len(am) != len(rw):
        raise ValueError(f"{len(rw)} pairs and {len(am)} amplicons")
    names = [_name(n) for n in names]
    pool, off = _pool(names, None)
    off = np.ascontiguousarray(off, dtype=np.int32)
    return _text("ribbit_bed_marker_text", text_in, len(text_in), _ptr(rw), _ptr(am), pool, off.ctypes.data, len(names), len(rw))


def panel_params(**fields) -> PanelParams:
    """ribbit_panel_params_default with the given fields replaced, e.g. panel_params(pool_size=12, size_gap=20); the ranges are
    checked by the calls that take it (include/ribbit_hip.h)"""
    return _params(PanelParams, "ribbit_panel_params_default", "RibbitPanelParams", fields)


def _panel_args(pairs, extra, params):
    """the pairs, the extra ints (or an empty array and a null pointer) and the parameters as the C ABI takes them"""
    rw, params = _records(pairs, PRIMER_PAIRS_DT), _params_arg(params, panel_params, PanelParams)
    ex = np.zeros((0, 3), np.int32)
    if extra is not None:
        ex = np.asarray(extra)
        if ex.size != 3 * len(rw):
            raise ValueError(f"{len(rw)} pairs want {3 * len(rw)} extra values")
        _all_int32(ex.reshape(-1), "an extra value is not an int32")
        ex = np.ascontiguousarray(ex, dtype=np.int32).reshape(-1, 3)
    return rw, ex, (ex.ctypes.data if extra is not None else None), params


def _panel_pools(call, pairs, extra, params):
    """-> a PANEL_DT array, one record per pair, and the number of pools"""
    rw, ex, ex_ptr, params = _panel_args(pairs, extra, params)
    pools = C.c_int32()
    rows = _array(call, _ptr(rw), ex_ptr, len(rw), C.byref(params), dt=PANEL_DT, free="ribbit_panel_free", count=len(rw), tail=(C.byref(pools),))
    return rows, int(pools.value)


def host_panel_pools(pairs, extra=None, params: PanelParams | None = None):
    """ribbit_host_panel_pools: the pairs of `pairs` (a PRIMER_PAIRS_DT array; only the two primers and the product are read) pooled
    into multiplex panels: two pairs conflict when a primer of one binds a primer of the other, when their product sizes lie less
    than size_gap apart, or when they lie on one record within max_cross_product; the pairs are taken by descending number of
    conflicts and each goes into the first pool that has room and no member in conflict with it -> (a PANEL_DT array: the pool and
    the conflicts of every pair, in all and by rule; the number of pools).  extra: (group, size_lo, size_hi) per pair, or None for
    (-1, product, product).  The low-numbered pools fill first.  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _panel_pools(_host("ribbit_host_panel_pools"), pairs, extra, params)


def bed_panel_text(marker_text, rows) -> bytes:
    """ribbit_bed_panel_text: the lines of `marker_text` (bed_marker_text's, pair i on line i) of the pairs that have a pool in
    `rows` (a PANEL_DT array), each with five more columns: pool, conflicts, dimer, size, near; sorted by (pool, designed product,
    input order)."""
    text_in, rw = _bytes(marker_text), _records(rows, PANEL_DT)
    return _text("ribbit_bed_panel_text", text_in, len(text_in), _ptr(rw), len(rw))


def pair_amplicon_sizes(amplicons) -> np.ndarray:
    """ribbit_pair_amplicon_sizes: one sample's row of the genotype matrix from its summed amplicons (a PAIR_AMPLICONS_DT array,
    record_pair_amplicons merged over the sample's records) -> int32 cells: the size of the one product, 0 absent, -1 several
    products, -2 a primer with too many sites."""
    am = _records(amplicons, PAIR_AMPLICONS_DT)
    cells = np.zeros(len(am), np.int32)
    _call("ribbit_pair_amplicon_sizes", _ptr(am), len(am), _ptr(cells))
    return cells


def _alleles_args(cells, designed, motif_lengths):
    """the sample-major matrix (S rows of n cells), the designed products and the motif lengths as the C ABI takes them"""
    cl = np.asarray(cells)
    if cl.ndim != 2:
        raise ValueError("the cells are a matrix, one row per sample")
    ds, ml = np.asarray(designed).reshape(-1), np.asarray(motif_lengths).reshape(-1)
    if len(ds) != cl.shape[1] or len(ml) != cl.shape[1]:
        raise ValueError(f"{cl.shape[1]} markers, {len(ds)} designed products and {len(ml)} motif lengths")
    for a, what in ((cl.reshape(-1), "a cell"), (ds, "a designed product"), (ml, "a motif length")):
        if a.dtype != np.int32:      # (a matrix of a billion cells is not walked to learn what its type says)
            _all_int32(a, f"{what} is not an int32")
    return np.ascontiguousarray(cl, dtype=np.int32), np.ascontiguousarray(ds, dtype=np.int32), np.ascontiguousarray(ml, dtype=np.int32)


def _marker_alleles(call, cells, designed, motif_lengths) -> np.ndarray:
    cl, ds, ml = _alleles_args(cells, designed, motif_lengths)
    n = cl.shape[1]
    return _array(call, cl.ctypes.data if cl.size else None, cl.shape[0], n, _ptr(ds), _ptr(ml), dt=ALLELES_DT, free="ribbit_alleles_free", count=n)


def host_marker_alleles(cells, designed, motif_lengths) -> np.ndarray:
    """ribbit_host_marker_alleles: every marker's alleles over the samples.  cells: the genotype matrix, one row per sample (1 ..
    1024) and one column per marker (pair_amplicon_sizes makes a row); designed: the designed product of every marker, <= 0 for a
    row without a pair; motif_lengths: the length of its motif -> an ALLELES_DT array: the cells by kind, the distinct sizes, the
    least, the largest and the most frequent one, the cells equal to the designed size, those off the motif's step, and the
    numerators of He (over typed^2) and PIC (over typed^4).  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _marker_alleles(_host("ribbit_host_marker_alleles"), cells, designed, motif_lengths)


def bed_alleles_text(bed, pairs, rows, n_samples: int) -> bytes:
    """ribbit_bed_alleles_text: the lines of `bed` (the targets' BED rows, target i on line i), each with 23 more columns: the eight
    primer columns and the designed product of row i of `pairs`, the number of samples and row i of `rows` (an ALLELES_DT array)
    with He and PIC to four decimals."""
    text_in, rw, al = _bytes(bed), _records(pairs, PRIMER_PAIRS_DT), _records(rows, ALLELES_DT)
    if len(al) != len(rw):
        raise ValueError(f"{len(rw)} pairs and {len(al)} records of alleles")
    return _text("ribbit_bed_alleles_text", text_in, len(text_in), _ptr(rw), _ptr(al), int(n_samples), len(rw))


def allele_matrix_text(bed, cells, designed, names) -> bytes:
    """ribbit_allele_matrix_text: a header line, then for every line of `bed` its first four columns, the designed product and one
    field per sample of `cells` (as host_marker_alleles takes them): the size, "." absent, "+" several, "*" over.  names: the
    samples' names, one per row of `cells`."""
    text_in = _bytes(bed)
    cl, ds, _ = _alleles_args(cells, designed, designed)
    names = [_name(n) for n in names]
    if len(names) != cl.shape[0]:
        raise ValueError(f"{cl.shape[0]} samples and {len(names)} names")
    pool, off = _pool(names, None)
    off = np.ascontiguousarray(off, dtype=np.int32)
    return _text("ribbit_allele_matrix_text", text_in, len(text_in), cl.ctypes.data if cl.size else None, cl.shape[0], cl.shape[1], _ptr(ds), pool, off.ctypes.data)


def _record_best(call, intervals):
    iv, bases = _pairs(intervals), C.c_int64()
    rows = _array(call, _ptr(iv), len(iv), dt=_I4, free="ribbit_intervals_free", tail=(C.byref(bases),))
    return rows, int(bases.value)


def host_record_best(length: int, intervals):
    """ribbit_host_record_best: the rows of a record of `length` bases of which no two overlap and which cover the most bases ->
    (their indices by ascending start, int32; the bases they cover).  The contract is in include/ribbit_hip.h.  No GPU needed."""
    return _record_best(_host("ribbit_host_record_best", int(length)), intervals)


def _class_args(intervals, motifs, offsets):
    """the rows, the motif pool and its offsets as the C ABI takes them; `motifs` may also be a list of strings (offsets None)"""
    iv = _pairs(intervals)
    pool, off = _pool(motifs, offsets)
    if off.ndim != 1 or len(off) != len(iv) + 1:
        raise ValueError(f"{len(iv)} rows want {len(iv) + 1} offsets")
    _all_int32(off, "an offset is not an int32")
    return iv, pool, np.ascontiguousarray(off, dtype=np.int32)


def _record_classes(call, intervals, motifs, offsets):
    iv, pool, off = _class_args(intervals, motifs, offsets)
    classes, strands, groups, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    owned = _call(call, _ptr(iv), len(iv), pool, off.ctypes.data, C.byref(classes), C.byref(strands), C.byref(groups), C.byref(n))
    try:
        return C.string_at(classes.value, int(off[-1])), C.string_at(strands.value, len(iv)), _copy(groups.value, n.value, MOTIF_CLASS_DT)
    finally:
        _free(owned, "ribbit_text_free", classes, strands)
        _free(owned, "ribbit_motif_classes_free", groups)


def host_record_classes(length: int, intervals, motifs, offsets=None):
    """ribbit_host_record_classes: the rows of a record of `length` bases by canonical motif class -> (the rows' classes
    concatenated at the motifs' offsets, bytes; a strand byte per row, bytes; the groups in class order, a MOTIF_CLASS_DT array).
    motifs, offsets: as bed_motifs returns them, or a list of strings and None.  The contract is in include/ribbit_hip.h.  No
    GPU needed."""
    return _record_classes(_host("ribbit_host_record_classes", int(length)), intervals, motifs, offsets)


def _record_compounds(call, intervals, labels, gap: int):
    iv, gap = _rows_arg(intervals, gap, "gap")
    lab = np.asarray(labels)
    if lab.ndim != 1 or len(lab) != len(iv):
        raise ValueError(f"{len(iv)} rows want {len(iv)} labels")
    _all_int32(lab, "a label is not an int32")
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    chains, n, members, m = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
    owned = _call(call, _ptr(iv), _ptr(lab), len(iv), gap, C.byref(chains), C.byref(n), C.byref(members), C.byref(m))
    try:
        return _copy(chains.value, n.value, COMPOUND_DT), _copy(members.value, m.value, _I4)
    finally:
        _free(owned, "ribbit_compounds_free", chains)
        _free(owned, "ribbit_intervals_free", members)


def host_record_compounds(length: int, intervals, labels, gap: int = 100):
    """ribbit_host_record_compounds: the rows of a record of `length` bases, each with an int32 label, chained while a row starts
    at most `gap` bases behind everything before it -> (the chains by ascending start, a COMPOUND_DT array; the non-empty rows'
    indices in (start, end, index) order, int32: chain c owns members[first : first + rows]).  The contract is in
    include/ribbit_hip.h.  No GPU needed."""
    return _record_compounds(_host("ribbit_host_record_compounds", int(length)), intervals, labels, gap)


def _record_interruptions(call, intervals, motif_lengths, cigars, offsets):
    iv = _pairs(intervals)
    pool, off = _pool(cigars, offsets)
    k = np.asarray(motif_lengths)
    if off.ndim != 1 or len(off) != len(iv) + 1:
        raise ValueError(f"{len(iv)} rows want {len(iv) + 1} offsets")
    if k.ndim != 1 or len(k) != len(iv):
        raise ValueError(f"{len(iv)} rows want {len(iv)} motif lengths")
    for a in (off, k):
        _all_int32(a, "an offset or a motif length is not an int32")
    k, off = np.ascontiguousarray(k, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32)
    rows, sites, m, observed, offsets_out = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_void_p()
    owned = _call(call, _ptr(iv), _ptr(k), len(iv), pool, off.ctypes.data, C.byref(rows), C.byref(sites), C.byref(m), C.byref(observed),
                  C.byref(offsets_out))
    try:
        seen = _copy(offsets_out.value, m.value + 1, _I4) if m.value else np.zeros(1, np.int32)
        return (_copy(rows.value, len(iv), ROW_PURITY_DT), _copy(sites.value, m.value, INTERRUPTION_DT),
                C.string_at(observed.value, int(seen[-1])) if m.value else b"", seen)
    finally:
        _free(owned, "ribbit_row_purity_free", rows)
        _free(owned, "ribbit_interruptions_free", sites)
        _free(owned, "ribbit_text_free", observed)
        _free(owned, "ribbit_intervals_free", offsets_out)


def host_record_interruptions(sequence: bytes, intervals, motif_lengths, cigars, offsets=None):
    """ribbit_host_record_interruptions: every row's CIGAR decoded -> (a ROW_PURITY_DT record per row; the interruptions by row,
    then in CIGAR order, an INTERRUPTION_DT array; their observed bases concatenated, bytes; the n_sites + 1 offsets of those,
    int32).  cigars, offsets: as bed_cigars returns them, or a list of strings and None.  The contract is in
    include/ribbit_hip.h.  No GPU needed."""
    return _record_interruptions(_host_bases("ribbit_host_record_interruptions", sequence), intervals, motif_lengths, cigars, offsets)


# BED text: readers and writers ----------------------------------------------------------------
def bed_intervals(text) -> np.ndarray:
    """ribbit_bed_intervals: (start, end) of every row of BED text as refine_bed writes it, an (n, 2) int32 array."""
    raw = _bytes(text)
    pairs, n = C.c_void_p(), C.c_size_t()
    _call("ribbit_bed_intervals", raw, len(raw), C.byref(pairs), C.byref(n))
    try:
        return _copy(pairs.value, 2 * n.value, _I4).reshape(-1, 2)
    finally:
        _free(True, "ribbit_intervals_free", pairs)


def _bed_column(symbol: str, text):
    """-> (a column of every row of BED text concatenated, bytes; the n + 1 offsets, int32)"""
    raw = _bytes(text)
    pool, offsets, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    _call(symbol, raw, len(raw), C.byref(pool), C.byref(offsets), C.byref(n))
    try:
        off = _copy(offsets.value, n.value + 1, _I4)
        return C.string_at(pool.value, int(off[-1])), off
    finally:
        _free(True, "ribbit_text_free", pool)
        _free(True, "ribbit_intervals_free", offsets)


def bed_motifs(text):
    """ribbit_bed_motifs: column 4 of every row of BED text as refine_bed writes it -> (the motifs concatenated, bytes; their
    n + 1 offsets, int32)."""
    return _bed_column("ribbit_bed_motifs", text)


def bed_cigars(text):
    """ribbit_bed_cigars: column 11 of every row of BED text as refine_bed writes it -> (the CIGARs concatenated, bytes; their
    n + 1 offsets, int32)."""
    return _bed_column("ribbit_bed_cigars", text)


def _bed_rows_text(symbol: str, bed, rows, dt) -> bytes:
    """a writer that takes BED text and one array with a record per row (dt None: pairs of int32)"""
    text_in = _bytes(bed)
    rw = _pairs(rows) if dt is None else _records(rows, dt)
    return _text(symbol, text_in, len(text_in), _ptr(rw), len(rw))


def bed_loci_text(name, bed, loci) -> bytes:
    """ribbit_bed_loci_text: one line per locus of one record: name, start, end, rows, covered and the last ten columns of the
    locus's best row of `bed` (the record's BED text, row i on line i)."""
    raw, text_in, lo = _name(name), _bytes(bed), _records(loci, LOCUS_DT)
    return _text("ribbit_bed_loci_text", raw, text_in, len(text_in), _ptr(lo), len(lo))


def bed_overlap_text(bed, per_row) -> bytes:
    """ribbit_bed_overlap_text: the lines of `bed` (one record's BED text, row i on line i), each with row i's two values of
    `per_row` appended as two more columns."""
    return _bed_rows_text("ribbit_bed_overlap_text", bed, per_row, None)


def bed_nearest_text(bed, nearest, targets, labels, label_offsets=None) -> bytes:
    """ribbit_bed_nearest_text: the lines of `bed` (one record's BED text, row i on line i), each with eight more columns: what
    `nearest` (record_nearest with the rows as queries) names among `targets`.  labels, label_offsets: a pool and its offsets, or
    a list of strings and None."""
    text_in, near = _bytes(bed), _records(nearest, NEAREST_DT)
    iv, pool, off = _class_args(targets, labels, label_offsets)
    return _text("ribbit_bed_nearest_text", text_in, len(text_in), _ptr(near), len(near), _ptr(iv), pool, off.ctypes.data, len(iv))


def nearest_other_text(name, targets, labels, nearest, rows, motifs, label_offsets=None, motif_offsets=None) -> bytes:
    """ribbit_nearest_other_text: one line per interval of `targets` (a second BED's intervals on one record, with their labels): name,
    start, end, label and the eight columns of what `nearest` (record_nearest with the intervals as queries) names among the
    record's `rows`, a row's label being its motif.  Pools with offsets, or lists of strings and None."""
    raw = _name(name)
    iv, pool, off = _class_args(targets, labels, label_offsets)
    rw, motif_pool, motif_off = _class_args(rows, motifs, motif_offsets)
    near = _records(nearest, NEAREST_DT)
    if len(near) != len(iv):
        raise ValueError(f"{len(iv)} intervals want {len(iv)} nearest records, not {len(near)}")
    return _text("ribbit_nearest_other_text", raw, _ptr(iv), pool, off.ctypes.data, len(iv), _ptr(near), _ptr(rw), motif_pool, motif_off.ctypes.data,
                 len(rw))


def bed_composition_text(bed, rows) -> bytes:
    """ribbit_bed_composition_text: the lines of `bed` (one record's BED text, row i on line i), each with the 13 values of row i of
    `rows` (record_composition) appended as 13 more columns."""
    return _bed_rows_text("ribbit_bed_composition_text", bed, rows, COMPOSITION_DT)


def base_windows_text(name, length: int, window: int, windows) -> bytes:
    """ribbit_base_windows_text: one line per window of a record of `length` bases: name, start, end and the five counts of
    `windows` (record_base_windows)."""
    raw, window, w = _name(name), _int32(window, "window"), _records(windows, BASE_COUNTS_DT)
    return _text("ribbit_base_windows_text", raw, int(length), window, _ptr(w), len(w))


def bed_primers_text(bed, rows) -> bytes:
    """ribbit_bed_primers_text: the lines of `bed` (the targets' BED rows, target i on line i), each with the primers of row i of
    `rows` (record_primers) appended as 11 more columns."""
    return _bed_rows_text("ribbit_bed_primers_text", bed, rows, PRIMERS_DT)


def bed_primer_pairs_text(bed, rows) -> bytes:
    """ribbit_bed_primer_pairs_text: the lines of `bed` (the targets' BED rows, target i on line i), each with the primer pair of
    row i of `rows` (record_primer_pairs) appended as 21 more columns."""
    return _bed_rows_text("ribbit_bed_primer_pairs_text", bed, rows, PRIMER_PAIRS_DT)


def bed_primer_products_text(bed, pairs, products) -> bytes:
    """ribbit_bed_primer_products_text: the lines of bed_primer_pairs_text(bed, pairs), each with six more columns from row i of
    `products` (record_primer_products): the four site counts, the products other than the pair's own and the shortest of them."""
    text_in, rw, pr = _bytes(bed), _records(pairs, PRIMER_PAIRS_DT), _records(products, PRIMER_PRODUCTS_DT)
    if len(pr) != len(rw):
        raise ValueError(f"{len(rw)} pairs and {len(pr)} products")
    return _text("ribbit_bed_primer_products_text", text_in, len(text_in), _ptr(rw), _ptr(pr), len(rw))


def bed_primer_specific_text(bed, pairs, products, specific) -> bytes:
    """ribbit_bed_primer_specific_text: the lines of bed_primer_products_text(bed, pairs, products) for the chosen pairs, each with four
    more columns from row i of `specific` (record_specific_primer_pairs): the pair's place among the admissible pairs ('.' without a
    pair) and the specific, over and other pairs."""
    text_in, rw, pr, sp = _bytes(bed), _records(pairs, PRIMER_PAIRS_DT), _records(products, PRIMER_PRODUCTS_DT), _records(specific, PRIMER_SPECIFIC_DT)
    if not len(pr) == len(rw) == len(sp):
        raise ValueError(f"{len(rw)} pairs, {len(pr)} products and {len(sp)} summaries")
    return _text("ribbit_bed_primer_specific_text", text_in, len(text_in), _ptr(rw), _ptr(pr), _ptr(sp), len(rw))


def oligo_duplex(a, b) -> tuple:
    """ribbit_host_oligo_duplex: (any, end) of two oligos of 1 .. 32 letters of ACGT, each read 5' to 3': the longest run of
    bonded pairs over all ungapped antiparallel placements, and the longest that holds a 3' base (include/ribbit_hip.h)"""
    any_, end = C.c_int32(), C.c_int32()
    _call("ribbit_host_oligo_duplex", _bytes(a), _bytes(b), C.byref(any_), C.byref(end))
    return any_.value, end.value


def oligo_hairpin(a) -> int:
    """ribbit_host_oligo_hairpin: the longest stem an oligo closes on itself around a loop of 3 bases or more"""
    out = C.c_int32()
    _call("ribbit_host_oligo_hairpin", _bytes(a), C.byref(out))
    return out.value


def bed_rows_text(bed, rows) -> bytes:
    """ribbit_bed_rows_text: lines rows[0], rows[1], ... of `bed` (one record's BED text, row i on line i), byte for byte."""
    return _bed_rows_text("ribbit_bed_rows_text", bed, rows, np.int32)


def _class_offsets(classes, offsets, rows: int | None):
    """the rows' classes and the offsets into them, as record_classes returns them"""
    cls, off = bytes(classes), _records(offsets, np.int32)
    if rows is None and (len(off) < 1 or len(cls) < int(off[-1])):
        raise ValueError("n rows want n + 1 offsets into the classes")
    if rows is not None and (len(off) != rows + 1 or len(cls) < int(off[-1])):
        raise ValueError(f"{rows} rows want {rows + 1} offsets into the classes")
    return cls, off


def bed_class_text(bed, classes, offsets, strands) -> bytes:
    """ribbit_bed_class_text: the lines of `bed` (one record's BED text, row i on line i), each with row i's class and strand
    appended as two more columns."""
    text_in, st = _bytes(bed), bytes(strands)
    cls, off = _class_offsets(classes, offsets, len(st))
    return _text("ribbit_bed_class_text", text_in, len(text_in), cls, off.ctypes.data, st, len(st))


def class_summary_text(name, intervals, classes, offsets, groups) -> bytes:
    """ribbit_class_summary_text: one line per group of one record: name, class, length, rows, bases, start and end of the
    group's longest row as `intervals` (the rows the groups were made from) has them."""
    raw, iv = _name(name), _pairs(intervals)
    cls, off = _class_offsets(classes, offsets, len(iv))
    gr = _records(groups, MOTIF_CLASS_DT)
    return _text("ribbit_class_summary_text", raw, _ptr(iv), len(iv), cls, off.ctypes.data, _ptr(gr), len(gr))


def class_labels(classes, offsets, groups) -> np.ndarray:
    """ribbit_class_labels: per row the index, in class order, of the group whose class is the row's, int32.  classes, offsets,
    groups: what record_classes / host_record_classes return for the rows (offsets: the motifs')."""
    cls, off = _class_offsets(classes, offsets, None)
    gr = _records(groups, MOTIF_CLASS_DT)
    return _array("ribbit_class_labels", cls, off.ctypes.data, len(off) - 1, _ptr(gr), len(gr), dt=_I4, free="ribbit_intervals_free", count=len(off) - 1)


def compound_text(name, bed, length: int, intervals, compounds, members) -> bytes:
    """ribbit_compound_text: one line per chain of one record: name, start, end, kind (p, i or c, with * when members overlap),
    rows, classes, bases and the structure, e.g. (CA)12n5(GA)8, read from the members' lines of `bed` (row i on line i)."""
    raw, text_in, iv = _name(name), _bytes(bed), _pairs(intervals)
    ch, mem = _records(compounds, COMPOUND_DT), _records(members, np.int32)
    return _text("ribbit_compound_text", raw, text_in, len(text_in), int(length), _ptr(iv), len(iv), _ptr(ch), len(ch), _ptr(mem), len(mem))


def interruption_text(name, bed, intervals, rows, sites, cigars, observed, observed_offsets):
    """ribbit_interruption_text: one line per interruption of every consistent row of one record -> (the text: name, start, end,
    the interruption's ops, the observed bases or '.', the row's start and end, its motif and the 0-based repeat unit the site
    falls in; the number of inconsistent rows, whose interruptions are left out).  cigars: the pool the sites point into."""
    raw, pool = _bytes(name), _bytes(cigars)
    if b"\0" in raw or b"\0" in pool:
        raise ValueError("a record name or a CIGAR pool cannot hold a NUL byte")
    text_in, iv = _bytes(bed), _pairs(intervals)
    per_row, st, off = _records(rows, ROW_PURITY_DT), _records(sites, INTERRUPTION_DT), _records(observed_offsets, np.int32)
    if len(per_row) != len(iv) or len(off) != len(st) + 1:
        raise ValueError(f"{len(iv)} rows want {len(iv)} records, {len(st)} interruptions {len(st) + 1} offsets")
    obs = bytes(observed)
    if len(off) and len(obs) < int(off.max()):
        raise ValueError("the offsets reach behind the observed bases")
    left = C.c_size_t()
    text = _text("ribbit_interruption_text", raw, text_in, len(text_in), _ptr(iv), len(iv), _ptr(per_row), _ptr(st), len(st), pool, obs, off.ctypes.data,
                 tail=(C.byref(left),))
    return text, left.value


def bed_purity_text(bed, intervals, motif_lengths, rows) -> bytes:
    """ribbit_bed_purity_text: the lines of `bed` (one record's BED text, row i on line i), each with seven more columns: count,
    x, ins, del, pure_start, pure_end and pure_units (the last three '.' for a row whose CIGAR does not span it)."""
    text_in, iv = _bytes(bed), _pairs(intervals)
    k, per_row = _records(motif_lengths, np.int32), _records(rows, ROW_PURITY_DT)
    if len(k) != len(iv) or len(per_row) != len(iv):
        raise ValueError(f"{len(iv)} rows want {len(iv)} motif lengths and records")
    return _text("ribbit_bed_purity_text", text_in, len(text_in), _ptr(iv), _ptr(k), _ptr(per_row), len(iv))


def host_perfect_runs_from_events(min_motif: int, max_motif: int, event_parts, count_parts):
    """ribbit_host_perfect_runs_from_events: per-rank (events, per-motif counts) -> paired runs. No GPU needed."""
    params = _scan_params(min_motif, max_motif)
    ev = np.ascontiguousarray(np.concatenate(event_parts) if len(event_parts) else np.zeros(0, "<u8"), dtype="<u8")
    cnt = np.ascontiguousarray(np.concatenate(count_parts), dtype="<u8")
    return _array("ribbit_host_perfect_runs_from_events", C.byref(params), len(event_parts), ev.ctypes.data, cnt.ctypes.data, dt=RUN_DT,
                  free="ribbit_runs_free")


def pair_halves(halves) -> np.ndarray:
    """Cross-rank pairing of the edge events of chunk-local pairing (Scanner.perfect_runs_partial): sorted by
    (motif, position) they alternate START, END."""
    hv = np.sort(np.asarray(halves, dtype="<u8").view("<u8"), kind="stable") if len(halves) else np.zeros(0, "<u8")
    if len(hv) == 0:
        return np.zeros(0, RUN_DT)
    pos = (hv & np.uint64(0xFFFFFFFF)).astype(np.int64)
    mlen = ((hv >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
    kind = ((hv >> np.uint64(48)) & np.uint64(0xF)).astype(np.int64)
    order = np.lexsort((pos, mlen))
    pos, mlen, kind = pos[order], mlen[order], kind[order]
    if len(hv) % 2 or np.any(kind[0::2] != 0) or np.any(kind[1::2] == 0) or np.any(mlen[0::2] != mlen[1::2]):
        raise RibbitHipError("edge events of the chunks do not pair up")
    out = np.zeros(len(hv) // 2, RUN_DT)
    out["start"], out["end"], out["mlen"] = pos[0::2], pos[1::2], mlen[0::2]
    out["term"] = kind[1::2] - 1
    return out


RUN_NOT_OWNED, RUN_HALF_START, RUN_HALF_END = -1, 3, 4


def join_run_halves(halves) -> np.ndarray:
    """Half records of all chunks of one record (Scanner.scan_perfect_chunk) -> the runs they form: ordered by
    (motif, position) every open START is closed by the next orphan END of its motif."""
    hv = np.concatenate([np.asarray(h, dtype=RUN_DT) for h in halves]) if len(halves) else np.zeros(0, RUN_DT)
    hs = hv[hv["term"] == RUN_HALF_START]
    he = hv[hv["term"] >= RUN_HALF_END]
    if len(hs) + len(he) != len(hv) or len(hs) != len(he):
        raise RibbitHipError(f"{len(hs)} open run starts but {len(he)} orphan run ends across the chunks")
    hs = hs[np.lexsort((hs["start"], hs["mlen"]))]
    he = he[np.lexsort((he["end"], he["mlen"]))]
    if np.any(hs["mlen"] != he["mlen"]) or np.any(he["end"] <= hs["start"]) or \
            np.any((hs["mlen"][1:] == hs["mlen"][:-1]) & (hs["start"][1:] <= he["end"][:-1])):
        raise RibbitHipError("run halves of the chunks do not pair up")
    joined = np.zeros(len(hs), RUN_DT)
    joined["start"], joined["end"], joined["mlen"], joined["term"] = hs["start"], he["end"], hs["mlen"], he["term"] - RUN_HALF_END
    return joined


def merge_chunk_runs(parts, halves) -> np.ndarray:
    """All chunks' run records and halves -> the record's runs ordered by (mlen, start) (copies; for tests and
    small inputs -- a streaming consumer walks the parts in place and skips term == RUN_NOT_OWNED)."""
    allr = np.concatenate([np.asarray(p) for p in parts] + [join_run_halves(halves)])
    allr = allr[allr["term"] >= 0]
    return allr[np.lexsort((allr["start"], allr["mlen"]))]


def read_fasta(path: str, pinned: bool = False):
    """records of a FASTA file as ribbit_fasta_* delimits them (the reference's reader loop, ribbit.cpp:269-280):
    [(name, bases bytes, is_last)]"""
    L = load_library()
    r = C.c_void_p()
    if L.ribbit_fasta_open(path.encode(), int(pinned), C.byref(r)) != 0:
        raise RibbitHipError(L.ribbit_fasta_last_error().decode())
    out = []
    try:
        while True:
            name, bases, n, last = C.c_char_p(), C.c_void_p(), C.c_int64(), C.c_int()
            got = L.ribbit_fasta_next(r, C.byref(name), C.byref(bases), C.byref(n), C.byref(last))
            if got < 0:
                raise RibbitHipError(L.ribbit_fasta_last_error().decode())
            if got == 0:
                break
            out.append((name.value.decode(), C.string_at(bases.value, n.value), bool(last.value)))
            L.ribbit_fasta_release(r, bases)
    finally:
        L.ribbit_fasta_close(r)
    return out


class PinnedBuffer:
    """page-locked host memory (ribbit_hip_host_alloc) as a writable numpy uint8 view"""

    def __init__(self, nbytes: int):
        self._L = load_library()
        p = C.c_void_p()
        _ok("ribbit_hip_host_alloc", self._L.ribbit_hip_host_alloc(max(int(nbytes), 1), C.byref(p)))
        self.ptr = p.value
        self.nbytes = int(nbytes)
        self.array = np.frombuffer((C.c_char * max(self.nbytes, 1)).from_address(self.ptr), dtype=np.uint8)[:self.nbytes]

    def close(self):
        if self.ptr:
            self.array = None
            self._L.ribbit_hip_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Scanner:
    """One GPU-resident FASTA record and the scans over it.

    Method names follow the reference functions they stand in for
    (parse_perfect_shiftxor.h:10, fasta_utils.cpp:59-250).
    """

    def __init__(self, min_motif: int = 2, max_motif: int = 100, device: int = 0):
        self._L = load_library()
        self.params = ScanParams()
        self._L.ribbit_scan_params_default(C.byref(self.params), min_motif, max_motif)
        h = C.c_void_p()
        self._h = None
        self._check(self._L.ribbit_hip_open(C.byref(self.params), device, C.byref(h)))
        self._h = h
        self.length = 0
        self.min_shift = min_motif - 2 if min_motif > 2 else 1     # ribbit.cpp:241
        self.max_shift = max_motif + 2                              # ribbit.cpp:242

    def _check(self, rc):
        if rc != 0:          # (tested here as well: the scan and chunk methods pay no second Python call for a status of 0)
            _ok("ribbit_hip", rc)

    def _dev(self, symbol: str) -> tuple:
        """the device form of a row output's call (see _host): the results are the handle's and are not freed"""
        return symbol, (self._h,), "ribbit_hip", False

    def _refine_params(self, refine_params) -> RefineParams:
        return _refine_params(refine_params, self.params.min_motif, self.params.max_motif)

    def close(self):
        if self._h is not None:
            self._L.ribbit_hip_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_pair_events(self, events: np.ndarray, length: int):
        """-> (runs, flags): the device-side pairing on a caller-made event stream (uint64 events in buffer order)"""
        ev = np.ascontiguousarray(events, dtype="<u8")
        runs = np.zeros(max(len(ev), 1), RUN_DT)
        n, flags = C.c_size_t(), C.c_uint32()
        self._check(self._L.ribbit_hip_debug_pair_events(self._h, ev.ctypes.data, len(ev), length, runs.ctypes.data, len(runs), C.byref(n), C.byref(flags)))
        return runs[:min(n.value, len(runs))], flags.value

    def debug_pair_events_sharded(self, events: np.ndarray, counters: np.ndarray, region_cap: int, length: int,
                                  own_lo: int = 0, own_hi: int = 2 ** 63 - 1, pos_offset: int = 0) -> dict:
        """The device-side pairing, and the legacy compaction and chunk table, on events placed by the caller: `events` holds 64 regions
        of region_cap words, `counters` the 64 region counters (they may exceed region_cap).  -> dict: runs (every slot, place holders
        included), halves, flags, total, n_halves, published (64 counters), dense, summary, overflow, table ((motifs, ntile, 2) of
        {first + 1, end}), table_status."""
        ev = np.ascontiguousarray(events, dtype="<u8").reshape(-1)
        cnt = np.ascontiguousarray(counters, dtype="<u4").reshape(-1)
        assert region_cap >= 1 and len(ev) == 64 * region_cap and len(cnt) == 64
        nm, ntile = self.params.max_motif - self.params.min_motif + 1, length // 16384 + 1
        runs, halves = np.zeros(32 * region_cap, RUN_DT), np.zeros(2 * nm, RUN_DT)
        dense, table = np.zeros(len(ev), "<u8"), np.zeros(nm * ntile, "<u8")
        out = DebugPairing(runs.ctypes.data, len(runs), halves.ctypes.data, len(halves), dense.ctypes.data, len(dense), table.ctypes.data, len(table))
        self._check(self._L.ribbit_hip_debug_pair_events_sharded(self._h, ev.ctypes.data, cnt.ctypes.data, region_cap, length, own_lo, own_hi,
                                                                 pos_offset, C.byref(out)))
        flags, total, n_halves = (int(x) for x in out.status)
        return {"runs": runs[:min(total, len(runs))], "halves": halves[:min(n_halves, len(halves))], "flags": flags, "total": total,
                "n_halves": n_halves, "published": np.array(out.published, dtype="<u4"), "dense": dense[:min(out.summary, len(dense))],
                "summary": int(out.summary), "overflow": int(out.overflow),
                "table": np.stack((table & np.uint64(0xFFFFFFFF), table >> np.uint64(32)), axis=-1).astype("<u4").reshape(nm, ntile, 2),
                "table_status": int(out.table_status)}

    def debug_window_calls(self, stage: int, streaks: np.ndarray, full: bool = False, min_span=None, own_lo: int = 0, own_hi: int = 2 ** 32 - 1,
                           z_lo: int = 0, keep_flush: bool = True, pos_offset: int = 0, dropped_ends=(), first_edge_cap: int = 0) -> dict:
        """ribbit_hip_debug_window_calls: the window stage behind the scan and the pairing on caller-made streaks (RUN_DT, ordered by
        (mlen, start)) of the loaded record; min_span: one int per motif size (not needed with full); dropped_ends: ascending ends
        of groups that are not among the streaks -> dict(calls, pend (or None), tail_pend, flush, inexact, n_edge) (copies)"""
        sk = np.ascontiguousarray(streaks, dtype=RUN_DT)
        sp = None if min_span is None else np.ascontiguousarray(min_span, dtype="<i4")
        assert sp is None or len(sp) == self.params.max_motif - self.params.min_motif + 1
        de = np.ascontiguousarray(dropped_ends, dtype="<i4").reshape(-1)
        arg = DebugWindowStage(sk.ctypes.data if len(sk) else None, len(sk), None if sp is None else sp.ctypes.data,
                               de.ctypes.data if len(de) else None, len(de), own_lo, own_hi, z_lo, pos_offset, first_edge_cap, int(bool(full)),
                               int(bool(keep_flush)))
        cc, n_edge = ChunkCalls(), C.c_uint32()
        self._check(self._L.ribbit_hip_debug_window_calls(self._h, stage, C.byref(arg), C.byref(cc), C.byref(n_edge)))
        return {"calls": _copy(cc.calls, cc.n, CALL_DT), "pend": _copy(cc.pend, cc.n, _I4) if cc.pend else None,
                "tail_pend": int(cc.tail_pend), "flush": _copy(cc.flush, cc.n_flush, CALL_DT), "inexact": bool(cc.inexact),
                "n_edge": int(n_edge.value)}

    def debug_set_event_capacity(self, events: int) -> None:
        self._check(self._L.ribbit_hip_debug_set_event_capacity(self._h, events))

    def debug_set_scan_split(self, kernel: int, motifs_per_block: int) -> None:
        """motifs per block of a scan kernel (SCAN_PERFECT .. SCAN_XA_WINDOW, or SCAN_ALL); 0 = automatic"""
        self._check(self._L.ribbit_hip_debug_set_scan_split(self._h, kernel, motifs_per_block))

    def debug_last_scan_split(self, kernel: int) -> tuple:
        """-> (gridDim.y, motifs per block) of the kernel's last launch on the loaded record; (0, 0) if it has not run"""
        gy, mpb = C.c_int32(), C.c_int32()
        self._check(self._L.ribbit_hip_debug_last_scan_split(self._h, kernel, C.byref(gy), C.byref(mpb)))
        return gy.value, mpb.value

    def set_timing(self, enabled: bool) -> None:
        self._check(self._L.ribbit_hip_set_timing(self._h, int(enabled)))

    def set_stream(self, hip_stream: int | None):
        self._check(self._L.ribbit_hip_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    # fasta_utils.cpp:78-122 -------------------------------------------------------------
    def load_record(self, sequence: bytes):
        self._keep = bytes(sequence)
        self.length = len(self._keep)
        self._check(self._L.ribbit_hip_load_record(self._h, self._keep, self.length))

    def load_record_pinned(self, host_ptr: int, length: int):
        """bases in page-locked memory (PinnedBuffer) that stays valid until the next load: async upload, no host copy"""
        self.length = int(length)
        self._check(self._L.ribbit_hip_load_record_pinned(self._h, C.c_void_p(host_ptr), self.length))

    def load_record_device(self, dev_ptr: int, length: int):
        self.length = int(length)
        self._check(self._L.ribbit_hip_load_record_device(self._h, C.c_void_p(dev_ptr), self.length))

    def _list(self, fn, dt, copy=True):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(fn(self._h, C.byref(p), C.byref(n)))
        return _copy(p.value, n.value, dt) if copy else _view(p.value, n.value, dt)

    # parse_perfect_shiftxor.cpp:146-226 ---------------------------------------------------
    def scan_perfect_runs(self, copy=True):
        """Runs of the perfect scan ordered by (mlen, start).  copy=False returns a read-only view of the
        library's pinned result buffer, valid until the next call on this Scanner (what a C caller gets)."""
        return self._list(self._L.ribbit_hip_scan_perfect_runs, RUN_DT, copy)

    def perfect_calls(self):
        return self._list(self._L.ribbit_hip_perfect_calls, CALL_DT)

    def processShiftXORsPerfect(self, copy=True):
        """copy=False: a read-only view of the library's list, valid until the next call on this Scanner (what a C caller gets)"""
        return self._list(self._L.ribbit_hip_seeds_perfect, SEED_DT, copy)

    # parse_substitute_shiftxor.cpp:391-577 ------------------------------------------------
    def subst_calls(self):
        return self._list(self._L.ribbit_hip_subst_calls, CALL_DT)

    def processShiftXORswithSubstitutions(self):
        """-> (seed_positions_perfect as re-typed by this stage, seed_positions_substut)"""
        pp, np_, ps, ns = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self._check(self._L.ribbit_hip_seeds_substitutions(self._h, C.byref(pp), C.byref(np_), C.byref(ps), C.byref(ns)))
        return _copy(pp.value, np_.value, SEED_DT), _copy(ps.value, ns.value, SEED_DT)

    # parse_anchored_shiftxor.cpp:20-56, 538-726; fasta_utils.cpp:143-224 --------------------
    def anchored_calls(self):
        return self._list(self._L.ribbit_hip_anchored_calls, CALL_DT)

    def processShiftXORsAnchored(self, copy=True):
        """-> (perfect, substitution, anchored seed lists as the anchored stage leaves them); copy=False: read-only views of
        the library's lists, valid until the next call on this Scanner (what a C caller gets: three pointers)"""
        ptrs = [C.c_void_p() for _ in range(3)]
        ns = [C.c_size_t() for _ in range(3)]
        args = []
        for p, n in zip(ptrs, ns):
            args += [C.byref(p), C.byref(n)]
        self._check(self._L.ribbit_hip_seeds_anchored(self._h, *args))
        if copy:
            return tuple(_copy(p.value, n.value, SEED_DT) for p, n in zip(ptrs, ns))
        return tuple(_view(p.value, n.value, SEED_DT) for p, n in zip(ptrs, ns))

    def dispatch_seeds(self, copy=True):
        return self._list(self._L.ribbit_hip_dispatch_seeds, SEED_DT, copy)

    # parse_seed.cpp:26-44 (batched on the GPU), parse_smallmotif_seed.cpp:76-270, parse_seed.cpp:153-404 ----
    def seed_longest_runs(self):
        return self._list(self._L.ribbit_hip_seed_longest_runs, _I4)

    def seed_best_rows(self, refine_params=None):
        """ribbit_hip_seed_best_rows: per dispatched seed the window start mostFrequentLongerMotif selects (GPU), -1 where it is not asked"""
        rp = self._refine_params(refine_params)
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.ribbit_hip_seed_best_rows(self._h, C.byref(rp), C.byref(p), C.byref(n)))
        return _copy(p.value, n.value, _I4)

    def refine_jobs(self, refine_params=None):
        rp = self._refine_params(refine_params)
        jobs, n, pool = C.c_void_p(), C.c_size_t(), C.c_void_p()
        self._check(self._L.ribbit_hip_refine_jobs(self._h, C.byref(rp), C.byref(jobs), C.byref(n), C.byref(pool)))
        arr = _copy(jobs.value, n.value, JOB_DT)
        size = int((arr["motif_offset"] + arr["atomicity"]).max()) if len(arr) else 0
        return arr, (C.string_at(pool.value, size) if size else b"")

    def small_motifs(self, refine_params=None):
        """ribbit_hip_small_motifs: (head [n_seeds, 4] int32, records [n_records, 4] uint32) -- possibleMotifs of the
        dispatched seeds with m <= 10 as the GPU computed it"""
        rp = self._refine_params(refine_params)
        head, n, rec, nr = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self._check(self._L.ribbit_hip_small_motifs(self._h, C.byref(rp), C.byref(head), C.byref(n), C.byref(rec), C.byref(nr)))
        return _copy(head.value, 4 * n.value, _I4).reshape(-1, 4), _copy(rec.value, 4 * nr.value, np.dtype("<u4")).reshape(-1, 4)

    def _refine_bed(self, sequence_id: str, refine_params):
        """-> (address, length) of the handle's BED text"""
        rp = self._refine_params(refine_params)
        text, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.ribbit_hip_refine_bed(self._h, C.byref(rp), sequence_id.encode(), C.byref(text), C.byref(n)))
        return text.value, n.value

    def refine_bed(self, sequence_id: str = "seq", refine_params=None) -> str:
        """BED rows of the loaded record (fasta_utils.cpp:211-242 and everything below it)"""
        return C.string_at(*self._refine_bed(sequence_id, refine_params)).decode()

    def refine_bed_view(self, sequence_id: str = "seq", refine_params=None) -> np.ndarray:
        """The same BED text as the C ABI hands it out: a uint8 view of the library's buffer (valid until the handle's next
        refine_bed call or its close), without the copy and the decoding into a Python string that refine_bed adds -- 150 MB
        twice over for a chromosome, which a C caller (ribbit-hip writes the buffer straight to its output file) never pays."""
        text, n = self._refine_bed(sequence_id, refine_params)
        if not n:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(C.cast(text, C.POINTER(C.c_uint8)), shape=(n,))

    def mask_record(self, intervals, mode: str = "soft", line_width: int = 60) -> bytes:
        """The loaded record's masked, line-wrapped FASTA body on the GPU (ribbit_hip_mask_record); see host_mask_record"""
        return _mask_record(self._dev("ribbit_hip_mask_record"), intervals, mode, line_width)

    def repeat_sequences(self, name, intervals, flank: int = 100) -> bytes:
        """The loaded record's repeat sequences with their flanks on the GPU (ribbit_hip_repeat_sequences), every batch of the
        handle's text budget joined; see host_repeat_sequences"""
        return b"".join(text for text, _ in self.repeat_sequence_batches(name, intervals, flank))

    def repeat_sequence_batches(self, name, intervals, flank: int = 100):
        """-> [(text, rows)] of the calls repeat_sequences makes, in order"""
        raw, iv, f = _repeat_args(name, intervals, flank)
        out, done = [], 0
        while True:
            text, n, k = C.c_void_p(), C.c_size_t(), C.c_size_t()
            ptr = iv[done:].ctypes.data if done < len(iv) else None
            self._check(self._L.ribbit_hip_repeat_sequences(self._h, raw, ptr, len(iv) - done, f, C.byref(text), C.byref(n), C.byref(k)))
            if done < len(iv):          # (no rows at all: the one call still checks the handle's state)
                out.append((C.string_at(text.value, n.value), k.value))
                done += k.value
            if done == len(iv):
                return out

    def record_loci(self, intervals, gap: int = 0) -> np.ndarray:
        """The loaded record's rows merged into loci on the GPU (ribbit_hip_record_loci); see host_record_loci"""
        return _record_loci(self._dev("ribbit_hip_record_loci"), intervals, gap)

    def record_overlap(self, rows, other):
        """The loaded record's rows against the intervals `other` on the GPU (ribbit_hip_record_overlap); see host_record_overlap"""
        return _record_overlap(self._dev("ribbit_hip_record_overlap"), rows, other)

    def record_nearest(self, queries, targets) -> np.ndarray:
        """The loaded record's queries against `targets` on the GPU (ribbit_hip_record_nearest); see host_record_nearest"""
        return _record_nearest(self._dev("ribbit_hip_record_nearest"), queries, targets)

    def record_composition(self, intervals, flank: int = 100) -> np.ndarray:
        """The loaded record's rows' and flanks' base counts on the GPU (ribbit_hip_record_composition); see host_record_composition"""
        return _record_composition(self._dev("ribbit_hip_record_composition"), intervals, flank)

    def record_base_windows(self, window: int) -> np.ndarray:
        """The loaded record's base counts per window on the GPU (ribbit_hip_record_base_windows); see host_record_base_windows"""
        return _record_base_windows(self._dev("ribbit_hip_record_base_windows"), window)

    def record_primers(self, intervals, targets, params: PrimerParams | None = None) -> np.ndarray:
        """A forward and a reverse primer in the flanks of every target of the loaded record on the GPU, clear of the rows
        `intervals` (ribbit_hip_record_primers); see host_record_primers"""
        return _record_primers(self._dev("ribbit_hip_record_primers"), intervals, targets, params)

    def record_primer_pairs(self, intervals, targets, params: PrimerParams | None = None, pair_params: PrimerPairParams | None = None) -> np.ndarray:
        """The two primers of every target of the loaded record chosen as a pair on the GPU, checked for dimers and hairpins
        (ribbit_hip_record_primer_pairs); see host_record_primer_pairs"""
        return _record_primer_pairs(self._dev("ribbit_hip_record_primer_pairs"), intervals, targets, params, pair_params)

    def record_oligo_sites(self, oligos, params: ProductParams | None = None):
        """Where every oligo (text, 5' to 3') primes on either strand of the loaded record, on the GPU: equal oligos are searched
        once, the record's bit planes are read once (ribbit_hip_record_oligo_sites); see host_record_oligo_sites.  Counts add up
        over records: for a genome, load each record in turn and sum."""
        return _record_oligo_sites(self._dev("ribbit_hip_record_oligo_sites"), oligos, params)

    def record_primer_products(self, pairs, params: ProductParams | None = None) -> np.ndarray:
        """An in-silico PCR of every primer pair on the loaded record, on the GPU (ribbit_hip_record_primer_products); see
        host_record_primer_products"""
        return _record_primer_products(self._dev("ribbit_hip_record_primer_products"), pairs, params)

    def record_pair_amplicons(self, pairs, motifs, record: int = 0, params: ProductParams | None = None) -> np.ndarray:
        """Every primer pair typed on the loaded record, which may be any record, on the GPU (ribbit_hip_record_pair_amplicons); see
        host_record_pair_amplicons"""
        return _record_pair_amplicons(self._dev("ribbit_hip_record_pair_amplicons"), pairs, motifs, record, params)

    def panel_pools(self, pairs, extra=None, params: PanelParams | None = None):
        """The pairs pooled into multiplex panels on the GPU (ribbit_hip_panel_pools): the conflict matrix, the order and the first
        fit; no record need be loaded; see host_panel_pools"""
        return _panel_pools(self._dev("ribbit_hip_panel_pools"), pairs, extra, params)

    def marker_alleles(self, cells, designed, motif_lengths) -> np.ndarray:
        """Every marker's alleles over the samples on the GPU (ribbit_hip_marker_alleles): one wavefront per marker, the typed sizes
        sorted in LDS; no record need be loaded; see host_marker_alleles"""
        return _marker_alleles(self._dev("ribbit_hip_marker_alleles"), cells, designed, motif_lengths)

    def debug_panel_conflicts(self, pairs, extra=None, params: PanelParams | None = None) -> np.ndarray:
        """The conflict matrix of the pairs as the kernel leaves it (ribbit_hip_debug_panel_conflicts; at most 8192 pairs) -> an
        (n, (n + 63) // 64) uint64 array: bit j % 64 of word j // 64 of row i is the conflict of i and j"""
        rw, ex, ex_ptr, params = _panel_args(pairs, extra, params)
        words = np.zeros((len(rw), (len(rw) + 63) // 64), dtype=np.uint64)
        _call(self._dev("ribbit_hip_debug_panel_conflicts"), _ptr(rw), ex_ptr, len(rw), C.byref(params), words.ctypes.data if words.size else None)
        return words

    def record_specific_primer_pairs(self, intervals, targets, params: PrimerParams | None = None, pair_params: PrimerPairParams | None = None,
                                     product_params: ProductParams | None = None):
        """The best primer pair of every target of the loaded record that amplifies nothing else in it, on the GPU: all pairs of the
        two shortlists judged by an in-silico PCR, a wavefront per target (ribbit_hip_record_specific_primer_pairs); see
        host_record_specific_primer_pairs"""
        return _record_specific_primer_pairs(self._dev("ribbit_hip_record_specific_primer_pairs"), intervals, targets, params, pair_params, product_params)

    def record_primer_shortlists(self, intervals, targets, params: PrimerParams | None = None, pair_params: PrimerPairParams | None = None) -> np.ndarray:
        """The two shortlists of every target of the loaded record, on the GPU, in a form that leaves the record
        (ribbit_hip_record_primer_shortlists); see host_record_primer_shortlists"""
        return _record_primer_shortlists(self._dev("ribbit_hip_record_primer_shortlists"), intervals, targets, params, pair_params)

    def record_shortlist_verdicts(self, lists, home, pair_params: PrimerPairParams | None = None, product_params: ProductParams | None = None) -> np.ndarray:
        """Every admissible pair of every target's shortlists judged on the loaded record, which may be any record, on the GPU: one
        site scan per batch of targets, a wavefront per target (ribbit_hip_record_shortlist_verdicts); see
        host_record_shortlist_verdicts"""
        return _record_shortlist_verdicts(self._dev("ribbit_hip_record_shortlist_verdicts"), lists, home, pair_params, product_params)

    def record_best(self, intervals):
        """The loaded record's best non-overlapping rows on the GPU (ribbit_hip_record_best); see host_record_best"""
        return _record_best(self._dev("ribbit_hip_record_best"), intervals)

    def record_classes(self, intervals, motifs, offsets=None):
        """The loaded record's rows by canonical motif class on the GPU (ribbit_hip_record_classes); see host_record_classes"""
        return _record_classes(self._dev("ribbit_hip_record_classes"), intervals, motifs, offsets)

    def record_compounds(self, intervals, labels, gap: int = 100):
        """The loaded record's rows chained into compound loci on the GPU (ribbit_hip_record_compounds); see host_record_compounds"""
        return _record_compounds(self._dev("ribbit_hip_record_compounds"), intervals, labels, gap)

    def record_interruptions(self, intervals, motif_lengths, cigars, offsets=None):
        """The loaded record's rows' CIGARs decoded on the GPU (ribbit_hip_record_interruptions); see host_record_interruptions"""
        return _record_interruptions(self._dev("ribbit_hip_record_interruptions"), intervals, motif_lengths, cigars, offsets)

    def record_density(self, intervals, window: int) -> np.ndarray:
        """The loaded record's covered bases per window on the GPU (ribbit_hip_record_density); see host_record_density"""
        return _record_density(self._dev("ribbit_hip_record_density"), intervals, window)

    def debug_set_repeat_text_budget(self, nbytes: int) -> None:
        """the text budget of one ribbit_hip_repeat_sequences call in bytes (0: the default, 64 MiB)"""
        self._check(self._L.ribbit_hip_debug_set_repeat_text_budget(self._h, int(nbytes)))

    def debug_set_specific_batch(self, targets: int) -> None:
        """the targets of one batch of record_specific_primer_pairs (0: as many as 256 MiB of site lists hold)"""
        self._check(self._L.ribbit_hip_debug_set_specific_batch(self._h, int(targets)))

    def debug_set_small_record_capacity(self, records: int) -> None:
        """records the arena of small_motifs holds (0 = automatic); seeds that find it full get flags 2 and go to the host twin"""
        self._check(self._L.ribbit_hip_debug_set_small_record_capacity(self._h, int(records)))

    def adopt_dispatch(self, seeds) -> None:
        """ribbit_hip_adopt_dispatch: this handle (same record loaded) refines a slice of another handle's dispatch list"""
        d = np.ascontiguousarray(seeds, dtype=SEED_DT)
        self._check(self._L.ribbit_hip_adopt_dispatch(self._h, d.ctypes.data, len(d)))

    def refine_met_empty_query(self) -> bool:
        return bool(self._L.ribbit_hip_refine_met_empty_query(self._h))

    def guard_hits(self) -> int:
        return int(self._L.ribbit_hip_guard_hits(self._h))

    # chunk-sharded operation --------------------------------------------------------------
    def perfect_runs_partial(self, own_lo: int, own_hi: int, pos_offset: int = 0):
        """-> (complete runs of this chunk, unmatched edge events as uint64)"""
        r, nr, hv, nh = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self._check(self._L.ribbit_hip_perfect_runs_partial(self._h, own_lo, own_hi, pos_offset, C.byref(r), C.byref(nr), C.byref(hv), C.byref(nh)))
        return _copy(r.value, nr.value, RUN_DT), _copy(hv.value, nh.value, np.dtype("<u8"))

    def scan_perfect_chunk(self, own_lo: int, own_hi: int, pos_offset: int = 0, out: np.ndarray | None = None,
                           halves_out: np.ndarray | None = None):
        """ribbit_hip_scan_perfect_chunk: device-paired run records of one chunk.
        Without out -> (read-only view of the library's pinned run records, copy of the halves).
        With out / halves_out (RUN_DT arrays to fill in place, e.g. over registered shared memory) -> (n, n_halves).
        Records with term == RUN_NOT_OWNED are place holders to skip."""
        p, n, hp, nh = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        if out is not None:
            assert out.dtype == RUN_DT and out.flags.c_contiguous and halves_out is not None and halves_out.dtype == RUN_DT
            self._check(self._L.ribbit_hip_scan_perfect_chunk(self._h, own_lo, own_hi, pos_offset, out.ctypes.data, len(out),
                                                              halves_out.ctypes.data, len(halves_out),
                                                              C.byref(p), C.byref(n), C.byref(hp), C.byref(nh)))
            return n.value, nh.value
        self._check(self._L.ribbit_hip_scan_perfect_chunk(self._h, own_lo, own_hi, pos_offset, None, 0, None, 0,
                                                          C.byref(p), C.byref(n), C.byref(hp), C.byref(nh)))
        halves = _copy(hp.value, nh.value, RUN_DT)
        if n.value == 0:
            return np.zeros(0, RUN_DT), halves
        view = np.frombuffer((C.c_char * (n.value * RUN_DT.itemsize)).from_address(p.value), dtype=RUN_DT)
        view.flags.writeable = False
        return view, halves

    def scan_perfect_begin(self, own_lo: int = 0, own_hi: int = (1 << 63) - 1, pos_offset: int = 0) -> None:
        """Enqueue the perfect scan of the loaded record (or of one chunk of it) and return without waiting."""
        self._check(self._L.ribbit_hip_scan_perfect_begin(self._h, own_lo, own_hi, pos_offset))

    def scan_perfect_end_device(self):
        """Finish the scan begun by scan_perfect_begin WITHOUT copying anything to the host:
        -> (device pointer of the run records, their number, device pointer of the half records, their number).
        The memory is the handle's and stays valid until its next scan (ribbit_hip_scan_perfect_end_device)."""
        p, n, hp, nh = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self._check(self._L.ribbit_hip_scan_perfect_end_device(self._h, C.byref(p), C.byref(n), C.byref(hp), C.byref(nh)))
        return p.value or 0, n.value, hp.value or 0, nh.value

    def scan_perfect_wait(self) -> None:
        self._check(self._L.ribbit_hip_scan_perfect_wait(self._h))

    def scan_perfect_end(self, out: np.ndarray | None = None, halves_out: np.ndarray | None = None, wait: bool = True):
        """Finish the scan begun by scan_perfect_begin; returns like scan_perfect_chunk.  wait=False: the records
        (and halves) are still in flight until scan_perfect_wait(); halves are then returned as a view, not a copy."""
        p, n, hp, nh = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        if out is not None:
            assert out.dtype == RUN_DT and out.flags.c_contiguous and halves_out is not None and halves_out.dtype == RUN_DT
            self._check(self._L.ribbit_hip_scan_perfect_end(self._h, out.ctypes.data, len(out), halves_out.ctypes.data, len(halves_out),
                                                            int(wait), C.byref(p), C.byref(n), C.byref(hp), C.byref(nh)))
            return n.value, nh.value
        self._check(self._L.ribbit_hip_scan_perfect_end(self._h, None, 0, None, 0, int(wait), C.byref(p), C.byref(n), C.byref(hp), C.byref(nh)))
        if wait or nh.value == 0:
            halves = _copy(hp.value, nh.value, RUN_DT)
        else:
            halves = np.frombuffer((C.c_char * (nh.value * RUN_DT.itemsize)).from_address(hp.value), dtype=RUN_DT)
        if n.value == 0:
            return np.zeros(0, RUN_DT), halves
        view = np.frombuffer((C.c_char * (n.value * RUN_DT.itemsize)).from_address(p.value), dtype=RUN_DT)
        view.flags.writeable = False
        return view, halves

    def ssw_passes(self, jobs: np.ndarray, motif_pool: bytes, mask_len: int = 15) -> np.ndarray:
        """ribbit_hip_ssw_passes: the striped passes of every job (JOB_DT) on the GPU -> ENDS_DT records."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DT)
        out = np.zeros(len(jobs), ENDS_DT)
        self._check(self._L.ribbit_hip_ssw_passes(self._h, jobs.ctypes.data, len(jobs), motif_pool, len(motif_pool), mask_len, out.ctypes.data))
        return out

    def ssw_align_jobs(self, jobs: np.ndarray, motif_pool: bytes, mask_len: int = 15):
        """ribbit_hip_ssw_align_jobs: whole alignments, passes and path search on the GPU where the kernels take them.
        -> (list of (result dict, cigar string), on_gpu array: 0 host, 1 passes on the GPU, 2 passes and path)"""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DT)
        n = len(jobs)
        out = (Alignment * max(n, 1))()
        cap = int(16 * (jobs["query_length"].astype(np.int64) + jobs["ppr_length"]).sum()) + 64 * n + 64
        buf = C.create_string_buffer(cap)
        off = np.zeros(max(n, 1), dtype=np.int64)
        on_gpu = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self._L.ribbit_hip_ssw_align_jobs(self._h, jobs.ctypes.data, n, motif_pool, len(motif_pool), mask_len, out, buf, cap,
                                                      off.ctypes.data, on_gpu.ctypes.data))
        res = []
        for j in range(n):
            res.append(({name: getattr(out[j], name) for name, _ in Alignment._fields_}, C.string_at(C.addressof(buf) + int(off[j])).decode()))
        return res, on_gpu[:n]

    def host_register(self, address: int, nbytes: int) -> None:
        """Page-lock caller-owned host memory so that scan_perfect_chunk(out=...) DMAs straight into it."""
        self._check(self._L.ribbit_hip_host_register(address, nbytes))

    def host_unregister(self, address: int) -> None:
        self._check(self._L.ribbit_hip_host_unregister(address))

    def stage_calls_chunk(self, stage: int, own_lo: int, own_hi: int, pos_offset: int, record_length: int) -> dict:
        """ribbit_hip_stage_calls_chunk: the kept calls of one window stage (STAGE_SUBST / STAGE_ANCHORED) of the loaded
        piece, in record coordinates -> dict(calls, pend (or None), tail_pend, flush, inexact, streaks) (copies)"""
        cc = ChunkCalls()
        self._check(self._L.ribbit_hip_stage_calls_chunk(self._h, stage, own_lo, min(own_hi, (1 << 62)), pos_offset, record_length, C.byref(cc)))
        return {"calls": _copy(cc.calls, cc.n, CALL_DT), "pend": _copy(cc.pend, cc.n, _I4) if cc.pend else None,
                "tail_pend": int(cc.tail_pend), "flush": _copy(cc.flush, cc.n_flush, CALL_DT), "inexact": bool(cc.inexact),
                "streaks": int(cc.streaks)}

    def xa_words_into(self, word_lo: int, word_hi: int, out: np.ndarray, out_word: int) -> None:
        """ribbit_hip_xa_words_strided: this piece's words [word_lo, word_hi) of every composed plane into out[:, out_word:...]
        (out: (motifs, stride) uint32, C-contiguous -- e.g. the record's planes in a segment every rank maps)"""
        assert out.dtype == np.dtype("<u4") and out.flags.c_contiguous and out.ndim == 2
        assert out_word >= 0 and out_word + (word_hi - word_lo) <= out.shape[1]
        self._check(self._L.ribbit_hip_xa_words_strided(self._h, word_lo, word_hi, out.ctypes.data + 4 * out_word, out.shape[1]))

    def xa_words(self, word_lo: int, word_hi: int):
        nm = self.params.max_motif - self.params.min_motif + 1
        out = np.empty((nm, max(word_hi - word_lo, 0)), dtype="<u4")
        self._check(self._L.ribbit_hip_xa_words(self._h, word_lo, word_hi, out.ctypes.data_as(C.c_void_p)))
        return out

    # plane access -----------------------------------------------------------------------
    def plane_bits(self, shift: int, start: int = 0, end: int | None = None):
        end = self.length if end is None else end
        out = np.empty(max(end - start, 0), dtype=np.uint8)
        self._check(self._L.ribbit_hip_plane_bits(self._h, shift, start, end, out.ctypes.data_as(C.c_void_p)))
        return out

    def range_popcount(self, shift: int, start: int, end: int) -> int:
        c = C.c_int32()
        self._check(self._L.ribbit_hip_range_popcount(self._h, shift, start, end, C.byref(c)))
        return c.value

    def packed_plane(self, which: int):
        n = self._L.ribbit_hip_plane_words(self._h)
        out = np.empty(n, dtype=np.uint32)
        self._check(self._L.ribbit_hip_packed_plane(self._h, which, out.ctypes.data_as(C.c_void_p)))
        return out

    def timing_ms(self, what: int) -> float:
        ms = C.c_double()
        self._check(self._L.ribbit_hip_last_timing_ms(self._h, what, C.byref(ms)))
        return ms.value

    def debug_stream_read(self, nbytes: int) -> int:
        n = C.c_int64()
        self._check(self._L.ribbit_hip_debug_stream_read(self._h, nbytes, C.byref(n)))
        return n.value

    def last_event_count(self) -> int:
        return int(self._L.ribbit_hip_last_event_count(self._h))
