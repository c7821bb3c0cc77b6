"""ctypes binding of the C-ABI (include/kmx.h) — plumbing for tests, bench.py and smoke().  Three parts, in this order: the binding
itself (the structures, SIGNATURES, lib()); Result and the handle classes of the mapping chain (_Handle and its subclasses, whose
host() views are named tuples of the fields each class declares); Index with the chain builders.  The SAM text written from those
views is sam.py, pure numpy; its names are re-exported here, and the handles' string methods pass their host views to it.

Every search goes through libkmx.so (hand-written gfx950 kernels).  There is no Python or
CPU search path in this package: when the library or a device is missing, calls raise.
"""
import collections
import contextlib
import ctypes as C
import os

import numpy as np

from . import build as _build
from .sam import (CIGAR_OPS, NO_CONTIG, PAIR_CONCORDANT, _clip_fields, _first_given, _letters_table, _runs_strings,  # noqa: F401
                  concat_sequences, sa_strings, sam_header, sam_lines, sam_pair_fields, sam_supplementary_lines, supplementary_mapq, xa_strings)

KMX_MAX_KS = 32
KMX_MAX_DEVICES = 16
KMX_N_KERNELS = 16
TABLE_AUTO, TABLE_OPEN, TABLE_DENSE = 0, 1, 2
SEARCH_DEFAULT, SEARCH_KEEP_MASKS, SEARCH_COUNT_ONLY, SEARCH_ASYNC, SEARCH_REFERENCE_PLAN = 0, 1, 2, 4, 8
KIND_NONE, KIND_EXACT, KIND_STITCH, KIND_PREFIX = 0, 1, 2, 3
Q_OK, Q_TOO_LONG, Q_SUBK_FANOUT, Q_EMPTY_QUERY, Q_BAD_RANK, Q_TOO_SHORT = 0, 1, 2, 3, 4, 5
APPROX_MAX_SUBST = 3
APPROX_EDIT = 1
APPROX_LOCI, APPROX_BEST = 2, 4
TILE_Q_NONE, TILE_Q_PARTITION, TILE_Q_SCAN = 0, 1, 2
ALIGN_MAX_EDITS, ALIGN_MAX_READ, ALIGN_SKIPPED, ALIGN_NONE = 250, 1024, 254, 255
SCRIPT_ALL, SCRIPT_M = 1, 2
PAIR_FR, PAIR_RF, PAIR_FF = 0, 1, 2
PAIR_UNPLACED, PAIR_DISCORDANT, PAIR_MATE1_ONLY, PAIR_MATE2_ONLY = 0, 2, 3, 4         # (PAIR_CONCORDANT = 1, CIGAR_OPS, NO_CONTIG: from sam.py)
PAIR_NO_PENALTY, PAIR_NO_SCORE = 0xFFFFFFFF, 0xFFFF
RESCUE_DISCORDANT, RESCUE_MAX_INSERT = 1, 65536
RESCUE_NONE, RESCUE_FOUND, RESCUE_CONCORDANT, RESCUE_TAKEN = 0, 1, 2, 3
LOCATE_MATES = 1
SECONDARY_MAX, SECONDARY_NO_DELTA = 32, 0xFFFFFFFF
CLIP_LOW, CLIP_REALIGNED = 1, 2
SUPPLEMENTARY_MAX = 8
PILEUP_ADD, PILEUP_SKIP_LOW = 1, 2
PILEUP_AUTO, PILEUP_ATOMIC, PILEUP_TILED = 0, 1, 2


class KmxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"kmx status {status}: {msg}")
        self.status = status


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("table_kind", C.c_uint32),
                ("n_threads", C.c_uint32), ("query_size_range", C.c_uint32), ("keep_host_arena", C.c_uint32),
                ("host_flatten", C.c_uint32), ("no_aligned_copy", C.c_uint32),
                ("n_devices", C.c_uint32), ("devices", C.c_int32 * KMX_MAX_DEVICES), ("prefix_levels", C.c_int32)]


class ApproxOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_subst", C.c_uint32), ("flags", C.c_uint32), ("max_hits", C.c_uint32),
                ("complement", C.c_void_p)]


class WindowOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("w", C.c_uint32), ("stride", C.c_uint32), ("flags", C.c_uint32)]


class VoteOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("band", C.c_uint32), ("min_votes", C.c_uint32), ("max_occ", C.c_uint32), ("flags", C.c_uint32)]


class AlignOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_edits", C.c_uint32), ("max_span", C.c_uint32), ("flags", C.c_uint32)]


class ScriptOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("scratch_bytes", C.c_uint64)]


class FoldOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32)]


class PairOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_insert", C.c_uint32), ("max_insert", C.c_uint32), ("orientation", C.c_uint32),
                ("unpaired_penalty", C.c_uint32), ("flags", C.c_uint32)]


class RescueOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_insert", C.c_uint32), ("max_insert", C.c_uint32), ("orientation", C.c_uint32),
                ("max_edits", C.c_uint32), ("unpaired_penalty", C.c_uint32), ("segment", C.c_uint32), ("flags", C.c_uint32)]


class MdOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32)]


class MapqOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_edits", C.c_uint32), ("cap", C.c_uint32), ("per_edit", C.c_uint32),
                ("pair_bonus", C.c_uint32), ("flags", C.c_uint32)]


class LocateOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32)]


class SecondaryOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_secondary", C.c_uint32), ("max_delta", C.c_uint32), ("flags", C.c_uint32)]


class ClipOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("match", C.c_uint32), ("mismatch", C.c_uint32), ("gap_open", C.c_uint32),
                ("gap_extend", C.c_uint32), ("clip_penalty", C.c_uint32), ("min_score", C.c_int32), ("flags", C.c_uint32)]


class RealignOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("match", C.c_uint32), ("mismatch", C.c_uint32), ("gap_open", C.c_uint32),
                ("gap_extend", C.c_uint32), ("clip_penalty", C.c_uint32), ("min_score", C.c_int32), ("flags", C.c_uint32),
                ("scratch_bytes", C.c_uint64)]


class SupplementaryOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_supplementary", C.c_uint32), ("min_len", C.c_uint32), ("max_overlap", C.c_uint32),
                ("min_score", C.c_int32), ("flags", C.c_uint32)]


class PileupOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("lo", C.c_uint64), ("hi", C.c_uint64), ("min_score", C.c_int32),
                ("min_mapq", C.c_uint32), ("mode", C.c_uint32), ("tile", C.c_uint32)]


class SitesOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("frac_num", C.c_uint32), ("frac_den", C.c_uint32)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class IndexPathInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("fill_slots", C.c_uint32), ("fill_nontemporal", C.c_uint32), ("rec64", C.c_uint32),
                ("tiny_cells", C.c_uint32), ("scan_tile", C.c_uint32), ("n_ks", C.c_uint32), ("cell_shift", C.c_uint32 * KMX_MAX_KS),
                ("windows_tile", C.c_uint32)]


class ResultPathInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("small", C.c_uint32), ("lookup_items", C.c_uint32), ("lookup_pairs", C.c_uint32),
                ("deferred_long", C.c_uint32), ("tile_q_source", C.c_uint32), ("spec_fill", C.c_uint32), ("spec_ok", C.c_uint32),
                ("fill_blocks", C.c_uint32), ("fill_tiles", C.c_uint32),
                ("prefix_plain", C.c_uint32), ("prefix_small", C.c_uint32), ("prefix_merge_small", C.c_uint32), ("prefix_mid", C.c_uint32),
                ("prefix_long", C.c_uint32), ("prefix_large_chunks", C.c_uint32), ("prefix_large_elems", C.c_uint64)]


vp, u64, u32, i32, st, P = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int, C.POINTER

# every symbol include/kmx.h declares: (restype, argtypes); st is a kmx_status.  lib() applies it, tests/test_capi_cpu.py holds the
# number of argtypes against the header's prototypes.
SIGNATURES = {
    "kmx_index_build": (st, [vp, u64, u32, vp, u32, P(Options), P(vp)]),
    "kmx_index_free": (None, [vp]),
    "kmx_index_save": (st, [vp, C.c_char_p]),
    "kmx_index_load": (st, [C.c_char_p, P(Options), P(vp)]),
    "kmx_index_info": (st, [vp, P(u64), P(u32), P(u32), vp, vp, P(u64)]),
    "kmx_index_memory": (st, [vp] + [P(u64)] * 5),
    "kmx_index_arena_host": (st, [vp, P(vp), P(u64)]),
    "kmx_index_extend_query_size_range": (st, [vp, u32]),
    "kmx_index_devices": (st, [vp, P(u32), vp]),
    "kmx_index_bucket_host": (st, [vp, u32, vp, P(vp), P(u32)]),
    "kmx_index_levels": (st, [vp, vp]),
    "kmx_index_paths": (st, [vp, P(IndexPathInfo)]),
    "kmx_index_text": (st, [vp, vp, u64, P(u64)]),
    "kmx_index_set_contigs": (st, [vp, vp, u64]),
    "kmx_index_contigs": (st, [vp, P(u64), vp, u64]),
    "kmx_choose_best_k": (st, [vp, u64, u32, vp]),
    "kmx_plan": (st, [vp, u32, u32, vp, vp, vp, u64, P(u64)]),
    "kmx_plan_engine": (st, [vp, u32, u32, u32, vp]),
    "kmx_fast_pow": (u64, [u64, C.c_uint8]),
    "kmx_stats_enable": (st, [vp, C.c_int]),
    "kmx_stats_get": (st, [vp, P(KernelStat), P(u32)]),
    "kmx_stats_reset": (st, [vp]),
    "kmx_debug_words": (st, [vp, vp]),
    "kmx_last_error": (C.c_char_p, []),
    "kmx_status_string": (C.c_char_p, [C.c_int]),
    "kmx_version": (u32, []),
    # exact search
    "kmx_search_batch": (st, [vp, vp, vp, u64, u32, P(vp)]),
    "kmx_search_batch_device": (st, [vp, vp, vp, u64, u32, vp, P(vp)]),
    "kmx_search_windows": (st, [vp, vp, vp, u64, P(WindowOptions), P(vp)]),
    "kmx_search_windows_device": (st, [vp, vp, vp, u64, P(WindowOptions), vp, P(vp)]),
    "kmx_result_counts": (st, [vp] + [P(u64)] * 6),
    "kmx_result_view": (st, [vp] + [P(vp)] * 4),
    "kmx_result_view_device": (st, [vp] + [P(vp)] * 3),
    "kmx_result_masks": (st, [vp] + [P(vp)] * 4),
    "kmx_result_parts": (st, [vp, P(u32)]),
    "kmx_result_part_view_device": (st, [vp, u32, P(i32), P(u64), P(u64), P(vp), P(vp), P(vp)]),
    "kmx_result_gather_device": (st, [vp, i32, P(vp), P(vp), P(vp)]),
    "kmx_result_paths": (st, [vp, P(ResultPathInfo)]),
    "kmx_result_window_offsets": (st, [vp, P(vp), P(vp), P(u64)]),
    "kmx_result_free": (None, [vp]),
    # approximate search
    "kmx_search_approx": (st, [vp, vp, vp, u64, u32, u32, P(vp)]),
    "kmx_search_approx_strands": (st, [vp, vp, vp, u64, u32, u32, vp, P(vp)]),
    "kmx_search_approx_opts": (st, [vp, vp, vp, u64, P(ApproxOptions), P(vp)]),
    "kmx_approx_counts": (st, [vp, P(u64), P(u64), P(u64), P(u32)]),
    "kmx_approx_view": (st, [vp] + [P(vp)] * 4),
    "kmx_approx_lengths": (st, [vp, P(vp)]),
    "kmx_approx_strands": (st, [vp, P(vp)]),
    "kmx_approx_found": (st, [vp, P(vp)]),
    "kmx_approx_free": (None, [vp]),
    # the read-mapping chain: vote, align, scripts
    "kmx_windows_vote": (st, [vp, P(VoteOptions), P(vp)]),
    "kmx_loci_counts": (st, [vp] + [P(u64)] * 5),
    "kmx_loci_view": (st, [vp] + [P(vp)] * 5),
    "kmx_loci_view_device": (st, [vp] + [P(vp)] * 5),
    "kmx_loci_free": (None, [vp]),
    "kmx_loci_align": (st, [vp, vp, vp, vp, u64, P(AlignOptions), P(vp)]),
    "kmx_loci_align_device": (st, [vp, vp, vp, vp, u64, P(AlignOptions), vp, P(vp)]),
    "kmx_alignments_counts": (st, [vp] + [P(u64)] * 4),
    "kmx_alignments_view": (st, [vp] + [P(vp)] * 5),
    "kmx_alignments_view_device": (st, [vp] + [P(vp)] * 5),
    "kmx_alignments_contigs_view": (st, [vp, P(vp), P(u64)]),
    "kmx_alignments_contigs_view_device": (st, [vp, P(vp), P(u64)]),
    "kmx_alignments_free": (None, [vp]),
    "kmx_alignments_scripts": (st, [vp, vp, vp, vp, vp, u64, P(ScriptOptions), P(vp)]),
    "kmx_alignments_scripts_device": (st, [vp, vp, vp, vp, vp, u64, P(ScriptOptions), vp, P(vp)]),
    "kmx_scripts_counts": (st, [vp] + [P(u64)] * 4),
    "kmx_scripts_view": (st, [vp] + [P(vp)] * 4),
    "kmx_scripts_view_device": (st, [vp] + [P(vp)] * 4),
    "kmx_scripts_free": (None, [vp]),
    # both strands, pairs, rescue
    "kmx_reads_strands": (st, [vp, vp, vp, u64, vp, P(vp)]),
    "kmx_reads_strands_device": (st, [vp, vp, vp, u64, vp, vp, P(vp)]),
    "kmx_strand_reads_view_device": (st, [vp, P(vp), P(vp), P(u64), P(vp)]),
    "kmx_strand_reads_free": (None, [vp]),
    "kmx_alignments_fold_strands": (st, [vp, vp, P(FoldOptions), vp, P(vp)]),
    "kmx_placements_counts": (st, [vp] + [P(u64)] * 4),
    "kmx_placements_view": (st, [vp] + [P(vp)] * 7),
    "kmx_placements_view_device": (st, [vp] + [P(vp)] * 7),
    "kmx_placements_free": (None, [vp]),
    "kmx_placements_scripts": (st, [vp, vp, vp, vp, vp, P(ScriptOptions), P(vp)]),
    "kmx_alignments_fold_pairs": (st, [vp, vp, P(PairOptions), vp, P(vp), P(vp)]),
    "kmx_pairs_counts": (st, [vp] + [P(u64)] * 6),
    "kmx_pairs_view": (st, [vp] + [P(vp)] * 4),
    "kmx_pairs_view_device": (st, [vp] + [P(vp)] * 4),
    "kmx_pairs_free": (None, [vp]),
    "kmx_pairs_rescue": (st, [vp, vp, vp, vp, P(RescueOptions), vp, vp, P(vp)]),
    "kmx_rescues_counts": (st, [vp] + [P(u64)] * 5),
    "kmx_rescues_view": (st, [vp] + [P(vp)] * 8),
    "kmx_rescues_view_device": (st, [vp] + [P(vp)] * 8),
    "kmx_rescues_scripts": (st, [vp, vp, vp, P(ScriptOptions), P(vp)]),
    "kmx_rescues_free": (None, [vp]),
    # SAM tags, contigs, secondaries, clips
    "kmx_scripts_md": (st, [vp, vp, vp, vp, P(MdOptions), vp, P(vp)]),
    "kmx_rescues_md": (st, [vp, vp, vp, vp, P(MdOptions), vp, P(vp)]),
    "kmx_md_counts": (st, [vp] + [P(u64)] * 3),
    "kmx_md_view": (st, [vp] + [P(vp)] * 2),
    "kmx_md_view_device": (st, [vp] + [P(vp)] * 2),
    "kmx_md_free": (None, [vp]),
    "kmx_placements_mapq": (st, [vp, vp, P(MapqOptions), vp, P(vp)]),
    "kmx_mapq_counts": (st, [vp] + [P(u64)] * 3),
    "kmx_mapq_view": (st, [vp, P(vp)]),
    "kmx_mapq_view_device": (st, [vp, P(vp)]),
    "kmx_mapq_free": (None, [vp]),
    "kmx_placements_locate": (st, [vp, vp, vp, P(LocateOptions), vp, P(vp)]),
    "kmx_located_counts": (st, [vp] + [P(u64)] * 3),
    "kmx_located_view": (st, [vp] + [P(vp)] * 2),
    "kmx_located_view_device": (st, [vp] + [P(vp)] * 2),
    "kmx_located_free": (None, [vp]),
    "kmx_placements_secondaries": (st, [vp, vp, vp, P(SecondaryOptions), vp, P(vp)]),
    "kmx_secondaries_counts": (st, [vp] + [P(u64)] * 4),
    "kmx_secondaries_view": (st, [vp] + [P(vp)] * 7),
    "kmx_secondaries_view_device": (st, [vp] + [P(vp)] * 7),
    "kmx_secondaries_scripts": (st, [vp, vp, vp, P(ScriptOptions), P(vp)]),
    "kmx_secondaries_md": (st, [vp, vp, vp, vp, P(MdOptions), vp, P(vp)]),
    "kmx_secondaries_free": (None, [vp]),
    "kmx_scripts_clip": (st, [vp, P(ClipOptions), vp, P(vp)]),
    "kmx_clips_counts": (st, [vp] + [P(u64)] * 4),
    "kmx_clips_view": (st, [vp] + [P(vp)] * 9),
    "kmx_clips_view_device": (st, [vp] + [P(vp)] * 9),
    "kmx_clips_md": (st, [vp, vp, vp, vp, vp, P(MdOptions), vp, P(vp)]),
    "kmx_clips_rescues_md": (st, [vp, vp, vp, vp, vp, P(MdOptions), vp, P(vp)]),
    "kmx_clips_free": (None, [vp]),
    "kmx_scripts_realign": (st, [vp, vp, vp, vp, vp, u64, P(RealignOptions), P(vp)]),
    "kmx_scripts_realign_device": (st, [vp, vp, vp, vp, vp, u64, P(RealignOptions), vp, P(vp)]),
    # supplementary alignments
    "kmx_clips_supplementaries": (st, [vp, vp, vp, vp, vp, vp, P(SupplementaryOptions), vp, P(vp)]),
    "kmx_supplementaries_counts": (st, [vp] + [P(u64)] * 4),
    "kmx_supplementaries_view": (st, [vp] + [P(vp)] * 13),
    "kmx_supplementaries_view_device": (st, [vp] + [P(vp)] * 13),
    "kmx_supplementaries_free": (None, [vp]),
    # pileup and sites
    "kmx_clips_pileup_device": (st, [vp, vp, vp, vp, vp, vp, u64, vp, P(PileupOptions), vp, P(vp)]),
    "kmx_clips_rescues_pileup": (st, [vp, vp, vp, vp, vp, vp, P(PileupOptions), vp, P(vp)]),
    "kmx_pileup_counts": (st, [vp, P(u64), P(u64), P(u32)] + [P(u64)] * 4),
    "kmx_pileup_view": (st, [vp, P(vp)]),
    "kmx_pileup_view_device": (st, [vp, P(vp)]),
    "kmx_pileup_free": (None, [vp]),
    "kmx_pileup_sites": (st, [vp, vp, P(SitesOptions), vp, P(vp)]),
    "kmx_sites_counts": (st, [vp] + [P(u64)] * 2),
    "kmx_sites_view": (st, [vp] + [P(vp)] * 7),
    "kmx_sites_view_device": (st, [vp] + [P(vp)] * 7),
    "kmx_sites_free": (None, [vp]),
}
EXPORTS = list(SIGNATURES)


_lib = None


def lib():
    """Loads kmer_index_amd/libkmx.so, building it first when stale (hipcc, gfx950)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7 and finds no GPU when another copy
        # (the /opt/rocm one libkmx.so links to) was mapped first.  Importing torch first makes both share torch's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = _build.build()
        if not os.path.exists(path):
            raise RuntimeError("libkmx.so is missing and could not be built; the engine has no fallback")
        L = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _set_devices(o, devices):
    if devices is None:
        o.n_devices = 0
        return
    devices = list(devices)
    if not 1 <= len(devices) <= KMX_MAX_DEVICES:
        raise ValueError("devices: between 1 and KMX_MAX_DEVICES ordinals")
    o.n_devices = len(devices)
    for i, d in enumerate(devices):
        o.devices[i] = int(d)
    o.device = int(devices[0])


def _check(st):
    if st != 0:
        raise KmxError(st, lib().kmx_last_error().decode())


# rank orders of include/kmer_index_amd/alphabet.hpp and the complement of each letter (dna15: the IUPAC codes)
_COMPLEMENT_CHARS = {4: ("ACGT", "TGCA"), 5: ("ACGNT", "TGCNA"), 15: ("ABCDGHKMNRSTVWY", "TVGHCDMKNYSABWR")}


def complement_table(sigma):
    """The rank-to-rank complement table (uint8[sigma]) of dna4 (ACGT), dna5 (ACGNT, N maps to N) or dna15 (IUPAC)."""
    if sigma not in _COMPLEMENT_CHARS:
        raise ValueError(f"complement_table: no natural complement for an alphabet of {sigma} letters; pass a table")
    chars, comp = _COMPLEMENT_CHARS[sigma]
    return np.array([chars.index(c) for c in comp], np.uint8)


def fast_pow(base, exp):
    return int(lib().kmx_fast_pow(base, exp))


def choose_best_k(lengths, n_k=4):
    """kmx_choose_best_k (choose_best_k.hpp): recommended ks for a set of query lengths."""
    lengths = np.ascontiguousarray(lengths, np.uint64)
    out = np.zeros(n_k, np.uint32)
    _check(lib().kmx_choose_best_k(lengths.ctypes.data, lengths.size, n_k, out.ctypes.data))
    return out.tolist()


def plan(ks, rng=10000):
    """(use_multi[rng] bool, nk_sum list of lists) from kmx_plan (host only, no device needed)."""
    ks = np.ascontiguousarray(ks, np.uint32)
    multi = np.zeros(rng, np.uint8)
    off = np.zeros(rng + 1, np.uint32)
    n = C.c_uint64()
    _check(lib().kmx_plan(ks.ctypes.data, ks.size, rng, multi.ctypes.data, off.ctypes.data, None, 0, C.byref(n)))
    flat = np.zeros(max(n.value, 1), np.uint32)
    _check(lib().kmx_plan(ks.ctypes.data, ks.size, rng, multi.ctypes.data, off.ctypes.data, flat.ctypes.data, n.value, C.byref(n)))
    return multi.astype(bool), [flat[off[q]:off[q + 1]].tolist() for q in range(rng)]


def plan_engine(ks, sigma, rng=10000):
    """k_used[rng] from kmx_plan_engine: the k whose element the ENGINE answers a single-k length from (0: multi-k scheme)."""
    ks = np.ascontiguousarray(ks, np.uint32)
    out = np.zeros(rng, np.uint32)
    _check(lib().kmx_plan_engine(ks.ctypes.data, ks.size, rng, int(sigma), out.ctypes.data))
    return out


def _view(ptr, n, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype)
    ct = np.ctypeslib.as_ctypes_type(dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(int(n),))


class Result:
    """Owns a kmx_result handle."""

    def __init__(self):
        self._h = C.c_void_p()
        self._index = None        # the Index of the last search: a pending (SEARCH_ASYNC) search reads it when it completes

    def n_parts(self):
        n = C.c_uint32()
        _check(lib().kmx_result_parts(self._h, C.byref(n)))
        return int(n.value)

    def part_device_ptrs(self, part):
        """(device ordinal, q_begin, q_end, d_hit_off, d_positions, d_status) of one part of a multi-device result;
        hit_off is local to the part."""
        dev, qb, qe = C.c_int32(), C.c_uint64(), C.c_uint64()
        a, b, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().kmx_result_part_view_device(self._h, part, C.byref(dev), C.byref(qb), C.byref(qe), C.byref(a), C.byref(b), C.byref(s)))
        return int(dev.value), int(qb.value), int(qe.value), a.value, b.value, s.value

    def counts(self):
        v = [C.c_uint64() for _ in range(6)]
        _check(lib().kmx_result_counts(self._h, *[C.byref(x) for x in v]))
        return dict(zip(["nq", "n_hits", "n_exact", "n_stitch", "n_prefix", "n_error"], [int(x.value) for x in v]))

    def paths(self):
        """kmx_result_paths: which kernel variants the last finished search into this result ran."""
        v = ResultPathInfo()
        v.struct_size = C.sizeof(ResultPathInfo)
        _check(lib().kmx_result_paths(self._h, C.byref(v)))
        return {"small": bool(v.small), "lookup_items": int(v.lookup_items), "lookup_pairs": bool(v.lookup_pairs),
                "deferred_long": bool(v.deferred_long), "tile_q_source": int(v.tile_q_source), "spec_fill": bool(v.spec_fill),
                "spec_ok": bool(v.spec_ok), "fill_blocks": int(v.fill_blocks), "fill_tiles": int(v.fill_tiles),
                "prefix_plain": int(v.prefix_plain), "prefix_small": int(v.prefix_small), "prefix_merge_small": int(v.prefix_merge_small),
                "prefix_mid": int(v.prefix_mid), "prefix_long": int(v.prefix_long), "prefix_large_chunks": int(v.prefix_large_chunks),
                "prefix_large_elems": int(v.prefix_large_elems)}

    def host(self, copy=True):
        """(hit_off[nq+1], positions, status[nq], kinds[nq]) as numpy arrays: copies, or with copy=False views of the
        result's own host buffers (valid until the result is searched into again or closed)."""
        c = self.counts()
        a, b, s, k = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().kmx_result_view(self._h, C.byref(a), C.byref(b), C.byref(s), C.byref(k)))
        nq = c["nq"]
        hit_off = _view(a.value, nq + 1, np.uint64)
        n_pos = int(hit_off[nq]) if b.value else 0        # positions are NULL for COUNT_ONLY results
        out = (hit_off, _view(b.value, n_pos, np.uint32), _view(s.value, nq, np.uint8), _view(k.value, nq, np.uint8))
        return tuple(x.copy() for x in out) if copy else out

    def device_ptrs(self):
        a, b, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().kmx_result_view_device(self._h, C.byref(a), C.byref(b), C.byref(s)))
        return a.value, b.value, s.value

    def device_tensors(self, device):
        """(hit_off int64 [nq+1], positions int32 [n_hits]) as torch tensors aliasing the result's HBM buffers."""
        import torch

        class _Arr:
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}

        c = self.counts()
        a, b, _ = self.device_ptrs()
        t_off = torch.as_tensor(_Arr(a, c["nq"] + 1, "<i8"), device=device)
        t_pos = torch.as_tensor(_Arr(b, c["n_hits"], "<i4"), device=device) if c["n_hits"] else torch.empty(0, dtype=torch.int32, device=device)
        return t_off, t_pos

    def gather_device(self, dst_device):
        """kmx_result_gather_device: (d_hit_off, d_positions, d_status) of the whole batch in the HBM of dst_device."""
        a, b, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().kmx_result_gather_device(self._h, int(dst_device), C.byref(a), C.byref(b), C.byref(s)))
        return a.value, b.value, s.value

    def window_offsets(self, device=False):
        """kmx_result_window_offsets of a windows search: win_off[nr+1] as a numpy array (window j of read r is query
        win_off[r] + j); device=True: (win_off, device pointer of the same array, nr)."""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(lib().kmx_result_window_offsets(self._h, C.byref(a), C.byref(b), C.byref(n)))
        win_off = _view(a.value, n.value + 1, np.uint64).copy()
        return (win_off, b.value, int(n.value)) if device else win_off

    def vote(self, band=0, min_votes=1, max_occ=0, loci=None):
        """kmx_windows_vote on the result of a windows search: the candidate loci of every read (a Loci; `loci` reuses one)."""
        l = loci or Loci()
        o = VoteOptions(C.sizeof(VoteOptions), int(band), int(min_votes), int(max_occ), 0)
        _check(lib().kmx_windows_vote(self._h, C.byref(o), C.byref(l._h)))
        return l

    def masks(self):
        c = self.counts()
        a, b, cc, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().kmx_result_masks(self._h, C.byref(a), C.byref(b), C.byref(cc), C.byref(d)))
        nq = c["nq"]
        base = _view(a.value, nq, np.uint64).copy()
        cnt = _view(cc.value, nq, np.uint32).copy()
        src = _view(d.value, nq, np.uint64).copy()
        return base, b.value, cnt, src

    def close(self):
        if self._h:
            lib().kmx_result_free(self._h)
            self._h = C.c_void_p()
        self._index = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    """What the owners of a C handle share: the empty handle, close() through the class's free function, and counts(), host() and
    device_ptrs() from what the class declares:

    _counts_of = (the kmx_*_counts function, the names of its out-parameters in order): counts() is a dict under those names.
    _view_of = (stem, fields): kmx_<stem>_view fills one host pointer per field and kmx_<stem>_view_device one device pointer;
        a field is (name, dtype, length), the length a name of counts() or a function of that dict.  host() is the named tuple of
        the fields as numpy copies, device_ptrs() the tuple of the device pointers, both in the order of the fields.
    _optional = the names of the fields that the C view may hand out as NULL for "not there": host() has None for such a field."""

    _free = None                    # the name of the handle's kmx_*_free
    _counts_of = None
    _view_of = None
    _optional = ()
    _view_types = {}                # (class, number of fields): the named tuple of that prefix of the class's fields

    def __init__(self):
        self._h = C.c_void_p()
        self._reads = None          # the StrandReads whose stream the handle was filled on: it must outlive the views

    def counts(self):
        fn, names = self._counts_of
        v = [p._type_() for p in SIGNATURES[fn][1][1:]]
        _check(getattr(lib(), fn)(self._h, *[C.byref(x) for x in v]))
        return dict(zip(names, [int(x.value) for x in v]))

    def _ptrs(self, fn, n, n_null=0):
        """The first n out-parameters of a view function, which are pointers; NULL goes in for n_null further ones."""
        p = [C.c_void_p() for _ in range(n)]
        _check(getattr(lib(), fn)(self._h, *[C.byref(x) for x in p], *[None] * n_null))
        return tuple(x.value for x in p)

    def _arrays(self, ptrs):
        """Copies of the fields that the host pointers `ptrs` (those of the first len(ptrs) fields) point at, under their names."""
        c = self.counts()
        fields = self._view_of[1][:len(ptrs)]
        key = (type(self), len(fields))
        if key not in self._view_types:
            self._view_types[key] = collections.namedtuple(f"{type(self).__name__}View", [name for name, _, _ in fields])
        return self._view_types[key](*(None if name in self._optional and not p else _view(p, n(c) if callable(n) else c[n], dtype).copy()
                                       for p, (name, dtype, n) in zip(ptrs, fields)))

    def host(self):
        """The fields of _view_of as numpy copies under their names, in their order."""
        stem, fields = self._view_of
        return self._arrays(self._ptrs(f"kmx_{stem}_view", len(fields)))

    def device_ptrs(self):
        """The device pointer of every field of _view_of, in their order."""
        stem, fields = self._view_of
        return self._ptrs(f"kmx_{stem}_view_device", len(fields))

    def close(self):
        if self._h:
            getattr(lib(), self._free)(self._h)
            self._h = C.c_void_p()
        self._reads = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _made_from(new, *sources, reads=None):
    """`new` was filled from the handles `sources`, on the stream of `reads` where the call takes the StrandReads itself: it keeps
    alive the StrandReads that they keep alive (a reused handle takes the new owner too).  Returns new."""
    new._reads = reads if reads is not None else next((s._reads for s in sources if s._reads is not None), None)
    return new


class Loci(_Handle):
    """Owns a kmx_loci handle (kmx_windows_vote)."""

    _free = "kmx_loci_free"
    _counts_of = ("kmx_loci_counts", ("nr", "n_loci", "n_votes", "n_small", "n_large"))
    _view_of = ("loci", (("locus_off", np.uint64, lambda c: c["nr"] + 1), ("diag", np.int64, "n_loci"), ("span", np.uint32, "n_loci"),
                         ("votes", np.uint32, "n_loci"), ("skipped", np.uint32, "nr")))

    def align(self, index, ranks, roff, max_edits, max_span=0, alignments=None):
        """kmx_loci_align: every read (the reads of the windows search) against the text around each of its loci, within
        max_edits edits; loci with span > max_span are skipped.  Returns an Alignments (`alignments` reuses one)."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        a = alignments or Alignments()
        o = AlignOptions(C.sizeof(AlignOptions), int(max_edits), int(max_span), 0)
        _check(lib().kmx_loci_align(index._h, self._h, ranks.ctypes.data if ranks.size else None, roff.ctypes.data, roff.size - 1,
                                    C.byref(o), C.byref(a._h)))
        return _made_from(a, self)

    def align_device(self, index, d_ranks_ptr, d_roff_ptr, nr, max_edits, max_span=0, stream=0, alignments=None):
        """kmx_loci_align_device on a caller-owned hipStream_t: the stream of the vote, or one ordered behind it."""
        a = alignments or Alignments()
        o = AlignOptions(C.sizeof(AlignOptions), int(max_edits), int(max_span), 0)
        _check(lib().kmx_loci_align_device(index._h, self._h, d_ranks_ptr, d_roff_ptr, nr, C.byref(o), stream or None, C.byref(a._h)))
        return _made_from(a, self)


class Alignments(_Handle):
    """Owns a kmx_alignments handle (kmx_loci_align)."""

    _free = "kmx_alignments_free"
    _counts_of = ("kmx_alignments_counts", ("nr", "n_loci", "n_aligned", "n_skipped"))
    _view_of = ("alignments", (("dist", np.uint8, "n_loci"), ("start", np.uint32, "n_loci"), ("end", np.uint32, "n_loci"),
                               ("best", np.uint32, "nr"), ("aligned", np.uint32, "nr")))

    def contigs_host(self):
        """kmx_alignments_contigs_view: ctg[n_loci] u32 as a numpy copy, the contig of every locus (NO_CONTIG for a skipped one), or
        None when the alignments were made on an index without a contig table."""
        p, nc = C.c_void_p(), C.c_uint64()
        _check(lib().kmx_alignments_contigs_view(self._h, C.byref(p), C.byref(nc)))
        if nc.value == 0:
            return None
        return _view(p.value, self.counts()["n_loci"], np.uint32).copy()

    def contigs_device_ptr(self):
        """(d_ctg, nc): kmx_alignments_contigs_view_device; d_ctg is None without a table (nc == 0) or without a locus."""
        p, nc = C.c_void_p(), C.c_uint64()
        _check(lib().kmx_alignments_contigs_view_device(self._h, C.byref(p), C.byref(nc)))
        return p.value, int(nc.value)

    @staticmethod
    def _script_options(all, m, scratch_bytes):
        return ScriptOptions(C.sizeof(ScriptOptions), (SCRIPT_ALL if all else 0) | (SCRIPT_M if m else 0), int(scratch_bytes))

    def scripts(self, index, loci, ranks, roff, all=False, m=False, scratch_bytes=0, scripts=None):
        """kmx_alignments_scripts: the CIGAR of every read's best alignment (all: of every aligned locus; m: '=' and 'X' as M), from
        the index, the loci and the reads that were aligned.  scratch_bytes bounds the device scratch of the traceback (0: the
        default).  Returns a Scripts (`scripts` reuses one)."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        s = scripts or Scripts()
        o = self._script_options(all, m, scratch_bytes)
        _check(lib().kmx_alignments_scripts(index._h, loci._h, self._h, ranks.ctypes.data if ranks.size else None, roff.ctypes.data, roff.size - 1,
                                            C.byref(o), C.byref(s._h)))
        return _made_from(s, loci, self)

    def scripts_device(self, index, loci, d_ranks_ptr, d_roff_ptr, nr, all=False, m=False, scratch_bytes=0, stream=0, scripts=None):
        """kmx_alignments_scripts_device on a caller-owned hipStream_t: the stream of the alignment, or one ordered behind it."""
        s = scripts or Scripts()
        o = self._script_options(all, m, scratch_bytes)
        _check(lib().kmx_alignments_scripts_device(index._h, loci._h, self._h, d_ranks_ptr, d_roff_ptr, nr, C.byref(o), stream or None, C.byref(s._h)))
        return _made_from(s, loci, self)

    def fold_strands(self, loci, stream=0, placements=None):
        """kmx_alignments_fold_strands: these are the alignments of a doubled batch (StrandReads) and `loci` its loci; one placement
        per public read.  stream=0: the stream that filled this handle.  Returns a Placements (`placements` reuses one)."""
        p = placements or Placements()
        o = FoldOptions(C.sizeof(FoldOptions), 0)
        _check(lib().kmx_alignments_fold_strands(loci._h, self._h, C.byref(o), stream or None, C.byref(p._h)))
        return _made_from(p, loci, self)

    def fold_pairs(self, loci, min_insert, max_insert, orientation=PAIR_FR, unpaired_penalty=None, stream=0, placements=None, pairs=None):
        """kmx_alignments_fold_pairs: these are the alignments of a doubled batch of interleaved mates (public read 2p is mate 1 of
        pair p, 2p + 1 its mate 2) and `loci` its loci; the concordant pair of loci with the least score where there is one with a
        template length in [min_insert, max_insert], else the placements of fold_strands.  unpaired_penalty=None: a concordant
        pair always wins.  Returns (Placements, Pairs) (`placements` and `pairs` reuse handles)."""
        pl = placements or Placements()
        pr = pairs or Pairs()
        o = PairOptions(C.sizeof(PairOptions), int(min_insert), int(max_insert), int(orientation),
                        PAIR_NO_PENALTY if unpaired_penalty is None else int(unpaired_penalty), 0)
        _check(lib().kmx_alignments_fold_pairs(loci._h, self._h, C.byref(o), stream or None, C.byref(pl._h), C.byref(pr._h)))
        return _made_from(pl, loci, self), _made_from(pr, loci, self)


class Scripts(_Handle):
    """Owns a kmx_scripts handle (kmx_alignments_scripts)."""

    _free = "kmx_scripts_free"
    _counts_of = ("kmx_scripts_counts", ("nr", "n_sel", "n_ops", "n_mismatched"))
    _view_of = ("scripts", (("read_sel_off", np.uint64, lambda c: c["nr"] + 1), ("sel", np.uint32, "n_sel"),
                            ("cig_off", np.uint64, lambda c: c["n_sel"] + 1), ("cigar", np.uint32, "n_ops")))
    _md_of = {"Alignments": "kmx_scripts_md", "Rescues": "kmx_rescues_md", "Secondaries": "kmx_secondaries_md"}     # by the source's type

    def strings(self):
        """One CIGAR string per entry, e.g. "50=1X30=1D69=" ("" for an entry without a script)."""
        h = self.host()
        return _runs_strings(h.cig_off, h.cigar)

    def clip(self, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, min_score=0, stream=0, clips=None):
        """kmx_scripts_clip: every entry trimmed to the best-scoring part of its runs under the affine scoring (a gap run of len
        letters costs gap_open + len gap_extend; clip_penalty once per clipped end); an entry whose best value is below min_score
        stays whole and carries CLIP_LOW.  Post-alignment trimming of the edit-optimal script, not a realignment.  Serves the
        Scripts of every source; stream=0: the stream that filled this handle.  Returns a Clips (`clips` reuses one)."""
        out = clips or Clips()
        o = ClipOptions(C.sizeof(ClipOptions), int(match), int(mismatch), int(gap_open), int(gap_extend), int(clip_penalty), int(min_score), 0)
        _check(lib().kmx_scripts_clip(self._h, C.byref(o), stream or None, C.byref(out._h)))
        out.scripts = self
        return _made_from(out, self)

    @staticmethod
    def _realign_options(match, mismatch, gap_open, gap_extend, clip_penalty, min_score, scratch_bytes):
        return RealignOptions(C.sizeof(RealignOptions), int(match), int(mismatch), int(gap_open), int(gap_extend), int(clip_penalty), int(min_score), 0,
                              int(scratch_bytes))

    def realign(self, index, alignments, ranks, roff, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, min_score=0, scratch_bytes=0,
                clips=None):
        """kmx_scripts_realign: every entry aligned again, locally and with affine gaps, inside the rectangle read x text[start, end)
        and the band |j - i| <= dist of its script, under the scoring of clip(); an entry without a path, or whose best value is
        below min_score, keeps its script and carries CLIP_LOW, every other one carries CLIP_REALIGNED.  These are the Scripts of
        Alignments.scripts[_device] or of Placements.scripts; alignments: the Alignments they were made from; ranks, roff: the
        reads that were aligned (host arrays).  scratch_bytes bounds the device scratch of the traceback (0: the default).  Returns
        a Clips (`clips` reuses one)."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        out = clips or Clips()
        o = self._realign_options(match, mismatch, gap_open, gap_extend, clip_penalty, min_score, scratch_bytes)
        _check(lib().kmx_scripts_realign(index._h, alignments._h, self._h, ranks.ctypes.data if ranks.size else None, roff.ctypes.data, roff.size - 1,
                                         C.byref(o), C.byref(out._h)))
        out.scripts = self
        return _made_from(out, self)

    def realign_device(self, index, alignments, d_ranks_ptr, d_roff_ptr, nr, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5,
                       min_score=0, scratch_bytes=0, stream=0, clips=None):
        """kmx_scripts_realign_device on a caller-owned hipStream_t: the stream that filled these scripts, or one ordered behind it."""
        out = clips or Clips()
        o = self._realign_options(match, mismatch, gap_open, gap_extend, clip_penalty, min_score, scratch_bytes)
        _check(lib().kmx_scripts_realign_device(index._h, alignments._h, self._h, d_ranks_ptr, d_roff_ptr, nr, C.byref(o), stream or None,
                                                C.byref(out._h)))
        out.scripts = self
        return _made_from(out, self)

    def md(self, index, source, letters, stream=0, md=None):
        """kmx_scripts_md (source: the Alignments these scripts were made from), kmx_rescues_md (source: the Rescues) or
        kmx_secondaries_md (source: the Secondaries): the MD string of every entry, from the runs and the index's text.  letters:
        sigma output bytes by rank (a str, bytes or uint8 array, e.g. "ACGT").  stream=0: the stream that filled this handle.
        Returns an Md (`md` reuses one)."""
        fn = self._md_of.get(type(source).__name__)
        if fn is None:
            raise TypeError("Scripts.md: source is an Alignments, a Rescues or a Secondaries")
        return _made_from(_md_call(fn, index, (self, source), letters, stream, md), self)

    def pileup(self, index, source, reads, lo=0, hi=None, min_score=-2**31, mapq=None, min_mapq=0, skip_low=False, add=False, mode=PILEUP_AUTO, tile=0,
               stream=0, pileup=None):
        """kmx_clips_pileup_device (source: the Alignments these scripts were made from) or kmx_clips_rescues_pileup (source: the
        Rescues) with clips = NULL: the scripts' own runs counted per text position of [lo, hi) (hi=None: the text's end) into the
        sigma + 3 planes of a Pileup.  reads: the StrandReads the scripts run over.  mapq (a Mapq or a device pointer) with min_mapq
        filters by read; min_score and skip_low need clips (Clips.pileup).  add=True adds to `pileup`; mode (PILEUP_AUTO, _ATOMIC,
        _TILED) and tile never change the result.  stream=0: the stream that filled this handle.  The call leaves its kernels in
        flight; Pileup.counts / planes wait for them.  Returns a Pileup (`pileup` reuses one)."""
        return _pileup_call("Scripts.pileup", index, self, None, source, reads, mapq, stream, pileup,
                            _pileup_options(lo, hi, min_score, min_mapq, skip_low, add, mode, tile))

    def pileup_device(self, index, alignments, d_ranks_ptr, d_roff_ptr, nr, lo=0, hi=None, min_score=-2**31, mapq=None, min_mapq=0, skip_low=False,
                      add=False, mode=PILEUP_AUTO, tile=0, stream=0, pileup=None, clips=None):
        """kmx_clips_pileup_device on reads that are on the device (d_ranks_ptr, d_roff_ptr, nr: those the scripts were made over, e.g.
        the single-strand reads of map_reads) and a caller-owned hipStream_t; clips: the Clips of these scripts, or None."""
        out = pileup or Pileup()
        o = _pileup_options(lo, hi, min_score, min_mapq, skip_low, add, mode, tile)
        _check(lib().kmx_clips_pileup_device(index._h, alignments._h, self._h, clips._h if clips is not None else None, d_ranks_ptr, d_roff_ptr, nr,
                                             _mapq_ptr(mapq), C.byref(o), stream or None, C.byref(out._h)))
        return _made_from(out, self)


def _pileup_options(lo, hi, min_score, min_mapq, skip_low, add, mode, tile):
    return PileupOptions(C.sizeof(PileupOptions), (PILEUP_ADD if add else 0) | (PILEUP_SKIP_LOW if skip_low else 0), int(lo), int(hi or 0),
                         int(min_score), int(min_mapq), int(mode), int(tile))


def _mapq_ptr(mapq):
    """The device array of a Mapq, or a raw device pointer, or None."""
    return mapq.device_ptrs()[0] if isinstance(mapq, Mapq) else (mapq or None)


def _pileup_call(who, index, scripts, clips, source, reads, mapq, stream, pileup, options):
    """kmx_clips_pileup_device (source: the Alignments the scripts were made from) or kmx_clips_rescues_pileup (source: the Rescues)
    over the doubled batch `reads` (a StrandReads).  Returns the Pileup (`pileup` reuses one)."""
    out = pileup or Pileup()
    kind = type(source).__name__
    ch = clips._h if clips is not None else None
    if kind == "Alignments":
        d_ranks2, d_roff2, nr2, _ = reads.device_ptrs()
        _check(lib().kmx_clips_pileup_device(index._h, source._h, scripts._h, ch, d_ranks2, d_roff2, nr2, _mapq_ptr(mapq), C.byref(options),
                                             stream or None, C.byref(out._h)))
    elif kind == "Rescues":
        _check(lib().kmx_clips_rescues_pileup(index._h, reads._h, source._h, scripts._h, ch, _mapq_ptr(mapq), C.byref(options), stream or None,
                                              C.byref(out._h)))
    else:
        raise TypeError(f"{who}: source is an Alignments or a Rescues")
    return _made_from(out, scripts, reads=reads)


def _md_call(fn, index, handles, letters, stream, md):
    """One of the kmx_*_md functions, which differ in the handles they take behind the index.  Returns the Md (`md` reuses one)."""
    table = None if letters is None else _letters_table(letters)
    out = md or Md()
    o = MdOptions(C.sizeof(MdOptions), 0)
    _check(getattr(lib(), fn)(index._h, *[h._h for h in handles], table.ctypes.data if table is not None else None, C.byref(o), stream or None,
                              C.byref(out._h)))
    return out


class Clips(_Handle):
    """Owns a kmx_clips handle (kmx_scripts_clip): every entry of a Scripts trimmed to the best-scoring part of its runs, with the
    score and the letters clipped off either side.  Entry e is entry e of the Scripts."""

    _free = "kmx_clips_free"
    _counts_of = ("kmx_clips_counts", ("n_sel", "n_ops", "n_clipped", "n_low"))
    _view_of = ("clips", (("score", np.int32, "n_sel"), ("sl", np.uint16, "n_sel"), ("sr", np.uint16, "n_sel"), ("tl", np.uint16, "n_sel"),
                          ("tr", np.uint16, "n_sel"), ("nm", np.uint16, "n_sel"), ("cflags", np.uint8, "n_sel"),
                          ("cig_off", np.uint64, lambda c: c["n_sel"] + 1), ("cigar", np.uint32, "n_ops")))
    _md_of = {"Alignments": "kmx_clips_md", "Rescues": "kmx_clips_rescues_md"}      # by the source's type

    def __init__(self):
        super().__init__()
        self.scripts = None         # the Scripts the clips were made from (set by Scripts.clip)

    def close(self):
        super().close()
        self.scripts = None

    def strings(self):
        """One CIGAR string per entry with S at the clipped ends, e.g. "1S149=" ("" for an entry without a script)."""
        h = self.host()
        return _runs_strings(h.cig_off, h.cigar)

    def md(self, index, scripts, source, letters, stream=0, md=None):
        """kmx_clips_md (source: the Alignments the scripts were made from) or kmx_clips_rescues_md (source: the Rescues): the MD
        string of every clipped entry, over the text interval [start + tl, end - tr).  scripts: the Scripts these clips were made
        from.  stream=0: the stream that filled the scripts.  Returns an Md (`md` reuses one)."""
        fn = self._md_of.get(type(source).__name__)
        if fn is None:
            raise TypeError("Clips.md: source is an Alignments or a Rescues")
        return _made_from(_md_call(fn, index, (scripts, self, source), letters, stream, md), self)

    def pileup(self, index, scripts, source, reads, lo=0, hi=None, min_score=-2**31, mapq=None, min_mapq=0, skip_low=False, add=False,
               mode=PILEUP_AUTO, tile=0, stream=0, pileup=None):
        """Scripts.pileup over the runs of these clips (trimmed or realigned): the text interval of every entry is [start + tl,
        end - tr), entries that score below min_score are filtered, and with skip_low those that carry CLIP_LOW.  scripts: the Scripts
        these clips were made from; source: the Alignments or the Rescues behind them.  Returns a Pileup (`pileup` reuses one)."""
        return _pileup_call("Clips.pileup", index, scripts, self, source, reads, mapq, stream, pileup,
                            _pileup_options(lo, hi, min_score, min_mapq, skip_low, add, mode, tile))

    def pileup_device(self, index, scripts, alignments, d_ranks_ptr, d_roff_ptr, nr, **kw):
        """Scripts.pileup_device over the runs of these clips."""
        return scripts.pileup_device(index, alignments, d_ranks_ptr, d_roff_ptr, nr, clips=self, **kw)

    def supplementaries(self, reads, loci, alignments, placements, scripts, max_supplementary=4, min_len=20, max_overlap=10, min_score=20,
                        stream=0, supplementaries=None):
        """kmx_clips_supplementaries: these are the clips of `scripts`, the all=True scripts of the doubled batch `reads` (no m=True);
        up to max_supplementary (<= SUPPLEMENTARY_MAX) further parts per read, chosen greedily by (score, entry) among the clipped
        entries of both strands that keep min_len read letters, score at least min_score and share at most max_overlap read letters
        with the primary and with every part taken before.  The parts are the best-scoring parts of the edit-optimal scripts, not
        realignments.  The four defaults are judgements (a part of 20 letters at k = 10 has seeds enough to be voted for; 10 letters
        of overlap is what microhomology at a breakpoint may share): nothing measures them.  stream=0: the stream that filled this
        handle.  Returns a Supplementaries (`supplementaries` reuses one)."""
        out = supplementaries or Supplementaries()
        o = SupplementaryOptions(C.sizeof(SupplementaryOptions), int(max_supplementary), int(min_len), int(max_overlap), int(min_score), 0)
        _check(lib().kmx_clips_supplementaries(reads._h, loci._h, alignments._h, placements._h, scripts._h, self._h, C.byref(o), stream or None,
                                               C.byref(out._h)))
        if not out._owns:
            out.all_scripts, out.all_clips = scripts, self
        return _made_from(out, self, reads=reads)


class Md(_Handle):
    """Owns a kmx_md handle (kmx_scripts_md, kmx_rescues_md): the MD string of every entry of a Scripts."""

    _free = "kmx_md_free"
    _counts_of = ("kmx_md_counts", ("n_sel", "n_bytes", "n_mismatched"))
    _view_of = ("md", (("md_off", np.uint64, lambda c: c["n_sel"] + 1), ("md", np.uint8, "n_bytes")))

    def strings(self):
        """One MD string per entry, e.g. "50A30^C69" ("" for an entry without a script)."""
        md_off, md = self.host()
        raw = md.tobytes()
        return [raw[int(a):int(b)].decode("latin-1") for a, b in zip(md_off[:-1], md_off[1:])]


class Mapq(_Handle):
    """Owns a kmx_mapq handle (kmx_placements_mapq): one MAPQ per public read."""

    _free = "kmx_mapq_free"
    _counts_of = ("kmx_mapq_counts", ("nr", "n_zero", "n_cap"))
    _view_of = ("mapq", (("mapq", np.uint8, "nr"),))

    def host(self):
        """The one field itself, not a tuple of one."""
        return super().host().mapq


class Pileup(_Handle):
    """Owns a kmx_pileup handle (kmx_clips_pileup_device, kmx_clips_rescues_pileup): sigma + 3 planes of u32 counters over the text
    region [lo, hi), channel-major: the letters by rank, OTHER, DEL, INS."""

    _free = "kmx_pileup_free"
    _counts_of = ("kmx_pileup_counts", ("lo", "hi", "n_channels", "n_added", "n_filtered", "n_mismatched", "n_cells"))
    _view_of = ("pileup", (("counts", np.uint32, lambda c: c["n_channels"] * (c["hi"] - c["lo"])),))

    def planes(self):
        """The counters as a (n_channels, hi - lo) uint32 array (a copy); waits for the kernels of the last call."""
        c = self.counts()
        return self.host().counts.reshape(c["n_channels"], c["hi"] - c["lo"])

    def sites(self, index, min_depth=1, min_alt=1, frac=(1, 5), stream=0, sites=None):
        """kmx_pileup_sites: one record per position and channel other than the reference letter (a letter, DEL or INS; never OTHER)
        whose count is at least min_alt and at least frac[0] / frac[1] of the depth, at positions of depth >= min_depth.  stream=0:
        the stream of the last call into this handle.  Returns a Sites (`sites` reuses one)."""
        out = sites or Sites()
        o = SitesOptions(C.sizeof(SitesOptions), int(min_depth), int(min_alt), int(frac[0]), int(frac[1]))
        _check(lib().kmx_pileup_sites(index._h, self._h, C.byref(o), stream or None, C.byref(out._h)))
        return _made_from(out, self)


class Sites(_Handle):
    """Owns a kmx_sites handle (kmx_pileup_sites): the records (pos, ref, alt, depth, count, ref_count[, ctg]) ordered by (pos, alt)."""

    _free = "kmx_sites_free"
    _counts_of = ("kmx_sites_counts", ("n_sites", "n_covered"))
    _view_of = ("sites", (("pos", np.uint32, "n_sites"), ("ref", np.uint8, "n_sites"), ("alt", np.uint8, "n_sites"), ("depth", np.uint32, "n_sites"),
                          ("count", np.uint32, "n_sites"), ("ref_count", np.uint32, "n_sites"), ("ctg", np.uint32, "n_sites")))
    _optional = ("ctg",)            # None when the index has no contig table


class StrandReads(_Handle):
    """Owns a kmx_strand_reads handle (kmx_reads_strands): every read and its reverse complement, on the device.  After
    Index.strand_reads the handle owns the stream everything behind it runs on: close it last."""

    _free = "kmx_strand_reads_free"

    def counts(self):
        _, _, nr2, _ = self.device_ptrs()
        return {"nr": nr2 // 2, "nr2": nr2}

    def device_ptrs(self):
        """(d_ranks2, d_roff2, nr2, stream): kmx_strand_reads_view_device."""
        a, b, n, s = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_void_p()
        _check(lib().kmx_strand_reads_view_device(self._h, C.byref(a), C.byref(b), C.byref(n), C.byref(s)))
        return a.value, b.value, int(n.value), s.value


class _PerRead:
    """The per-read lookups of a handle whose scripts() has at most one entry per public read.  The class supplies
    _entries(scripts): that entry for every public read, -1 where the read has none."""

    def _per_read(self, scripts, values, none=""):
        """values holds one value per entry of `scripts`: the value of every public read's entry, `none` where it has none"""
        return [values[e] if e >= 0 else none for e in self._entries(scripts)]

    def cigars(self, scripts, clips=None):
        """One CIGAR string per public read from the Scripts of scripts(): "" where the read has no entry (it is unplaced, or was
        not rescued).  clips (the Clips of scripts.clip()): the clipped CIGARs, with S."""
        return self._per_read(scripts, scripts.strings() if clips is None else clips.strings())

    def mds(self, md, scripts):
        """One MD string per public read from the Md of scripts.md(): "" where cigars(scripts) has none."""
        return self._per_read(scripts, md.strings())

    def clip_fields(self, clips, scripts):
        """(tl, nm, score, has) per public read from the Clips of scripts().clip(): the text letters clipped off the left, the
        clipped NM and the score of the read's entry, has False (and zeros) where cigars(scripts) has none.  For sam_lines (the
        rescue's as the second of a tuple)."""
        return _clip_fields(self._entries(scripts), clips.host())


class Placements(_PerRead, _Handle):
    """Owns a kmx_placements handle (kmx_alignments_fold_strands): one placement per public read of a doubled batch."""

    _free = "kmx_placements_free"
    _counts_of = ("kmx_placements_counts", ("nr", "n_placed", "n_reverse", "n_ambiguous"))
    _view_of = ("placements", (("locus", np.uint32, "nr"), ("strand", np.uint8, "nr"), ("dist", np.uint8, "nr"), ("start", np.uint32, "nr"),
                               ("end", np.uint32, "nr"), ("second", np.uint8, "nr"), ("best2", np.uint32, lambda c: 2 * c["nr"])))

    def host(self, best2=True):
        """best2=False leaves the last field on the device (the tuple then has six entries)."""
        return super().host() if best2 else self._arrays(self._ptrs("kmx_placements_view", 6, n_null=1))

    def scripts(self, index, reads, loci, alignments, m=False, scratch_bytes=0, scripts=None):
        """kmx_placements_scripts: the CIGAR of every placed read's winner (for a reverse placement that of the reverse complement
        against the forward text, as SAM has it), on the stream of `reads`.  Returns a Scripts over the internal reads."""
        s = scripts or Scripts()
        o = Alignments._script_options(False, m, scratch_bytes)
        _check(lib().kmx_placements_scripts(index._h, reads._h, loci._h, alignments._h, self._h, C.byref(o), C.byref(s._h)))
        return _made_from(s, reads=reads)

    def _entries(self, scripts):
        """the entry of every public read's winner, -1 for an unplaced read"""
        strand = self.host(best2=False).strand
        read_sel_off = scripts.host().read_sel_off
        out = []
        for i, s in enumerate(strand):
            r = 2 * i + int(s)
            out.append(int(read_sel_off[r]) if s != 255 and read_sel_off[r + 1] > read_sel_off[r] else -1)
        return out

    def mapq(self, max_edits, pairs=None, cap=60, per_edit=10, pair_bonus=40, stream=0, mapq=None):
        """kmx_placements_mapq: one MAPQ per read by the gap rule of include/kmx.h (a heuristic), from dist and second and, with
        `pairs`, from the score and second_score of concordant pairs.  max_edits: the budget the alignments (and the rescue) were
        made with.  stream=0: the stream that filled this handle.  Returns a Mapq (`mapq` reuses one)."""
        q = mapq or Mapq()
        o = MapqOptions(C.sizeof(MapqOptions), int(max_edits), int(cap), int(per_edit), int(pair_bonus), 0)
        _check(lib().kmx_placements_mapq(self._h, pairs._h if pairs is not None else None, C.byref(o), stream or None, C.byref(q._h)))
        return _made_from(q, self)

    def locate(self, index, alignments, mates=False, stream=0, located=None):
        """kmx_placements_locate: the contig and the position inside it of every placement, from the contig table of `index` and
        the contigs that `alignments` recorded per locus.  mates=True (LOCATE_MATES): the reads are interleaved mates, a rescued read
        takes its mate's contig.  stream=0: the stream that filled this handle.  Returns a Located (`located` reuses one)."""
        out = located or Located()
        o = LocateOptions(C.sizeof(LocateOptions), LOCATE_MATES if mates else 0)
        _check(lib().kmx_placements_locate(index._h, alignments._h, self._h, C.byref(o), stream or None, C.byref(out._h)))
        return _made_from(out, self)

    def secondaries(self, loci, alignments, max_secondary, max_delta=None, stream=0, secondaries=None):
        """kmx_placements_secondaries: up to max_secondary (<= SECONDARY_MAX) further places per read, chosen greedily by
        (dist, locus) among the aligned loci of both strands that lie elsewhere from the primary and from every place taken before.
        max_delta=None: no bound, else a candidate has dist <= the primary's + max_delta.  stream=0: the stream that filled this
        handle.  Returns a Secondaries (`secondaries` reuses one)."""
        out = secondaries or Secondaries()
        o = SecondaryOptions(C.sizeof(SecondaryOptions), int(max_secondary), SECONDARY_NO_DELTA if max_delta is None else int(max_delta), 0)
        _check(lib().kmx_placements_secondaries(loci._h, alignments._h, self._h, C.byref(o), stream or None, C.byref(out._h)))
        return _made_from(out, self)


class Secondaries(_Handle):
    """Owns a kmx_secondaries handle (kmx_placements_secondaries): up to N further places per public read, the entries of internal
    read 2i + s being those of read i on strand s."""

    _free = "kmx_secondaries_free"
    _counts_of = ("kmx_secondaries_counts", ("nr", "n_sec", "n_multi", "n_truncated"))
    _view_of = ("secondaries", (("sec_off", np.uint64, lambda c: 2 * c["nr"] + 1), ("locus", np.uint32, "n_sec"), ("dist", np.uint8, "n_sec"),
                                ("start", np.uint32, "n_sec"), ("end", np.uint32, "n_sec"), ("ctg", np.uint32, "n_sec"), ("more", np.uint8, "nr")))
    _optional = ("ctg",)            # None when the alignments carried no contig table

    def scripts(self, index, reads, m=False, scratch_bytes=0, scripts=None):
        """kmx_secondaries_scripts: the CIGAR of every entry (for a reverse entry that of the reverse complement against the forward
        text, as SAM has it), on the stream of `reads`.  Returns a Scripts over the internal reads, sel[e] == e."""
        s = scripts or Scripts()
        o = Alignments._script_options(False, m, scratch_bytes)
        _check(lib().kmx_secondaries_scripts(index._h, reads._h, self._h, C.byref(o), C.byref(s._h)))
        return _made_from(s, reads=reads)

    def cigars(self, scripts):
        """One CIGAR string per entry from the Scripts of scripts()."""
        return scripts.strings()

    def md(self, index, scripts, letters, stream=0, md=None):
        """kmx_secondaries_md: the MD string of every entry from the Scripts of scripts().  Returns an Md (`md` reuses one)."""
        return _made_from(scripts.md(index, self, letters, stream, md), self, scripts)

    def xa(self, scripts, strand_names="+-", located=None, rname=None, clips=None):
        """One XA:Z: value per public read: "" or items rname,<strand><pos>,CIGAR,NM; in bwa's form (pos 1-based), in the order of
        the entries.  located=(names, ctg_off): the name of the entry's contig and a contig-local pos (the handle must carry ctg);
        otherwise `rname` names the one reference.  scripts: the Scripts of scripts().  clips (the Clips of scripts.clip()): every
        entry's position is shifted by its tl, and its CIGAR and NM are the clipped ones."""
        h = self.host()
        if clips is None:
            return xa_strings(h.sec_off, h.dist, h.start, h.ctg, self.cigars(scripts), strand_names, located, rname)
        if clips.counts()["n_sel"] != h.dist.size:
            raise ValueError("xa: the clips are not those of these entries")
        c = clips.host()
        return xa_strings(h.sec_off, c.nm, h.start, h.ctg, _runs_strings(c.cig_off, c.cigar), strand_names, located, rname, shift=c.tl)


class Supplementaries(_Handle):
    """Owns a kmx_supplementaries handle (kmx_clips_supplementaries): up to N further parts per public read, the entries of read i
    being [sup_off[i], sup_off[i + 1]); ent[x] indexes the entries of the all-loci Scripts and Clips the handle was made from.
    all_scripts / all_clips are those two when the chain keyword supplementary= made the handle, and close() then closes them too
    (the chain registers every handle it makes as it makes it, so nothing leaks when a later stage raises); a handle of
    Clips.supplementaries has all_clips (and all_clips.scripts) for reference only and closes neither."""

    _free = "kmx_supplementaries_free"
    _counts_of = ("kmx_supplementaries_counts", ("nr", "n_sup", "n_split", "n_truncated"))
    _view_of = ("supplementaries", (("sup_off", np.uint64, lambda c: c["nr"] + 1), ("ent", np.uint32, "n_sup"), ("locus", np.uint32, "n_sup"),
                                    ("strand", np.uint8, "n_sup"), ("q0", np.uint16, "n_sup"), ("q1", np.uint16, "n_sup"), ("t0", np.uint32, "n_sup"),
                                    ("t1", np.uint32, "n_sup"), ("score", np.int32, "n_sup"), ("second_score", np.int32, "n_sup"),
                                    ("nm", np.uint16, "n_sup"), ("ctg", np.uint32, "n_sup"), ("more", np.uint8, "nr")))
    _optional = ("ctg",)            # None when the alignments carried no contig table

    def __init__(self):
        super().__init__()
        self.all_scripts = self.all_clips = None
        self._owns = False          # the chain made all_scripts / all_clips for this handle alone

    def close(self):
        super().close()
        if self._owns:
            for h in (self.all_clips, self.all_scripts):
                if h is not None:
                    h.close()
        self.all_scripts = self.all_clips = None
        self._owns = False

    def mapq(self, cap=60):
        """supplementary_mapq of every entry (u8[n_sup])."""
        h = self.host()
        return supplementary_mapq(h.score, h.second_score, cap)

    def cigars(self, clips=None):
        """One clipped CIGAR string per entry, from `clips` (default all_clips), the Clips the handle was made from."""
        strings = (clips or self.all_clips).strings()
        return [strings[int(e)] for e in self.host().ent]

    def mds(self, md):
        """One MD string per entry from the Md of the all-loci clips (Clips.md over the all-loci scripts and the alignments)."""
        strings = md.strings()
        return [strings[int(e)] for e in self.host().ent]

    def sa(self, placements_host, cigars, clip_fields, mapq, cap=60, located=None, located_host=None, rname=None, clips=None, strand_names="+-"):
        """sa_strings of this handle: per public read the SA:Z: values of its primary and of its entries.  placements_host:
        Placements.host(); cigars, clip_fields: the primaries' clipped CIGARs and (tl, nm, score, has) per read (Placements.cigars(
        scripts, clips) and .clip_fields(clips, scripts) over the placements' own scripts); mapq: Mapq.host().  The entries take
        their CIGARs from `clips` (default all_clips) and their MAPQ from mapq(cap).  located=(names, ctg_off) with located_host
        (Located.host()): contig names and contig-local positions; otherwise `rname` names the one reference."""
        h = self.host()
        _, strand, _, start = placements_host[:4]
        tl, nm = clip_fields[:2]
        ctg, _ = (None, None) if located_host is None else located_host
        pos = np.asarray(start, np.int64) + np.asarray(tl, np.int64)
        primary = (pos, np.where(np.asarray(strand) == 1, 1, 0), cigars, mapq, nm, ctg)
        entries = (h.t0, h.strand, self.cigars(clips), self.mapq(cap), h.nm, h.ctg)
        return sa_strings(h.sup_off, primary, entries, located, rname, strand_names)


class Located(_Handle):
    """Owns a kmx_located handle (kmx_placements_locate): the contig and the contig-local position of every public read, NO_CONTIG
    and 0 for an unplaced one."""

    _free = "kmx_located_free"
    _counts_of = ("kmx_located_counts", ("nr", "n_located", "n_mismatched"))
    _view_of = ("located", (("ctg", np.uint32, "nr"), ("pos", np.uint32, "nr")))


class Pairs(_Handle):
    """Owns a kmx_pairs handle (kmx_alignments_fold_pairs): one entry per pair of a doubled batch of interleaved mates."""

    _free = "kmx_pairs_free"
    _counts_of = ("kmx_pairs_counts", ("np", "n_concordant", "n_discordant", "n_single", "n_unplaced", "n_ambiguous"))
    _view_of = ("pairs", (("cls", np.uint8, "np"), ("tlen", np.int32, "np"), ("score", np.uint16, "np"), ("second_score", np.uint16, "np")))

    def rescue(self, index, reads, loci, alignments, placements, min_insert, max_insert, max_edits, orientation=PAIR_FR, discordant=False,
               unpaired_penalty=None, segment=0, rescues=None):
        """kmx_pairs_rescue: every mate that the pair fold left without a locus (the ONLY classes; discordant=True: the mates of
        DISCORDANT pairs too) is aligned within max_edits edits against the insert window that its placed partner implies, and where
        that alignment is concordant `placements` and these pairs are rewritten in place.  The handles are those of one map_pairs
        chain; min_insert / max_insert / orientation as for fold_pairs.  unpaired_penalty=None: a rescued pair always wins (it is only
        looked at for DISCORDANT pairs).  segment: end columns per thread, 0 = the default; the result never depends on it.  Returns a
        Rescues (`rescues` reuses one)."""
        r = rescues or Rescues()
        o = RescueOptions(C.sizeof(RescueOptions), int(min_insert), int(max_insert), int(orientation), int(max_edits),
                          PAIR_NO_PENALTY if unpaired_penalty is None else int(unpaired_penalty), int(segment), RESCUE_DISCORDANT if discordant else 0)
        _check(lib().kmx_pairs_rescue(index._h, reads._h, loci._h, alignments._h, C.byref(o), placements._h, self._h, C.byref(r._h)))
        return _made_from(r, reads=reads)


class Rescues(_PerRead, _Handle):
    """Owns a kmx_rescues handle (kmx_pairs_rescue): one job per mate that was looked for in its partner's insert window."""

    _free = "kmx_rescues_free"
    _counts_of = ("kmx_rescues_counts", ("nr2", "n_jobs", "n_found", "n_concordant", "n_taken"))
    _view_of = ("rescues", (("job_off", np.uint64, lambda c: c["nr2"] + 1), ("read", np.uint32, "n_jobs"), ("lo", np.uint32, "n_jobs"),
                            ("hi", np.uint32, "n_jobs"), ("dist", np.uint8, "n_jobs"), ("start", np.uint32, "n_jobs"), ("end", np.uint32, "n_jobs"),
                            ("status", np.uint8, "n_jobs")))

    def scripts(self, index, reads, m=False, scratch_bytes=0, scripts=None):
        """kmx_rescues_scripts: the CIGAR of every taken job (for a reverse placement that of the reverse complement against the
        forward text, as SAM has it), on the stream of `reads`.  Returns a Scripts over the internal reads, sel = the job."""
        s = scripts or Scripts()
        o = Alignments._script_options(False, m, scratch_bytes)
        _check(lib().kmx_rescues_scripts(index._h, reads._h, self._h, C.byref(o), C.byref(s._h)))
        return _made_from(s, reads=reads)

    def _entries(self, scripts):
        """the entry of every rescued public read, -1 for every other"""
        h = self.host()
        read_sel_off = scripts.host().read_sel_off
        out = [-1] * ((h.job_off.size - 1) // 2)
        for r, taken in zip(h.read, h.status == RESCUE_TAKEN):
            if taken and read_sel_off[int(r) + 1] > read_sel_off[int(r)]:
                out[int(r) // 2] = int(read_sel_off[int(r)])
        return out


# what map_reads_strands / map_pairs append with tags=True: the Mapq, the Md of the scripts, and after a rescue the Scripts of the
# rescued mates and their Md (else None)
SamTags = collections.namedtuple("SamTags", "mapq md rescue_scripts rescue_md")


class ApproxResult(_Handle):
    """Owns a kmx_approx_result handle (kmx_search_approx)."""

    _free = "kmx_approx_free"
    _counts_of = ("kmx_approx_counts", ("nq", "n_hits", "n_candidates", "n_chunks"))
    _view_of = ("approx", (("hit_off", np.uint64, lambda c: c["nq"] + 1), ("positions", np.uint32, "n_hits"), ("mismatches", np.uint8, "n_hits"),
                           ("status", np.uint8, "nq")))             # on the host only: the C-ABI has no kmx_approx_view_device

    def _column(self, fn, dtype, count):
        return _view(self._ptrs(fn, 1)[0], self.counts()[count], dtype).copy()

    def lengths(self):
        """kmx_approx_lengths: the window length of every hit (u32, parallel to positions) of a search with edit=True."""
        return self._column("kmx_approx_lengths", np.uint32, "n_hits")

    def strands(self):
        """kmx_approx_strands: the strand of every hit (u8, parallel to positions; 0 forward, 1 reverse) of a search with
        strands=True."""
        return self._column("kmx_approx_strands", np.uint8, "n_hits")

    def found(self):
        """kmx_approx_found: per query the hits left after loci / best and before the max_hits cap (u64[nq]) of a search with
        any of the three reporting options; more than the query's list holds when the cap cut it."""
        return self._column("kmx_approx_found", np.uint64, "nq")


class Index:
    """kmx_index handle: the flattened kmer_index<alphabet_t, uint32_t, ks...> resident in HBM."""

    def __init__(self, ranks, sigma, ks, table=TABLE_AUTO, device=-1, n_threads=0, keep_host_arena=False,
                 query_size_range=0, host_flatten=False, aligned_copy=True, devices=None, prefix_levels=0):
        """devices: None = one replica on `device` (KMX_DEVICES in the environment may widen it); a list of ordinals =
        built on devices[0] and replicated onto the others (host-buffer searches then shard over the replicas).
        prefix_levels: kmx_options.prefix_levels (0 = default, -1 = none, N = at most N pre-merged levels per element)."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        ks = np.ascontiguousarray(ks, np.uint32)
        self.ks = ks.tolist()
        self.sigma = int(sigma)
        self.n = int(ranks.size)
        o = Options()
        o.struct_size = C.sizeof(Options)
        o.device = device
        o.table_kind = table
        o.n_threads = n_threads
        o.query_size_range = query_size_range
        o.keep_host_arena = int(keep_host_arena)
        o.host_flatten = int(host_flatten)
        o.no_aligned_copy = int(not aligned_copy)
        o.prefix_levels = int(prefix_levels)
        _set_devices(o, devices)
        self._h = C.c_void_p()
        _check(lib().kmx_index_build(ranks.ctypes.data, ranks.size, self.sigma, ks.ctypes.data, ks.size,
                                     C.byref(o), C.byref(self._h)))

    @classmethod
    def load(cls, path, device=-1, keep_host_arena=False, devices=None, prefix_levels=0):
        """kmx_index_load: an index from an image written by save()."""
        self = cls.__new__(cls)
        o = Options()
        o.struct_size = C.sizeof(Options)
        o.device = device
        o.keep_host_arena = int(keep_host_arena)
        o.prefix_levels = int(prefix_levels)
        _set_devices(o, devices)
        self._h = C.c_void_p()
        _check(lib().kmx_index_load(os.fsencode(path), C.byref(o), C.byref(self._h)))
        info = self.info()
        self.ks, self.sigma, self.n = info["ks"], info["sigma"], info["n"]
        return self

    def save(self, path):
        _check(lib().kmx_index_save(self._h, os.fsencode(path)))

    def set_contigs(self, ctg_off):
        """kmx_index_set_contigs: contig c is text[ctg_off[c]:ctg_off[c + 1]); every chain call behind this one (map_reads,
        map_reads_strands, map_pairs and their stages) keeps alignments, pairs and rescues inside one contig.  None or an empty
        array removes the table.  The table is not part of a saved image: set it again after load()."""
        ctg_off = np.zeros(0, np.uint64) if ctg_off is None else np.ascontiguousarray(ctg_off, np.uint64)
        nc = max(int(ctg_off.size) - 1, 0)
        _check(lib().kmx_index_set_contigs(self._h, ctg_off.ctypes.data if nc else None, nc))

    def contigs(self):
        """kmx_index_contigs: ctg_off[nc + 1] u64 of the table, or None when the index has none."""
        nc = C.c_uint64()
        _check(lib().kmx_index_contigs(self._h, C.byref(nc), None, 0))
        if nc.value == 0:
            return None
        out = np.zeros(nc.value + 1, np.uint64)
        _check(lib().kmx_index_contigs(self._h, C.byref(nc), out.ctypes.data, out.size))
        return out

    def info(self):
        n, sigma, nks, dbytes = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        ks = np.zeros(KMX_MAX_KS, np.uint32)
        tk = np.zeros(KMX_MAX_KS, np.uint32)
        _check(lib().kmx_index_info(self._h, C.byref(n), C.byref(sigma), C.byref(nks), ks.ctypes.data, tk.ctypes.data, C.byref(dbytes)))
        return {"n": n.value, "sigma": sigma.value, "ks": ks[:nks.value].tolist(), "tables": tk[:nks.value].tolist(),
                "device_bytes": dbytes.value}

    def memory(self):
        """kmx_index_memory: device bytes of one replica by part (positions, aligned_copy, cells, prefix_levels, tables)."""
        v = [C.c_uint64() for _ in range(5)]
        _check(lib().kmx_index_memory(self._h, *[C.byref(x) for x in v]))
        return dict(zip(["positions", "aligned_copy", "cells", "prefix_levels", "tables"], [int(x.value) for x in v]))

    def paths(self):
        """kmx_index_paths: the k_fill variant in effect (slots per thread, non-temporal stores, 64-bit records), tiny_cells, the
        scan's tile in queries and the cell shift of every element (info()["ks"] order, 0 = no cells)."""
        v = IndexPathInfo()
        v.struct_size = C.sizeof(IndexPathInfo)
        _check(lib().kmx_index_paths(self._h, C.byref(v)))
        return {"fill_slots": int(v.fill_slots), "fill_nontemporal": bool(v.fill_nontemporal), "rec64": bool(v.rec64),
                "tiny_cells": bool(v.tiny_cells), "scan_tile": int(v.scan_tile), "cell_shift": [int(v.cell_shift[i]) for i in range(v.n_ks)],
                "windows_tile": int(v.windows_tile)}

    def devices(self):
        n = C.c_uint32()
        d = (C.c_int32 * KMX_MAX_DEVICES)()
        _check(lib().kmx_index_devices(self._h, C.byref(n), d))
        return [int(d[i]) for i in range(n.value)]

    def levels(self):
        """kmx_index_levels: prefix levels built per element (info()["ks"] order)."""
        lv = np.zeros(KMX_MAX_KS, np.uint32)
        _check(lib().kmx_index_levels(self._h, lv.ctypes.data))
        return lv[:len(self.ks)].tolist()

    def bucket_host(self, k, ranks):
        """kmx_index_bucket_host: the bucket of one k-mer out of the host arena (search_k, kmer_index.hpp:183-190); None on a miss."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        if ranks.size != k:
            raise ValueError("bucket_host: k letters expected")
        p, n = C.c_void_p(), C.c_uint32()
        _check(lib().kmx_index_bucket_host(self._h, int(k), ranks.ctypes.data, C.byref(p), C.byref(n)))
        return _view(p.value, n.value, np.uint32).copy() if p.value else None

    def extend_query_size_range(self, new_maximum):
        _check(lib().kmx_index_extend_query_size_range(self._h, new_maximum))

    def arena_host(self):
        p, n = C.c_void_p(), C.c_uint64()
        _check(lib().kmx_index_arena_host(self._h, C.byref(p), C.byref(n)))
        return _view(p.value, n.value, np.uint32)

    def search(self, qranks, qoff, flags=SEARCH_DEFAULT, result=None):
        """Host-buffer batch search (kmx_search_batch)."""
        qranks = np.ascontiguousarray(qranks, np.uint8)
        qoff = np.ascontiguousarray(qoff, np.uint64)
        r = result or Result()
        _check(lib().kmx_search_batch(self._h, qranks.ctypes.data if qranks.size else None, qoff.ctypes.data,
                                      qoff.size - 1, flags, C.byref(r._h)))
        r._index = self
        return r

    def search_approx(self, qranks, qoff, max_subst, edit=False, strands=False, complement=None, loci=False, best=False, max_hits=0):
        """kmx_search_approx: every window within Hamming distance max_subst (<= APPROX_MAX_SUBST) of each query; edit=True
        (KMX_APPROX_EDIT): every start of a window within that many edits, its distance in `mismatches`, ApproxResult.lengths().
        strands=True (kmx_search_approx_strands): the same for each query and its reverse complement under `complement`
        (rank to rank, uint8[sigma]; default complement_table(sigma)), hits ordered by (position, strand), ApproxResult.strands().
        loci / best / max_hits (kmx_search_approx_opts; any of them routes there): one hit per alignment locus (edit only), the
        best stratum only, at most max_hits hits per query; ApproxResult.found() tells what the cap cut."""
        qranks = np.ascontiguousarray(qranks, np.uint8)
        qoff = np.ascontiguousarray(qoff, np.uint64)
        r = ApproxResult()
        comp = None
        if strands:
            comp = np.ascontiguousarray(complement_table(self.sigma) if complement is None else complement, np.uint8)
            if comp.size != self.sigma:
                raise ValueError("search_approx: the complement table needs sigma entries")
        if loci or best or max_hits:
            flags = (APPROX_EDIT if edit else 0) | (APPROX_LOCI if loci else 0) | (APPROX_BEST if best else 0)
            o = ApproxOptions(C.sizeof(ApproxOptions), int(max_subst), flags, int(max_hits), comp.ctypes.data if strands else None)
            _check(lib().kmx_search_approx_opts(self._h, qranks.ctypes.data if qranks.size else None, qoff.ctypes.data, qoff.size - 1,
                                                C.byref(o), C.byref(r._h)))
            return r
        if strands:
            _check(lib().kmx_search_approx_strands(self._h, qranks.ctypes.data if qranks.size else None, qoff.ctypes.data,
                                                   qoff.size - 1, int(max_subst), APPROX_EDIT if edit else 0, comp.ctypes.data, C.byref(r._h)))
            return r
        _check(lib().kmx_search_approx(self._h, qranks.ctypes.data if qranks.size else None, qoff.ctypes.data,
                                       qoff.size - 1, int(max_subst), APPROX_EDIT if edit else 0, C.byref(r._h)))
        return r

    def text(self):
        """kmx_index_text: the text reconstructed on the device from the index, as ranks (uint8)."""
        n = int(self.info()["n"])
        out = np.zeros(n, np.uint8)
        _check(lib().kmx_index_text(self._h, out.ctypes.data, n, None))
        return out

    def text_packed_bytes(self):
        """kmx_index_text with no output: derives the packed copy (first call) and returns its size in bytes."""
        b = C.c_uint64()
        _check(lib().kmx_index_text(self._h, None, 0, C.byref(b)))
        return int(b.value)

    def search_device(self, d_qranks_ptr, d_qoff_ptr, nq, flags=SEARCH_DEFAULT, stream=0, result=None):
        """Device-buffer batch search (kmx_search_batch_device) on a caller-owned hipStream_t."""
        r = result or Result()
        _check(lib().kmx_search_batch_device(self._h, d_qranks_ptr, d_qoff_ptr, nq, flags, stream or None, C.byref(r._h)))
        r._index = self
        return r

    def search_windows(self, ranks, roff, w, stride=1, flags=SEARCH_DEFAULT, result=None):
        """kmx_search_windows: every w-letter window of every read (ranks / roff shaped like qranks / qoff), at offsets 0, stride,
        2 * stride ... of each read, as one query each; w must be one of the index's ks.  Result.window_offsets() maps reads to
        queries; everything else is an ordinary Result."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        r = result or Result()
        o = WindowOptions(C.sizeof(WindowOptions), int(w), int(stride), int(flags))
        _check(lib().kmx_search_windows(self._h, ranks.ctypes.data if ranks.size else None, roff.ctypes.data, roff.size - 1,
                                        C.byref(o), C.byref(r._h)))
        r._index = self
        return r

    def search_windows_device(self, d_ranks_ptr, d_roff_ptr, nr, w, stride=1, flags=SEARCH_DEFAULT, stream=0, result=None):
        """kmx_search_windows_device on a caller-owned hipStream_t; `result` may be a handle of search_device and the other way round."""
        r = result or Result()
        o = WindowOptions(C.sizeof(WindowOptions), int(w), int(stride), int(flags))
        _check(lib().kmx_search_windows_device(self._h, d_ranks_ptr, d_roff_ptr, nr, C.byref(o), stream or None, C.byref(r._h)))
        r._index = self
        return r

    def vote_windows(self, ranks, roff, w, stride=1, band=0, min_votes=1, max_occ=0):
        """kmx_search_windows and kmx_windows_vote in a row: the Loci of a batch of reads."""
        r = self.search_windows(ranks, roff, w, stride)
        try:
            return r.vote(band, min_votes, max_occ)
        finally:
            r.close()

    def map_reads(self, ranks, roff, w, stride=1, band=0, min_votes=1, max_occ=0, max_edits=0, max_span=None, scripts=False):
        """kmx_search_windows, kmx_windows_vote and kmx_loci_align in a row: (Loci, Alignments) of a batch of reads.  max_span=None
        sets no limit on the span of the loci that are aligned.  scripts=True adds kmx_alignments_scripts (the CIGAR of every read's
        best alignment): (Loci, Alignments, Scripts)."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        if max_span is None:
            max_span = 0xFFFFFFFF
        with contextlib.ExitStack() as opened:                         # closes what was made, the last first, when a later call raises
            with contextlib.closing(self.search_windows(ranks, roff, w, stride)) as r:
                loci = r.vote(band, min_votes, max_occ)
            opened.callback(loci.close)
            al = loci.align(self, ranks, roff, max_edits, max_span)
            opened.callback(al.close)
            out = (loci, al, al.scripts(self, loci, ranks, roff)) if scripts else (loci, al)
            opened.pop_all()
        return out

    def strand_reads(self, ranks, roff, complement, reads=None):
        """kmx_reads_strands: the reads go up once and the doubled batch (read i, then its reverse complement under the rank table
        `complement`) is made on the device, on a stream the returned StrandReads owns (`reads` reuses one)."""
        ranks = np.ascontiguousarray(ranks, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        comp = None if complement is None else np.ascontiguousarray(complement, np.uint8)
        s = reads or StrandReads()
        _check(lib().kmx_reads_strands(self._h, ranks.ctypes.data if ranks.size else None, roff.ctypes.data, roff.size - 1,
                                       comp.ctypes.data if comp is not None else None, C.byref(s._h)))
        return s

    def strand_reads_device(self, d_ranks_ptr, d_roff_ptr, nr, complement, stream=0, reads=None):
        """kmx_reads_strands_device: the doubled batch from reads that are on the device already, on a caller-owned hipStream_t."""
        comp = None if complement is None else np.ascontiguousarray(complement, np.uint8)
        s = reads or StrandReads()
        _check(lib().kmx_reads_strands_device(self._h, d_ranks_ptr, d_roff_ptr, nr, comp.ctypes.data if comp is not None else None,
                                              stream or None, C.byref(s._h)))
        return s

    def map_reads_strands(self, ranks, roff, w, complement, stride=1, band=0, min_votes=1, max_occ=0, max_edits=0, max_span=None, scripts=False,
                          tags=False, letters=None, secondaries=0, clip=None, supplementary=None, realign=None, pileup=None):
        """map_reads on both strands: kmx_reads_strands, kmx_search_windows_device, kmx_windows_vote, kmx_loci_align_device and
        kmx_alignments_fold_strands in a row, all on the stream of the StrandReads.  Returns (StrandReads, Loci, Alignments,
        Placements): the loci and alignments are those of the doubled batch (internal read 2i is read i, 2i + 1 its reverse
        complement), the placements one per read.  scripts=True appends kmx_placements_scripts (the CIGARs of the winners).
        tags=True (needs `letters`, the rank -> letter table; implies scripts) appends a SamTags(mapq, md, None, None):
        kmx_placements_mapq and kmx_scripts_md.  secondaries=N > 0 appends, behind everything else, the Secondaries of
        kmx_placements_secondaries with max_secondary = N and no max_delta.  clip (a dict of the scoring arguments of Scripts.clip,
        {} for the defaults; needs scripts=True) appends, as the very last element, the Clips of kmx_scripts_clip over the scripts;
        with tags=True the Md then is kmx_clips_md, that of the clipped entries.  supplementary (a dict of the arguments of
        Clips.supplementaries, {} for the defaults; needs scripts=True and clip) runs last: the KMX_SCRIPT_ALL scripts of the
        doubled batch, their clips under the same `clip` scoring and kmx_clips_supplementaries on the placements, and appends, as
        the very last element, the Supplementaries; its all_scripts / all_clips are those two handles and its close() closes them.
        realign (a dict that may hold scratch_bytes, {} for the default; needs scripts=True and clip): the Clips of the placements and
        the all-loci Clips behind supplementary come from kmx_scripts_realign_device under the `clip` scoring in the place of
        kmx_scripts_clip; the secondaries are untouched.  With realign=None every returned tuple is what it was without the keyword.
        pileup (a dict that may hold into, lo, hi, min_score, min_mapq, skip_low, mode, tile; {} for the defaults; needs scripts=True,
        and tags=True when min_mapq > 0) runs last of all: Clips.pileup on the placements' Clips when clip is given (trimmed or
        realigned), else Scripts.pileup on the scripts, with the Mapq of the tags when min_mapq > 0, and appends the Pileup as the very
        last element.  into: a Pileup the call adds to (add=True); it is the caller's, and stays open when a later step raises.  With
        pileup=None every call and every returned tuple is what it was without the keyword."""
        return self._map_chain("map_reads_strands", ranks, roff, w, complement, None, None, stride, band, min_votes, max_occ, max_edits, max_span,
                               scripts, tags, letters, secondaries, clip, supplementary, realign, pileup)

    def map_pairs(self, ranks, roff, w, complement, min_insert, max_insert, orientation=PAIR_FR, unpaired_penalty=None, stride=1, band=0,
                  min_votes=1, max_occ=0, max_edits=0, max_span=None, scripts=False, rescue=False, rescue_edits=None, rescue_discordant=False,
                  tags=False, letters=None, secondaries=0, clip=None, supplementary=None, realign=None, pileup=None):
        """map_reads_strands for paired reads: the reads are interleaved mates (read 2p is mate 1 of pair p, read 2p + 1 its mate 2, so
        their number is even), and kmx_alignments_fold_pairs stands in the fold's place.  Returns (StrandReads, Loci, Alignments,
        Placements, Pairs); scripts=True appends kmx_placements_scripts (the CIGARs of the chosen loci).  rescue=True runs
        kmx_pairs_rescue behind the fold (within rescue_edits edits, None: max_edits; rescue_discordant: DISCORDANT pairs too) and
        appends its Rescues as the last element; the scripts then are those of the placements after the rescue.  tags=True (needs
        `letters`, the rank -> letter table; implies scripts) appends, behind everything else, a SamTags(mapq, md, rescue_scripts,
        rescue_md): kmx_placements_mapq with the pairs (its budget the larger of max_edits and rescue_edits), kmx_scripts_md, and
        after a rescue kmx_rescues_scripts and kmx_rescues_md (else None).  secondaries=N > 0 appends, behind everything else, the
        Secondaries of kmx_placements_secondaries (max_secondary = N, no max_delta) on the placements as they then are: after the
        rescue, so that the primaries are final.  clip (a dict of the scoring arguments of Scripts.clip, {} for the defaults; needs
        scripts=True) appends, as the very last elements, the Clips of kmx_scripts_clip over the scripts and, with rescue=True, the
        Clips of the rescued mates' scripts.  Clips.scripts is the Scripts they were made from: SamTags.rescue_scripts with tags=True;
        without tags that Scripts is returned nowhere else, Clips.close() does not close it, and the caller closes it;
        with tags=True md and rescue_md then are kmx_clips_md and kmx_clips_rescues_md, those of the clipped entries.
        supplementary (a dict of the arguments of Clips.supplementaries, {} for the defaults; needs scripts=True and clip) runs
        last, on the placements as the rescue left them (a rescued mate has no parts), and appends the Supplementaries behind the
        Clips, as in map_reads_strands.  realign: as in map_reads_strands; the clips of the rescued mates stay those of kmx_scripts_clip
        (their scripts index the rescue's jobs, not alignments).  pileup: as in map_reads_strands; after a rescue the rescued mates'
        Clips (or Scripts) go into the same Pileup; a Scripts of the rescued mates that is made for this alone is closed by the chain."""
        return self._map_chain("map_pairs", ranks, roff, w, complement, (min_insert, max_insert, orientation, unpaired_penalty),
                               (max_edits if rescue_edits is None else rescue_edits, rescue_discordant) if rescue else None,
                               stride, band, min_votes, max_occ, max_edits, max_span, scripts, tags, letters, secondaries, clip, supplementary, realign,
                               pileup)

    def _map_chain(self, who, ranks, roff, w, complement, insert, rescue, stride, band, min_votes, max_occ, max_edits, max_span, scripts, tags,
                   letters, secondaries, clip, supplementary=None, realign=None, pileup=None):
        """What map_reads_strands (insert=None) and map_pairs (insert: min_insert, max_insert, orientation, unpaired_penalty; rescue:
        None or the rescue's edits and whether it takes DISCORDANT pairs) return: the front and the fold, then the stages that were
        asked for, every one on the stream of the StrandReads."""
        if tags and letters is None:
            raise ValueError(f"{who}: tags=True needs letters")
        if clip is not None and not scripts:
            raise ValueError(f"{who}: clip needs scripts=True")
        if supplementary is not None and (not scripts or clip is None):
            raise ValueError(f"{who}: supplementary needs scripts=True and clip")
        if realign is not None and (not scripts or clip is None):
            raise ValueError(f"{who}: realign needs scripts=True and clip")
        if pileup is not None:
            unknown = set(pileup) - {"into", "lo", "hi", "min_score", "min_mapq", "skip_low", "mode", "tile"}
            if unknown:
                raise ValueError(f"{who}: pileup holds unknown keys {sorted(unknown)}")
            if not scripts:
                raise ValueError(f"{who}: pileup needs scripts=True")
            if pileup.get("min_mapq", 0) > 0 and not tags:
                raise ValueError(f"{who}: pileup with min_mapq > 0 needs tags=True")
        if insert is not None:
            roff = np.ascontiguousarray(roff, np.uint64)
            if (roff.size - 1) % 2:
                raise ValueError(f"{who}: an odd number of reads; the reads are interleaved mates")
        if max_span is None:
            max_span = 0xFFFFFFFF
        pairs = res = sc = cl = rsc = rcl = sam = sec = sup = pu = None
        with contextlib.ExitStack() as opened:                         # closes what was made, the last first, when a later call raises

            def keep(h):
                opened.callback(h.close)
                return h

            reads = keep(self.strand_reads(ranks, roff, complement))
            d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
            with contextlib.closing(self.search_windows_device(d_ranks2, d_roff2, nr2, w, stride, stream=stream)) as r:
                loci = keep(r.vote(band, min_votes, max_occ))
            al = keep(loci.align_device(self, d_ranks2, d_roff2, nr2, max_edits, max_span, stream=stream))
            loci._reads = al._reads = reads                            # every handle below is made from these two, or from `reads`
            if insert is None:
                pl = keep(al.fold_strands(loci, stream=stream))
            else:
                pl, pairs = keep(Placements()), keep(Pairs())
                min_insert, max_insert, orientation, unpaired_penalty = insert
                al.fold_pairs(loci, min_insert, max_insert, orientation, unpaired_penalty, stream=stream, placements=pl, pairs=pairs)
                if rescue is not None:
                    res = keep(Rescues())
                    pairs.rescue(self, reads, loci, al, pl, min_insert, max_insert, rescue[0], orientation, rescue[1], unpaired_penalty, rescues=res)
            if scripts or tags:
                sc = keep(pl.scripts(self, reads, loci, al))

            def clipped(s, **on):                                      # the Clips of the scripts s of the alignments, trimmed or realigned
                if realign is None:
                    return s.clip(**clip, **on)
                return s.realign_device(self, al, d_ranks2, d_roff2, nr2, **clip, **realign, stream=stream)

            if clip is not None:
                cl = keep(clipped(sc))
                if res is not None:
                    rsc = keep(res.scripts(self, reads))
                    rcl = keep(rsc.clip(**clip))
            if tags:
                mq = keep(pl.mapq(max_edits if rescue is None else max(max_edits, rescue[0]), pairs))
                md = keep(sc.md(self, al, letters) if cl is None else cl.md(self, sc, al, letters))
                rmd = None
                if res is not None:
                    rsc = rsc or keep(res.scripts(self, reads))
                    rmd = keep(rsc.md(self, res, letters) if rcl is None else rcl.md(self, rsc, res, letters))
                sam = SamTags(mq, md, rsc, rmd)
            if secondaries:
                sec = keep(pl.secondaries(loci, al, secondaries))       # last, on the placements as the rescue left them
            if supplementary is not None:                              # last too: every aligned locus of both strands, clipped as the winners are
                asc = keep(al.scripts_device(self, loci, d_ranks2, d_roff2, nr2, all=True, stream=stream))
                acl = keep(clipped(asc, stream=stream))
                sup = keep(acl.supplementaries(reads, loci, al, pl, asc, **supplementary, stream=stream))
                sup.all_scripts, sup.all_clips, sup._owns = asc, acl, True
            if pileup is not None:                                     # last of all: the per-read answers into a per-position one
                opt = {k: v for k, v in pileup.items() if k != "into"}
                into = pileup.get("into")
                mapq = sam.mapq if opt.get("min_mapq", 0) > 0 else None
                pu = into if into is not None else keep(Pileup())     # (an `into` handle is the caller's: not closed when a step raises)

                def piled(s, c, source, add):                          # the scripts s, or their clips c, over `source` into pu
                    on = dict(mapq=mapq, add=add, stream=stream, pileup=pu, **opt)
                    return s.pileup(self, source, reads, **on) if c is None else c.pileup(self, s, source, reads, **on)

                piled(sc, cl, al, into is not None)
                if res is not None:
                    own = rsc is None                                  # made for this alone: closed here
                    rs = rsc if rsc is not None else res.scripts(self, reads)
                    try:
                        piled(rs, rcl, res, True)
                    finally:
                        if own:
                            if pu._h:
                                pu.counts()                            # (waits: the kernels that read rs have finished)
                            rs.close()
            opened.pop_all()
        # the four of every chain, then in this order whatever was asked for: a stage that did not run leaves no gap
        return tuple(x for x in (reads, loci, al, pl, pairs, sc, res, sam, sec, cl, rcl, sup, pu) if x is not None)

    def debug_words(self):
        w = np.zeros(16, np.uint64)
        _check(lib().kmx_debug_words(self._h, w.ctypes.data))
        return w

    def stats_enable(self, on=True):
        _check(lib().kmx_stats_enable(self._h, int(on)))

    def stats_reset(self):
        _check(lib().kmx_stats_reset(self._h))

    def stats(self):
        arr = (KernelStat * KMX_N_KERNELS)()
        n = C.c_uint32()
        _check(lib().kmx_stats_get(self._h, arr, C.byref(n)))
        return {arr[i].name.decode(): {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms)} for i in range(n.value)}

    def close(self):
        if self._h:
            lib().kmx_index_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_hits(hit_off, positions):
    """List of per-query position arrays."""
    return [positions[int(hit_off[i]):int(hit_off[i + 1])] for i in range(len(hit_off) - 1)]
