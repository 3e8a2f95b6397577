"""Loader of libnohuman_engine.so (ctypes).  Fails loudly if the library is missing."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NOHUMAN_ENGINE_LIB", os.path.join(_HERE, "libnohuman_engine.so"))
_LIB = None


class nh_result(C.Structure):
    _fields_ = [("call", C.c_uint32), ("total_kmers", C.c_uint32), ("clade_hits", C.c_uint32),
                ("hit_groups", C.c_uint32)]


class nh_stats(C.Structure):
    _fields_ = [("total_sequences", C.c_uint64), ("classified", C.c_uint64),
                ("unclassified", C.c_uint64), ("total_bases", C.c_uint64),
                ("table_lookups", C.c_uint64), ("seconds", C.c_double)]


class nh_db_info(C.Structure):
    _fields_ = [("k", C.c_uint64), ("l", C.c_uint64), ("spaced_seed_mask", C.c_uint64),
                ("toggle_mask", C.c_uint64), ("minimum_acceptable_hash_value", C.c_uint64),
                ("revcom_version", C.c_int32), ("dna_db", C.c_int32), ("capacity", C.c_uint64),
                ("size", C.c_uint64), ("key_bits", C.c_uint64), ("value_bits", C.c_uint64),
                ("node_count", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32)]


class nh_db_check(C.Structure):
    _fields_ = [("non_empty_cells", C.c_uint64), ("max_value", C.c_uint64), ("load_factor", C.c_double),
                ("seconds", C.c_double)]


class nh_options(C.Structure):
    _fields_ = [("minimum_hit_groups", C.c_uint32), ("linear_probing", C.c_int32),
                ("reset_per_mate", C.c_int32), ("ambiguity_rule", C.c_int32)]


class nh_run_args(C.Structure):
    _fields_ = [("db_dir", C.c_char_p), ("in1", C.c_char_p), ("in2", C.c_char_p),
                ("out1", C.c_char_p), ("out2", C.c_char_p), ("kraken_output", C.c_char_p),
                ("report", C.c_char_p), ("confidence", C.c_double), ("threads", C.c_uint32),
                ("keep_human", C.c_int32), ("n_devices", C.c_int32),
                ("device_ids", C.POINTER(C.c_int32)), ("out_codec", C.c_int32), ("codec_threads", C.c_uint32)]


class nh_run_extras(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mask", C.c_int32), ("human_out1", C.c_char_p),
                ("human_out2", C.c_char_p), ("calls", C.c_char_p), ("human_ids", C.c_char_p)]


NH_RS_QBINS = 94


class nh_read_class(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("min_len", C.c_uint64), ("max_len", C.c_uint64),
                ("gc", C.c_uint64), ("other", C.c_uint64), ("qual_reads", C.c_uint64), ("qual_bases", C.c_uint64),
                ("qhist", C.c_uint64 * NH_RS_QBINS)]


class nh_read_stats(C.Structure):
    _fields_ = [("cls", (nh_read_class * 2) * 2), ("median_len", (C.c_uint64 * 2) * 3), ("n50", (C.c_uint64 * 2) * 3),
                ("mates", C.c_int32), ("reserved", C.c_int32)]


NH_MAX_TAXON_OUTS = 8
NH_TAXON_OTHER = 0


class nh_taxon_out(C.Structure):
    _fields_ = [("taxid", C.c_uint64), ("out1", C.c_char_p), ("out2", C.c_char_p), ("fragments", C.c_uint64)]


class nh_taxon_minimizers(C.Structure):
    _fields_ = [("taxid", C.c_uint64), ("reads_clade", C.c_uint64), ("reads_own", C.c_uint64), ("minimizers_clade", C.c_uint64),
                ("minimizers_own", C.c_uint64), ("distinct_clade", C.c_uint64), ("distinct_own", C.c_uint64),
                ("db_cells_clade", C.c_uint64), ("db_cells_own", C.c_uint64)]


class nh_minimizer_data(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("in_report", C.c_int32), ("table", C.c_char_p),
                ("taxa", C.POINTER(nh_taxon_minimizers)), ("taxa_cap", C.c_uint32), ("n_taxa", C.c_uint32)]


NH_MAX_HOST_TAXA = 16


class nh_host_filter(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_host", C.c_uint32), ("n_keep", C.c_uint32), ("reserved", C.c_uint32),
                ("host_taxids", C.POINTER(C.c_uint64)), ("keep_taxids", C.POINTER(C.c_uint64)),
                ("host_fragments", C.c_uint64), ("spared_fragments", C.c_uint64)]


class nh_read_dust(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_uint32), ("masked_bases", C.c_uint64)]


class nh_host_intervals(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("path", C.c_char_p),
                ("fragments", C.c_uint64), ("intervals", C.c_uint64), ("covered_bases", C.c_uint64)]


class nh_host_bases(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_uint32), ("gap", C.c_uint32), ("reserved", C.c_uint32),
                ("host_bases", C.c_uint64), ("masked_bases", C.c_uint64), ("closed_bases", C.c_uint64)]


NH_HOST_GAP_MAX = 4096


class nh_host_cut(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_uint32), ("gap", C.c_uint32), ("min_piece", C.c_uint32),
                ("host_bases", C.c_uint64), ("pieces", C.c_uint64), ("piece_bases", C.c_uint64), ("cut_bases", C.c_uint64),
                ("short_bases", C.c_uint64), ("dropped_reads", C.c_uint64), ("closed_bases", C.c_uint64)]


HOST_CUT_COUNTS = ("host_bases", "pieces", "piece_bases", "cut_bases", "short_bases", "dropped_reads")  # nh_host_cut_device's d_counts


class nh_gzip_model_opts(C.Structure):
    _fields_ = [("ways", C.c_uint32), ("region_bytes", C.c_uint32), ("chunk_bytes", C.c_uint64), ("prices", C.c_int32),
                ("bgzf", C.c_int32), ("threads", C.c_uint32), ("reserved", C.c_uint32),
                ("region_sizes", C.POINTER(C.c_uint32)), ("region_sizes_cap", C.c_uint64)]


class nh_build_args(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_fasta", C.c_uint32), ("fasta", C.POINTER(C.c_char_p)),
                ("out_dir", C.c_char_p), ("taxid", C.c_uint64), ("taxon_name", C.c_char_p), ("load_factor", C.c_double),
                ("capacity", C.c_uint64), ("piece_kmers", C.c_uint64), ("device", C.c_int32), ("threads", C.c_uint32),
                ("force", C.c_int32)]


class nh_build_stats(C.Structure):
    _fields_ = [("sequences", C.c_uint64), ("bases", C.c_uint64), ("kmers", C.c_uint64), ("ambiguous_kmers", C.c_uint64),
                ("distinct_minimizers", C.c_uint64), ("capacity", C.c_uint64), ("size", C.c_uint64),
                ("seconds_read", C.c_double), ("seconds_count", C.c_double), ("seconds_insert", C.c_double),
                ("seconds_write", C.c_double)]


# The two structs above are the header's FIRST layout (NH_BUILD_ARGS_SIZE_V1 / NH_BUILD_STATS_SIZE_V1), which the library goes
# on accepting by struct_size; the _v2 pair is its second (NH_BUILD_ARGS_SIZE_V2 / NH_BUILD_STATS_SIZE_V2: masking), accepted
# likewise; the _v3 pair is the header's present structs: the same fields, then what was added at the end (several taxa).
class nh_build_args_v2(nh_build_args):
    _fields_ = [("mask_low_complexity", C.c_int32), ("reserved1", C.c_int32)]


class nh_build_stats_v2(nh_build_stats):
    _fields_ = [("masked_bases", C.c_uint64), ("seconds_mask", C.c_double)]


class nh_build_taxon_stats(C.Structure):
    _fields_ = [("taxid", C.c_uint64), ("sequences", C.c_uint64), ("bases", C.c_uint64), ("kmers", C.c_uint64),
                ("cells", C.c_uint64)]


class nh_build_args_v3(nh_build_args_v2):
    _fields_ = [("taxa_file", C.c_char_p), ("taxon_stats", C.POINTER(nh_build_taxon_stats)), ("taxon_stats_cap", C.c_uint32),
                ("reserved2", C.c_uint32)]


class nh_build_stats_v3(nh_build_stats_v2):
    _fields_ = [("taxa", C.c_uint64)]


class nh_extend_args(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("base_cells_cap", C.c_uint32), ("base_dir", C.c_char_p),
                ("base_cells", C.POINTER(C.c_uint64))]


class nh_extend_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("base_size", C.c_uint64), ("base_nodes", C.c_uint64),
                ("base_value_bits", C.c_uint64), ("nodes_added", C.c_uint64), ("cells_added", C.c_uint64),
                ("shadowed_cells", C.c_uint64), ("load", C.c_double), ("seconds_load", C.c_double), ("seconds_rekey", C.c_double)]


class nh_exclude_args(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_fasta", C.c_uint32), ("fasta", C.POINTER(C.c_char_p))]


class nh_exclude_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("sequences", C.c_uint64), ("bases", C.c_uint64),
                ("kmers", C.c_uint64), ("ambiguous_kmers", C.c_uint64), ("lookups", C.c_uint64),
                ("excluded_minimizers", C.c_uint64), ("kept_minimizers", C.c_uint64), ("seconds_read", C.c_double),
                ("seconds_exclude", C.c_double)]


class nh_bam_info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("records", C.c_uint64), ("reads", C.c_uint64),
                ("bases", C.c_uint64), ("skipped_secondary", C.c_uint64), ("skipped_empty", C.c_uint64),
                ("reverse_complemented", C.c_uint64), ("missing_qualities", C.c_uint64), ("digest", C.c_uint64)]


class nh_bam_pair_info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("paired", C.c_uint32), ("pairs", C.c_uint64), ("bases1", C.c_uint64),
                ("bases2", C.c_uint64), ("digest1", C.c_uint64), ("digest2", C.c_uint64)]


# every symbol include/nohuman_engine.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "nh_last_error": (C.c_char_p, []),
    "nh_abi_version": (C.c_int, []),
    "nh_probe": (C.c_int, [C.c_char_p, C.c_size_t]),
    "nh_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "nh_open": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "nh_open_images": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, C.c_int,
                                 C.POINTER(_P)]),
    "nh_open_synthetic": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int,
                                    C.POINTER(_P)]),
    "nh_synthetic_add_sequences": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, _P]),
    "nh_close": (C.c_int, [_P]),
    "nh_db_info_get": (C.c_int, [_P, C.POINTER(nh_db_info)]),
    "nh_db_check_get": (C.c_int, [_P, C.POINTER(nh_db_check)]),
    "nh_options_get": (C.c_int, [_P, C.POINTER(nh_options)]),
    "nh_options_set": (C.c_int, [_P, C.POINTER(nh_options)]),
    "nh_taxon_external": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64)]),
    "nh_table_download": (C.c_int, [_P, _P, C.c_uint64]),
    "nh_taxonomy_image": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "nh_opts_image": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "nh_classify_batch": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_double, _P, _P, _P,
                                    C.c_uint64]),
    "nh_kmer_taxa_entries": (C.c_uint64, [_P, _P, C.c_uint64, C.c_uint32]),
    "nh_classify_batch_device": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_double, _P, _P,
                                           _P, _P, _P]),
    "nh_classify_records_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_uint32, C.c_double, _P,
                                             _P, _P, _P, _P]),
    "nh_stats_get": (C.c_int, [_P, C.POINTER(nh_stats)]),
    "nh_stats_reset": (C.c_int, [_P]),
    "nh_compress_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32]),
    "nh_compress_file_device": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int32]),
    "nh_gzip_gpu_file": (C.c_int, [C.c_int32, _P, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64)]),
    "nh_bgzf_gpu_file": (C.c_int, [C.c_int32, _P, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64)]),
    "nh_gzip_model_file": (C.c_int, [_P, C.c_uint64, C.c_char_p, C.POINTER(nh_gzip_model_opts), C.POINTER(C.c_uint64)]),
    "nh_gunzip_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "nh_cache_bytes": (C.c_uint64, [C.c_int32, C.c_int32]),
    "nh_gunzip_device_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "nh_fastx_scan": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint64)]),
    "nh_bam_scan": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(nh_bam_info)]),
    "nh_bam_scan_pairs": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(nh_bam_info), C.POINTER(nh_bam_pair_info)]),
    "nh_bam_paired": (C.c_int, [C.c_char_p]),
    "nh_bam_select_pairs_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_int, _P, C.c_uint64, _P, _P, _P]),
    "nh_bam_to_fastq_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "nh_bam_select_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_int, _P, C.c_uint64, _P, _P, _P]),
    "nh_run": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_stats)]),
    "nh_run_engine":(C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_stats)]),
    "nh_run_split": (C.c_int, [C.POINTER(nh_run_args), C.c_char_p, C.c_char_p, C.POINTER(nh_stats)]),
    "nh_run_engine_split": (C.c_int, [_P, C.POINTER(nh_run_args), C.c_char_p, C.c_char_p, C.POINTER(nh_stats)]),
    "nh_run_mask": (C.c_int, [C.POINTER(nh_run_args), C.c_char_p, C.c_char_p, C.POINTER(nh_stats)]),
    "nh_run_engine_mask": (C.c_int, [_P, C.POINTER(nh_run_args), C.c_char_p, C.c_char_p, C.POINTER(nh_stats)]),
    "nh_run_ex": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.POINTER(nh_stats)]),
    "nh_run_engine_ex": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.POINTER(nh_stats)]),
    "nh_quality_mask_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P]),
    "nh_run_minq": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.POINTER(nh_stats)]),
    "nh_run_engine_minq": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.POINTER(nh_stats)]),
    "nh_read_stats_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint32, _P]),
    "nh_run_rstats": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                C.POINTER(nh_read_stats), C.POINTER(nh_stats)]),
    "nh_run_engine_rstats": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                       C.POINTER(nh_read_stats), C.POINTER(nh_stats)]),
    "nh_run_taxa": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                              C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_stats)]),
    "nh_run_engine_taxa": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                     C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_stats)]),
    "nh_run_mdata": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p, C.POINTER(nh_read_stats),
                               C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data), C.POINTER(nh_stats)]),
    "nh_run_engine_mdata": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                      C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data),
                                      C.POINTER(nh_stats)]),
    "nh_run_host": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p, C.POINTER(nh_read_stats),
                              C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data), C.POINTER(nh_host_filter),
                              C.POINTER(nh_stats)]),
    "nh_run_engine_host": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                     C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data),
                                     C.POINTER(nh_host_filter), C.POINTER(nh_stats)]),
    "nh_run_dust": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p, C.POINTER(nh_read_stats),
                              C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data), C.POINTER(nh_host_filter),
                              C.POINTER(nh_read_dust), C.POINTER(nh_stats)]),
    "nh_run_engine_dust": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                     C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data),
                                     C.POINTER(nh_host_filter), C.POINTER(nh_read_dust), C.POINTER(nh_stats)]),
    "nh_dust_reads_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, _P, _P, _P]),
    "nh_run_intervals": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p, C.POINTER(nh_read_stats),
                                   C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data), C.POINTER(nh_host_filter),
                                   C.POINTER(nh_read_dust), C.POINTER(nh_host_intervals), C.POINTER(nh_stats)]),
    "nh_run_engine_intervals": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                          C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data),
                                          C.POINTER(nh_host_filter), C.POINTER(nh_read_dust), C.POINTER(nh_host_intervals),
                                          C.POINTER(nh_stats)]),
    "nh_run_hostbases": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p, C.POINTER(nh_read_stats),
                                   C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data), C.POINTER(nh_host_filter),
                                   C.POINTER(nh_read_dust), C.POINTER(nh_host_intervals), C.POINTER(nh_host_bases), C.POINTER(nh_stats)]),
    "nh_run_engine_hostbases": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                          C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data),
                                          C.POINTER(nh_host_filter), C.POINTER(nh_read_dust), C.POINTER(nh_host_intervals),
                                          C.POINTER(nh_host_bases), C.POINTER(nh_stats)]),
    "nh_run_hostcut": (C.c_int, [C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p, C.POINTER(nh_read_stats),
                                 C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data), C.POINTER(nh_host_filter),
                                 C.POINTER(nh_read_dust), C.POINTER(nh_host_intervals), C.POINTER(nh_host_bases), C.POINTER(nh_host_cut),
                                 C.POINTER(nh_stats)]),
    "nh_run_engine_hostcut": (C.c_int, [_P, C.POINTER(nh_run_args), C.POINTER(nh_run_extras), C.c_uint32, C.c_char_p,
                                        C.POINTER(nh_read_stats), C.POINTER(nh_taxon_out), C.c_uint32, C.POINTER(nh_minimizer_data),
                                        C.POINTER(nh_host_filter), C.POINTER(nh_read_dust), C.POINTER(nh_host_intervals),
                                        C.POINTER(nh_host_bases), C.POINTER(nh_host_cut), C.POINTER(nh_stats)]),
    "nh_host_cut_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint64, C.c_int, _P, C.c_uint32, _P, C.c_uint64, _P, _P, _P, _P]),
    "nh_cover_close_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_uint32, _P, _P]),
    "nh_host_cover_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P]),
    "nh_cover_intervals_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P, _P]),
    "nh_host_table_image": (C.c_int, [_P, C.c_size_t, C.POINTER(nh_host_filter), _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "nh_host_filter_device": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P]),
    "nh_minimizer_marks_bytes": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "nh_minimizer_mark_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P]),
    "nh_minimizer_count_device": (C.c_int, [_P, _P, _P, _P]),
    "nh_read_stats_write": (C.c_int, [C.POINTER(nh_read_stats), C.c_char_p]),
    "nh_build_db": (C.c_int, [C.POINTER(nh_build_args), C.POINTER(nh_build_stats)]),  # (or their _v2 / _v3 subclasses)
    "nh_build_check": (C.c_int, [C.POINTER(nh_build_args), C.POINTER(nh_build_stats)]),
    "nh_extend_db": (C.c_int, [C.POINTER(nh_build_args), C.POINTER(nh_extend_args), C.POINTER(nh_build_stats),
                               C.POINTER(nh_extend_stats)]),
    "nh_extend_check": (C.c_int, [C.POINTER(nh_build_args), C.POINTER(nh_extend_args), C.POINTER(nh_build_stats),
                                  C.POINTER(nh_extend_stats)]),
    "nh_build_db_exclude": (C.c_int, [C.POINTER(nh_build_args), C.POINTER(nh_exclude_args), C.POINTER(nh_build_stats),
                                      C.POINTER(nh_exclude_stats)]),
    "nh_exclude_check": (C.c_int, [C.POINTER(nh_build_args), C.POINTER(nh_exclude_args), C.POINTER(nh_build_stats),
                                   C.POINTER(nh_exclude_stats)]),
    "nh_dust_mask": (C.c_int, [C.c_int32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64,
                               C.POINTER(C.c_uint64)]),
    "nh_allreduce_counters": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_uint64), C.c_char_p,
                                        C.c_size_t]),
}


def _preload_hip_runtime():
    """If PyTorch-ROCm is installed it bundles its own libamdhip64 (same SONAME as /opt/rocm's).
    Load that copy first so that this library and torch share ONE HIP runtime in the process;
    otherwise device pointers and streams could not be exchanged between the two."""
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    cand = os.path.join(libdir, "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libnohuman_engine.so is not built (%s missing): run `make -C nohuman_amd/csrc` "
                "or __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB
