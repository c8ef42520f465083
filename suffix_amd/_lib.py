"""ctypes binding of libsuffix_hip.so (C ABI: include/suffix_hip.h).

The product loads exactly one native library: the in-tree `libsuffix_hip.so`
built by hipcc for gfx950 (`python -c "import __graft_entry__ as g; g.build()"`).
There is NO CPU fallback: if the library is missing, or no HIP device is
visible, every compute entry point raises.

`Engine(lib_path=...)` exists so the test-suite can bind the same ABI exported
by the kernel-logic emulator (tests/emu/libsuffix_emu.so) and development
scripts the hook-enabled build (scripts/_devlib.py); product code never passes
it, and the package reads no environment variable.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libsuffix_hip.so")

SFX_OK = 0
SFX_ERR_TOO_LARGE = 2
SFX_ERR_NO_DEVICE = 3

_vp, _u64, _u32, _int = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", _u64),
                ("total_ms", ctypes.c_double), ("algo_bytes", ctypes.c_double)]


class BuildStats(ctypes.Structure):
    _fields_ = [("n", _u64), ("sigma", _u32), ("bits_per_symbol", _u32), ("key_bits", _u32),
                ("symbols_per_key", _u32), ("rounds", _u32), ("reserved", _u32),
                ("active_after_initial", _u64), ("radix_passes", _u64),
                ("elements_sorted", _u64), ("small_bucket_resolved", _u64),
                ("tile_sorted", _u64), ("large_sorted", _u64), ("text_rounds", _u32), ("rank_rounds", _u32),
                ("deep_gathers", _u64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class FmInfo(ctypes.Structure):
    _fields_ = [("n", _u64), ("bytes", _u64), ("sigma", _u32), ("occ_step", _u32), ("sample_step", _u32), ("nsamples", _u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ResourceStats(ctypes.Structure):
    _fields_ = [("device_bytes", _u64), ("device_allocs", _u64), ("pinned_bytes", _u64), ("pinned_allocs", _u64), ("streams", _u64),
                ("events", _u64), ("pooled_bytes", _u64), ("pooled_buffers", _u64), ("device_allocs_total", _u64), ("reserved", _u64 * 7)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class RunsFilter(ctypes.Structure):
    _fields_ = [("min_period", _u32), ("max_period", _u32), ("min_len", _u32), ("reserved", _u32)]


# every symbol include/suffix_hip.h declares: (name, restype, argtypes)
ABI = [
    ("sfx_strerror", ctypes.c_char_p, [_int]),
    ("sfx_device_count", _int, []),
    ("sfx_last_hip_error", ctypes.c_char_p, []),
    ("sfx_build_sa_u32", _int, [_vp, _u64, _vp]),
    ("sfx_release_cached_buffers", None, []),
    ("sfx_resource_stats", _int, [ctypes.POINTER(ResourceStats)]),
    ("sfx_build_sa_u64", _int, [_vp, _u64, _vp]),
    ("sfx_widen_u32_to_u64_dev", _int, [_vp, _u64, _vp, _vp]),
    ("sfx_sa_workspace_bytes", _u64, [_u64]),
    ("sfx_build_sa_u32_dev", _int, [_vp, _u64, _vp, _vp, _u64, _vp]),
    ("sfx_build_lcp_u32", _int, [_vp, _u64, _vp, _vp]),
    ("sfx_lcp_workspace_bytes", _u64, [_u64]),
    ("sfx_build_lcp_u32_dev", _int, [_vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_build_sa_lcp_u32", _int, [_vp, _u64, _vp, _vp]),
    ("sfx_sa_lcp_workspace_bytes", _u64, [_u64]),
    ("sfx_build_sa_lcp_u32_dev", _int, [_vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_index_create", _int, [_vp, _u64, _vp, ctypes.POINTER(_vp)]),
    ("sfx_index_create_dev", _int, [_vp, _u64, _vp, _vp, ctypes.POINTER(_vp)]),
    ("sfx_index_query_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_index_destroy", None, [_vp]),
    ("sfx_index_len", _u64, [_vp]),
    ("sfx_index_table", _int, [_vp, _vp]),
    ("sfx_positions_batch", _int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("sfx_contains_batch", _int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("sfx_query_batch_dev", _int, [_vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_lcp_intervals_workspace_bytes", _u64, [_u64]),
    ("sfx_lcp_intervals_dev", _int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_doc_lookup_dev", _int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    ("sfx_suffix_tree_workspace_bytes", _u64, [_u64]),
    ("sfx_suffix_tree_dev", _int, [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   ctypes.POINTER(_u64), ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_suffix_tree_u32", _int, [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_gsa_workspace_bytes", _u64, [_u64, _u64]),
    ("sfx_build_gsa_u32_dev", _int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_build_gsa_u32", _int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    ("sfx_gsa_merge_workspace_bytes", _u64, [_u64, _u64]),
    ("sfx_gsa_merge_dev", _int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp,
                                 ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_gsa_merge_u32", _int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp,
                                 ctypes.POINTER(_u64)]),
    ("sfx_gsa_extend_u32", _int, [_vp, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _u32, _int, _vp, _vp, _vp, ctypes.POINTER(_u64),
                                  ctypes.POINTER(_u32)]),
    ("sfx_gindex_create_dev", _int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, ctypes.POINTER(_vp)]),
    ("sfx_gindex_create", _int, [_vp, _u64, _vp, _u64, _vp, _vp, ctypes.POINTER(_vp)]),
    ("sfx_gindex_query_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_gindex_query", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_gindex_destroy", None, [_vp]),
    ("sfx_repeat_lens_workspace_bytes", _u64, [_u64, _int]),
    ("sfx_repeat_lens_dev", _int, [_vp, _vp, _vp, _u64, _int, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_repeat_spans_workspace_bytes", _u64, [_u64]),
    ("sfx_repeat_spans_dev", _int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _u64, ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_repeat_lens_u32", _int, [_vp, _vp, _vp, _u64, _int, _vp, _vp]),
    ("sfx_repeat_spans_u32", _int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _u64, ctypes.POINTER(_u64)]),
    ("sfx_match_stats_dev", _int, [_vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_index_match_stats_dev", _int, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_gindex_match_stats_dev", _int, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_index_match_stats", _int, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    ("sfx_gindex_match_stats", _int, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    ("sfx_bwt_sample_count", _u64, [_u64, _u32]),
    ("sfx_bwt_dev", _int, [_vp, _u64, _vp, _u32, _vp, _vp, _vp]),
    ("sfx_bwt_u32", _int, [_vp, _u64, _vp, _u32, _vp, _vp]),
    ("sfx_unbwt_workspace_bytes", _u64, [_u64]),
    ("sfx_unbwt_dev", _int, [_vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    ("sfx_unbwt", _int, [_vp, _u64, _vp, _u64, _u32, _vp]),
    ("sfx_fm_bytes", _u64, [_u64, _u32, _u32]),
    ("sfx_fm_create_dev", _int, [_vp, _u64, _vp, _u64, _u32, _u32, _vp, ctypes.POINTER(_vp)]),
    ("sfx_fm_create", _int, [_vp, _u64, _vp, _u64, _u32, _u32, ctypes.POINTER(_vp)]),
    ("sfx_fm_destroy", None, [_vp]),
    ("sfx_fm_info", _int, [_vp, ctypes.POINTER(FmInfo)]),
    ("sfx_fm_count_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    ("sfx_fm_count", _int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("sfx_fm_lookup_dev", _int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    ("sfx_fm_lookup", _int, [_vp, _vp, _u64, _u64, _vp]),
    ("sfx_lz_parse_workspace_bytes", _u64, [_u64]),
    ("sfx_lz_parse_dev", _int, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_lz_decode_workspace_bytes", _u64, [_u64, _u64]),
    ("sfx_lz_decode_dev", _int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp]),
    ("sfx_lz77_u32", _int, [_vp, _u64, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64)]),
    ("sfx_unlz", _int, [_vp, _vp, _vp, _u64, _u64, _vp]),
    ("sfx_mems_workspace_bytes", _u64, [_u64, _u64]),
    ("sfx_mems_dev", _int, [_vp, _u64, _vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                            _vp, _u64, _vp]),
    ("sfx_index_mems_dev", _int, [_vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                  _vp, _u64, _vp]),
    ("sfx_gindex_mems_dev", _int, [_vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                   _vp, _u64, _vp]),
    ("sfx_index_mems", _int, [_vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_gindex_mems", _int, [_vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_hamming_workspace_bytes", _u64, [_u64, _u32, _u64]),
    ("sfx_hamming_dev", _int, [_vp, _u64, _vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                               ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_index_hamming_dev", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                                     ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_gindex_hamming_dev", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                                      ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_index_hamming", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_gindex_hamming", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_edit_workspace_bytes", _u64, [_u64, _u32, _u64, _u64]),
    ("sfx_edit_dev", _int, [_vp, _u64, _vp, _vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                            ctypes.POINTER(_u64), ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_index_edit_dev", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                                  ctypes.POINTER(_u64), ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_gindex_edit_dev", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                                   ctypes.POINTER(_u64), ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_index_edit", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                              ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_gindex_edit", _int, [_vp, _vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                               ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    ("sfx_inverse_table_workspace_bytes", _u64, [_u64]),
    ("sfx_inverse_table_dev", _int, [_vp, _u64, _vp, _vp, _u64, _vp]),
    ("sfx_inverse_table_u32", _int, [_vp, _u64, _vp]),
    ("sfx_lce_bytes", _u64, [_u64]),
    ("sfx_lce_create_dev", _int, [_vp, _vp, _u64, _vp, _u64, _vp, ctypes.POINTER(_vp)]),
    ("sfx_lce_create", _int, [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_vp)]),
    ("sfx_lce_destroy", None, [_vp]),
    ("sfx_lce_query_dev", _int, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    ("sfx_lce_query", _int, [_vp, _vp, _vp, _u64, _u32, _vp]),
    ("sfx_lce_range_min_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("sfx_lce_range_min", _int, [_vp, _vp, _vp, _u64, _vp]),
    ("sfx_lce_ranks_dev", _int, [_vp, _vp, _u64, _vp, _vp]),
    ("sfx_lce_ranks", _int, [_vp, _vp, _u64, _vp]),
    ("sfx_lce_u32", _int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _u32, _vp]),
    ("sfx_lce_substr_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    ("sfx_lce_substr", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    ("sfx_lce_lca_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    ("sfx_lce_lca", _int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    ("sfx_lce_range_argmin_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("sfx_lce_range_argmin", _int, [_vp, _vp, _vp, _u64, _vp]),
    ("sfx_suffix_links_workspace_bytes", _u64, [_u64]),
    ("sfx_suffix_links_dev", _int, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_suffix_links_u32", _int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    ("sfx_doc_counts_workspace_bytes", _u64, [_u64]),
    ("sfx_doc_counts_dev", _int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_doc_counts_u32", _int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    ("sfx_common_substrings_workspace_bytes", _u64, [_u64]),
    ("sfx_common_substrings_dev", _int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_common_substrings_u32", _int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    ("sfx_doclist_bytes", _u64, [_u64]),
    ("sfx_doclist_create_workspace_bytes", _u64, [_u64]),
    ("sfx_doclist_create_dev", _int, [_vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, ctypes.POINTER(_vp)]),
    ("sfx_doclist_create", _int, [_vp, _u64, _vp, _u64, _u64, ctypes.POINTER(_vp)]),
    ("sfx_doclist_destroy", None, [_vp]),
    ("sfx_doclist_workspace_bytes", _u64, [_u64, _u64]),
    ("sfx_doclist_list_dev", _int, [_vp, _vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                                    ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_doclist_list", _int, [_vp, _vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                                ctypes.POINTER(_u64)]),
    ("sfx_lyndon_array_workspace_bytes", _u64, [_u64]),
    ("sfx_lyndon_array_dev", _int, [_vp, _u64, _vp, _vp, _u64, _vp]),
    ("sfx_lyndon_array_u32", _int, [_vp, _u64, _vp, _int, _vp]),
    ("sfx_runs_workspace_bytes", _u64, [_u64]),
    ("sfx_runs_dev", _int, [_vp, _u64, _vp, _vp, ctypes.POINTER(RunsFilter), _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_runs_u32", _int, [_vp, _u64, _vp, _vp, ctypes.POINTER(RunsFilter), _vp, _vp, _vp, _u64, ctypes.POINTER(_u64)]),
    ("sfx_byte_histogram_dev", _int, [_vp, _u64, _u64, _vp, _vp]),
    ("sfx_key_histogram_dev", _int, [_vp, _u64, _u64, _u64, _vp, _int, _vp, _vp]),
    ("sfx_sa_range_workspace_bytes", _u64, [_u64, _u64]),
    ("sfx_build_sa_range_u32_dev", _int, [_vp, _u64, _vp, _int, _u32, _u32, _u64, _vp,
                                          ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_pack_text_dev", _int, [_vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    ("sfx_build_sa_range_packed_u32_dev", _int, [_vp, _u64, _vp, _int, _u32, _u32, _u64, _vp,
                                                 ctypes.POINTER(_u64), _vp, _u64, _vp]),
    ("sfx_build_lcp_range_u32_dev", _int, [_vp, _u64, _vp, _u64, _u32, _vp, _vp]),
    ("sfx_query_batch_range_dev", _int, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("sfx_microbench", _int, [_int, _u64, _int, _int, _int, ctypes.POINTER(ctypes.c_double)]),
    ("sfx_profile_enable", None, [_int]),
    ("sfx_profile_reset", None, []),
    ("sfx_profile_report", _int, [ctypes.POINTER(KernelStat), _int]),
    ("sfx_last_build_stats", None, [ctypes.POINTER(BuildStats)]),
    ("sfx_build_stats_read", _u64, [_vp, _u64]),
    ("sfx_set_option", _int, [_int, _u64]),
    ("sfx_get_option", _u64, [_int]),
]
SFX_OPT_TINY_MAX = 1
SFX_GSA_ROUTE_NONE, SFX_GSA_ROUTE_MERGE, SFX_GSA_ROUTE_REBUILD = 0, 1, 2
SFX_REP_ANY, SFX_REP_EARLIER, SFX_REP_OTHER_DOC = 0, 1, 2
REP_SCOPES = {"any": SFX_REP_ANY, "earlier": SFX_REP_EARLIER, "other_doc": SFX_REP_OTHER_DOC}


class SuffixHipError(RuntimeError):
    pass


class Engine:
    """One loaded copy of the C ABI."""

    def __init__(self, lib_path=None):
        path = lib_path or DEFAULT_LIB
        if not os.path.exists(path):
            raise SuffixHipError(
                f"{path} not found: the HIP extension is not built (run "
                f"`python -c 'import __graft_entry__ as g; g.build()'`). "
                f"suffix_amd has no CPU fallback.")
        self.path = path
        # PyTorch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).
        # Two HIP runtimes in one process do not share the GPU ("No HIP GPUs are
        # available" from whichever initialises second), so let torch's copy load
        # first: the dynamic loader then resolves our NEEDED libamdhip64.so.7 to it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.lib = ctypes.CDLL(path)
        for name, restype, argtypes in ABI:
            fn = getattr(self.lib, name)          # AttributeError = ABI symbol missing
            fn.restype = restype
            fn.argtypes = argtypes

    # -- helpers -----------------------------------------------------------------
    def check(self, status, what):
        if status != SFX_OK:
            msg = self.lib.sfx_strerror(status).decode()
            detail = self.lib.sfx_last_hip_error().decode()
            if status == SFX_ERR_TOO_LARGE:
                # the reference panics here (src/table.rs:380)
                raise OverflowError(f"{what}: {msg}")
            raise SuffixHipError(f"{what}: {msg}" + (f" [{detail}]" if detail else ""))

    def device_count(self):
        return int(self.lib.sfx_device_count())

    def require_device(self):
        if self.device_count() <= 0:
            raise SuffixHipError("no HIP device visible; suffix_amd has no CPU fallback")

    def build_stats(self):
        # the size-aware form: a library whose struct is longer than this binding's copies only what fits
        s = BuildStats()
        self.lib.sfx_build_stats_read(ctypes.byref(s), ctypes.sizeof(s))
        return s.as_dict()

    MB_COPY, MB_SCATTER4, MB_GATHER1, MB_GATHER4, MB_RUNSCATTER = range(5)

    def microbench(self, kind, nbytes, param=0, param2=0, reps=5):
        """GB/s (algorithmic bytes) of one memory-system micro-benchmark (sfx_microbench)."""
        g = ctypes.c_double(0.0)
        self.check(self.lib.sfx_microbench(kind, nbytes, param, param2, reps, ctypes.byref(g)), "sfx_microbench")
        return float(g.value)

    def release_cached_buffers(self):
        """Return the pooled device buffers of the host-pointer entry points, and the calling thread's query scratch, to
        the driver."""
        self.lib.sfx_release_cached_buffers()

    def resource_stats(self):
        """What the library holds right now, process-wide (sfx_resource_stats): live device / pinned bytes and allocations,
        streams, events, the idle part of the pool and the number of device allocations ever made."""
        s = ResourceStats()
        self.check(self.lib.sfx_resource_stats(ctypes.byref(s)), "sfx_resource_stats")
        return s.as_dict()

    def profile(self, on):
        self.lib.sfx_profile_enable(1 if on else 0)

    def profile_reset(self):
        self.lib.sfx_profile_reset()

    def profile_report(self):
        arr = (KernelStat * 64)()
        n = self.lib.sfx_profile_report(arr, 64)
        return [{"name": arr[i].name.decode(), "launches": int(arr[i].launches),
                 "total_ms": float(arr[i].total_ms), "algo_bytes": float(arr[i].algo_bytes)}
                for i in range(min(n, 64))]


_default = None


def default_engine():
    global _default
    if _default is None:
        _default = Engine()
    return _default


def set_default_engine(engine):
    """Development and test harnesses only (scripts/_devlib.py): every later `default_engine()` returns `engine`."""
    global _default
    _default = engine
