"""ctypes binding of libmevi_hip.so (C ABI: include/mevi_hip.h).

The library is loaded lazily and loudly: a missing .so or a missing GPU raises --
there is no eager/CPU fallback anywhere in mevi_amd.
"""
import ctypes
import os
from ctypes import c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import torch  # noqa: F401  (loads the HIP runtime the extension binds to)

from .build import LIB

_lib = None


class MeviHipError(RuntimeError):
    pass


class IpTopkStats(ctypes.Structure):
    _fields_ = [("n_chunks", c_int64), ("n_failed_queries", c_int64), ("n_fallback_chunks", c_int64),
                ("filter_ms", c_double), ("compact_ms", c_double), ("filter_flops", c_double),
                ("max_err_ratio", c_double), ("err_bound", c_double), ("n_second_pass_queries", c_int64),
                ("n_filter_candidates", c_int64), ("max_launch_candidates", c_int64), ("n_list_overflows", c_int64),
                ("n_i8_queries", c_int64), ("n_i8_unproven", c_int64),
                ("n_predicted_launches", c_int64), ("dispersion", c_double)]


_SIGNATURES = {
    "mevi_abi_version": (c_int, []),
    "mevi_last_error": (ctypes.c_char_p, []),
    "mevi_ip_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "mevi_ip_topk_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                 c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_ip_index_bytes": (c_size_t, [c_int64, c_int64]),
    "mevi_ip_index_build_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_size_t, c_void_p]),
    "mevi_ip_topk_indexed_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "mevi_ip_topk_indexed_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_ip_index8_bytes": (c_size_t, [c_int64, c_int64]),
    "mevi_ip_index8_build_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_size_t, c_void_p]),
    "mevi_ip_topk_indexed8_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "mevi_ip_topk_indexed8_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                          c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_topk_merge_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "mevi_topk_merge_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_pack_lists_i64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "mevi_topk_merge_packed_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "mevi_ivf_scan_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int64]),
    "mevi_ivf_scan_query_tile": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int64]),
    "mevi_ivf_scan_topk_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                       c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_ivf_assign_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "mevi_ivf_assign_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_ivf_build_lists_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "mevi_ivf_build_lists": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_fine_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "mevi_fine_topk_query_tile": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "mevi_fine_topk_f32": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "mevi_rq_encode_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_rq_encode_fast_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "mevi_rq_encode_fast_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    "mevi_rq_encode_fast_stats": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_pq_encode_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_gemm_nt_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                 c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "mevi_split_kp": (c_int64, [c_int64]),
    "mevi_split_rows_f16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_rmsnorm_split_f16": (c_int, [c_void_p, c_int64, c_void_p, c_float, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "mevi_gemm_nt_split_to_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int64,
                                            c_int64, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_gemm_nt_split_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                       c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "mevi_gemm_rmsnorm_supported": (c_int, [c_int64, c_int64, c_int64]),
    "mevi_gemm_norm_fold_supported": (c_int, [c_int64]),
    "mevi_split_rows_ssq_f16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_row_rscale_f32": (c_int, [c_void_p, c_int64, c_int64, c_float, c_float, c_void_p, c_void_p]),
    "mevi_gemm_nt_split_normed_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int,
                                              c_void_p]),
    "mevi_gemm_nt_split_normed_to_split": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_float,
                                                   c_void_p, c_void_p, c_float, c_int64, c_int64, c_int64, c_void_p, c_float, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_gemm_nt_split_residual_stream": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_float, c_float, c_void_p,
                                                   c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                                   c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_gemm_nt_rmsnorm_split_f32": (c_int, [c_void_p, c_int64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                               c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "mevi_gemm_nt_rmsnorm_split_to_split": (c_int, [c_void_p, c_int64, c_void_p, c_float, c_void_p, c_void_p, c_float, c_int64, c_int64,
                                                    c_int64, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_rmsnorm_f32": (c_int, [c_void_p, c_int64, c_void_p, c_float, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "mevi_add_layernorm_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_float,
                                       c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "mevi_gather_rows_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "mevi_scatter_rows_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "mevi_scale_f32": (c_int, [c_void_p, c_float, c_int64, c_void_p, c_void_p]),
    "mevi_attention_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                   c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                   c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "mevi_attention_cached_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p,
                                          c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                          c_int64, c_int, c_float, c_void_p]),
    "mevi_attention_varlen_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                          c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                          c_int, c_float, c_void_p]),
    "mevi_attention_split_f16": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                         c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                         c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_float, c_void_p,
                                         c_void_p]),
    "mevi_attention_cached_split_f16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                                c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                                c_void_p, c_int64, c_int64, c_int64, c_int, c_float, c_void_p]),
    "mevi_attention_varlen_split_f16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                                c_int, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                                c_int64, c_int64, c_int, c_float, c_void_p]),
    "mevi_attention_route": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                     c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                     c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_float, c_void_p,
                                     c_void_p, c_int64, c_int]),
    "mevi_attention_varlen_route": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                            c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                            c_int, c_float, c_void_p, c_int64, c_int]),
    "mevi_attention_cached_route": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p,
                                            c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                            c_int64, c_int, c_float, c_void_p, c_int64, c_int]),
    "mevi_adaptive_logits_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                         c_int64, c_void_p, c_void_p]),
    "mevi_adaptive_logits_rows_f32": (c_int, [c_void_p, c_int64, c_float, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                              c_int64, c_void_p, c_void_p]),
    "mevi_gemm_nt_split_head_supported": (c_int, [c_int64, c_int64, c_int64, c_int64]),
    "mevi_gemm_nt_split_head_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                            c_int64, c_float, c_int64, c_void_p, c_void_p]),
    "mevi_logits_finish_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_beam_step_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "mevi_beam_step_tree_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_beam_step_var_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                       c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "mevi_beam_finalize_var_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mevi_row_softmax_f32": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "mevi_pair_dot_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                  c_void_p, c_void_p]),
    "mevi_segment_sort_desc_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mevi_segment_aggregate_sort_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                                c_void_p, c_void_p]),
    "mevi_query_pool_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64,
                                    c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                    c_int64, c_int, c_void_p, c_float, c_void_p, c_int64, c_void_p]),
    "mevi_rq_neg_dist_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "mevi_gather_sub_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_rq_beam_encode_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int]),
    "mevi_rq_beam_encode_tile_docs": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_int]),
    "mevi_rq_beam_encode_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_cluster_means_workspace_bytes": (ctypes.c_size_t, [c_int64, c_int64, c_int64]),
    "mevi_cluster_means_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "mevi_format_f32_list": (c_int64, [c_void_p, c_int64, c_void_p, c_int64]),
    "mevi_format_i64_list": (c_int64, [c_void_p, c_int64, c_void_p, c_int64]),
    "mevi_format_ranked_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, ctypes.c_int32]),
    "mevi_parse_i64_list": (c_int64, [ctypes.c_char_p, c_int64, c_void_p, c_int64]),
    "mevi_parse_f64_list": (c_int64, [ctypes.c_char_p, c_int64, c_void_p, c_int64]),
    "mevi_parse_tsv_columns": (c_int64, [c_void_p, c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_void_p,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64]),
    "mevi_cluster_ranks_i32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                       ctypes.c_int32, c_void_p, c_void_p, c_void_p]),
    "mevi_ensemble_rank_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                       c_int64, ctypes.c_int32, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "mevi_first_hits_i64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "mevi_ip_filter_tile_walk": (c_int64, [c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "mevi_ip_filter_steal_item": (c_int, [c_int64, c_int, c_int, c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32),
                                          ctypes.POINTER(ctypes.c_int32)]),
    "mevi_ip_topk_get_walk_counts": (c_int, [ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "mevi_ip_topk_set_growth": (None, [c_double]),
    "mevi_ip_topk_set_profiling": (None, [c_int]),
    "mevi_ip_topk_plan": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_double, c_int64, c_void_p, c_void_p, c_void_p]),
    "mevi_ip_topk_get_stats": (None, [ctypes.POINTER(IpTopkStats)]),
}


# include/mevi_hip_fine_agg.h (included by mevi_hip.h): the fine stage's call with merge and weights
_FINE_AGG_SIGNATURES = {
    "mevi_fine_topk_agg_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int]),
    "mevi_fine_topk_agg_query_tile": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int]),
    "mevi_fine_topk_agg_f32": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_float, c_float,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


# include/mevi_hip_ivfpq.h (included by mevi_hip.h): the ADC scan of product-quantised lists
_IVFPQ_SIGNATURES = {
    "mevi_ivfpq_scan_workspace_bytes": (c_size_t, [c_int64] * 8),
    "mevi_ivfpq_scan_query_tile": (c_int64, [c_int64] * 8),
    "mevi_ivfpq_scan_topk_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                         c_void_p, c_size_t, c_void_p]),
}


# include/mevi_hip_pqfs.h (included by mevi_hip.h): packed 4-bit PQ codes, their packer and their ADC scan
_PQFS_SIGNATURES = {
    "mevi_pq4_pack": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_pqfs_scan_workspace_bytes": (c_size_t, [c_int64] * 7),
    "mevi_pqfs_scan_query_tile": (c_int64, [c_int64] * 7),
    "mevi_pqfs_scan_topk_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                        c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
}


# include/mevi_hip_sq.h (included by mevi_hip.h): scalar-quantised rows, their encoder and their list scan
_SQ_SIGNATURES = {
    "mevi_sq_encode_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                   c_int64, c_void_p, c_void_p]),
    "mevi_sq_scan_workspace_bytes": (c_size_t, [c_int64] * 7),
    "mevi_sq_scan_query_tile": (c_int64, [c_int64] * 7),
    "mevi_sq_scan_topk_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                      c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
}


# include/mevi_hip_opq.h (included by mevi_hip.h): the corpus side of an OPQ rotation -- gather, rotate, subtract the rotated centroid
_OPQ_SIGNATURES = {
    "mevi_opq_rotate_rows_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                         c_void_p]),
}


# include/mevi_hip_opq_encode.h (included by mevi_hip.h): rotate + product-quantiser encode in one launch (ProductQuantization('opq'))
_OPQ_ENCODE_SIGNATURES = {
    "mevi_opq_encode_fused": (c_int, [c_int64] * 4),
    "mevi_opq_encode_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
}


# include/mevi_hip_refine.h (included by mevi_hip.h): exact re-ranking of the candidate ids a compressed index returned
_REFINE_SIGNATURES = {
    "mevi_refine_topk_workspace_bytes": (c_size_t, [c_int64] * 4),
    "mevi_refine_topk_query_tile": (c_int64, [c_int64] * 4),
    "mevi_refine_topk_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_refine_topk_set_score_body": (None, [c_int]),
}


# include/mevi_hip_aq.h (included by mevi_hip.h): additive (residual) quantiser indexes -- tables, their ADC scan, the encoder's residual
_AQ_SIGNATURES = {
    "mevi_aq_lut_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "mevi_aq_scan_workspace_bytes": (c_size_t, [c_int64] * 8),
    "mevi_aq_scan_query_tile": (c_int64, [c_int64] * 8),
    "mevi_aq_scan_topk_f32": _IVFPQ_SIGNATURES["mevi_ivfpq_scan_topk_f32"],
    "mevi_rq_residual_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
}


# include/mevi_hip_rq_errbeam.h (included by mevi_hip.h): one level of the residual quantiser's beam-search encoder, and its backtrack
_RQ_ERRBEAM_SIGNATURES = {
    "mevi_rq_errbeam_step_workspace_bytes": (c_size_t, [c_int64] * 5),
    "mevi_rq_errbeam_step_tile_docs": (c_int64, [c_int64] * 4),
    "mevi_rq_errbeam_step_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_rq_errbeam_codes_u8": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
}


# include/mevi_hip_graph.h (included by mevi_hip.h): the neighbour graph of "HNSW<M>", its linking and its search
_GRAPH_SIGNATURES = {
    "mevi_graph_link_workspace_bytes": (c_size_t, [c_int64] * 3),
    "mevi_graph_link": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mevi_graph_search_workspace_bytes": (c_size_t, [c_int64] * 8),
    "mevi_graph_search_topk_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                           c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
}


# include/mevi_hip_graph_levels.h (included by mevi_hip.h): the descent through the upper levels of that index
_GRAPH_LEVELS_SIGNATURES = {
    "mevi_graph_descend_workspace_bytes": (c_size_t, [c_int64] * 9),
    "mevi_graph_descend_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
}


# include/mevi_hip_attn_long.h (included by mevi_hip.h): attention over up to ATTN_LONG_MAX_KEYS keys
_ATTN_LONG_SIGNATURES = {
    "mevi_attention_long_f32": _SIGNATURES["mevi_attention_f32"],
    "mevi_attention_long_varlen_f32": _SIGNATURES["mevi_attention_varlen_f32"],
    "mevi_attention_long_route": (c_int, _SIGNATURES["mevi_attention_f32"][1][:-1]),            # the call without the stream
    "mevi_attention_long_varlen_route": (c_int, _SIGNATURES["mevi_attention_varlen_f32"][1][:-1]),
}
ATTN_LONG_MAX_KEYS = 2048     # MEVI_ATTN_LONG_MAX_KEYS
# MEVI_ATTN_ROUTE_* of that header: what mevi_attention_long*_route return besides NONE.  A table of their own: ATTN_ROUTES is
# the enum of mevi_hip.h, name for name, and every name of it has its cases in tests/attn_cases.py
ATTN_LONG_ROUTES = {"LONG_MFMA": 13, "LONG_ROWS": 14}


# MEVI_ATTN_ROUTE_* of include/mevi_hip.h: what mevi_attention*_route return (negative: the status of a refusal)
ATTN_ROUTES = {"NONE": 0, "GENERIC": 1, "TILE": 2, "GROUP": 3, "FEW_KEYS": 4, "KEYS16": 5, "VARLEN": 6, "VARLEN_SHORT64": 7,
               "MFMA": 8, "H16": 9, "MFMA16_SELF": 10, "MFMA16_SHARED": 11, "MFMA16_INDEXED": 12,
               "FEW_KEYS_STAGED64": 64, "FEW_KEYS_STAGED96": 96}     # the staged forms: + tk (1..7 / 1..6)


def attn_route_name(route):
    """'TILE', 'FEW_KEYS_STAGED64+3', 'LONG_MFMA', ... for a route value; 'REFUSED(-2)' for a refusal."""
    if route < 0:
        return f"REFUSED({route})"
    for base in ("FEW_KEYS_STAGED96", "FEW_KEYS_STAGED64"):
        if ATTN_ROUTES[base] < route <= ATTN_ROUTES[base] + 7:
            return f"{base}+{route - ATTN_ROUTES[base]}"
    return next(k for k, v in {**ATTN_ROUTES, **ATTN_LONG_ROUTES}.items() if v == route)


def exported_symbols(header="mevi_hip.h"):
    """Names every entry point the text of include/<header> declares (mevi_hip.h, or mevi_hip_fine_agg.h / mevi_hip_attn_long.h /
    mevi_hip_ivfpq.h / mevi_hip_pqfs.h / mevi_hip_sq.h / mevi_hip_opq.h / mevi_hip_opq_encode.h / mevi_hip_graph.h / mevi_hip_graph_levels.h /
    mevi_hip_refine.h / mevi_hip_aq.h / mevi_hip_rq_errbeam.h, which it includes)."""
    return sorted({"mevi_hip.h": _SIGNATURES, "mevi_hip_fine_agg.h": _FINE_AGG_SIGNATURES, "mevi_hip_refine.h": _REFINE_SIGNATURES,
                   "mevi_hip_aq.h": _AQ_SIGNATURES, "mevi_hip_rq_errbeam.h": _RQ_ERRBEAM_SIGNATURES,
                   "mevi_hip_attn_long.h": _ATTN_LONG_SIGNATURES, "mevi_hip_ivfpq.h": _IVFPQ_SIGNATURES, "mevi_hip_sq.h": _SQ_SIGNATURES,
                   "mevi_hip_pqfs.h": _PQFS_SIGNATURES, "mevi_hip_opq.h": _OPQ_SIGNATURES, "mevi_hip_opq_encode.h": _OPQ_ENCODE_SIGNATURES, "mevi_hip_graph.h": _GRAPH_SIGNATURES, "mevi_hip_graph_levels.h": _GRAPH_LEVELS_SIGNATURES}[header])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise MeviHipError(
                f"{LIB} not found: build it with `python -m mevi_amd.build` "
                "(or __graft_entry__.build()); mevi_amd has no CPU fallback")
        L = ctypes.CDLL(LIB)
        for name, (res, args) in {**_SIGNATURES, **_FINE_AGG_SIGNATURES, **_ATTN_LONG_SIGNATURES, **_IVFPQ_SIGNATURES,
                                  **_PQFS_SIGNATURES, **_SQ_SIGNATURES, **_OPQ_SIGNATURES, **_OPQ_ENCODE_SIGNATURES, **_GRAPH_SIGNATURES, **_GRAPH_LEVELS_SIGNATURES,
                                  **_REFINE_SIGNATURES, **_AQ_SIGNATURES, **_RQ_ERRBEAM_SIGNATURES}.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().mevi_last_error().decode("utf-8", "replace")
        raise MeviHipError(f"{what} failed with status {status}: {msg}")


def ip_walk_counts():
    """(tiles, stolen) of the ticketed filter walk in this thread's last dense search on the current device
    (mevi_ip_topk_get_walk_counts); call once the search has completed."""
    tiles, stolen = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().mevi_ip_topk_get_walk_counts(ctypes.byref(tiles), ctypes.byref(stolen)), "mevi_ip_topk_get_walk_counts")
    return tiles.value, stolen.value


def require_gpu():
    if not torch.cuda.is_available():
        raise MeviHipError("no MI355X visible (torch.cuda.is_available() is False); "
                           "mevi_amd has no CPU fallback")


# Host cost of a launch: the small-batch passes (the reference's own batch sizes) are ~250-550 launches during which the GPU
# mostly waits for Python.  cProfile of a 128-query tower pass (tools/prof_host.py, 4.5 ms for 247 launches): the public
# `torch.cuda.current_stream()` took 7.7 us per call and `with torch.cuda.device(...)` 4-8 us -- more than the ctypes call
# itself.  The raw hooks below are what torch's own Python wrappers end in.
# They are private: a torch build without them (CPU-only wheel, a rename) falls back to the public calls instead of failing
# the import -- `require_gpu()` / MeviHipError stay the way a missing GPU is reported.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)
_cur_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream_ptr():
    """The current device's current stream as an integer handle (ctypes passes it as void *); the capturing stream inside
    `torch.cuda.graph`."""
    return _raw_stream(_cur_device())


class _NoGuard:
    __slots__ = ()

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def device_guard(dev):
    """`with device_guard(t.device):` = `with torch.cuda.device(t.device):`, for free when that device is already current."""
    idx = dev.index
    if idx is None or idx == _cur_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


def on_device(fn):
    """Run `fn` with its first tensor argument's GPU as the current device, so that `stream_ptr()` and the launch refer
    to the device the pointers live on (the public classes take `device=`; callers need not torch.cuda.set_device)."""
    import functools

    @functools.wraps(fn)
    def run(*args, **kw):
        t = next((a for a in args if torch.is_tensor(a)), None)
        if t is None or not t.is_cuda or t.device.index == _cur_device():
            return fn(*args, **kw)
        with torch.cuda.device(t.device):
            return fn(*args, **kw)

    return run


def ptr(t):
    """Device address of a tensor's first element, as the integer ctypes passes for a void * argument."""
    return t.data_ptr()
