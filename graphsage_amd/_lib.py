"""ctypes binding of libgraphsage_amd.so (the C ABI declared in include/graphsage_amd.h).

The product path has NO CPU fallback: if the shared library is missing or a kernel reports an
error, a GraphsageAmdError is raised.  torch is used only as the owner of device memory.
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_C", "libgraphsage_amd.so")

ACT_IDENTITY = 0
ACT_RELU = 1
LAW_IID, LAW_REFERENCE, LAW_DISTINCT = 0, 1, 2      # GS_LAW_* (sampling law of the CSR sampler)
SAMPLER_LAWS = {"iid": LAW_IID, "reference": LAW_REFERENCE, "distinct": LAW_DISTINCT}
GS_PEER_HANDLE_BYTES = 64
GS_ABI_VERSION = 12     # must equal GS_ABI_VERSION of include/graphsage_amd.h (struct layouts below mirror that header)
WGRAD_TILED3_FORM_DEFAULT = 1    # initial value of g_wgrad_tiled3_form (csrc/gs_split.hip; gs_set_wgrad_tiled3_form)


class GraphsageAmdError(RuntimeError):
    pass


_P = c_void_p  # every device pointer crosses the boundary as void*

# name -> (argtypes) ; every function returns int except gs_last_error / gs_abi_version
_PROTOS = {
    "gs_device_info": [POINTER(c_int), POINTER(c_int), ctypes.c_char_p, c_int],
    "gs_sample_padded": [_P, c_int64, c_int32, _P, c_int64, _P, c_int32, _P, _P],
    "gs_sample_uniform_csr": [_P, _P, c_int64, c_int32, _P, c_int64, c_int32, c_uint64, c_uint64, _P, c_uint32,
                              c_int64, c_int32, c_int32, _P, _P],
    "gs_select_batch": [_P, c_int64, _P, c_int64, _P, _P],
    "gs_advance_counter": [_P, c_uint64, _P],
    "gs_gather_rows": [_P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P],
    "gs_gather_mean_fwd": [_P, c_int64, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, _P, c_int64, _P],
    "gs_mean_bwd": [_P, c_int64, c_int64, c_int32, c_int32, c_float, _P, c_int64, _P, c_int64, c_int, _P],
    "gs_sage_dense_fwd": [_P, c_int64, _P, c_int32, _P, c_int64, _P, c_int32, c_int64, _P, c_int64, _P, c_int64,
                          c_int32, c_int, c_int, _P, _P, c_int64, _P],
    "gs_dense_wgrad": [_P, c_int64, _P, c_int32, _P, c_int64, c_int32, c_int32, c_int64, c_int32, _P, c_int64, _P],
    "gs_dense_dgrad": [_P, c_int64, c_int32, c_int32, c_int64, _P, c_int64, c_int32, _P, c_int64, c_int, _P],
    "gs_act_bwd": [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int, _P, c_int64, _P],
    "gs_colsum_slabs": [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P],
    "gs_gemm_f32": [c_int, c_int, c_int64, c_int32, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int, _P, c_int64, _P],
    "gs_abi_struct_sizes": [_P, c_int32],
    "gs_dense_pool_max_fwd": [_P, c_int64, _P, c_int32, c_int64, c_int32, _P, c_int64, c_int32, _P, _P, c_int64, _P, c_int64, _P],
    "gs_segment_max_fwd": [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int64, _P],
    "gs_segment_max_bwd": [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P],
    "gs_l2norm_fwd": [_P, c_int64, c_int64, c_int32, _P, c_int64, _P, _P],
    "gs_l2norm_bwd": [_P, c_int64, _P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P],
    "gs_class_loss": [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int, _P, _P, c_int64, _P, c_int64, _P],
    "gs_reduce_slabs": [_P, c_int32, c_int64, c_int32, c_int32, c_int64, c_float, _P, c_int64, _P, c_int64, c_int, _P],
    "gs_adam_step": [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_float, c_float, _P, c_int32, _P],
    "gs_comm_available": [],
    "gs_comm_count": [_P, POINTER(c_int32)],
    "gs_comm_unique_id": [_P, c_int32],
    "gs_comm_init_rank": [POINTER(c_void_p), c_int32, c_int32, _P, c_int32],
    "gs_comm_allreduce_sum_f32": [_P, _P, c_int64, _P],
    "gs_comm_destroy": [_P],
    "gs_peer_create": [c_int64, c_int32, c_int32, c_int32, c_int64, POINTER(c_void_p)],
    "gs_peer_export": [_P, _P, c_int32],
    "gs_peer_attach": [_P, c_int32, _P, c_int32],
    "gs_peer_attach_local": [_P, _P],
    "gs_peer_allreduce_sum_f32": [_P, _P, c_int64, _P],
    "gs_peer_status": [_P, POINTER(c_int64), POINTER(c_int32)],
    "gs_peer_destroy": [_P],
    "gs_sum_scaled": [_P, c_int64, c_float, _P, c_int, _P],
    "gs_sumsq_scaled": [_P, c_int64, c_float, _P, c_int, _P],
    "gs_stream_create": [POINTER(c_void_p)],
    "gs_spin_us": [c_float, _P],
    "gs_stream_destroy": [_P],
    "gs_stream_sync": [_P],
    "gs_capture_begin": [_P],
    "gs_capture_end": [_P, POINTER(c_void_p)],
    "gs_graph_launch": [_P, _P],
    "gs_graph_destroy": [_P],
    "gs_event_create": [POINTER(c_void_p)],
    "gs_event_record": [_P, _P],
    "gs_stream_wait_event": [_P, _P],
    "gs_event_elapsed_ms": [_P, _P, POINTER(c_float)],
    "gs_event_destroy": [_P],
    "gs_build_csr_host": [_P, _P, _P, c_int64, c_int64, c_int, _P, _P, c_int64, POINTER(c_int64)],
    "gs_dense_wgrad_grouped": [_P, c_int32, _P],
    "gs_dense_wgrad_grouped_cogather": [_P, c_int32, _P, c_int32, _P],
    "gs_sage_dense_dgrad": [_P, c_int64, c_int64, c_int32, c_int, _P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P],
    "gs_flat_reduce_adam": [_P, c_int32, _P, _P, _P, _P, c_int64, c_float, c_int, c_float, c_float, c_float, c_float,
                            c_float, c_float, _P, c_int32, _P, c_int64, c_float, _P, c_int, _P],
    "gs_sage_dense_fwd_stream": [_P, c_int64, _P, _P, c_int64, c_int32, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int, _P, _P,
                                 c_int64, _P, c_int32, _P],
    "gs_sage_dense_fwd_stream2": [_P, c_int64, _P, c_int32, _P, c_int64, c_int32, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int, _P,
                                  _P, c_int64, _P, c_int32, _P],
    "gs_dense_wgrad_grouped_stream": [_P, c_int32, _P, c_int32, _P],
    "gs_dense_wgrad_grouped_tiled3": [_P, c_int32, _P, c_int32, _P],
    "gs_dense_wgrad_grouped_tiled3_sample": [_P, c_int32, _P, c_int32, _P, _P],
    "gs_set_wgrad_tiled3_form": [c_int],
    "gs_sage_dense_fwd_tiled3": [_P, c_int64, _P, c_int32, _P, c_int64, c_int32, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int, _P,
                                 _P, c_int64, _P, c_int32, _P],
    "gs_sage_dense_fwd_tiled3_means": [_P, c_int64, _P, c_int32, _P, c_int64, c_int32, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                       c_int, _P, _P, c_int64, _P, c_int32, c_int64, c_int32, _P, c_int64, _P],
    "gs_split_rows_bytes": [c_int32, c_int32, _P],
    "gs_split_rows": [_P, c_int64, c_int32, c_int32, _P, _P],
    "gs_dense_fwd_rows_split": [_P, c_int64, _P, c_int32, c_int64, _P, _P, c_int32, c_int, _P, _P, c_int64, _P],
    "gs_split_rows_f16_bytes": [c_int32, c_int32, _P],
    "gs_split_rows_f16": [_P, c_int64, c_int32, c_int32, _P, _P],
    "gs_split_table_f16_bytes": [c_int64, c_int32, _P, _P],
    "gs_split_table_f16": [_P, c_int64, c_int64, c_int32, _P, _P, _P],
    "gs_dense_fwd_rows_split16": [_P, _P, _P, c_int32, c_int64, _P, _P, c_int32, c_int, _P, _P, c_int64, _P, c_int64, _P],
    "gs_dense_fwd_rows_split_ws_bytes": [_P],
    "gs_dense_fwd_rows_split_ws": [_P, c_int64, _P, c_int32, c_int64, _P, _P, c_int32, c_int, _P, _P, c_int64, _P, c_int64, _P],
    "gs_flat_reduce_adam_sample": [_P, c_int32, _P, _P, _P, _P, c_int64, c_float, c_int, c_float, c_float, c_float, c_float,
                                   c_float, c_float, _P, c_int32, _P, c_int64, c_float, _P, c_int, _P, _P, c_int32, _P],
    "gs_sage_tail_supported": [c_int32, c_int32, c_int32],
    "gs_sage_tail_fwd_bwd": [_P, _P, c_int32, _P],
    "gs_sage_tail_z": [_P, _P, c_int32, _P],
    "gs_sage_tail_dh0": [_P, _P, c_int32, _P],
    "gs_sage_tail_fwd_bwd_means": [_P, _P, c_int32, _P],
    "gs_sage_tail_z_means": [_P, _P, c_int32, _P],
    "gs_dropout_rows": [_P, c_int64, _P, c_int64, c_int32, _P, _P, c_int64, _P],
    "gs_gather_mean_dropout_fwd": [_P, c_int64, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, _P, c_int64, _P, _P],
    "gs_scatter_add_rows": [_P, c_int64, c_int64, c_int32, c_int32, c_float, _P, _P, c_int64, _P],
    "gs_copy_cols": [_P, c_int64, _P, c_int64, c_int64, c_int32, _P],
    "gs_input_grad_pull": [_P, _P],
    "gs_advance_counters": [_P, c_uint64, _P, c_uint64, _P, c_uint64, _P],
    "gs_head_fwd_bwd": [_P, c_int64, c_int64, c_int32, _P, c_int64, _P, _P, c_int64, c_int32, c_int, _P, c_int64, _P,
                        c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P],
    "gs_sample_fanout_csr": [_P, _P, c_int64, c_int32, c_int32, _P, _P, _P, c_int64, c_uint64, c_uint64, _P, c_uint32,
                             c_int64, _P, c_int64, _P, _P, c_int64, c_int32, _P, c_int64, c_int32, c_int32, _P],
    "gs_finalize_step": [_P, c_int64, c_float, _P, c_int, _P, c_uint64, _P, c_uint64, _P, c_uint64, _P],
    "gs_sage_dense_fwd_cogather": [_P, c_int64, _P, c_int32, _P, c_int64, _P, c_int32, c_int64, _P, c_int64, _P, c_int64,
                                   c_int32, c_int, c_int, _P, _P, c_int64, _P, c_int32, _P],
    "gs_unsup_stage": [_P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_uint64, _P, c_int64, _P, _P],
    "gs_linkpred_fwd_bwd": [_P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, _P, _P, _P, c_int64, _P, c_int64,
                            _P, POINTER(c_int32), _P],
    "gs_linkpred_norm_fwd_bwd": [_P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, _P, c_int64, _P, _P, _P, c_int64,
                                 _P, c_int64, _P, _P],
    "gs_linkpred_norm_fwd_bwd_step": [_P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, _P, c_int64, _P, _P, _P, c_int64,
                                      _P, c_int64, _P, _P, c_int, _P, _P, c_uint64, _P, c_uint64, _P, c_uint64, _P],
    "gs_linkpred_loss_fwd_bwd": [c_int32, _P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, c_float, _P,
                                 c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P],
    "gs_linkpred_loss_fwd_bwd_step": [c_int32, _P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, c_float,
                                      _P, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int, _P, _P,
                                      c_uint64, _P, c_uint64, _P, c_uint64, _P],
    "gs_linkpred_infonce_ws_floats": [c_int64, c_int32, c_int32, c_int, POINTER(c_int64)],
    "gs_linkpred_infonce_fwd_bwd": [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, _P, _P, _P, _P, _P,
                                    c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P],
    "gs_linkpred_infonce_fwd_bwd_step": [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_float, c_float, _P, _P, _P, _P,
                                         _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int, _P, _P, c_uint64, _P,
                                         c_uint64, _P, c_uint64, _P],
    "gs_linkpred_tail_supported": [c_int32, c_int32, c_int32],
    "gs_linkpred_tail": [_P, _P, c_int32, _P],
    "gs_linkpred_tail_means": [_P, _P, c_int32, _P],
    "gs_linkpred_tail_neg": [_P, _P, c_int, _P, _P, c_uint64, _P, c_uint64, _P, c_uint64, _P, c_int32, _P],
    "gs_unique_ids": [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P],
    "gs_dense_fwd_rows_dev": [_P, c_int64, _P, c_int32, c_int64, _P, _P, c_int64, c_int32, c_int, _P, _P, c_int64, _P],
    "gs_segment_max_gather_fwd": [_P, c_int64, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int64, _P],
    "gs_segment_attn_fwd": [_P, c_int64, _P, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, _P],
    "gs_segment_attn_bwd": [_P, c_int64, _P, c_int64, _P, _P, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int32, _P],
    "gs_attn_scores": [_P, c_int64, c_int64, c_int32, _P, _P],
    "gs_sample_fanout_desc": [_P, _P],
    "gs_build_padded_table": [_P, _P, c_int64, c_int32, c_int32, c_uint64, _P, _P],
    "gs_finalize_step2": [_P, c_int64, c_float, _P, c_int, _P, c_float, _P, _P, c_uint64, _P, c_uint64, _P, c_uint64, _P],
    "gs_maxpool_sparse_wgrad": [_P, c_int64, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, c_int64, c_int32, c_int32, _P,
                                c_int64, _P],
    "gs_pool2_transpose": [_P, c_int64, c_int32, c_int32, _P, c_int64, _P],
    "gs_pool2_iota": [_P, c_int64, _P],
    "gs_pool2_dgrad_t": [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, c_int32, _P, c_int64,
                         _P],
    "gs_pool2_dgrad": [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, c_int32, _P, c_int64, _P],
    "gs_stage_batch": [_P, c_int64, _P, c_int64, _P, _P, c_int64, c_int32, _P, c_int64, _P],
    "gs_lstm_lengths": [_P, c_int32, c_int32, _P, _P],
    "gs_lstm_fwd": [_P, c_int32, c_int32, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P],
    "gs_lstm_bwd": [_P, c_int32, c_int32, _P, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P],
    "gs_n2v_stage": [_P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_uint64, _P, c_int64, _P, c_int32, _P, _P, _P],
    "gs_n2v_supported": [c_int32, c_int32],
    "gs_n2v_slabs": [c_int64, c_int32, c_int32],
    "gs_n2v_fwd_bwd": [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, c_int, _P, _P, _P, c_int64, _P,
                       c_int64, _P, _P, _P, _P, _P, _P],
    "gs_n2v_apply": [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, c_float, _P, _P, _P, _P, _P, c_int32,
                     _P, _P, _P, _P, _P, c_uint64, _P, c_uint64, _P],
    "gs_csr_reduce_ws_bytes": [c_int64, c_int32, POINTER(c_int64)],
    "gs_csr_reduce_fwd": [_P, _P],
    "gs_csr_reduce_rows": [_P, _P],
    "gs_frontier_ws_bytes": [c_int64, POINTER(c_int64)],
    "gs_frontier_expand": [_P, _P],
    "gs_rank_ws_bytes": [c_int64, c_int64, POINTER(c_int64)],
    "gs_rank_count": [_P, _P],
    "gs_topk_ws_bytes": [c_int64, c_int64, c_int32, POINTER(c_int64)],
    "gs_topk_select": [_P, _P],
    "gs_walk_paths": [_P, _P],
    "gs_walk_pairs": [_P, _P],
    "gs_importance_table": [_P, _P],
    "gs_logreg_ws_bytes": [c_int64, c_int32, c_int32, POINTER(c_int64)],
    "gs_logreg_eval": [_P, _P],
    "gs_logreg_joined_ws_bytes": [c_int64, c_int32, c_int32, POINTER(c_int64)],
    "gs_logreg_eval_joined": [_P, _P],
    "gs_col_moments": [_P, _P, c_int64, c_int32, c_int64, _P, _P, c_int64, c_int32, c_int64, c_int64, _P, _P, _P, c_int64, _P],
    "gs_kmeans_sqnorm": [_P, c_int64, c_int64, _P, c_int64, c_int32, _P, _P],
    "gs_kmeans_assign_ws_bytes": [c_int64, POINTER(c_int64)],
    "gs_kmeans_assign": [_P, _P],
    "gs_kmeans_members_ws_bytes": [c_int64, c_int32, c_int32, POINTER(c_int64)],
    "gs_kmeans_members": [_P, _P],
    "gs_ivf_ws_bytes": [c_int64, c_int32, c_int32, c_int32, POINTER(c_int64)],
    "gs_ivf_search": [_P, _P],
    "gs_prop_weights": [_P, _P, c_int64, c_int64, _P, _P, _P],
    "gs_prop_ws_bytes": [c_int64, c_int32, POINTER(c_int64)],
    "gs_prop_step": [_P, _P],
    "gs_prop_correct": [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_float, _P, c_int64, _P],
    "gs_nbr_rank_grid": [c_int64, c_int32, POINTER(c_int64)],
    "gs_nbr_rank_ws_bytes": [c_int64, c_int64, POINTER(c_int64)],
    "gs_nbr_rank": [_P, _P],
}


class WgradDesc(ctypes.Structure):
    """struct gs_wgrad_desc (include/graphsage_amd.h)"""
    _fields_ = [("A", c_void_p), ("a_idx", c_void_p), ("dZ", c_void_p), ("slabs", c_void_p),
                ("lda", c_int64), ("ldz", c_int64), ("ld_slab", c_int64), ("n", c_int64),
                ("d", c_int32), ("col0", c_int32), ("out_dim", c_int32), ("n_slabs", c_int32), ("a_rows", c_int64)]


class GatherDesc(ctypes.Structure):
    """struct gs_gather_desc (include/graphsage_amd.h)"""
    _fields_ = [("X", c_void_p), ("idx", c_void_p), ("self_src", c_void_p), ("self_idx", c_void_p), ("out", c_void_p),
                ("ldx", c_int64), ("ld_self", c_int64), ("ldo", c_int64), ("n", c_int64), ("s", c_int32), ("d", c_int32)]


class Dropout(ctypes.Structure):
    """struct gs_dropout (include/graphsage_amd.h)"""
    _fields_ = [("seed", c_uint64), ("clock_dev", c_void_p), ("site", c_uint32), ("rate", c_float), ("row0", c_int64),
                ("keep_bits", c_void_p), ("keep_ld", c_int64)]


GS_PULL_MAX = 6


class PullDesc(ctypes.Structure):
    """struct gs_pull_desc (include/graphsage_amd.h)"""
    _fields_ = [("d_self", c_void_p), ("ld_self", c_int64), ("n_self", c_int64), ("n_seg", c_int32), ("d", c_int32),
                ("src", c_void_p * GS_PULL_MAX), ("ld_src", c_int64 * GS_PULL_MAX), ("row0", c_int64 * GS_PULL_MAX),
                ("n", c_int64 * GS_PULL_MAX), ("s", c_int32 * GS_PULL_MAX), ("scale", c_float * GS_PULL_MAX),
                ("mask_y", c_void_p), ("ldy", c_int64), ("out", c_void_p), ("ldo", c_int64), ("rows", c_int64)]


class TailDesc(ctypes.Structure):
    """struct gs_tail_desc (include/graphsage_amd.h)"""
    _fields_ = [("h0", c_void_p), ("ldh", c_int64), ("n", c_int64),
                ("W_self", c_void_p), ("ldws", c_int64), ("W_neigh", c_void_p), ("ldwn", c_int64),
                ("W_head", c_void_p), ("ldwh", c_int64), ("b_head", c_void_p),
                ("labels", c_void_p), ("ldlab", c_int64),
                ("means", c_void_p), ("ldm", c_int64), ("z", c_void_p), ("ldz", c_int64), ("y", c_void_p), ("ldy", c_int64),
                ("logits", c_void_p), ("ldlo", c_int64), ("preds", c_void_p), ("ldp", c_int64),
                ("dlogits", c_void_p), ("lddl", c_int64), ("loss_rows", c_void_p),
                ("dz", c_void_p), ("lddz", c_int64), ("d_h0", c_void_p), ("lddh", c_int64),
                ("c0", c_void_p), ("d0", c_uint64), ("c1", c_void_p), ("d1", c_uint64), ("c2", c_void_p), ("d2", c_uint64),
                ("s", c_int32), ("d_in", c_int32), ("out_dim", c_int32), ("C", c_int32), ("sigmoid", c_int32),
                ("train", c_int32), ("sync", c_void_p), ("z_ready", c_int32), ("gcn", c_int32),
                ("ids_copy_src", c_void_p), ("ids_copy_dst", c_void_p), ("ids_copy_n", c_int64)]


class LpTailDesc(ctypes.Structure):
    """struct gs_lp_tail_desc (include/graphsage_amd.h)"""
    _fields_ = [("h0", c_void_p), ("ldh", c_int64), ("B", c_int64), ("n_neg", c_int32), ("s", c_int32), ("d_in", c_int32),
                ("out_dim", c_int32), ("train", c_int32),
                ("W_self", c_void_p), ("ldws", c_int64), ("W_neigh", c_void_p), ("ldwn", c_int64),
                ("means", c_void_p), ("ldm", c_int64), ("z", c_void_p), ("ldz", c_int64), ("y", c_void_p), ("ldy", c_int64),
                ("dz", c_void_p), ("lddz", c_int64), ("d_h0", c_void_p), ("lddh", c_int64),
                ("loss_rows", c_void_p), ("rr_rows", c_void_p), ("aff_all", c_void_p), ("ld_aff", c_int64),
                ("neg_slabs", c_void_p), ("neg_weight", c_float), ("scale", c_float), ("sync", c_void_p)]


class FanoutDesc(ctypes.Structure):
    """struct gs_fanout_desc (include/graphsage_amd.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("n_nodes", c_int64),
                ("ids_all", c_void_p), ("B", c_int64),
                ("seed", c_uint64), ("step", c_uint64), ("step_dev", c_void_p),
                ("root_offset", c_int64),
                ("order", c_void_p), ("n_order", c_int64), ("cursor_dev", c_void_p),
                ("label_table", c_void_p), ("ld_table", c_int64),
                ("labels_out", c_void_p), ("ld_out", c_int64),
                ("offsets", c_int64 * 4), ("fan", c_int32 * 3),
                ("pad_id", c_int32), ("n_hops", c_int32), ("C", c_int32), ("hop0", c_uint32),
                ("law", c_int32), ("max_degree", c_int32),
                ("pairs", c_void_p), ("n_pairs", c_int64), ("n_pair_roots", c_int64),
                ("cdf", c_void_p), ("guide", c_void_p), ("n_cdf", c_int64),
                ("n_neg", c_int32), ("guide_bits", c_int32), ("neg_seed", c_uint64), ("padded_table", c_void_p),
                ("seg_begin", c_int64 * 2)]


class VarDesc(ctypes.Structure):
    """struct gs_var_desc (include/graphsage_amd.h)"""
    _fields_ = [("offset", c_int64), ("size", c_int64), ("slabs", c_void_p), ("n_slabs", c_int32), ("decay", c_int32),
                ("clear", c_int32), ("reserved_", c_int32)]

GS_LSTM_MAX_SEG = 4


class LstmSeg(ctypes.Structure):
    """struct gs_lstm_seg (include/graphsage_amd.h)"""
    _fields_ = [("X", c_void_p), ("ids", c_void_p), ("ldx", c_int64), ("n", c_int64), ("row0", c_int64), ("seq0", c_int64),
                ("T", c_int32), ("reserved_", c_int32)]


assert ctypes.sizeof(LstmSeg) == 56      # static_assert in csrc/gs_lstm.hip (passed by pointer, not in gs_abi_struct_sizes)

CSR_MEAN, CSR_MEAN_SELF, CSR_MAX, CSR_SOFTMAX = 0, 1, 2, 3          # GS_CSR_* (ops of gs_csr_reduce_fwd)


class CsrReduceDesc(ctypes.Structure):
    """struct gs_csr_reduce_desc (include/graphsage_amd.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("items", c_void_p), ("splits", c_void_p), ("X", c_void_p),
                ("out", c_void_p), ("ws", c_void_p),
                ("n_rows", c_int64), ("nnz", c_int64), ("n_items", c_int64), ("n_split", c_int64),
                ("ldx", c_int64), ("x_rows", c_int64), ("ldo", c_int64), ("ws_bytes", c_int64),
                ("row0", c_int64), ("n", c_int64),
                ("item0", c_int64), ("item1", c_int64), ("split0", c_int64), ("split1", c_int64), ("slot0", c_int64),
                ("slot1", c_int64),
                ("d", c_int32), ("op", c_int32), ("act", c_int32), ("split_len", c_int32)]


assert ctypes.sizeof(CsrReduceDesc) == 200      # static_assert in csrc/gs_csr_reduce.hip (passed by pointer, as LstmSeg)


class CsrRowsDesc(ctypes.Structure):
    """struct gs_csr_rows_desc (include/graphsage_amd.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("items", c_void_p), ("splits", c_void_p), ("x_pos", c_void_p),
                ("out_pos", c_void_p), ("X", c_void_p), ("out", c_void_p), ("ws", c_void_p),
                ("n_rows", c_int64), ("nnz", c_int64), ("n_items", c_int64), ("n_split", c_int64), ("n_slots", c_int64),
                ("ldx", c_int64), ("x_rows", c_int64), ("ldo", c_int64), ("out_rows", c_int64), ("ws_bytes", c_int64),
                ("d", c_int32), ("op", c_int32), ("act", c_int32), ("split_len", c_int32)]


assert ctypes.sizeof(CsrRowsDesc) == 168      # static_assert in csrc/gs_csr_reduce.hip (passed by pointer, as CsrReduceDesc)


class FrontierDesc(ctypes.Structure):
    """struct gs_frontier_desc (include/graphsage_amd.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("rows_in", c_void_p), ("rows_out", c_void_p), ("pos", c_void_p),
                ("count", c_void_p), ("ws", c_void_p),
                ("n_rows", c_int64), ("nnz", c_int64), ("m", c_int64), ("rows_out_cap", c_int64), ("ws_bytes", c_int64)]


assert ctypes.sizeof(FrontierDesc) == 96      # static_assert in csrc/gs_frontier.hip (passed by pointer, as CsrReduceDesc)


class RankDesc(ctypes.Structure):
    """struct gs_rank_desc (include/graphsage_amd.h)"""
    _fields_ = [("Xq", c_void_p), ("Zc", c_void_p), ("dst", c_void_p), ("src", c_void_p), ("f_rowptr", c_void_p),
                ("f_col", c_void_p), ("t", c_void_p), ("n_gt", c_void_p), ("n_eq", c_void_p), ("ws", c_void_p),
                ("Q", c_int64), ("ldq", c_int64), ("n_rows", c_int64), ("n_cand", c_int64), ("ldz", c_int64),
                ("f_nnz", c_int64), ("ws_bytes", c_int64),
                ("d", c_int32), ("flags", c_int32)]


RANK_KEEP_SRC = 1                           # GS_RANK_KEEP_SRC (gs_rank_desc.flags)
assert ctypes.sizeof(RankDesc) == 144      # static_assert in csrc/gs_rank.hip (passed by pointer, as CsrReduceDesc)


class TopkDesc(ctypes.Structure):
    """struct gs_topk_desc (include/graphsage_amd.h)"""
    _fields_ = [("Xq", c_void_p), ("Zc", c_void_p), ("src", c_void_p), ("f_rowptr", c_void_p), ("f_col", c_void_p),
                ("ids", c_void_p), ("scores", c_void_p), ("count", c_void_p), ("ws", c_void_p),
                ("Q", c_int64), ("ldq", c_int64), ("n_rows", c_int64), ("n_cand", c_int64), ("ldz", c_int64),
                ("f_nnz", c_int64), ("ws_bytes", c_int64),
                ("d", c_int32), ("k", c_int32), ("flags", c_int32)]


TOPK_MAX = 128                              # GS_TOPK_MAX
assert ctypes.sizeof(TopkDesc) == 144      # static_assert in csrc/gs_topk.hip (passed by pointer, as RankDesc)


class WalkDesc(ctypes.Structure):
    """struct gs_walk_desc (include/graphsage_amd.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("starts", c_void_p), ("paths", c_void_p), ("counts", c_void_p),
                ("offsets", c_void_p), ("pairs", c_void_p),
                ("n_nodes", c_int64), ("nnz", c_int64), ("n_starts", c_int64), ("walk0", c_int64), ("n_walks", c_int64),
                ("ld_paths", c_int64), ("pairs_cap", c_int64),
                ("seed", c_uint64), ("thr_return", c_uint64), ("thr_common", c_uint64), ("thr_far", c_uint64),
                ("num_walks", c_int32), ("walk_len", c_int32)]


WALK_TAG = 0xA7 << 56                       # GS_WALK_TAG
WALK_ATTEMPTS = 256                         # GS_WALK_ATTEMPTS
WALK_MAX_LEN = 4096                         # GS_WALK_MAX_LEN
assert ctypes.sizeof(WalkDesc) == 152      # static_assert in csrc/gs_walk.hip (passed by pointer, as RankDesc)


class ImportanceDesc(ctypes.Structure):
    """struct gs_importance_desc (include/graphsage_amd.h)"""
    _fields_ = [("paths", c_void_p), ("table", c_void_p), ("stats", c_void_p),
                ("n_starts", c_int64), ("n_nodes", c_int64), ("ld_paths", c_int64),
                ("num_walks", c_int32), ("walk_len", c_int32), ("top", c_int32), ("slots", c_int32), ("pad_id", c_int32),
                ("reserved_", c_int32)]


IMPORTANCE_MAX_VISITS = 4096                # GS_IMPORTANCE_MAX_VISITS
IMPORTANCE_MAX_TOP = 4096                   # GS_IMPORTANCE_MAX_TOP
IMPORTANCE_MAX_SLOTS = 1024                 # GS_IMPORTANCE_MAX_SLOTS
assert ctypes.sizeof(ImportanceDesc) == 72  # static_assert in csrc/gs_importance.hip (passed by pointer, as WalkDesc)


class LogregDesc(ctypes.Structure):
    """struct gs_logreg_desc (include/graphsage_amd.h)"""
    _fields_ = [("X", c_void_p), ("rows", c_void_p), ("W", c_void_p), ("b", c_void_p), ("y_class", c_void_p),
                ("y_multi", c_void_p), ("loss", c_void_p), ("gW", c_void_p), ("gb", c_void_p), ("pred_class", c_void_p),
                ("pred_multi", c_void_p), ("ws", c_void_p),
                ("n", c_int64), ("n_rows", c_int64), ("ldx", c_int64), ("ldw", c_int64), ("ldy", c_int64), ("ldp", c_int64),
                ("ws_bytes", c_int64),
                ("d", c_int32), ("c", c_int32), ("mode", c_int32), ("flags", c_int32)]


LOGREG_FIT, LOGREG_PREDICT = 0, 1           # GS_LOGREG_FIT, GS_LOGREG_PREDICT (gs_logreg_desc.mode)
LOGREG_MAX_D, LOGREG_MAX_C = 512, 128       # GS_LOGREG_MAX_D, GS_LOGREG_MAX_C
assert ctypes.sizeof(LogregDesc) == 168    # static_assert in csrc/gs_logreg.hip (passed by pointer, as RankDesc)


class LogregJoinedDesc(ctypes.Structure):
    """struct gs_logreg_joined_desc (include/graphsage_amd.h)"""
    _fields_ = [("Xa", c_void_p), ("rows_a", c_void_p), ("Xb", c_void_p), ("rows_b", c_void_p), ("mu", c_void_p),
                ("inv", c_void_p), ("W", c_void_p), ("b", c_void_p), ("y_class", c_void_p), ("y_multi", c_void_p),
                ("loss", c_void_p), ("gW", c_void_p), ("gb", c_void_p), ("pred_class", c_void_p), ("pred_multi", c_void_p),
                ("ws", c_void_p),
                ("n", c_int64), ("n_rows_a", c_int64), ("lda", c_int64), ("n_rows_b", c_int64), ("ldb", c_int64),
                ("ldw", c_int64), ("ldy", c_int64), ("ldp", c_int64), ("ws_bytes", c_int64),
                ("da", c_int32), ("db", c_int32), ("c", c_int32), ("mode", c_int32), ("flags", c_int32), ("reserved_", c_int32)]


LOGREG_JOINED_MAX_D = 1024                  # GS_LOGREG_JOINED_MAX_D
COL_MOMENTS_MAX_CHUNKS = 256                # GS_COL_MOMENTS_MAX_CHUNKS
assert ctypes.sizeof(LogregJoinedDesc) == 224    # static_assert in csrc/gs_logreg.hip (passed by pointer, as LogregDesc)


class KmeansDesc(ctypes.Structure):
    """struct gs_kmeans_desc (include/graphsage_amd.h)"""
    _fields_ = [("X", c_void_p), ("rows", c_void_p), ("C", c_void_p), ("csq", c_void_p), ("xsq", c_void_p), ("prev", c_void_p),
                ("assign", c_void_p), ("dist", c_void_p), ("stats", c_void_p), ("ws", c_void_p),
                ("n", c_int64), ("n_rows", c_int64), ("ld", c_int64), ("ldc", c_int64), ("ws_bytes", c_int64),
                ("k", c_int32), ("d", c_int32)]


class KmeansMembersDesc(ctypes.Structure):
    """struct gs_kmeans_members_desc (include/graphsage_amd.h)"""
    _fields_ = [("assign", c_void_p), ("rows", c_void_p), ("rowptr", c_void_p), ("members", c_void_p), ("ws", c_void_p),
                ("n", c_int64), ("ws_bytes", c_int64),
                ("k", c_int32), ("chunk", c_int32), ("reserved_", c_int64)]


KMEANS_MAX_K = 4096                         # GS_KMEANS_MAX_K
KMEANS_CHUNK = 2048                         # GS_KMEANS_CHUNK
assert ctypes.sizeof(KmeansDesc) == 128    # static_assert in csrc/gs_kmeans.hip (passed by pointer, as LogregDesc)
assert ctypes.sizeof(KmeansMembersDesc) == 72


class IvfDesc(ctypes.Structure):
    """struct gs_ivf_desc (include/graphsage_amd.h)"""
    _fields_ = [("Xq", c_void_p), ("Zc", c_void_p), ("centers", c_void_p), ("list_ptr", c_void_p), ("list_ids", c_void_p),
                ("src", c_void_p), ("f_rowptr", c_void_p), ("f_col", c_void_p),
                ("ids", c_void_p), ("scores", c_void_p), ("count", c_void_p), ("scanned", c_void_p), ("ws", c_void_p),
                ("Q", c_int64), ("ldq", c_int64), ("n_rows", c_int64), ("n_cand", c_int64), ("ldz", c_int64), ("ldc", c_int64),
                ("n_list", c_int64), ("f_nnz", c_int64), ("ws_bytes", c_int64),
                ("d", c_int32), ("k", c_int32), ("nprobe", c_int32), ("n_clusters", c_int32), ("flags", c_int32),
                ("stop_after", c_int32)]


IVF_MAX_PROBE = 128                         # GS_IVF_MAX_PROBE
assert ctypes.sizeof(IvfDesc) == 200       # static_assert in csrc/gs_ivf.hip (passed by pointer, as TopkDesc)


class PropDesc(ctypes.Structure):
    """struct gs_prop_desc (include/graphsage_amd.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("items", c_void_p), ("splits", c_void_p), ("X", c_void_p),
                ("R", c_void_p), ("w", c_void_p), ("out", c_void_p), ("ws", c_void_p),
                ("n_rows", c_int64), ("nnz", c_int64), ("n_items", c_int64), ("n_split", c_int64), ("n_slots", c_int64),
                ("pad", c_int64), ("ldx", c_int64), ("ldr", c_int64), ("ldo", c_int64), ("ws_bytes", c_int64),
                ("alpha", c_float), ("lo", c_float), ("hi", c_float),
                ("d", c_int32), ("split_len", c_int32), ("reserved_", c_int32)]


PROP_MAX_D = 256                            # GS_PROP_MAX_D
assert ctypes.sizeof(PropDesc) == 176      # static_assert in csrc/gs_propagate.hip (passed by pointer, as CsrReduceDesc)


class NbrRankDesc(ctypes.Structure):
    """struct gs_nbr_rank_desc (include/graphsage_amd.h)"""
    _fields_ = [(n, c_void_p) for n in ("rowptr", "col", "q", "deg", "f_rowptr", "f_col", "group_ptr", "group_src", "dst", "t",
                                        "n_gt", "n_eq", "ws")] + \
               [(n, c_int64) for n in ("n_nodes", "n_groups", "n_queries", "ws_stride", "ws_bytes")] + \
               [(n, c_int32) for n in ("kind", "tile", "max_workgroups", "reserved_")]


NBR_TILE, NBR_MIN_TILE, NBR_MAX_TILE = 8192, 64, 16384      # GS_NBR_TILE, GS_NBR_MIN_TILE, GS_NBR_MAX_TILE
NBR_PARTNER_CHUNK, NBR_CURSORS = 64, 2048                   # GS_NBR_PARTNER_CHUNK, GS_NBR_CURSORS
NBR_SUM, NBR_JACCARD = 0, 1                                 # GS_NBR_SUM, GS_NBR_JACCARD
assert ctypes.sizeof(NbrRankDesc) == 160   # static_assert in csrc/gs_nbr_rank.hip (passed by pointer, as PropDesc)

EXPORTED_SYMBOLS = sorted(list(_PROTOS.keys()) + ["gs_last_error", "gs_abi_version"])

_lib = None


def load(build_if_missing=True):
    """Load (building first if hipcc is available and the sources changed) and return the CDLL."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64 (SONAME libamdhip64.so.7); it must be mapped BEFORE this library so that the
    # dynamic linker binds our NEEDED libamdhip64.so.7 to that same runtime.  Loading ours first would map
    # /opt/rocm's copy and torch would then bring in a second HIP runtime (its NEEDED entry is the un-versioned
    # name) -- two runtimes in one process do not share streams or allocations ("no ROCm-capable device").
    import torch  # noqa: F401
    alt = os.environ.get("GS_LIB")          # A/B hook: load this prebuilt library instead (no build / digest check)
    if alt:
        build_if_missing = False
    if build_if_missing:
        try:
            from . import build as _build
            _build.build()
        except Exception as e:  # no hipcc on this box: fall through to the prebuilt library check
            if not os.path.exists(LIB_PATH):
                raise GraphsageAmdError("libgraphsage_amd.so is missing and could not be built: %s" % e)
    path = alt or LIB_PATH
    if not os.path.exists(path):
        raise GraphsageAmdError("HIP extension not found at %s (run python -m graphsage_amd.build)" % path)
    lib = ctypes.CDLL(path)
    lib.gs_last_error.restype = c_char_p
    lib.gs_last_error.argtypes = []
    lib.gs_abi_version.restype = c_int
    lib.gs_abi_version.argtypes = []
    got = lib.gs_abi_version()
    if got != GS_ABI_VERSION:
        raise GraphsageAmdError("%s has ABI version %d but this package binds version %d: the ctypes struct layouts "
                                "would not match (rebuild with python -m graphsage_amd.build --force)"
                                % (LIB_PATH, got, GS_ABI_VERSION))
    for name, argtypes in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = c_int
        fn.argtypes = argtypes
    # struct layouts: the library's sizeof() of every descriptor must equal the ctypes mirror's
    mirrors = [GatherDesc, WgradDesc, VarDesc, FanoutDesc, TailDesc, Dropout, PullDesc, LpTailDesc]
    sizes = (c_int32 * 16)()
    n = lib.gs_abi_struct_sizes(sizes, 16)
    if n != len(mirrors):
        raise GraphsageAmdError("%s exports %d descriptor structs, this package mirrors %d" % (LIB_PATH, n, len(mirrors)))
    for cls, size in zip(mirrors, sizes):
        if ctypes.sizeof(cls) != size:
            raise GraphsageAmdError("struct layout mismatch: sizeof(%s) is %d in %s but %d in graphsage_amd/_lib.py"
                                    % (cls.__doc__.split()[1], size, LIB_PATH, ctypes.sizeof(cls)))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().gs_last_error()
        raise GraphsageAmdError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


_DEBUG_SYNC = os.environ.get("GS_DEBUG_SYNC", "0") == "1"


def call(name, *args):
    lib = load()
    if _DEBUG_SYNC:
        import sys
        import torch
        sys.stderr.write("[gs] %s %s\n" % (name, " ".join(str(a) for a in args)))
        sys.stderr.flush()
    rc = getattr(lib, name)(*args)
    check(rc, name)
    if _DEBUG_SYNC and not name.startswith(("gs_capture", "gs_graph", "gs_stream", "gs_event")):
        torch.cuda.synchronize()


def set_wgrad_tiled3_form(form):
    """gs_set_wgrad_tiled3_form: which kernel the next gs_dense_wgrad_grouped_tiled3[_sample] launches take (0 | 1).  A host-side
    switch that launches nothing, so it does not go through call() (the per-launch debug sync / log)."""
    check(load().gs_set_wgrad_tiled3_form(int(form)), "gs_set_wgrad_tiled3_form")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL).  Refuses CPU tensors: no CPU fallback."""
    if t is None:
        return None
    if not t.is_cuda:
        raise GraphsageAmdError("graphsage_amd kernels need device (HIP) tensors; got a CPU tensor")
    return t.data_ptr()


def host_ptr(a):
    """Pointer of a contiguous numpy array (host-side entry points only)."""
    if a is None:
        return None
    return a.ctypes.data
