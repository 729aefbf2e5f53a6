"""The C ABI of ``libxfmr_hip.so`` as ctypes: the Structures and one signature table per header.

``SIGNATURES`` has one row per prototype of ``include/xfmr_hip.h`` (the public ``xfmr_*`` entries), ``INTERNAL_SIGNATURES`` one
per ``extern "C"`` prototype of ``csrc/internal.h`` (the ``xf_*`` entries that tests and probes call directly),
``SESSION_SIGNATURES`` one per prototype of ``include/xfmr_session.h`` (the session encoder), ``SEARCH_SIGNATURES`` one per
prototype of ``include/xfmr_search.h`` (the refined item search); ``bind`` applies them to a ``CDLL``. No other file keeps a signature: ``tests/test_abi_tables_host.py`` holds every row and every Structure to its
header. This module imports ``ctypes`` only, so that a child process without torch can load it by file path.
"""

from __future__ import annotations

import ctypes as C


class EncoderCfg(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("seq_len", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32),
        ("inter", C.c_int32), ("layers", C.c_int32), ("max_pos", C.c_int32), ("precision", C.c_int32),
        ("ln_eps", C.c_float), ("hidden_dropout", C.c_float), ("attn_dropout", C.c_float),
        ("flags", C.c_uint32), ("seed", C.c_uint64),
        ("step_device", C.c_void_p), ("embed_event", C.c_void_p), ("context", C.c_void_p),
        ("grads_half_event", C.c_void_p),
        ("profile_kernel", C.c_int32), ("profile_layer", C.c_int32), ("profile_events", C.c_void_p * 2),
        # ABI 3: packed rows (all NULL / 0 = the padded (B, L) layout)
        ("seq_offsets", C.c_void_p), ("row_pos", C.c_void_p), ("packed_rows", C.c_int64),
    ]


class LossCfg(C.Structure):
    _fields_ = [
        ("train_head", C.c_int32), ("all_heads", C.c_int32), ("mask_false_negatives", C.c_int32),
        ("mode", C.c_int32), ("precision", C.c_int32), ("scale", C.c_float), ("margin", C.c_float),
        ("num_hard_negatives", C.c_int32), ("flags", C.c_uint32),
        ("profile_grad", C.c_void_p * 2), ("profile_log", C.c_void_p * 2),
        ("padded_positions", C.c_int64),  # ABI 3
    ]


class OptCfg(C.Structure):
    _fields_ = [
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
        ("grad_scale", C.c_float), ("clip_mode", C.c_int32), ("clip_val", C.c_float), ("sched", C.c_int32),
        ("step_offset", C.c_int32), ("warmup_steps", C.c_int64), ("total_steps", C.c_int64), ("step", C.c_int64),
        ("step_device", C.c_void_p),
    ]


class Seed(C.Structure):
    """csrc/common.h XfSeed, by value: the dropout seed argument of the internal entry points. A plain int converts to
    (seed, no device-side counter)."""

    _fields_ = [("seed", C.c_uint64), ("dyn", C.c_void_p)]

    @classmethod
    def from_param(cls, v):
        return v if isinstance(v, cls) else cls(int(v), None)


class DwItem(C.Structure):  # csrc/internal.h XfDwItem: one weight gradient of xf_linear_bwd_dw_group / xf_dw_ring_*
    _fields_ = [("dy", C.c_void_p), ("x", C.c_void_p), ("N", C.c_int32), ("K", C.c_int32), ("slabs", C.c_void_p),
                ("bias_part", C.c_void_p), ("splits", C.c_void_p)]


class ReduceSeg(C.Structure):  # csrc/internal.h XfReduceSeg: one segment of xf_multi_rowsum
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("ld", C.c_int),
                ("pad", C.c_int)]


class LnResidual(C.Structure):  # csrc/internal.h XfLnResidual: the re-derived residual of the xf_*_re forward entries
    _fields_ = [("pre", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("dropout_p", C.c_float), ("site", C.c_uint32)]


_P = C.c_void_p
_I32, _U32, _I64, _U64, _F = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float
_PI32 = C.POINTER(C.c_int32)  # a host array of int32 (plan records, switches, counts written back to the caller)

# include/xfmr_hip.h, in the order the package came to bind them
SIGNATURES = {
    "xfmr_strerror": (C.c_char_p, [C.c_int]),
    "xfmr_abi_version": (C.c_int, []),
    "xfmr_low_priority_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "xfmr_context_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "xfmr_context_destroy": (C.c_int, [_P]),
    "xfmr_stream_destroy": (C.c_int, [_P]),
    "xfmr_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "xfmr_event_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32]),
    "xfmr_event_destroy": (C.c_int, [_P]),
    "xfmr_event_record": (C.c_int, [_P, _P]),
    "xfmr_stream_wait_event": (C.c_int, [_P, _P]),
    "xfmr_event_elapsed_ms": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "xfmr_event_synchronize": (C.c_int, [_P]),
    "xfmr_event_query": (C.c_int, [_P]),
    "xfmr_batch_upload": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P]),
    "xfmr_param_count": (C.c_int64, [C.POINTER(EncoderCfg)]),
    "xfmr_param_half_offset": (C.c_int64, [C.POINTER(EncoderCfg)]),
    "xfmr_param_offsets": (C.c_int32, [C.POINTER(EncoderCfg), C.POINTER(C.c_int64), C.c_int32]),
    "xfmr_embed_ln_fwd": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_uint32, _P]),
    "xfmr_pack_rows": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "xfmr_pack_rows_ordered": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "xfmr_embed_param_grads": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "xfmr_layernorm_fwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P]),
    "xfmr_layernorm_bwd_workspace": (C.c_size_t, [C.c_int64, C.c_int32]),
    "xfmr_layernorm_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float,
                                     C.c_uint64, C.c_uint32, _P, _P]),
    "xfmr_linear_fwd": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_float,
                                  C.c_uint64, C.c_uint32, C.c_int32, _P]),
    "xfmr_linear_bwd_dx": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    "xfmr_linear_bwd_dw_workspace": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "xfmr_linear_bwd_dw": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, _P]),
    "xfmr_colsum_workspace": (C.c_size_t, [C.c_int64, C.c_int32]),
    "xfmr_colsum": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    "xfmr_attn_fwd": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64,
                                C.c_uint32, C.c_int32, _P]),
    "xfmr_attn_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                C.c_uint64, C.c_uint32, C.c_int32, _P]),
    "xfmr_attn_fwd_mode": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64,
                                     C.c_uint32, C.c_int32, C.c_int32, _P]),
    "xfmr_attn_bwd_mode": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                     C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _P]),
    "xfmr_encoder_workspace_bytes": (C.c_size_t, [C.POINTER(EncoderCfg)]),
    "xfmr_encoder_fwd": (C.c_int, [C.POINTER(EncoderCfg), _P, _P, _P, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_encoder_bwd": (C.c_int, [C.POINTER(EncoderCfg), _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_encoder_infer_workspace_bytes": (C.c_size_t, [C.POINTER(EncoderCfg)]),
    "xfmr_encoder_infer": (C.c_int, [C.POINTER(EncoderCfg), _P, _P, _P, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_mean_pool": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "xfmr_pool": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "xfmr_pool_rows": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P]),
    "xfmr_l2_normalize_fwd": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P]),
    "xfmr_l2_normalize_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P]),
    "xfmr_sampled_loss_workspace": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int64]),
    "xfmr_sampled_loss_workspace_cfg": (C.c_size_t, [C.POINTER(LossCfg), C.c_int64, C.c_int32, C.c_int64]),
    "xfmr_sampled_loss": (C.c_int, [C.POINTER(LossCfg), _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32,
                                    _P, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_sampled_loss_prepare": (C.c_int, [C.POINTER(LossCfg), _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P,
                                            C.c_size_t, _P]),
    "xfmr_sampled_loss_prepared": (C.c_int, [C.POINTER(LossCfg), _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64,
                                             C.c_int32, _P, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_sampled_loss_lists_workspace": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int64]),
    "xfmr_sampled_loss_lists_workspace_cfg": (C.c_size_t, [C.POINTER(LossCfg), C.c_int64, C.c_int64, C.c_int32,
                                                           C.c_int64]),
    "xfmr_sampled_loss_lists": (C.c_int, [C.POINTER(LossCfg), _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64,
                                          C.c_int32, _P, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_dense_loss_workspace": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "xfmr_dense_loss": (C.c_int, [C.POINTER(LossCfg), _P, _P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P,
                                  _P, _P, C.c_size_t, _P]),
    "xfmr_dense_loss_grads": (C.c_int, [C.POINTER(LossCfg), _P, _P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P,
                                        _P, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_table_rnorm": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "xfmr_table_prepare": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P]),
    "xfmr_seq_sample_workspace": (C.c_size_t, [C.c_int32, C.c_int64]),
    "xfmr_seq_sample": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                  C.c_uint64, _P, _P, _P, _P, C.c_size_t, _P]),
    "xfmr_seq_sample_rows_workspace": (C.c_size_t, [C.c_int32, C.c_int32]),
    "xfmr_seq_sample_rows": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P,
                                       C.c_size_t, _P]),
    "xfmr_topk_workspace": (C.c_size_t, [C.c_int64, C.c_int64]),
    "xfmr_topk": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P,
                            C.c_size_t, _P]),
    "xfmr_retrieval_metrics": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "xfmr_retrieval_metrics_sum_workspace": (C.c_size_t, [C.c_int64]),
    "xfmr_retrieval_metrics_sum": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_size_t,
                                             _P]),
    "xfmr_topk_tiled_workspace": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "xfmr_topk_tiled": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P,
                                  _P, C.c_size_t, _P]),
    "xfmr_target_ranks_workspace": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "xfmr_target_ranks": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, C.c_int64, C.c_int32,
                                    _P, _P, _P, C.c_size_t, _P]),
    "xfmr_candidate_ranks": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32,
                                       _P, _P, _P, _P]),
    "xfmr_rank_metrics_sum_workspace": (C.c_size_t, [C.c_int64, C.c_int32]),
    "xfmr_rank_metrics_sum": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int32), C.c_int32, _P, _P, _P, _P,
                                        C.c_size_t, _P]),
    "xfmr_table_sqnorm": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "xfmr_adamw": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                             C.c_int64, C.c_float, _P]),
    "xfmr_adamw_dev": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                 _P, C.c_int32, C.c_float, _P]),
    "xfmr_step_advance": (C.c_int, [_P, _P]),
    "xfmr_lr_lambda": (C.c_float, [C.c_int32, C.c_int64, C.c_int64, C.c_int64]),
    "xfmr_opt_workspace": (C.c_size_t, [C.c_int64]),
    "xfmr_opt_prepare": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "xfmr_adamw_ctl": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _P, _P]),
    "xfmr_grad_accumulate": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "xfmr_scale_by_device_scalar": (C.c_int, [_P, C.c_int64, _P, _P]),
    "xfmr_selftest_mfma": (C.c_int, [_P, _P]),
    "xfmr_comm_unique_id": (C.c_int, [_P]),
    "xfmr_comm_create": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "xfmr_comm_destroy": (C.c_int, [_P]),
    "xfmr_allreduce_flat": (C.c_int, [_P, _P, C.c_int64, _P]),
    "xfmr_comm_last_error": (C.c_char_p, []),
}

# The tails several rows share, as csrc/internal.h writes them.
_SEED_SITE = [_F, Seed, _U32]  # float dropout_p, XfSeed seed, uint32_t site
_LN_OUT = [_P, _P, _F, _P, _P, _P, _P]  # gamma, beta, eps, y, y16, mean, rstd



def _ln_fwd(res):  # xf_linear_ln_fwd_{ex,re}: x, w, bias, pre, M, N, K, the residual, ..., precision, s16, stream
    return [_P, _P, _P, _P, _I64, _I32, _I32, res] + _SEED_SITE + _LN_OUT + [_I32, _U32, _P]


def _ffn_fwd(res):  # xf_ffn_fwd_fused_{ex,re}: x16, w1_16, b1, w2_16, b2, u16, g16, pre, M, H, I, the residual, ..., stream
    return [_P] * 8 + [_I64, _I32, _I32, res] + _SEED_SITE + _LN_OUT + [_P]


_LNBWD_TAIL = [_P] * 5 + _SEED_SITE + [_P, _P, _P, _PI32]  # residual_grad, ln_x/mean/rstd/gamma, ..., dx, d_lin16, partials, blocks_out
_EMBED_HEAD = [_P, _P, _I64] + [_P] * 10  # item_idx, table, n_rows, pos/type emb, gamma, beta, out, out16, pre, mean, rstd, key_mask
_LOSS_KEY = [_I64, _I32, _I64] + [_I32] * 6 + [_U32, _I32, _I32, _I32, _U64, _PI32]

# csrc/internal.h, in the header's order; C++ default arguments are rows at full arity
INTERNAL_SIGNATURES = {
    "xf_row_plan": (C.c_int, [_I32, _I64, _I32, _I32, _I32, _PI32]),
    "xf_gemm_plan": (C.c_int, [_I32, _I64, _I32, _I32, _I32, _U32, _I32, _I32, _PI32, _PI32]),
    "xf_gemm_switches": (None, [_PI32]),
    "xf_linear_fwd_ex": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I32, _I32, _P, _P] + _SEED_SITE + [_I32, _U32, _P]),
    "xf_ffn_fwd_fused_ex": (C.c_int, _ffn_fwd(_P)),
    "xf_ffn_fwd_fused_re": (C.c_int, _ffn_fwd(C.POINTER(LnResidual))),
    "xf_linear_ln_fwd_re": (C.c_int, _ln_fwd(C.POINTER(LnResidual))),
    "xf_linear_gelu_fwd_infer": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I32, _I32, _U32, _P]),
    "xf_linear_ln_fwd_infer": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _P, _F, _P, _P, _I32, _U32, _P]),
    "xf_ffn_fwd_fused_infer": (C.c_int, [_P] * 5 + [_I64, _I32, _I32, _P, _P, _P, _F, _P, _P, _P]),
    "xf_ffn_bwd_dx_fused_ex": (C.c_int, [_P] * 5 + [_I64, _I32, _I32] + _LNBWD_TAIL + [_P]),
    "xf_linear_bwd_dx_ex": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _I32, _U32, _P]),
    "xf_linear_bwd_dw_ex": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _I32, _P, C.c_size_t, _U32, _P]),
    "xf_colsum_ex": (C.c_int, [_P, C.c_bool, _P, _I64, _I32, _P, _P]),
    "xf_linear_bwd_dw_slab_bytes": (C.c_size_t, [_I64, _I32, _I32]),
    "xf_linear_bwd_dw_deferred": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _U32, _P, _P, _PI32, _P]),
    "xf_linear_bwd_dw_group": (C.c_int, [C.POINTER(DwItem), C.c_int, _I64, _I32, _U32, _P]),
    "xf_dw_split_plan": (C.c_int, [_I64, _I32, _I32, _PI32]),
    "xf_dw_ring_takes": (C.c_bool, [C.POINTER(DwItem), C.c_int, _I64, _I32, _U32]),
    "xf_dw_ring_launch": (C.c_int, [C.POINTER(DwItem), C.c_int, _I64, _P]),
    "xf_multi_rowsum": (C.c_int, [C.POINTER(ReduceSeg), C.c_int, _P]),
    "xf_rowsum": (C.c_int, [_P, _P, _I64, _I64, _P]),
    "xf_attn_fwd_ex": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32] + _SEED_SITE
                       + [_I32, C.c_bool, C.c_bool, _P, _P, C.c_bool]),
    "xf_attn_bwd_ex": (C.c_int, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32] + _SEED_SITE
                       + [_I32, C.c_bool, C.c_bool, _P, _P, C.c_bool]),
    "xf_loss_finalize": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _I64, _I64, _P, _P, _P, _P]),
    "xf_linear_ln_fwd_ex": (C.c_int, _ln_fwd(_P)),
    "xf_linear_bwd_dx_lnbwd_ex": (C.c_int, [_P, _P, _I64, _I32, _I32] + _LNBWD_TAIL + [_I32, _U32, _P, _F, _U32]),
    "xf_ln_row_tiles": (C.c_int, [_I64]),
    "xf_layernorm_fwd_ex": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _F, _P]),
    "xf_embed_ln_fwd_ex": (C.c_int, _EMBED_HEAD + [_I32, _I32, _I32, _F] + _SEED_SITE + [_P]),
    "xf_embed_ln_fwd_packed_ex": (C.c_int, _EMBED_HEAD + [_I64, _P, _I32, _F] + _SEED_SITE + [_P]),
    "xf_embed_param_grads_packed": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "xf_encoder_plan": (C.c_int, [C.POINTER(EncoderCfg), _PI32]),
    "xf_attn_plan": (C.c_int, [_I32] * 11 + [_PI32]),
    "xf_attn_switches": (C.c_int, []),
    "xf_loss_plan": (C.c_int, _LOSS_KEY),
    "xf_loss_plan_ext": (C.c_int, _LOSS_KEY),
    "xf_loss_switches": (_U64, []),
}

# include/xfmr_session.h (the session encoder), in the header's order; tests/test_session_abi_host.py holds it to the header
SESSION_SIGNATURES = {
    "xfmr_session_state_bytes": (C.c_size_t, [C.POINTER(EncoderCfg), _I32]),
    "xfmr_session_workspace_bytes": (C.c_size_t, [C.POINTER(EncoderCfg), _I64]),
    "xfmr_session_plan": (C.c_int, [C.POINTER(EncoderCfg), _PI32]),
    "xfmr_session_init": (C.c_int, [C.POINTER(EncoderCfg), _P, _P, C.c_size_t, _I32, _P]),
    "xfmr_session_append": (C.c_int, [C.POINTER(EncoderCfg), _P, _P, C.c_size_t, _I32, _P, _P, _P, _I64, _P, _I64, _P, _P,
                                      C.c_size_t, _P]),
    "xfmr_session_pool": (C.c_int, [C.POINTER(EncoderCfg), _P, C.c_size_t, _I32, _P, _P, _I32, _I32, _I32, _F, _P, _P]),
}

# include/xfmr_search.h (the refined item search), in the header's order; tests/test_search_refined_host.py holds it to the header
SEARCH_SIGNATURES = {
    "xfmr_search_refined_workspace": (C.c_size_t, [_I64, _I64, _I32]),
    "xfmr_search_refined_plan": (C.c_int, [_I64, _I64, _I32, _I32, _I32, _PI32]),
    "xfmr_search_refined": (C.c_int, [_P, _P, _P, _P, _P, _F, _F, _I64, _I64, _I32, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P,
                                      C.c_size_t, _P]),
}

# prototypes of csrc/internal.h that ctypes cannot call, each with its reason
NOT_BOUND = (
    ("xf_layernorm_bwd_impl", "takes XfDropout by value, a C++ struct with no mirror here"),
    ("xf_dw_ring_launch_plans", "takes GemmPlan*, the library's own C++ plan record"),
)


def bind(cdll: C.CDLL) -> C.CDLL:
    """Give every entry of the tables its restype and argtypes on ``cdll``; a symbol the library lacks is named."""
    for table in (SIGNATURES, INTERNAL_SIGNATURES, SESSION_SIGNATURES, SEARCH_SIGNATURES):
        for name, (res, args) in table.items():
            try:
                fn = getattr(cdll, name)
            except AttributeError as e:
                raise AttributeError(f"{getattr(cdll, '_name', cdll)} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
    return cdll
