"""ctypes binding of ``libdaisyrec_hip.so`` (declared in ``include/daisyrec_amd.h``).

The HIP library IS the product: there is no CPU or PyTorch fallback.  Importing
this module without the built library raises ``ImportError`` with the build
command, and every call checks the status code and raises.
"""
from __future__ import annotations

import ctypes as C
import os

# torch bundles its own HIP/HSA runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).
# It MUST be mapped before our library so that the dynamic linker binds our NEEDED
# libamdhip64.so.7 to that same copy: two HIP runtimes in one process do not share streams
# or device state (observed: "no ROCm-capable device is detected" from the second copy).
import torch  # noqa: F401  (side effect: loads torch's HIP runtime first)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DAISY_LIB_OVERRIDE") or os.path.join(_HERE, "lib", "libdaisyrec_hip.so")

DAISY_OK, DAISY_ERR_ARG, DAISY_ERR_HIP, DAISY_ERR_STATE = 0, 1, 2, 3
LOSS_BPR, LOSS_HL, LOSS_TL, LOSS_CL, LOSS_SL = 0, 1, 2, 3, 4
ITEM_ATOMIC, ITEM_SORTED, ITEM_CHUNKED, ITEM_FUSED = 0, 1, 2, 3
ORDER_IDENTITY, ORDER_PERM, ORDER_FEISTEL = 0, 1, 2
PLAN_TRIPLES_USER_SORTED = 1
PLAN_POINTWISE = 2
STATS_LEN = 16
ST_LOSS_DATA, ST_L1_U, ST_L1_I, ST_L1_J, ST_SQ_U, ST_SQ_I, ST_SQ_J = range(7)
ST_LOSS, ST_NORM_U, ST_NORM_I, ST_NORM_J = 7, 8, 9, 10
ST_SUM_COEF = 12
ST_SQ_U_PRE = 13
ABI_VERSION = 8
NGCF_MAX_WIDTH, NGCF_NODE_STREAM, NGCF_MESS_STREAM = 256, 0x100, 0x200

_p = C.c_void_p
_i32, _i64, _u64, _f32, _sz = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_size_t

NEUMF_MAX_LAYERS = 8
NEUMF_FULL, NEUMF_GMF, NEUMF_MLP = 0, 1, 2
NST_LOSS_DATA, NST_L1, NST_SQ, NST_LOSS, NST_NORM, NST_LOSS_SUM, NEUMF_STATS_LEN = 0, 1, 6, 11, 12, 17, 24


class NeumfParams(C.Structure):
    """daisy_neumf_params: table of device pointers (include/daisyrec_amd.h)."""
    _fields_ = [("uG", _p), ("iG", _p), ("uM", _p), ("iM", _p),
                ("W", _p * NEUMF_MAX_LAYERS), ("b", _p * NEUMF_MAX_LAYERS), ("Wp", _p), ("bp", _p)]


_pp = C.POINTER(NeumfParams)

SMALL_TRIAL_WS_BYTES = 192


class SmallTrial(C.Structure):
    """daisy_small_trial: one model of daisy_bpr_fit_epoch_sgd_many (include/daisyrec_amd.h)."""
    _fields_ = [("ctx", _p), ("plan", _p), ("P", _p), ("Q", _p), ("loss_type", C.c_int32), ("gamma", C.c_float),
                ("lr", C.c_float), ("reg_1", C.c_float), ("reg_2", C.c_float),
                ("stats", _p), ("epoch_acc", _p), ("step_losses", _p)]


GEMM_LAUNCH, GEMM_LAUNCH_H, GEMM_LAUNCH_PAIR = 0, 1, 2
GEMM_EPI_STORE, GEMM_EPI_BIAS_RELU, GEMM_EPI_GATE, GEMM_EPI_ATOMIC = 0, 1, 2, 3
GEMM_F32, GEMM_BF16IN, GEMM_H, GEMM_PAIR = 0, 1, 2, 3          # kernel family in daisy_gemm_desc.path


class GemmDesc(C.Structure):
    """daisy_gemm_desc: one product of daisy_gemm_case (include/daisyrec_amd.h)."""
    _fields_ = [("launcher", C.c_int32), ("epilogue", C.c_int32), ("bf16", C.c_int32), ("c_bf16", C.c_int32),
                ("A", _p), ("B", _p), ("C", _p), ("bias", _p), ("gate", _p),
                ("sam", C.c_int64), ("sak", C.c_int64), ("sbn", C.c_int64), ("sbk", C.c_int64),
                ("ldc", C.c_int64), ("scn", C.c_int64), ("ldg", C.c_int64),
                ("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64), ("k_chunk", C.c_int64), ("slice_stride", C.c_int64),
                ("n_A", C.c_int64), ("n_B", C.c_int64), ("n_C", C.c_int64), ("n_bias", C.c_int64), ("n_gate", C.c_int64),
                ("gate_scale", C.c_float), ("drop_p", C.c_float), ("drop_seed", C.c_uint64),
                ("drop_stream", C.c_uint32), ("dry_run", C.c_int32), ("path", C.c_uint32), ("reserved", C.c_uint32)]


_gd = C.POINTER(GemmDesc)


def gemm_path(word):
    """daisy_gemm_desc.path decoded: (family, WN, FAST, DROP, AK, BK, k slices, k slices of a pair's second product)."""
    w = int(word)
    return (w & 3, (w >> 2) & 3, (w >> 4) & 1, (w >> 5) & 1, (w >> 6) & 1, (w >> 7) & 1, (w >> 8) & 0xFFF, (w >> 20) & 0xFFF)

NFM_MAX_LAYERS, NFM_MAX_FACTORS, NFM_DROP_STREAM, NFM_SMALL_MAX_B = 8, 256, 0x300, 256
NFM_PATHS = {"auto": 0, "small": 1, "layered": 2}
NFM_ACT = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}
NFST_LOSS, NFST_LOSS_SUM, NFST_LOSS_DATA, NFST_NORM_U, NFST_NORM_I, NFST_NORM_J, NFST_NONFINITE = range(7)
NFM_STATS_LEN = 8


class NfmParams(C.Structure):
    """daisy_nfm_params: table of device pointers (include/daisyrec_amd.h)."""
    _fields_ = [("P", _p), ("Q", _p), ("ub", _p), ("ib", _p), ("bias", _p),
                ("bn_w", _p * (NFM_MAX_LAYERS + 1)), ("bn_b", _p * (NFM_MAX_LAYERS + 1)),
                ("W", _p * NFM_MAX_LAYERS), ("b", _p * NFM_MAX_LAYERS), ("wp", _p)]


class NfmBnState(C.Structure):
    """daisy_nfm_bn_state: the BatchNorm buffers of every stage."""
    _fields_ = [("mean", _p * (NFM_MAX_LAYERS + 1)), ("var", _p * (NFM_MAX_LAYERS + 1)),
                ("nbt", _p * (NFM_MAX_LAYERS + 1))]


_np = C.POINTER(NfmParams)
_nb = C.POINTER(NfmBnState)

VAE_MAX_HIDDEN, VAE_KEEP_STREAM, VAE_EPS_STREAM = 8, 0x400, 0x401
VST_LOSS, VST_LOSS_SUM, VST_CE, VST_KL, VST_NONFINITE, VST_BAD_ROWS = range(6)
VAE_STATS_LEN = 8
SLIM_LDS_ITEMS, SLIM_MAX_TOPK = 9984, 1024
SLIM_PATHS = {"auto": 0, "lds": 1, "global": 2}
PSVD_MAX_C, PSVD_CONVERGED, PSVD_NOT_CONVERGED = 256, 0, 1
EASE_BLOCK = 64
IALS_MAX_D = 128
KNN_MAX_K = 1024
WALK2_LDS_COLS = 32768
KNN_CENTER = {"none": 0, "row": 1, "col": 2, "binary": 3}
KNN_MODES = {"cosine": 0, "asymmetric": 1, "tanimoto": 2, "dice": 3, "tversky": 4, "plain": 5}
# daisy_ranking_kpis: bit (1 << id) of the metrics mask; the first KPI_PER_USER have a value per list
KPI_IDS = {"precision": 0, "recall": 1, "hit": 2, "mrr": 3, "map": 4, "ndcg": 5, "f1": 6, "auc": 7, "popularity": 8,
           "diversity": 9, "coverage": 10}
KPI_PER_USER = 10
KPI_FULL_AUC = 11        # daisy_position_kpis only: the exact AUC over all eligible items
METRICS_MAX_K, METRICS_MAX_CUTOFFS, METRICS_MAX_CATS = 256, 12, 256

# name -> (restype, argtypes); every symbol include/daisyrec_amd.h declares
SIGNATURES = {
    "daisy_last_error": (C.c_char_p, []),
    "daisy_abi_version": (C.c_int, []),
    "daisy_bpr_ctx_create": (C.c_int, [C.POINTER(_p), _i64, _i32, _i64, _i64]),
    "daisy_bpr_ctx_destroy": (C.c_int, [_p]),
    "daisy_bpr_ctx_scratch_bytes": (_sz, [_p]),
    "daisy_bpr_set_batch_from_triples": (C.c_int, [_p, _p, _i64, _p, _i64, _i64, _i32, _p]),
    "daisy_bpr_set_batch": (C.c_int, [_p, _p, _p, _p, _i64, _p]),
    "daisy_bpr_set_batch_from_plan": (C.c_int, [_p, _p, _i64, _p]),
    "daisy_bpr_ctx_set_pointwise": (C.c_int, [_p, _i32]),
    "daisy_bpr_ctx_set_bias": (C.c_int, [_p, _p, _p, _p, _p, _p, _p]),
    "daisy_epoch_plan_create": (C.c_int, [C.POINTER(_p), _i64, _i64, _i64]),
    "daisy_epoch_plan_destroy": (C.c_int, [_p]),
    "daisy_epoch_plan_bytes": (_sz, [_p]),
    "daisy_epoch_plan_build": (C.c_int, [_p, _p, _i64, _p, _i32, _u64, _u64, _i64, _i32, _i32, _p]),
    "daisy_epoch_plan_num_batches": (_i64, [_p]),
    "daisy_epoch_plan_validate": (C.c_int, [_p, _p]),
    "daisy_bpr_ctx_validate_batch": (C.c_int, [_p, _p]),
    "daisy_epoch_plan_read_batch": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _p, C.POINTER(_i64), _p]),
    "daisy_feistel_positions": (C.c_int, [_i64, _u64, _u64, _p, _p]),
    "daisy_feistel_positions_at": (C.c_int, [_p, _i64, _i64, _u64, _u64, _p, _p]),
    "daisy_train_index_create": (C.c_int, [C.POINTER(_p), _p, _i64, _i64, _i64, _i32, _i32, _p]),
    "daisy_train_index_destroy": (C.c_int, [_p]),
    "daisy_train_index_bytes": (_sz, [_p]),
    "daisy_epoch_plan_build_indexed": (C.c_int, [_p, _p, _p, _i32, _u64, _u64, _i64, _p]),
    "daisy_epoch_plan_build_positions": (C.c_int, [_p, _p, _p, _i64, _i64, _p]),
    "daisy_epoch_plan_batch_rows": (_i64, [_p, _i64]),
    "daisy_bpr_ctx_invalidate_cache": (C.c_int, [_p]),
    "daisy_bpr_ctx_set_p_stream": (C.c_int, [_p, C.c_int32]),
    "daisy_bpr_staged_prenorm": (C.c_int, [_p, _p, _p, _p]),
    "daisy_bpr_staged_user": (C.c_int, [_p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _p]),
    "daisy_bpr_staged_item": (C.c_int, [_p, _i32, _p, _p, _p, _f32, _f32, _f32, _p, _p]),
    "daisy_item_apply_counts": (C.c_int, [_p, _p, _p, _i64, _i32, _f32, _f32, _f32, _p, _p]),
    "daisy_bpr_staged_item_slices": (C.c_int, [_p, _p, _i32, _p]),
    "daisy_bpr_staged_item_slice": (C.c_int, [_p, _i32, _p, _p, _i32, _f32, _f32, _f32, _p, _p]),
    "daisy_bpr_staged_adam_step": (C.c_int, [_p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _p, _p, _p, _p, _p, _p,
                                             _f32, _f32, _f32, _i64, _p, _p, _p, _p]),
    "daisy_bpr_staged_adam_catchup_users": (C.c_int, [_p, _p, _p, _p, _p, _p, _f32, _f32, _f32, _i64, _p]),
    "daisy_bpr_staged_user_adam": (C.c_int, [_p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _p, _p, _f32, _f32, _f32, _i64,
                                             _p, _p]),
    "daisy_item_apply_counts_adam": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _i64,
                                               _p, _p]),
    "daisy_bpr_forward": (C.c_int, [_p, _p, _p, _i32, _f32, _p, _p]),
    "daisy_bpr_finalize": (C.c_int, [_p, _p, _f32, _f32, _p, _p, _p]),
    "daisy_bpr_item_grad": (C.c_int, [_p, _p, _p, _p, _f32, _f32, _p, _i32, _p]),
    "daisy_bpr_item_grad_data": (C.c_int, [_p, _p, _p, _p, _p, _i32, _p]),
    "daisy_bpr_item_grad_reg": (C.c_int, [_p, _p, _p, _f32, _f32, _p, _p]),
    "daisy_bpr_user_sgd": (C.c_int, [_p, _p, _p, _p, _f32, _f32, _f32, _p]),
    "daisy_bpr_user_grad": (C.c_int, [_p, _p, _p, _p, _f32, _f32, _p, _p]),
    "daisy_bpr_item_sgd_apply": (C.c_int, [_p, _p, _p, _f32, _i32, _p]),
    "daisy_adam_dense": (C.c_int, [_p, _p, _p, _p, _i64, _f32, _f32, _f32, _f32, _i64, _p]),
    "daisy_adam_lazy_table": (C.c_int, [_f32, _f32, _f32, _i64, _p]),
    "daisy_adam_lazy_catchup": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f32, _f32, _f32, _i64, _p]),
    "daisy_adam_lazy_step": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f32, _f32, _f32, _i64, _p]),
    "daisy_adam_lazy_flush": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p, _f32, _f32, _f32, _i64, _p]),
    "daisy_adagrad_dense": (C.c_int, [_p, _p, _p, _i64, _f32, _f32, _p]),
    "daisy_rmsprop_dense": (C.c_int, [_p, _p, _p, _i64, _f32, _f32, _f32, _p]),
    "daisy_bpr_sgd_step": (C.c_int, [_p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _p, _p, _p,
                                     _i32, _p]),
    "daisy_bpr_fit_epoch_sgd": (C.c_int, [_p, _p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _p, _p,
                                          _p, _i32, _p]),
    "daisy_bpr_fit_epoch_adam": (C.c_int, [_p, _p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _p, _p, _p, _p, _p, _p, _i64,
                                           _f32, _f32, _f32, _i64, _i32, _p, _p, _p, _p]),
    "daisy_bpr_small_epoch_supported": (C.c_int, [_p, _p, _i32]),
    "daisy_bpr_fit_epoch_sgd_many": (C.c_int, [C.POINTER(SmallTrial), _i32, _p, _sz, _p]),
    "daisy_mf_predict": (C.c_int, [_p, _p, _i32, _p, _p, _i64, _p, _p]),
    "daisy_mf_rank_workspace_bytes": (_sz, [_i64, _i64]),
    "daisy_mf_rank_topk": (C.c_int, [_p, _p, _i32, _p, _p, _i64, _i64, _i32, _p, _p, _p, _sz, _p]),
    "daisy_mf_full_rank_workspace_bytes": (_sz, [_i64]),
    "daisy_mf_full_rank": (C.c_int, [_p, _p, _i32, _i64, _i64, _i32, _p, _p, _sz, _p]),
    "daisy_fm_predict": (C.c_int, [_p, _p, _p, _p, _p, _i32, _p, _p, _i64, _p, _p]),
    "daisy_fm_rank_topk": (C.c_int, [_p, _p, _p, _p, _p, _i32, _p, _p, _i64, _i64, _i32, _p, _p, _p, _sz, _p]),
    "daisy_fm_full_rank": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _i64, _i32, _p, _p, _sz, _p]),
    "daisy_full_rank_users_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "daisy_full_rank_users": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _p, _i64, _p, _p, _i32, _i32, _p, _p, _p, _sz, _p]),
    "daisy_full_rank_positions_workspace_bytes": (_sz, [_i64, _i64]),
    "daisy_full_rank_positions": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _p, _i64, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _p,
                                             _sz, _p]),
    "daisy_neumf_ctx_create": (C.c_int, [C.POINTER(_p), _i64, _i32, _i32, _i32, _i64, _i64]),
    "daisy_neumf_ctx_destroy": (C.c_int, [_p]),
    "daisy_neumf_ctx_bytes": (_sz, [_p]),
    "daisy_neumf_ctx_set_precision": (C.c_int, [_p, _i32]),
    "daisy_neumf_scores": (C.c_int, [_p, _pp, _p, _p, _i64, _i64, _p, _p]),
    "daisy_neumf_scores_users": (C.c_int, [_p, _pp, _p, _i64, _p, _p]),
    "daisy_neumf_step_grads":(C.c_int, [_p, _pp, _pp, _p, _p, _p, _i64, _i32, _f32, _f32, _f32, _f32, _u64, _p, _p]),
    "daisy_neumf_fit_epoch": (C.c_int, [_p, _pp, _pp, _p, _p, _p, _i64, _i64, _i32, _f32, _f32, _f32, _f32, _u64, _i64,
                                        _i32, _f32, _p, _p, _p, _p, _i64, _p, _p]),
    "daisy_sgd_dense": (C.c_int, [_p, _p, _i64, _f32, _p]),
    "daisy_topk_from_scores": (C.c_int, [_p, _p, _i64, _i64, _i32, _p, _p, _sz, _p]),
    "daisy_full_topk_from_scores": (C.c_int, [_p, _i64, _i32, _p, _p, _sz, _p]),
    "daisy_gemm_nt_f32": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _p]),
    "daisy_gemm_nt_bf16": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _p]),
    "daisy_gemm_tn_bf16": (C.c_int, [_p, _p, _p, _i64, _i32, _i64, _i64, _p]),
    "daisy_gemm_nt": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "daisy_gemm_case": (C.c_int, [_gd, _gd, _p]),
    "daisy_lgcn_graph_create": (C.c_int, [C.POINTER(_p), _p, _p, _i64, _i64, _i64, _p]),
    "daisy_lgcn_graph_destroy": (C.c_int, [_p]),
    "daisy_lgcn_graph_nnz": (_i64, [_p]),
    "daisy_lgcn_graph_set_reproducible": (C.c_int, [_p, _i32]),
    "daisy_lgcn_graph_bytes": (_sz, [_p]),
    "daisy_lgcn_graph_read": (C.c_int, [_p, _p, _p, _p, _p]),
    "daisy_lgcn_spmm": (C.c_int, [_p, _p, _p, _i32, _p]),
    "daisy_lgcn_spmm_rows": (C.c_int, [_p, _p, _p, _i32, _i64, _i64, _p]),
    "daisy_lgcn_propagate": (C.c_int, [_p, _p, _i32, _i32, _p, _p, _p]),
    "daisy_lgcn_backprop": (C.c_int, [_p, _p, _i32, _i32, _p, _p, _p]),
    "daisy_lgcn_reg_grad": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _f32, _f32, _p, _p, _p, _p]),
    "daisy_axpby_f32": (C.c_int, [_p, _f32, _f32, _p, _i64, _i32, _p]),
    "daisy_csr_row_sum": (C.c_int, [_p, _p, _p, _i64, _i32, _p, _p]),
    "daisy_lgcn_spmm_ex": (C.c_int, [_p, _p, _i64, _p, _i64, _i32, _i32, _f32, _u64, _i32, _p]),
    "daisy_dropout_mask": (C.c_int, [_u64, C.c_uint32, _i64, _f32, _p, _p]),
    "daisy_nfm_ctx_create": (C.c_int, [C.POINTER(_p), _i64, _i32, _i32, _i32, _i32, _i64, _i64]),
    "daisy_nfm_ctx_destroy": (C.c_int, [_p]),
    "daisy_nfm_ctx_bytes": (_sz, [_p]),
    "daisy_nfm_ctx_set_path": (C.c_int, [_p, _i32]),
    "daisy_nfm_step_grads": (C.c_int, [_p, _np, _np, _nb, _p, _p, _p, _i64, _i32, _f32, _f32, _f32, _f32, _u64, _p, _p]),
    "daisy_nfm_fit_epoch": (C.c_int, [_p, _np, _np, _nb, _p, _p, _p, _i64, _i64, _i32, _f32, _f32, _f32, _f32, _u64,
                                      _i64, _i64, _i32, _f32, _p, _p, _p, _p, _i64, _p, _p]),
    "daisy_nfm_scores": (C.c_int, [_p, _np, _nb, _p, _p, _i64, _i64, _i32, _f32, _u64, _p, _p]),
    "daisy_nfm_scores_users": (C.c_int, [_p, _np, _nb, _p, _i64, _p, _p]),
    "daisy_vae_ctx_create":(C.c_int, [C.POINTER(_p), _i64, _i64, _i64, _i32, _p, _i32]),
    "daisy_vae_ctx_destroy": (C.c_int, [_p]),
    "daisy_vae_ctx_bytes": (_sz, [_p]),
    "daisy_vae_param_count": (_i64, [_p]),
    "daisy_vae_step_grads": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _p, _i32, _f32, _f32, _u64, _p,
                                       _p]),
    "daisy_vae_fit_epoch": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _f32, C.c_double, _i64, _i64, _u64,
                                      _i64, _i64, _i32, _f32, _p, _p, _p, _p]),
    "daisy_vae_scores": (C.c_int, [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _p, _i32, _f32, _u64, _p, _p]),
    "daisy_slim_gram_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "daisy_slim_gram_fits": (C.c_int, [_i64, _i64, _i64, _sz]),
    "daisy_slim_gram": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _sz, _p]),
    "daisy_slim_cd_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "daisy_slim_cd": (C.c_int, [_p, _i64, _i64, C.c_double, C.c_double, C.c_double, _i32, _i32, _i64, _i64, _p, _p, _p, _p,
                                _p, _p, _i32, _p, _sz, _p]),
    "daisy_slim_scores": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _p, _i64, _p, _i64, _p, _i32, _p]),
    "daisy_psvd_spmm": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _i32, _p, _p]),
    "daisy_psvd_gram_block_rows": (_i64, [_i64, _i64]),
    "daisy_psvd_gram_workspace_bytes": (_sz, [_i64, _i32, _i64]),
    "daisy_psvd_gram": (C.c_int, [_p, _i64, _i32, _p, _i64, _p, _sz, _p]),
    "daisy_psvd_chol": (C.c_int, [_p, _i32, _i64, _p, _p, _p, _p]),
    "daisy_psvd_gemm": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _p]),
    "daisy_psvd_jacobi_workspace_bytes": (_sz, [_i32]),
    "daisy_psvd_jacobi": (C.c_int, [_p, _i32, _i32, _p, _p, _p, _p, _p, _sz, _p]),
    "daisy_psvd_rank": (C.c_int, [_p, _p, _i64, _i64, _i32, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "daisy_ease_workspace_bytes": (_sz, [_i64]),
    "daisy_ease_fit_bytes": (_sz, [_i64]),
    "daisy_ease_fits": (C.c_int, [_i64, _sz]),
    "daisy_ease_system": (C.c_int, [_p, _i64, C.c_double, _p, _p]),
    "daisy_ease_potrf": (C.c_int, [_p, _i64, _p, _p, _sz, _p]),
    "daisy_ease_potri": (C.c_int, [_p, _i64, _p, _p, _p, _sz, _p]),
    "daisy_ease_weights": (C.c_int, [_p, _i64, _p, _p, _sz, _p]),
    "daisy_ease_rank": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "daisy_ials_gram_workspace_bytes": (_sz, [_i64, _i32]),
    "daisy_ials_gram": (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _sz, _p]),
    "daisy_ials_half_sweep": (C.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _i64, _i32, _p, C.c_double, C.c_double, _p, _i64,
                                        _p, _p, _p, _p]),
    "daisy_ials_objective_workspace_bytes": (_sz, [_i64]),
    "daisy_ials_objective": (C.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _i64, _i32, _p, C.c_double, C.c_double, _p,
                                       _p, _sz, _p]),
    "daisy_knn_row_means": (C.c_int, [_p, _p, _i64, _p, _p]),
    "daisy_knn_center": (C.c_int, [_p, _p, _p, _i64, _i64, _i32, _p, _p, _p]),
    "daisy_knn_diag": (C.c_int, [_p, _i64, _i32, _p, _p]),
    "daisy_knn_select": (C.c_int, [_p, _p, _i64, _i32, _f32, _f32, _i32, _p, _p, _p, _p]),
    "daisy_knn_rank": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _i32, _p, _p, _i32, _p]),
    "daisy_knn_fit_bytes": (_sz, [_i64, _i64, _i32]),
    "daisy_knn_fits": (C.c_int, [_i64, _i64, _i32, _sz]),
    "daisy_walk2_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "daisy_walk2_topk": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _i64, _p, _i32, _i32, _i32, _p, _p, _p, _i32, _i32, _p,
                                   _sz, _p]),
    "daisy_rank_f64_users_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "daisy_ease_full_rank_users": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _p, _i64, _p, _p, _i32, _p, _p, _p]),
    "daisy_slim_full_rank_users": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _p, _i64, _p, _p, _i32, _p, _p, _i32, _p]),
    "daisy_knn_full_rank_users": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _i64, _p, _i64, _p, _p, _i32, _p, _p, _i32,
                                            _p]),
    "daisy_psvd_full_rank_users": (C.c_int, [_p, _p, _i64, _i64, _i32, _p, _i64, _p, _p, _i32, _p, _p, _p]),
    "daisy_rank_rows_f32": (C.c_int, [_p, _i64, _i64, _i64, _p, _p, _p, _i32, _p, _p, _p]),
    # exact ranks of held-out items: the sibling's operands, then users, n, the exclusion CSR, the target CSR,
    # out_indptr, n_targets, out_pos, out_scores, out_eligible[, path], stream
    "daisy_ease_full_rank_positions": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p]),
    "daisy_slim_full_rank_positions": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _p,
                                                 _p, _i32, _p]),
    "daisy_knn_full_rank_positions": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _p, _p, _i64, _p,
                                                _p, _p, _i32, _p]),
    "daisy_psvd_full_rank_positions": (C.c_int, [_p, _p, _i64, _i64, _i32, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p]),
    "daisy_rank_rows_positions_f32": (C.c_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p]),
    "daisy_pop_fit":(C.c_int, [_p, _i32, _i64, _i64, _p, _p, _p]),
    "daisy_pop_rank": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p]),
    "daisy_ranking_kpis_workspace_bytes": (_sz, [_i64, _i32, _i64, C.c_uint32]),
    "daisy_ranking_kpis": (C.c_int, [_p, _i32, _i64, _i32, _p, _p, _i64, _p, C.POINTER(_i32), _i32, _p, _p, _i64, _p, _i32,
                                     _i32, _p, C.c_uint32, _p, _p, _p, _p, _sz, _p]),
    "daisy_position_kpis_workspace_bytes": (_sz, [_i64, _i32, C.c_uint32]),
    "daisy_position_kpis": (C.c_int, [_p, _p, _p, _p, _i64, C.POINTER(_i32), _i32, _p, _p, _i64, C.c_uint32, _p, _p, _p, _sz, _p]),
    "daisy_prep_encode": (C.c_int, [_p, _i64, _p, _p, C.POINTER(_i64), _p]),
    "daisy_prep_process": (C.c_int, [_p, _p, _p, _p, _i64, _i32, C.c_double, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p,
                                     C.POINTER(_i64), _p]),
    "daisy_split_ids": (C.c_int, [_i32, _p, _p, _i64, _i64, C.c_double, C.c_double, _u64, _u64, _p, _p, C.POINTER(_i64), _p]),
    "daisy_history_counts": (C.c_int, [_p, _i64, _i64, _p, _p, _p, C.POINTER(_i64), _p]),
    "daisy_history_fill": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "daisy_history_csr": (C.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _p, _p, C.POINTER(_i64), _p]),
    "daisy_history_first_seen": (C.c_int, [_p, _i64, _i64, _p, C.POINTER(_i64), _p]),
    "daisy_ngcf_ws_bytes": (_sz, [_i64, _i32, _i32]),
    "daisy_ngcf_layer_forward": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _i32, _i32, _f32, _u64,
                                           _i32, _p]),
    "daisy_ngcf_layer_backward": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p, _p, _p, _p, _i64, _p, _p, _p, _i64,
                                            _i32, _i32, _f32, _u64, _i32, _p]),
    "daisy_ngcf_wgrad_reduce": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _p, _p, _p]),
    "daisy_csr_workspace_bytes": (_sz, [_i64]),
    "daisy_build_user_csr": (C.c_int, [_p, _p, _i64, _i64, _p, _p, _p, _sz, _p]),
    "daisy_sample_neg_per_user": (C.c_int, [_p, _p, _i64, _i64, _i32, _u64, _u64, _p, _p]),
    "daisy_skipgram_samples": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p, _p, _i64, _u64, _u64, _p, _p, _p]),
    "daisy_sample_categorical": (C.c_int, [_p, _i64, _i64, _i32, _u64, _u64, _p, _i32, _i32, _p]),
    "daisy_expand_triples": (C.c_int, [_p, _p, _i64, _p, _i32, _p, _p]),
    "daisy_resample_neg_per_interaction": (C.c_int, [_p, _p, _i64, _p, _i64, _u64, _u64, _p]),
    "daisy_build_candidates": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _i32, _u64, _p, _p]),
    "daisy_randperm_workspace_bytes": (_sz, [_i64]),
    "daisy_randperm": (C.c_int, [_i64, _u64, _u64, _p, _p, _sz, _p]),
    "daisy_membench": (C.c_int, [_i32, _p, _i64, _i32, _p, _i64, _p, _p]),
}


class DaisyHipError(RuntimeError):
    """A HIP runtime call inside the native library failed."""


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is the product path and has no "
            "fallback.  Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C daisyrec_amd/csrc` (needs hipcc, targets gfx950).")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.daisy_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {got}, binding expects {ABI_VERSION}; rebuild")
    return lib


lib = _load()


def last_error() -> str:
    msg = lib.daisy_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int) -> None:
    """Map the C status code to the Python exception the reference path would raise."""
    if rc == DAISY_OK:
        return
    msg = last_error()
    if rc == DAISY_ERR_ARG:
        if msg.startswith("Invalid loss type"):
            raise NotImplementedError(msg)          # MFRecommender.py:90-91
        raise ValueError(msg)
    if rc == DAISY_ERR_HIP:
        raise DaisyHipError(msg)
    raise RuntimeError(msg)
