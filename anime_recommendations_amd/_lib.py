"""ctypes binding of libanirec.so (include/anirec.h).

The product path has NO fallback: if the HIP library is missing or a call fails,
this module raises.  Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ANIREC_LIB_PATH") or os.path.join(_PKG, "libanirec.so")   # override: A/B of two builds on one box

DIM = 128
WIDTHS = (32, 64, 128, 256)   # row widths the *_w entry points implement (a row is width / 4 lanes of float4)
MAX_BATCH = 16384
CHUNK = 32
ADAM_BLOCKS = 8192
MAX_TOPK = 128
MAX_SEG = 16
ABI_VERSION = 5
TOPK_MAX_BATCHES = 64
RCCL_ID_BYTES = 128
LAZY_WINDOW = 8
MMR_IMAGE_FLOATS = 32768    # anirec_mmr_max_cand(dim) = MMR_IMAGE_FLOATS // dim: the candidates' rows of a list in LDS
EXPLAIN_MAX_M = 8           # ANIREC_EXPLAIN_MAX_M: the most history entries anirec_explain_lists picks per listed anime
EXPLAIN_MAX_K = 128         # anirec_explain_max_k(dim) = min(EXPLAIN_MAX_K, EXPLAIN_IMAGE_FLOATS // dim)
EXPLAIN_IMAGE_FLOATS = 16384
EXPLAIN_TILE_FLOATS = 8192  # anirec_explain_tile(dim, k): dim * tile and k * (tile | 1) floats both within this
KMEANS_MAX_K = 4096         # ANIREC_KMEANS_MAX_K: the most centroids anirec_kmeans_assign / anirec_kmeans_fit take
KMEANS_MAX_ITER = 1000      # anirec_kmeans_fit: the most iterations one call enqueues
KMEANS_IMAGE_FLOATS = 32768  # anirec_kmeans_tile(dim) = KMEANS_IMAGE_FLOATS // dim: the centroids of one LDS image
TSNE_MAX_ROWS = 1 << 20     # ANIREC_TSNE_MAX_ROWS: the most rows anirec_tsne_forces / anirec_tsne_fit take
TSNE_MAX_ITER = 4096        # ANIREC_TSNE_MAX_ITER: the most iterations one anirec_tsne_fit enqueues
TSNE_TILE = 1024            # anirec_tsne_tile(): the j points of one LDS tile of the all-pairs kernel
TSNE_MAX_SPLITS = 1024      # the largest j_splits
ALS_MAX_CG = 16             # ANIREC_ALS_MAX_CG: the most conjugate-gradient steps of anirec_als_half_sweep
ALS_GRAM_CHUNK = 1024       # ANIREC_ALS_GRAM_CHUNK: rows of one chunk of anirec_als_gram
BPR_MAX_TRIES = 16          # ANIREC_BPR_MAX_TRIES: the most negative candidates of a slot of anirec_bpr_steps
BPR_ERR_INDEX, BPR_ERR_DIVERGED = 1, 2   # ANIREC_BPR_ERR_*: the bits of anirec_bpr_steps' error flag
CALIBRATE_MAX_CAND = 1024   # anirec_calibrate_max_cand(): the longest list anirec_calibrate_rerank / _list_calibration take
CALIBRATE_MAX_CAT = 128     # the most categories of a profile (anirec_fave_profile's limit)
CALIBRATE_PROFILE_MAX = 1 << 24   # the largest profile entry: the integer numerator then stays below 2**53
# anirec_train_desc.optimizer (ANIREC_OPT_*)
OPT_ADAM, OPT_SGD, OPT_RMSPROP, OPT_ADAGRAD = 0, 1, 2, 3
# anirec_train_desc.loss (ANIREC_LOSS_*) and .activation / the predict calls' activation (ANIREC_ACT_*)
LOSS_BCE, LOSS_MSE, LOSS_MAE, LOSS_HUBER, LOSS_LOGCOSH = 0, 1, 2, 3, 4
ACT_SIGMOID, ACT_LINEAR, ACT_TANH, ACT_RELU, ACT_SOFTPLUS = 0, 1, 2, 3, 4
# Keras metrics accumulated on the GPU (ANIREC_METRIC_*): the bit of each kind; anirec_metric_acc.sum holds bits 0..5
METRIC_MAE, METRIC_MAPE, METRIC_MSLE, METRIC_LOGCOSH, METRIC_BCE, METRIC_ACC, METRIC_AUC = 1, 2, 4, 8, 16, 32, 64
METRIC_KINDS = 6
AUC_BINS = 200
AUC_ONE = 1 << 20
# anirec_group_topk: the aggregate over a group's members (ANIREC_GROUP_*) and the most members of one group
GROUP_MEAN, GROUP_MIN, GROUP_MAX = 0, 1, 2
GROUP_MODES = {"mean": GROUP_MEAN, "least_misery": GROUP_MIN, "min": GROUP_MIN, "most_pleasure": GROUP_MAX,
               "max": GROUP_MAX}
GROUP_MAX_MEMBERS = 64
# anirec_cooc_scores: the similarity of two items' liked-by sets (ANIREC_COOC_*)
COOC_COSINE, COOC_JACCARD, COOC_CONFIDENCE = 0, 1, 2
COOC_MEASURES = {"cosine": COOC_COSINE, "jaccard": COOC_JACCARD, "confidence": COOC_CONFIDENCE}
WCOOC_MAX_Q = 16383         # ANIREC_WCOOC_MAX_Q: the largest user weight of anirec_wcooc_scores (two 7-bit limbs)
WCOOC_MAX_USERS = 1 << 24   # and the most users: 127 * 2^24 < 2^31 keeps a limb's int32 accumulator exact
COVER_MAX_PICKS = 1024      # ANIREC_COVER_MAX_PICKS: the longest list anirec_cover_greedy picks
# anirec_fuse_rows: the fusion of several systems' score rows (ANIREC_FUSE_*)
FUSE_RRF, FUSE_MINMAX = 0, 1
FUSE_METHODS = {"rrf": FUSE_RRF, "minmax": FUSE_MINMAX}
FUSE_MAX_SYS = 8            # ANIREC_FUSE_MAX_SYS: the most systems of one call
FUSE_MAX_ITEMS = 20480      # anirec_fuse_max_items(): one row's sort image (8 B an item) in the LDS of a workgroup
FUSE_MAX_RRF_C = 1 << 20    # the largest rrf_c: c + 1 + rank stays below 2^24, exact in fp32
FUSE_MAX_GRID = 4095        # ANIREC_FUSE_MAX_GRID: the most weight vectors of anirec_fuse_rank_grid (BOOT_MAX_COL - 1)


class AnirecError(RuntimeError):
    pass


class Step(C.Structure):
    _fields_ = [("start", C.c_int32), ("count", C.c_int32), ("alpha", C.c_float),
                ("global_count", C.c_int32)]


# numpy mirror of anirec_step / anirec_state (device buffers are viewed through these)
STEP_DTYPE = np.dtype([("start", "<i4"), ("count", "<i4"), ("alpha", "<f4"), ("global_count", "<i4")])
STATE_DTYPE = np.dtype([
    ("w", "<f4"), ("b", "<f4"), ("gamma", "<f4"), ("beta", "<f4"),
    ("adam_m", "<f4", (4,)), ("adam_v", "<f4", (4,)),
    ("mov_mean", "<f4"), ("mov_var", "<f4"), ("reg_sumsq", "<f4"),
    ("bn_mu", "<f4"), ("bn_var", "<f4"), ("last_loss", "<f4"), ("last_mse", "<f4"),
    ("step_fwd", "<i4"), ("step_bwd", "<i4"), ("pad0", "<i4"),
    ("loss_wsum", "<f8"), ("se_sum", "<f8"), ("n_seen", "<f8"),
    ("val_bce_sum", "<f8"), ("val_se_sum", "<f8"), ("val_n", "<f8"),
    ("bce_wsum", "<f8"), ("reg_user_wsum", "<f8"), ("reg_anime_wsum", "<f8"),
    ("reg_user_sumsq", "<f4"), ("reg_anime_sumsq", "<f4"),
], align=True)
# anirec_metric_acc
METRIC_ACC_DTYPE = np.dtype([("sum", "<f8", (METRIC_KINDS,)), ("auc_pos", "<u8", (AUC_BINS,)),
                             ("auc_neg", "<u8", (AUC_BINS,))])
assert STEP_DTYPE.itemsize == 16
assert METRIC_ACC_DTYPE.itemsize == 8 * (METRIC_KINDS + 2 * AUC_BINS)
assert STATE_DTYPE.itemsize == 168, STATE_DTYPE.itemsize


class TrainDesc(C.Structure):
    _fields_ = [
        ("n_user_rows", C.c_int32), ("n_anime_rows", C.c_int32), ("max_batch", C.c_int32),
        ("arena_steps", C.c_int32), ("dense_mode", C.c_int32), ("n_seg", C.c_int32),
        ("my_seg", C.c_int32), ("dense_rows", C.c_int32), ("l2", C.c_float), ("adam_row_lo", C.c_int32),
        ("adam_row_hi", C.c_int32), ("lazy", C.c_int32),
        ("W", C.c_void_p), ("M", C.c_void_p), ("V", C.c_void_p), ("rowmap", C.c_void_p),
        ("state", C.c_void_p), ("user_idx", C.c_void_p), ("anime_idx", C.c_void_p),
        ("rating", C.c_void_p), ("sched", C.c_void_p), ("n_steps", C.c_int32), ("loss", C.c_int32),
        ("packets", C.c_void_p), ("dense_grad", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t), ("lazy_state", C.c_void_p), ("optimizer", C.c_int32),
        ("activation", C.c_int32),
    ]


class Head(C.Structure):
    _fields_ = [("w", C.c_float), ("b", C.c_float), ("gamma", C.c_float), ("beta", C.c_float),
                ("mov_mean", C.c_float), ("mov_var", C.c_float)]


class IngestOpts(C.Structure):
    _fields_ = [("num_reviews", C.c_int32), ("drop_unwatched", C.c_int32), ("drop_plan", C.c_int32),
                ("drop_half_watched", C.c_int32), ("user_id_bound", C.c_int32), ("anime_id_bound", C.c_int32)]


_vp, _i32, _sz, _f32, _i64 = C.c_void_p, C.c_int32, C.c_size_t, C.c_float, C.c_int64
_DP = C.POINTER(TrainDesc)

# name -> (restype, argtypes); must list every function include/anirec.h declares
PROTOTYPES = {
    "anirec_abi_version": (C.c_int, []),
    "anirec_status_string": (C.c_char_p, [C.c_int]),
    "anirec_device_name": (C.c_int, [C.c_char_p, _sz]),
    "anirec_packet_floats": (_sz, [_i32]),
    "anirec_train_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_train_lazy_bytes": (_sz, [_i32]),
    "anirec_train_init_reg": (C.c_int, [_DP, _vp]),
    "anirec_train_prep": (C.c_int, [_DP, _i32, _i32, _vp]),
    "anirec_train_fwd": (C.c_int, [_DP, _vp]),
    "anirec_train_head": (C.c_int, [_DP, _vp]),
    "anirec_train_bwd": (C.c_int, [_DP, _vp]),
    "anirec_train_adam": (C.c_int, [_DP, _vp]),
    "anirec_train_adam_part": (C.c_int, [_DP, _i32, _vp]),
    "anirec_train_stage_ticks": (C.c_int, [_DP, _i32, C.POINTER(C.c_float), C.POINTER(C.c_int32), _vp]),
    "anirec_dist_stepper_create": (C.c_int, [_DP, C.POINTER(_vp)]),
    "anirec_dist_stepper_destroy": (C.c_int, [_vp]),
    "anirec_dist_step_front": (C.c_int, [_vp, _vp]),
    "anirec_dist_step_mid": (C.c_int, [_vp, _vp]),
    "anirec_dist_step_back": (C.c_int, [_vp, _vp]),
    "anirec_dist_stepper_begin": (C.c_int, [_vp, _i32, _i32, _vp]),
    "anirec_dist_stepper_block": (C.c_int, [_vp, _i32]),
    "anirec_rccl_load": (C.c_int, [C.c_char_p]),
    "anirec_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "anirec_dist_comm_create": (C.c_int, [C.c_char_p, _i32, _i32, C.POINTER(_vp)]),
    "anirec_dist_comm_destroy": (C.c_int, [_vp]),
    "anirec_dist_run": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "anirec_trainer_create": (C.c_int, [_DP, C.POINTER(_vp)]),
    "anirec_trainer_destroy": (C.c_int, [_vp]),
    "anirec_trainer_run": (C.c_int, [_vp, _i32, _i32, _i32, _vp]),
    "anirec_eval": (C.c_int, [_DP, _vp, _vp, _vp, _i32, _vp]),
    "anirec_trainer_set_metrics": (C.c_int, [_vp, C.c_uint32, _vp]),
    "anirec_dist_stepper_set_metrics": (C.c_int, [_vp, C.c_uint32, _vp]),
    "anirec_eval_metrics": (C.c_int, [_DP, C.c_uint32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "anirec_adam_flat": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _vp]),
    "anirec_opt_flat": (C.c_int, [_i32, _vp, _vp, _vp, _sz, _f32, _vp]),
    "anirec_selftest_lazy_math": (C.c_int, [C.c_uint64, _vp, _vp]),
    "anirec_selftest_lazy_div": (C.c_int, [_i32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "anirec_selftest_lazy_replay": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _f32, _i32, _vp, _vp, _vp, _vp]),
    "anirec_gather_ratings": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "anirec_rownorm": (C.c_int, [_vp, _i32, _vp, _vp]),
    "anirec_cosine_scores": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "anirec_topk_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_cosine_topk": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "anirec_topk_large_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_cosine_topk_large": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "anirec_cosine_topk_job_plan": (C.c_int, [_i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32)]),
    "anirec_cosine_topk_job_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_cosine_topk_allpairs_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_cosine_topk_allpairs_plan": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32)]),
    "anirec_cosine_topk_job": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, C.c_float, C.POINTER(C.c_int32), _i32,
                                         _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "anirec_topk_mfma_timing": (C.c_int, [_i32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "anirec_predict_pairs": (C.c_int, [_vp, _vp, _vp, _vp, _i32, C.POINTER(Head), _vp, _vp]),
    "anirec_predict_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_predict_grid": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _vp, _vp, _sz, _vp]),
    "anirec_predict_mfma_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_predict_grid_mfma": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _vp, _vp, _sz, _vp]),
    "anirec_predict_topk": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _vp, _i32, _vp,
                                      _vp, _vp, _sz, _vp]),
    "anirec_predict_pairs_act": (C.c_int, [_vp, _vp, _vp, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp]),
    "anirec_predict_grid_act": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp, _sz, _vp]),
    "anirec_predict_grid_mfma_act": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp, _sz, _vp]),
    "anirec_predict_topk_act": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _i32, _vp,
                                          _vp, _vp, _sz, _vp]),
    "anirec_predict_topk_large_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_predict_topk_large_act": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _i32, _vp,
                                                _vp, _vp, _sz, _vp]),
    "anirec_predict_topk_mfma_act": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _i32, _vp,
                                               _vp, _vp, _vp, _sz, _vp]),
    "anirec_predict_topk_mfma_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_predict_topk_mfma": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.POINTER(Head), _vp, _i32, _vp,
                                           _vp, _vp, _vp, _sz, _vp]),
    "anirec_fav_workspace_bytes": (_sz, [_i64, _i32]),
    "anirec_user_favourites": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp, _sz, _vp]),
    "anirec_user_recs": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "anirec_user_recs_ex": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "anirec_fave_profile": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "anirec_ingest_id_max": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "anirec_ingest_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "anirec_ingest_preprocess": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(IngestOpts), _vp, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "anirec_ingest_half_columns": (C.c_int, [_vp, _vp, _i64, C.POINTER(IngestOpts), _vp, _vp, _vp, _sz, _vp]),
    "anirec_ingest_encode_workspace_bytes": (_sz, [_i64, _i32]),
    "anirec_ingest_encode": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # the twins that take the row width (`int32_t dim`; NAME(...) == NAME_w(..., 128))
    "anirec_train_workspace_bytes_w": (_sz, [_i32, _i32, _i32]),
    "anirec_train_init_reg_w": (C.c_int, [_DP, _i32, _vp]),
    "anirec_train_prep_w": (C.c_int, [_DP, _i32, _i32, _i32, _vp]),
    "anirec_train_fwd_w": (C.c_int, [_DP, _i32, _vp]),
    "anirec_train_head_w": (C.c_int, [_DP, _i32, _vp]),
    "anirec_train_bwd_w": (C.c_int, [_DP, _i32, _vp]),
    "anirec_train_adam_w": (C.c_int, [_DP, _i32, _vp]),
    "anirec_trainer_create_w": (C.c_int, [_DP, _i32, C.POINTER(_vp)]),
    "anirec_eval_metrics_w": (C.c_int, [_DP, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "anirec_rownorm_w": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "anirec_cosine_scores_w": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "anirec_cosine_topk_w": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "anirec_cosine_topk_large_w": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "anirec_predict_pairs_w": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp]),
    "anirec_predict_workspace_bytes_w": (_sz, [_i32, _i32, _i32, _i32]),
    "anirec_predict_grid_w": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp, _sz, _vp]),
    "anirec_predict_topk_w": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _i32, _vp,
                                        _vp, _vp, _sz, _vp]),
    "anirec_predict_topk_large_workspace_bytes_w": (_sz, [_i32, _i32, _i32, _i32]),
    "anirec_predict_topk_large_w": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _i32, _vp,
                                              _vp, _vp, _sz, _vp]),
    # ranks of held-out anime (one entry point, `int32_t dim` among its arguments) and the watched bits of a rating list
    "anirec_predict_rank_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "anirec_predict_rank": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp, _vp, _i32, _vp,
                                      _vp, _vp, _vp, _sz, _vp]),
    "anirec_seen_bits": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    # the same ranks under one score vector shared by all users (the popularity baseline)
    "anirec_score_rank": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    # rows of new users fitted to their own ratings, the rest of the model frozen
    "anirec_fold_in_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_fold_in": (C.c_int, [_vp, _i32, _i32, C.POINTER(Head), _i32, _i32, _f32, _vp, _vp, _vp, _i32, _vp, _vp, _i32,
                                 _vp, _vp, _vp, _vp, _sz, _vp]),
    # the same fit for a few rows with long lists (new anime against the user table): lists split across workgroups
    "anirec_fold_in_split_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "anirec_fold_in_split": (C.c_int, [_vp, _i32, _i32, C.POINTER(Head), _i32, _i32, _f32, _vp, _vp, _vp, _i32, _vp, _vp,
                                       _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    # greedy MMR re-rank of candidate lists (diversified recommendations)
    "anirec_mmr_max_cand": (_sz, [_i32]),
    "anirec_mmr_rerank": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    # pairwise similarity structure of many lists (list evaluation)
    "anirec_list_similarity": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    # one list per group of users: the aggregate of the members' ratings through the exact select
    "anirec_group_topk_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "anirec_group_topk": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, C.POINTER(Head), _i32, _vp, _vp, _vp, _i32, _i32,
                                    _i32, _vp, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # the top contributing history entries of every listed anime (explained recommendations)
    "anirec_explain_max_k": (_sz, [_i32]),
    "anirec_explain_tile": (_sz, [_i32, _i32]),
    "anirec_explain_lists": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    # spherical k-means on an embedding table (clustered tables)
    "anirec_kmeans_tile": (_sz, [_i32]),
    "anirec_kmeans_assign": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "anirec_kmeans_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_kmeans_fit": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # exact t-SNE on a neighbour graph (mapped tables)
    "anirec_tsne_tile": (_sz, []),
    "anirec_tsne_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_tsne_forces": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "anirec_tsne_fit": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i64, _i32, _i32, C.c_double, C.c_double, _i32, _vp, _vp,
                                  _vp, _vp, _sz, _vp]),
    # item-kNN from co-occurrence: popcount similarity rows, the select / the rank over rows a caller holds, history scores
    "anirec_cooc_chunk_words": (_sz, []),
    "anirec_cooc_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_cooc_scores": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                     _vp]),
    "anirec_rows_topk_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_rows_topk": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "anirec_rows_rank": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "anirec_itemknn_lds_items": (_sz, []),
    "anirec_itemknn_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_itemknn_scores": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "anirec_content_lds_tokens": (_sz, []),
    "anirec_content_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_content_scores": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    # onboarding lists: greedy maximum coverage over the rated-by bit rows, and the levels of any list
    "anirec_cover_step_words": (_sz, []),
    "anirec_cover_lds_words": (_sz, []),
    "anirec_cover_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_cover_greedy": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "anirec_cover_levels": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    # greedy calibrated re-rank of candidate lists towards a favourite profile, and the miscalibration of lists held
    "anirec_calibrate_max_cand": (_sz, []),
    "anirec_calibrate_rerank": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                                          _vp]),
    "anirec_list_calibration": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    # ranks to per-unit metric sums, and the Poisson bootstrap of those sums over units (thr: a host table)
    "anirec_boot_tile": (_sz, []),
    "anirec_boot_col_tile": (_sz, [_i32]),
    "anirec_boot_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_rank_gain_rows": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "anirec_boot_sums": (C.c_int, [_vp, _vp, _i32, _i32, C.c_uint32, _i32, C.POINTER(C.c_uint32), _i32, _vp, _vp, _vp,
                                   _sz, _vp]),
    "anirec_boot_weights": (C.c_int, [_vp, _i32, C.c_uint32, _i32, C.POINTER(C.c_uint32), _i32, _vp, _vp]),
    # implicit-feedback ALS: the Gram matrix of a table, one conjugate-gradient half-sweep, score rows from two tables
    "anirec_als_gram_workspace_bytes": (_sz, [_i32, _i32]),
    "anirec_als_gram": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "anirec_als_half_sweep": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _f32, _i32, _vp, _vp,
                                        _vp]),
    "anirec_dot_scores": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _i64, _vp]),
    # BPR matrix factorisation: SGD steps over hashed triples with integer gradient sums, and the sampler on its own
    "anirec_bpr_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "anirec_bpr_sample": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i64, _i32, _i32, C.c_uint32, _i32, _i32, _vp, _vp, _vp]),
    "anirec_bpr_steps": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i32, _i32, C.c_uint32, _i32, _i32,
                                   _f32, _f32, _i32, _vp, _vp, _vp, _sz, _vp]),
    # EASE: the fp64 inverse of a symmetric positive definite matrix, the weights from it, score rows from histories
    "anirec_spd_inverse_block": (_i32, []),
    "anirec_spd_inverse_workspace_bytes": (_sz, [_i32]),
    "anirec_spd_inverse": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _sz, _vp]),
    "anirec_ease_weights": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _vp]),
    "anirec_ease_scores_col_tile": (_i32, []),
    "anirec_ease_scores_entry_tile": (_i32, []),
    "anirec_ease_scores": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp]),
    # user-weighted co-occurrence on the i8 matrix cores (the graph baselines)
    "anirec_wcooc_chunk_words": (_sz, []),
    "anirec_wcooc_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "anirec_wcooc_scores": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # hybrid lists: several systems' score rows fused into one (the pointers, pitches and weights: host arrays)
    "anirec_fuse_max_items": (_sz, []),
    "anirec_fuse_rows": (C.c_int, [C.POINTER(_vp), C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp, C.POINTER(_f32), _i32,
                                   _i32, _vp, _i64, _vp]),
    # the rank of every target under every weight vector of a grid (the weights: a device array)
    "anirec_fuse_rank_grid_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "anirec_fuse_rank_grid": (C.c_int, [C.POINTER(_vp), C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32,
                                        _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
}


def check_width(width) -> int:
    """The row width as an int, or a ValueError that lists the supported ones (Keras takes any positive int; the
    kernels map a row to a power-of-two group of lanes)."""
    try:
        w = int(width)
    except (TypeError, ValueError):
        w = None
    if w is None or w != width or w not in WIDTHS:
        raise ValueError("embedding_size %r is not supported: the libanirec kernels take the widths %s"
                         % (width, ", ".join(str(x) for x in WIDTHS)))
    return w


def mmr_max_cand(width) -> int:
    """anirec_mmr_max_cand: the longest candidate list anirec_mmr_rerank takes at a (checked) row width."""
    return MMR_IMAGE_FLOATS // check_width(width)


def explain_max_k(width) -> int:
    """anirec_explain_max_k: the longest list anirec_explain_lists takes at a (checked) row width."""
    return min(EXPLAIN_MAX_K, EXPLAIN_IMAGE_FLOATS // check_width(width))


def explain_tile(width, k) -> int:
    """anirec_explain_tile: the history entries anirec_explain_lists stages per pass for lists of ``k`` slots."""
    w, k = check_width(width), int(k)
    if not 1 <= k <= explain_max_k(w):
        raise ValueError("explain_tile: k = %d must be in 1 .. %d at width %d" % (k, explain_max_k(w), w))
    return min(EXPLAIN_TILE_FLOATS // w, (EXPLAIN_TILE_FLOATS // k - 1) & ~7)


def fuse_max_items() -> int:
    """anirec_fuse_max_items: the longest row anirec_fuse_rows takes."""
    return FUSE_MAX_ITEMS


def kmeans_tile(width) -> int:
    """anirec_kmeans_tile: the centroids anirec_kmeans_assign holds in LDS at once at a (checked) row width."""
    return KMEANS_IMAGE_FLOATS // check_width(width)


_lib = None


def load() -> C.CDLL:
    """Load libanirec.so (built in-tree by anime_recommendations_amd.build).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AnirecError(
            "libanirec.so not found at %s — run `python -m anime_recommendations_amd.build` "
            "(needs hipcc); there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    v = lib.anirec_abi_version()
    if v != ABI_VERSION:
        raise AnirecError("libanirec ABI %d != binding ABI %d" % (v, ABI_VERSION))
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().anirec_status_string(status).decode()
        raise AnirecError("%s failed: %s (status %d)" % (what or "libanirec call", msg, status))


def ptr(t) -> int:
    """Device pointer of a torch tensor (must be contiguous); None -> NULL."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise AnirecError("non-contiguous tensor passed to libanirec")
    return t.data_ptr()


def call(name, *args) -> None:
    """``name(*args)`` of the loaded library, its status checked under that name.  An argument with a ``data_ptr`` (a
    tensor) goes through ``ptr``; None is NULL; ints, floats, ctypes arrays, ``byref``s and ``c_void_p`` handles pass as
    they are.  Size queries return sizes, not statuses: they are called on ``load()`` directly."""
    fn = getattr(load(), name)
    check(fn(*[ptr(a) if hasattr(a, "data_ptr") else a for a in args]), name)
