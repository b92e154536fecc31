"""ctypes binding of liburso_hip.so (C ABI declared in include/ursonet_hip.h).

The library is the only compute path of this package: if it is missing or fails to
load, importing this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import build as _build                              # the libraries' paths (it imports os, subprocess and sys only)

LIB_PATH = _build.LIB                                      # the variant under URSO_LIB_VARIANT (kernel experiments: see ursonet_amd/build.py)

F32, BF16, F16 = 0, 1, 2
EPI_RELU, EPI_OUT_F32, EPI_MASK_BITS, EPI_EMIT_BITS, EPI_ADD_SRCGRID = 1, 2, 4, 8, 16
K_IGEMM, K_WGRAD, K_PREP, K_FINALIZE, K_POOL, K_LOSS, K_OPTIM, K_DECODE, K_MOLD = range(1, 10)
KERNEL_NAMES = {K_IGEMM: "conv_igemm", K_WGRAD: "conv_wgrad", K_PREP: "weight_prep", K_FINALIZE: "param_grad_finalize",
                K_POOL: "maxpool", K_LOSS: "loss", K_OPTIM: "optimizer", K_DECODE: "quat_decode", K_MOLD: "mold"}

TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DT_OF_TORCH = {v: k for k, v in TORCH_DT.items()}
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


class ConvGeom(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("B", "H", "W", "C", "OH", "OW", "N", "KH", "KW", "SH", "SW", "PH", "PW", "DH", "DW",
                 "FH", "FW", "OSH", "OSW")]

    def __repr__(self):
        return "ConvGeom(" + ", ".join("%s=%d" % (n, getattr(self, n)) for n, _ in self._fields_) + ")"


class ProfRecord(C.Structure):
    _fields_ = [("kernel_id", C.c_int32), ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double)]


import threading
# Held while a hipGraph is being captured (Engine.capture, DataParallelEngine.capture) AND by any other thread around its own HIP work
# (ursonet_amd/feeder.py producers: pinned allocations, augmentation kernels, device-to-host copies): HIP refuses such calls from any
# thread while a global-mode capture is in progress and may invalidate the capture.
capture_lock = threading.RLock()


class ProfRecordEx(C.Structure):
    _fields_ = [("kernel_id", C.c_int32), ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double), ("n_launches", C.c_int32),
                ("symbol", C.c_char * 228), ("l2_bytes", C.c_double)]


class UrsoHipError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError("liburso_hip.so not found at %s -- build it with `python -m ursonet_amd.build` "
                      "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
_lib = C.CDLL(LIB_PATH)

_vp, _fp, _i, _f, _sz = C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_size_t
_gp = C.POINTER(ConvGeom)


class ParamDesc(C.Structure):
    """urso_param_desc (include/ursonet_hip.h): one weight layer's parameter-side tensors for the batched phases."""
    _fields_ = ([(n, C.c_int32) for n in ("KH", "KW", "C", "N", "npad", "K", "splits", "ks", "kb", "trainable", "bn_trainable", "bias_from")] +
                [(n, C.c_float) for n in ("eps", "regc", "regb")] +
                [(n, C.c_void_p) for n in ("w", "b", "gamma", "beta", "mean", "var", "wf", "wd", "biasf", "scale", "part", "colpart",
                                           "dw_raw", "colsum", "dotpart", "gw", "gb", "ggamma", "gbeta")])


class DenseLayer(C.Structure):
    """urso_dense_layer (include/ursonet_hip.h): one Dense layer of a urso_dense_multi launch."""
    _fields_ = ([(n, C.c_void_p) for n in ("src0", "wgt0", "src1", "wgt1", "bias", "add", "mask", "dst")] +
                [(n, C.c_int32) for n in ("M", "N", "K0", "K1", "flags")])


class PoseEvalArgs(C.Structure):
    """urso_pose_eval_args (include/ursonet_hip.h): one batch of urso_pose_eval."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] +
                [(n, C.c_int32) for n in ("loc_mode", "ori_mode", "loc_ld", "ori_ld", "loc_bins", "loc_map_rows", "ori_bins", "ori_map_rows",
                                          "gmm_modes", "pad0")] +
                [(n, C.c_void_p) for n in ("loc", "ori", "ori2", "loc_map", "ori_map", "enc_loc", "enc_ori", "loc_gt", "q_gt", "gmm_mean",
                                           "gmm_nmodes", "table")])


# urso_pose_eval modes and table columns (include/ursonet_hip.h)
EVAL_LOC_REGRESS, EVAL_LOC_CLASS = 0, 1
EVAL_ORI_QUAT, EVAL_ORI_EULER, EVAL_ORI_ANGLE_AXIS, EVAL_ORI_SOFT, EVAL_ORI_KEYPOINTS = range(5)
EVAL_LOC_EST, EVAL_Q_EST, EVAL_LOC_ERR, EVAL_ORI_ERR, EVAL_ESA, EVAL_DIST = 0, 3, 7, 8, 9, 10
EVAL_LOC_ENC_ERR, EVAL_ORI_ENC_ERR, EVAL_ORI_ERR_SOFT, EVAL_MODE, EVAL_COLS = 11, 12, 13, 14, 16


class PoseDecodeArgs(C.Structure):
    """urso_pose_decode_args (include/ursonet_hip.h): one batch of urso_pose_decode."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] +
                [(n, C.c_int32) for n in ("loc_mode", "ori_mode", "loc_ld", "ori_ld", "loc_bins", "loc_map_rows", "ori_bins", "ori_map_rows",
                                          "ori_logits_ld", "pad0")] +
                [(n, C.c_void_p) for n in ("loc", "ori", "ori2", "loc_map", "ori_logits", "ori_scatter", "table")])


# urso_pose_decode table columns (include/ursonet_hip.h); the modes are urso_pose_eval's
DEC_LOC_EST, DEC_Q_EST, DEC_LOC_PEAK, DEC_ORI_PEAK, DEC_ORI_LAMBDA, DEC_COLS = 0, 3, 7, 8, 9, 12


class PoseFuseViewsArgs(C.Structure):
    """urso_pose_fuse_views_args (include/ursonet_ext.h): one batch of urso_pose_fuse_views."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64), ("V", C.c_int32), ("est_ld", C.c_int32), ("est_view_rows", C.c_int64)] +
                [(n, C.c_void_p) for n in ("est", "r", "qr", "loc_gt", "q_gt", "table")])


# urso_pose_fuse_views table columns (include/ursonet_ext.h); columns 0..10 are urso_pose_eval's
FUSE_LOC_EST, FUSE_Q_EST, FUSE_LOC_ERR, FUSE_ORI_ERR, FUSE_ESA, FUSE_DIST = 0, 3, 7, 8, 9, 10
FUSE_LOC_SPREAD, FUSE_ORI_SPREAD, FUSE_VIEW_LAMBDA, FUSE_N_VIEWS, FUSE_COLS, FUSE_MAX_VIEWS = 11, 12, 13, 14, 16, 64
EMA_DECAY, EMA_WARMUP, EMA_UPDATES, EMA_NEXT_DECAY, EMA_FIELDS = 0, 1, 2, 3, 8       # URSO_EMA_* of include/ursonet_ext.h


class EnsAddArgs(C.Structure):
    """urso_ens_add_args (include/ursonet_train.h): one member's logits of one batch."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] + [(n, C.c_int32) for n in ("K", "ld", "first", "pad")] +
                [(n, C.c_void_p) for n in ("logits", "acc", "stat")])


class EnsSettleArgs(C.Structure):
    """urso_ens_settle_args (include/ursonet_train.h): the accumulated rows of one chunk."""
    _fields_ = ([("n", C.c_int32), ("row0", C.c_int64), ("K", C.c_int32), ("M", C.c_int32)] +
                [(n, C.c_void_p) for n in ("acc", "stat", "logp", "table")])


# urso_ens_* sizes and table columns (include/ursonet_train.h)
ENS_MAX_MEMBERS, ENS_STAT, ENS_COLS = 64, 4, 8
ENS_H_MEAN, ENS_H_MEMBERS, ENS_MI, ENS_PEAK, ENS_ARGMAX, ENS_N_MEMBERS = range(6)
# urso_temp_* sizes and table columns (include/ursonet_train.h): LSE, M1 and VAR of temperature j are at + 3 j
TEMP_MAX_J, TEMP_COLS, TEMP_TOTALS = 8, 26, 4
TEMP_SY, TEMP_YZ, TEMP_LSE, TEMP_M1, TEMP_VAR = range(5)


class TempStatsArgs(C.Structure):
    """urso_temp_stats_args (include/ursonet_train.h): one batch of logits and encoded targets at J inverse temperatures."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] + [(n, C.c_int32) for n in ("K", "ld_z", "ld_y", "J")] +
                [("beta", C.c_double * TEMP_MAX_J)] + [(n, C.c_void_p) for n in ("logits", "target", "out")])


class TempReduceArgs(C.Structure):
    """urso_temp_reduce_args (include/ursonet_train.h): the rows 0 .. N - 1 of a table of urso_temp_stats."""
    _fields_ = ([("N", C.c_int64), ("J", C.c_int32), ("pad", C.c_int32), ("beta", C.c_double * TEMP_MAX_J)] +
                [(n, C.c_void_p) for n in ("rows", "totals")])


class TempScaleArgs(C.Structure):
    """urso_temp_scale_args (include/ursonet_train.h): one batch of logits times beta."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "n", "K", "ld_in", "ld_out", "pad")] + [("beta", C.c_double)] +
                [(n, C.c_void_p) for n in ("in_", "out")])


class ConfScoreArgs(C.Structure):
    """urso_conf_score_args (include/ursonet_infer.h): one batch of logits, the estimates' rows and the truth."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] +
                [(n, C.c_int32) for n in ("K", "ld_z", "metric", "ld_est", "ld_ref", "pad")] +
                [(n, C.c_void_p) for n in ("logits", "map", "est", "ref", "out")])


class ConfBoundArgs(C.Structure):
    """urso_conf_bound_args (include/ursonet_infer.h): one batch of logits and the estimates' rows at the level q."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] + [(n, C.c_int32) for n in ("K", "ld_z", "metric", "ld_est")] +
                [("q", C.c_double)] + [(n, C.c_void_p) for n in ("logits", "map", "est", "out")])


# urso_conf_* sizes, metrics and table columns (include/ursonet_infer.h)
CONF_SHIFT, CONF_MAX_K, CONF_COLS, CONF_DIGIT, CONF_PASSES = 34, 1 << 18, 8, 11, 6
CONF_ANGLE, CONF_EUCLID = 0, 1
CONF_SCORE, CONF_C, CONF_W, CONF_KEY_REF, CONF_ERR, CONF_NEAR = range(6)
CONF_BOUND, CONF_KEY, CONF_MASS, CONF_COUNT, CONF_BW = range(5)


class FeatPoolArgs(C.Structure):
    """urso_feat_pool_args (include/ursonet_feat.h): one batch of bottleneck features into rows of an fp64 table."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] + [(n, C.c_int32) for n in ("h", "w", "C", "gh", "gw", "dtype")] +
                [("ld", C.c_int64)] + [(n, C.c_void_p) for n in ("act", "out")])


class FeatGramArgs(C.Structure):
    """urso_feat_gram_args (include/ursonet_feat.h): rows of a feature table into the running sums s and G."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64), ("D", C.c_int32), ("pad", C.c_int32), ("ld_x", C.c_int64), ("ld_g", C.c_int64)] +
                [(n, C.c_void_p) for n in ("x", "centre", "s", "g")])


class FeatMahaArgs(C.Structure):
    """urso_feat_maha_args (include/ursonet_feat.h): a batch's feature rows against a mean and a transposed whitening matrix."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64), ("D", C.c_int32), ("pad", C.c_int32), ("ld_x", C.c_int64), ("ld_w", C.c_int64)] +
                [(n, C.c_void_p) for n in ("x", "mean", "wt", "out")])


# urso_feat_* sizes and table columns (include/ursonet_feat.h)
FEAT_MAX_D, FEAT_COLS, FEAT_MAHA_ROWS = 4096, 4, 8
FEAT_SCORE, FEAT_DIST2, FEAT_ZMAX, FEAT_ZARG = range(4)
# urso_occl_* sizes and table columns (include/ursonet_explain.h): a head's KL, TV, DROP and ARGMAX are four columns in that order
OCCL_COLS, OCCL_MAX_MAPS = 10, 8
OCCL_D_ORI, OCCL_D_LOC, OCCL_ORI_KL, OCCL_ORI_TV, OCCL_ORI_DROP, OCCL_ORI_ARGMAX, OCCL_LOC_KL, OCCL_LOC_TV, OCCL_LOC_DROP, OCCL_LOC_ARGMAX = range(10)


class OcclFillArgs(C.Structure):
    """urso_occl_fill_args (include/ursonet_explain.h): one frame into n occluded rows of a batch."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "n", "H", "W", "C")] + [("fill", C.c_uint8 * 4)] + [(n, C.c_void_p) for n in ("src", "rects", "out")])


class OcclScoreArgs(C.Structure):
    """urso_occl_score_args (include/ursonet_explain.h): a batch's DEC rows and logits against the baseline's."""
    _fields_ = ([("B", C.c_int32), ("n", C.c_int32), ("row0", C.c_int64)] + [(n, C.c_int32) for n in ("ori_K", "ori_ld", "loc_K", "loc_ld")] +
                [(n, C.c_void_p) for n in ("dec0", "dec", "ori_z0", "ori_z", "loc_z0", "loc_z", "out")])


class OcclSplatArgs(C.Structure):
    """urso_occl_splat_args (include/ursonet_explain.h): chosen columns of a patch-score table into per-pixel maps of a window."""
    _fields_ = ([(n, C.c_int32) for n in ("P", "M", "wy0", "wx0", "h", "w")] + [("cols", C.c_int32 * OCCL_MAX_MAPS), ("ld", C.c_int64)] +
                [(n, C.c_void_p) for n in ("scores", "rects", "out")])


class HeatOverlayArgs(C.Structure):
    """urso_heat_overlay_args (include/ursonet_explain.h): one map blended through a colour table onto a window of a picture."""
    _fields_ = ([(n, C.c_int32) for n in ("h", "w", "alpha", "pad")] + [("ld_img", C.c_int64), ("lo", C.c_double), ("scale", C.c_double)] +
                [(n, C.c_void_p) for n in ("map", "lut", "img")])


class DenseWgradLayer(C.Structure):
    """urso_dense_wgrad_layer (include/ursonet_hip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("x", "dz", "part", "colpart")] + [(n, C.c_int32) for n in ("M", "K", "N")]


DENSE_MULTI_MAX = 4
PB_PREP, PB_REDUCE, PB_FINALIZE_MAT, PB_FINALIZE_VEC = 0, 1, 2, 3
WGRAD_PART_PAD = 64            # URSO_WGRAD_PART_PAD: floats between consecutive wgrad partial tensors
_dp = C.POINTER(ParamDesc)
_SIGS = {
    "urso_last_error": (C.c_char_p, []),
    "urso_abi_version": (_i, []),
    "urso_set_option": (_i, [C.c_char_p, _i]),
    "urso_get_option": (_i, [C.c_char_p, C.POINTER(C.c_int)]),
    "urso_conv_igemm": (_i, [_gp, _i, _i, _vp, _vp, _fp, _vp, _vp, _vp, _vp]),
    "urso_conv_igemm_ws_bytes": (_sz, [_gp, _i]),
    "urso_conv_igemm_ws": (_i, [_gp, _i, _i, _vp, _vp, _fp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "urso_conv_igemm_bits_ok": (_i, [_gp, _i, _i, _sz]),
    "urso_conv_igemm_algorithmic": (_i, [_gp, _i, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "urso_conv_igemm_halo_ok": (_i, [_gp, _i, _i, _i]),
    "urso_conv_igemm_halo2_shape": (_i, [_gp, _i, _i, _i, _i]),
    "urso_conv_igemm_halo_ws_bytes": (_sz, []),
    "urso_conv_igemm_ex": (_i, [_gp, _i, _i, _vp, _vp, _fp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "urso_conv_wgrad_ws_bytes": (_sz, [_gp, _i]),
    "urso_conv_wgrad": (_i, [_gp, _i, _vp, _vp, _vp, _sz, _fp, _fp, _vp]),
    "urso_conv_wgrad_splits": (_i, [_gp, _i]),
    "urso_conv_wgrad_partial": (_i, [_gp, _i, _vp, _vp, _vp, _sz, _vp]),
    "urso_param_desc_init": (_i, [_dp, _i, _i, _i, _i, _i, _i, _f, _f]),
    "urso_param_batch_plan": (_i, [_i, _dp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _i]),
    "urso_wgrad_group_fits": (_i, [_gp, _i]),
    "urso_conv_wgrad_pair_splits": (_i, [_gp, _gp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "urso_conv_wgrad_partial2": (_i, [_gp, _gp, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "urso_wgrad_group_plan": (_i, [_i, _vp, _i, C.POINTER(C.c_int32), _i]),
    "urso_wgrad_group_run": (_i, [_i, _vp, _vp, _i, _vp, _i, _vp]),
    "urso_param_batch_run": (_i, [_i, _i, _vp, _vp, _i, _vp]),
    "urso_conv_weight_prep": (_i, [_i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _f, _vp, _vp, _fp, _fp, _vp]),
    "urso_stem_weight_pack": (_i, [_i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _f, _vp, _fp, _fp, _vp]),
    "urso_stem_wgrad_unpack": (_i, [_i, _fp, _fp, _vp]),
    "urso_param_grad_finalize": (_i, [_i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _f, _f, _i, _i,
                                      _fp, _fp, _fp, _fp, _fp, _sz, _vp]),
    "urso_param_grad_finalize_ws_bytes": (_sz, [_i, _i]),
    "urso_param_grad_finalize_sq": (_i, [_i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _f, _f, _i, _i,
                                         _fp, _fp, _fp, _fp, _fp, _sz, _fp, _vp]),
    "urso_param_grad_finalize_sq_slots": (_i, [_i, _i]),
    "urso_param_batch_run_sq": (_i, [_i, _i, _vp, _vp, _i, _fp, _vp]),
    "urso_sqnorm_final": (_i, [_i, _fp, _fp, _vp]),
    "urso_bn_ws_bytes": (_sz, [_i, _i]),
    "urso_bn_batch_stats": (_i, [_i, _i, _i, _vp, _vp, _sz, _fp, _fp, _fp, _fp, _f, _f, _vp]),
    "urso_bn_apply": (_i, [_i, _i, _i, _vp, _fp, _fp, _fp, _fp, _f, _vp, _i, _vp, _vp]),
    "urso_bn_backward": (_i, [_i, _i, _i, _vp, _vp, _fp, _fp, _fp, _f, _vp, _sz, _fp, _fp, _i, _fp, _fp, _vp, _vp]),
    "urso_mold_images": (_i, [_i, _i, _i, _i, _vp, _fp, _i, _vp, _vp]),
    "urso_maxpool3x3s2_fwd": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "urso_maxpool3x3s2_bwd": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "urso_softmax_xent_fwd_bwd": (_i, [_i, _i, _fp, _fp, _f, _i, _i, _fp, _vp, _fp, _vp]),
    "urso_rel_l2_fwd_bwd": (_i, [_i, _i, _i, _fp, _fp, _f, _i, _fp, _vp, _fp, _vp]),
    "urso_rel_l2_norms": (_i, [_i, _i, _i, _fp, _fp, _fp, _vp]),
    "urso_rel_l2_from_norms": (_i, [_i, _i, _i, _fp, _fp, _f, _fp, _i, _fp, _fp, _vp, _vp]),
    "urso_absdot_fwd_bwd": (_i, [_i, _i, _i, _i, _fp, _fp, _f, _i, _fp, _fp, _vp, _vp]),
    "urso_mse_fwd_bwd": (_i, [_i, _i, _i, _fp, _fp, _f, _i, _fp, _vp, _vp]),
    "urso_sqnorm_ws_bytes": (_sz, [_sz]),
    "urso_sqnorm": (_i, [_sz, _fp, _vp, _sz, _fp, _vp]),
    "urso_sgd_momentum_clip": (_i, [_sz, _fp, _fp, _fp, _fp, _fp, _vp]),
    "urso_adam_amsgrad_clip": (_i, [_sz, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    "urso_scale_f32": (_i, [_sz, _fp, _f, _vp]),
    "urso_quat_wavg_decode": (_i, [_i, _i, _fp, _fp, _fp, _fp, _vp]),
    "urso_quat_gmm_fit": (_i, [_i, _i, _fp, _i, _fp, _f, _i, _i, _fp, _fp, _fp, _fp, _vp, _vp]),
    "urso_pose_eval": (_i, [C.POINTER(PoseEvalArgs), _vp]),
    "urso_pose_decode": (_i, [C.POINTER(PoseDecodeArgs), _vp]),
    "urso_warp_perspective": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "urso_encode_ori": (_i, [_i, _i, _vp, _fp, _vp, C.c_double, _fp, _vp]),
    "urso_encode_loc": (_i, [_i, _i, _vp, _vp, C.c_double, _fp, _vp]),
    "urso_comm_unique_id": (_i, [_vp]),
    "urso_comm_init": (_i, [C.POINTER(_vp), _i, _i, _vp]),
    "urso_comm_allreduce_bucket": (_i, [_vp, _vp, _sz, _i, _vp]),
    "urso_comm_wait": (_i, [_vp, _vp]),
    "urso_comm_destroy": (_i, [_vp]),
    "urso_bucket_round_ef": (_i, [_sz, _fp, _fp, _vp, _vp]),
    "urso_dense_multi": (_i, [_i, C.POINTER(DenseLayer), _i, _vp]),
    "urso_dense_wgrad_multi": (_i, [_i, C.POINTER(DenseWgradLayer), _i, _vp]),
    "urso_bucket_expand_bf16": (_i, [_sz, _vp, _fp, _vp]),
    "urso_conv_pair_ok": (_i, [C.c_longlong, _i, _i, _i]),
    "urso_conv_pair": (_i, [C.c_longlong, _i, _i, _i, _vp, _vp, _fp, _vp, _vp, _vp, _vp, _fp, _vp, _vp, _i, _i, _vp]),
    "urso_conv_pair_shortcut": (_i, [C.c_longlong, _i, _vp, _vp, _fp, _vp, _vp, _fp, _vp, _vp, _vp, _fp, _vp, _vp]),
    "urso_conv_dgrad_wgrad_pw": (_i, [C.c_longlong, _i, _vp, _vp, _vp, _i, _vp, _fp, _fp, _sz, _vp]),
    "urso_conv_pair_wgrad_entry": (_i, [C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _fp, _fp, _fp, _fp, _sz, _vp]),
    "urso_stem_wgrad_pooled": (_i, [_gp, _i, _vp, _vp, _vp, _vp, _sz, _fp, _fp, _vp]),
    "urso_stem_conv_pool_ok": (_i, [_gp, _i]),
    "urso_stem_conv_pool": (_i, [_gp, _i, _vp, _vp, _fp, _vp, _vp, _vp]),
    "urso_conv_pair_wgrad_splits": (_i, [C.c_longlong, _i]),
    "urso_conv_pair_wgrad": (_i, [C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _fp, _fp, _sz, _vp]),
    "urso_conv_pointwise_sampled_ok": (_i, [_gp, _i, _i, _i]),
    "urso_conv_pointwise_sampled": (_i, [_gp, _i, _i, _vp, _vp, _fp, _vp, _vp, _vp, _vp, _vp]),
    "urso_rows_subsample2": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "urso_rows_expand2": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "urso_rows_scatter2": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "urso_zero_fill": (_i, [_vp, C.c_size_t, _vp]),
    "urso_rgb_to_grey3": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    "urso_sim2real_op": (_i, [_i, _i, _i, _vp, _vp, _vp, _fp, _vp, _vp, _i, _vp]),
    "urso_pad_images_u8": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "urso_resize_images_u8": (_i, [_i] * 10 + [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "urso_frames_grey_flags_u8": (_i, [_i, _i, _vp, _vp, _vp]),
    "urso_frames_put_u8": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "urso_frames_gather_u8": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "urso_video_prep_u8": (_i, [_i] * 8 + [C.c_double] * 3 + [_vp, _vp, _vp]),
    "urso_draw_prims_u8": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "urso_pmf_sheet_u8": (_i, [_i, _i, _i, _i, _fp, _fp, _vp, _vp, _vp, _vp, _vp]),
    "urso_conv_winograd_ws_bytes": (_sz, [_gp, _i]),
    "urso_conv_winograd_fwd": (_i, [_gp, _i, _i, _vp, _vp, _fp, _vp, _vp, _sz, _vp]),
    "urso_prof_enable": (_i, [_i]),
    "urso_prof_collect": (_i, [C.POINTER(ProfRecord), _i]),
    "urso_prof_collect_ex": (_i, [C.POINTER(ProfRecordEx), _i]),
    "urso_conv_pointwise2_ok": (_i, [_i] * 8),
    "urso_conv_pointwise2": (_i, [_i] * 8 + [_vp, _vp, _vp, _vp, _fp, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)                      # the entry points of include/ursonet_hip.h
# the loss-scaling extension, include/ursonet_loss_scale.h (ursonet_amd/loss_scale.py): the plain signatures + the state buffer in front of the stream
_LS_SIGS = {
    "urso_softmax_xent_fwd_bwd_ls": (_i, [_i, _i, _fp, _fp, _f, _i, _i, _fp, _vp, _fp, _fp, _vp]),
    "urso_rel_l2_fwd_bwd_ls": (_i, [_i, _i, _i, _fp, _fp, _f, _i, _fp, _vp, _fp, _fp, _vp]),
    "urso_absdot_fwd_bwd_ls": (_i, [_i, _i, _i, _i, _fp, _fp, _f, _i, _fp, _fp, _vp, _fp, _vp]),
    "urso_mse_fwd_bwd_ls": (_i, [_i, _i, _i, _fp, _fp, _f, _i, _fp, _vp, _fp, _vp]),
    "urso_param_batch_run_ls": (_i, [_i, _i, _vp, _vp, _i, _fp, _fp, _vp]),
    "urso_param_grad_finalize_ls": (_i, [_i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _f, _f, _i, _i,
                                         _fp, _fp, _fp, _fp, _fp, _sz, _fp, _fp, _vp]),
    "urso_bn_backward_ls": (_i, [_i, _i, _i, _vp, _vp, _fp, _fp, _fp, _f, _vp, _sz, _fp, _fp, _i, _fp, _fp, _vp, _fp, _vp]),
    "urso_sgd_momentum_clip_ls": (_i, [_sz, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    "urso_adam_amsgrad_clip_ls": (_i, [_sz, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    "urso_loss_scale_update": (_i, [_fp, _fp, _vp]),
}
LOSS_SCALE_SYMBOLS = sorted(_LS_SIGS)
# the libraries behind the main one (build.SIDE_SOURCES): name -> signatures of include/ursonet_<name>.h, bound by side_lib(name) on first use
SIDE_SIGS = {
    "ext": {
        "urso_pose_fuse_views": (_i, [C.POINTER(PoseFuseViewsArgs), _vp]),
        # learnable loss weights (ursonet_amd/loss_weights.py): the plain signatures + s, ds and the loss-scale state in front of the stream
        "urso_softmax_xent_fwd_bwd_lw": (_i, [_i, _i, _fp, _fp, _f, _i, _i, _fp, _vp, _fp, _fp, _fp, _fp, _vp]),
        "urso_rel_l2_fwd_bwd_lw": (_i, [_i, _i, _i, _fp, _fp, _f, _i, _fp, _vp, _fp, _fp, _fp, _fp, _vp]),
        "urso_absdot_fwd_bwd_lw": (_i, [_i, _i, _i, _i, _fp, _fp, _f, _i, _fp, _fp, _vp, _fp, _fp, _fp, _vp]),
        # the weights' moving average (ursonet_amd/weight_ema.py): n, w, ema, state, loss-scale state | n, a, b
        "urso_ema_update": (_i, [C.c_int64, _fp, _fp, _fp, _fp, _vp]),
        "urso_ema_swap": (_i, [C.c_int64, _fp, _fp, _vp]),
        # gradient accumulation (ursonet_amd/grad_accum.py): n, g, acc, first | n | n, g, acc, c, sqpart, nparts
        "urso_grad_accum": (_i, [C.c_int64, _fp, _fp, _i, _vp]),
        "urso_grad_accum_parts": (_i, [C.c_int64]),
        "urso_grad_accum_close": (_i, [C.c_int64, _fp, _fp, _f, _fp, _i, _vp]),
        # layer-wise adaptive rate scaling (ursonet_amd/lars.py): T, n_h | T, n_h, NB, blockmap_h, first_h | T, off_h, n_h, tab, blockmap, NB, w, g,
        # part | T, first, adapt, NB, part, hyper, normsq, eta, eps, clip mode, trust, stat, loss-scale state | ... w, g, v, trust, hyper, normsq, ls
        "urso_lars_blocks": (_i, [_i, _vp]),
        "urso_lars_plan": (_i, [_i, _vp, _i, _vp, _vp]),
        "urso_lars_norms": (_i, [_i, _vp, _vp, _vp, _vp, _i, _fp, _fp, _fp, _vp]),
        "urso_lars_trust": (_i, [_i, _vp, _vp, _i, _fp, _fp, _fp, C.c_double, C.c_double, _i, _fp, _vp, _fp, _vp]),
        "urso_lars_sgd": (_i, [_i, _vp, _vp, _vp, _vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    },
    "opt": {
        # LAMB (ursonet_amd/lamb.py): T, off_h, n_h, tab, blockmap, NB, w, g, m, v, vhat, hyper, state, normsq, part, loss-scale state | T, first,
        # adapt, NB, part, normsq, eta, eps, clip mode, trust, stat, ls | T, off_h, n_h, tab, blockmap, NB, w, m, vhat, trust, hyper, state, normsq, ls
        "urso_lamb_moments": (_i, [_i, _vp, _vp, _vp, _vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
        "urso_lamb_trust": (_i, [_i, _vp, _vp, _i, _fp, _fp, C.c_double, C.c_double, _i, _fp, _vp, _fp, _vp]),
        "urso_lamb_apply": (_i, [_i, _vp, _vp, _vp, _vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    },
    "train": {
        # SAM (ursonet_amd/sam.py): n, w, g, w0, state | n, w, w0 | state, normsq, guard
        "urso_sam_ascend": (_i, [C.c_int64, _fp, _fp, _fp, _fp, _vp]),
        "urso_sam_descend": (_i, [C.c_int64, _fp, _fp, _vp]),
        "urso_sam_settle": (_i, [_fp, _fp, _i, _vp]),
        # BN recalibration (ursonet_amd/bn_recal.py): L, layers_h, n_stats, layers_d | L, layers_h, layers_d, n_stats, acc, t | ... acc, stats, t
        "urso_bn_recal_plan": (_i, [_i, _vp, C.c_int64, _vp]),
        "urso_bn_recal_add": (_i, [_i, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp]),
        "urso_bn_recal_settle": (_i, [_i, _vp, _vp, C.c_int64, _vp, _fp, C.c_int64, _vp]),
        # SWA / SWAG-diagonal (ursonet_amd/swa.py): n, w, mean, sq | null, state, loss-scale state | n, first, mean, sq, out, z_out | null, s, seed, sample
        "urso_swa_update": (_i, [C.c_int64, _fp, _fp, _fp, _vp, _fp, _vp]),
        "urso_swag_sample": (_i, [C.c_int64, C.c_int64, _fp, _fp, _fp, _fp, C.c_float, C.c_uint64, _i, _vp]),
        # ensemble inference (ursonet_amd/ensemble.py): urso_ens_add_args* | urso_ens_settle_args*
        "urso_ens_add": (_i, [C.POINTER(EnsAddArgs), _vp]),
        "urso_ens_settle": (_i, [C.POINTER(EnsSettleArgs), _vp]),
        # temperature scaling (ursonet_amd/calibrate.py): urso_temp_stats_args* | urso_temp_reduce_args* | urso_temp_scale_args*
        "urso_temp_stats": (_i, [C.POINTER(TempStatsArgs), _vp]),
        "urso_temp_reduce": (_i, [C.POINTER(TempReduceArgs), _vp]),
        "urso_temp_scale": (_i, [C.POINTER(TempScaleArgs), _vp]),
    },
    "infer": {
        # conformal bounds (ursonet_amd/conformal.py): urso_conf_score_args* | urso_conf_bound_args*
        "urso_conf_score": (_i, [C.POINTER(ConfScoreArgs), _vp]),
        "urso_conf_bound": (_i, [C.POINTER(ConfBoundArgs), _vp]),
    },
    "feat": {
        # domain-shift scores (ursonet_amd/domain.py): urso_feat_pool_args* | urso_feat_gram_args* | urso_feat_maha_args*
        "urso_feat_pool": (_i, [C.POINTER(FeatPoolArgs), _vp]),
        "urso_feat_gram_add": (_i, [C.POINTER(FeatGramArgs), _vp]),
        "urso_feat_maha": (_i, [C.POINTER(FeatMahaArgs), _vp]),
    },
    "explain": {
        # occlusion sensitivity (ursonet_amd/explain.py): urso_occl_fill_args* | urso_occl_score_args* | urso_occl_splat_args* | urso_heat_overlay_args*
        "urso_occl_fill_u8": (_i, [C.POINTER(OcclFillArgs), _vp]),
        "urso_occl_score": (_i, [C.POINTER(OcclScoreArgs), _vp]),
        "urso_occl_splat": (_i, [C.POINTER(OcclSplatArgs), _vp]),
        "urso_heat_overlay_u8": (_i, [C.POINTER(HeatOverlayArgs), _vp]),
    },
}
SIDE_SYMBOLS = {name: sorted(sigs) for name, sigs in SIDE_SIGS.items()}
LAMB_STATE_INIT = (1.0, 1.0, 0.0)                                     # URSO_LAMB_STATE floats {p1, p2, kt} before the first step
SAM_STATE = 8                                                         # URSO_SAM_STATE floats (ursonet_amd/sam.py names the fields)
SWA_STATE = 8                                                         # URSO_SWA_STATE int32s (ursonet_amd/swa.py names the fields)


def _bind(lib, sigs):
    for _name, (_res, _args) in sigs.items():
        _fn = getattr(lib, _name)       # AttributeError here == symbol missing from the .so
        _fn.restype = _res
        _fn.argtypes = _args


_bind(_lib, dict(_SIGS, **_LS_SIGS))
_side = {}


def side_lib(name):
    """liburso_<name>.so, loaded and bound on first use.  It calls into the main library (error text, launch profiler), so that one's
    symbols are first made visible to later loads (RTLD_NOLOAD | RTLD_GLOBAL promotes the copy already loaded, whichever variant it is)."""
    if name not in _side:
        path = _build.SIDE_LIBS[name]
        if not os.path.exists(path):
            raise ImportError("liburso_%s.so not found at %s -- build it with `python -m ursonet_amd.build` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % (name, path))
        C.CDLL(LIB_PATH, mode=os.RTLD_NOLOAD | os.RTLD_GLOBAL | os.RTLD_NOW)
        lib = C.CDLL(path)
        _bind(lib, SIDE_SIGS[name])
        _side[name] = lib
    return _side[name]


def last_error():
    return (_lib.urso_last_error() or b"").decode()


def _chk(rc, what):
    if rc != 0:
        raise UrsoHipError("%s failed (%d): %s" % (what, rc, last_error()))


def set_option(name, value):
    """urso_set_option: explicit kernel-policy switch (include/ursonet_hip.h)."""
    _chk(_lib.urso_set_option(name.encode(), int(value)), "urso_set_option")


def get_option(name):
    v = C.c_int(0)
    _chk(_lib.urso_get_option(name.encode(), C.byref(v)), "urso_get_option")
    return int(v.value)


class options(object):
    """Context manager: `with hip.options(grid_cap=16): ...` sets options and restores the previous values."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


# A/B experiments inside one process launch: every URSO_OPT_<NAME>=<int> in the environment of the PYTHON host is applied once at
# import (the C library itself never reads the environment).  <NAME> lowercased is the option's name; one the library refuses
# (a misspelt variable, a dropped option) raises here instead of leaving the run on the defaults.
for _k in sorted(os.environ):
    if _k.startswith("URSO_OPT_"):
        try:
            set_option(_k[len("URSO_OPT_"):].lower(), int(os.environ[_k]))
        except (UrsoHipError, ValueError) as _err:
            raise ImportError("environment variable %s=%r: %s" % (_k, os.environ[_k], _err))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous device tensor"
    return t.data_ptr()


def stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def geom(B, H, W, Cin, OH, OW, N, KH, KW, SH=1, SW=1, PH=0, PW=0, DH=1, DW=1, FH=0, FW=0, OSH=0, OSW=0):
    return ConvGeom(B, H, W, Cin, OH, OW, N, KH, KW, SH, SW, PH, PW, DH, DW, FH, FW, OSH, OSW)


# ---------------------------------------------------------------- thin typed wrappers
def conv_igemm(g, dt, flags, src, wgt, bias, add, mask, dst, stream=None):
    _chk(_lib.urso_conv_igemm(C.byref(g), dt, flags, ptr(src), ptr(wgt), ptr(bias), ptr(add), ptr(mask), ptr(dst),
                              stream_ptr(stream)), "urso_conv_igemm")


class DenseMulti(object):
    """Up to DENSE_MULTI_MAX Dense layers of the heads in one launch (urso_dense_multi).  layers: dicts with src0, wgt0, dst, M, N, K0 and
    optionally src1, wgt1, K1 (a second reduction segment), bias, add, mask, flags -- tensors are kept alive by the object."""

    def __init__(self, layers, dt):
        assert 1 <= len(layers) <= DENSE_MULTI_MAX
        self.dt, self.n = dt, len(layers)
        self.host = (DenseLayer * self.n)()
        self.keep = []
        for it, L in zip(self.host, layers):
            for f in ("src0", "wgt0", "src1", "wgt1", "bias", "add", "mask", "dst"):
                t = L.get(f)
                self.keep.append(t)
                setattr(it, f, t.data_ptr() if t is not None else None)
            it.M, it.N, it.K0, it.K1, it.flags = int(L["M"]), int(L["N"]), int(L["K0"]), int(L.get("K1", 0)), int(L.get("flags", 0))

    def run(self, stream=None):
        _chk(_lib.urso_dense_multi(self.n, self.host, self.dt, stream_ptr(stream)), "urso_dense_multi")


class DenseWgradMulti(object):
    """The weight gradients of up to DENSE_MULTI_MAX Dense layers in one launch (urso_dense_wgrad_multi).  layers: dicts with x [M][K], dz [M][N],
    part (fp32, >= K * N) and colpart (fp32, >= N, or None) tensors and M, K, N."""

    def __init__(self, layers, dt):
        assert 1 <= len(layers) <= DENSE_MULTI_MAX
        self.dt, self.n = dt, len(layers)
        self.host = (DenseWgradLayer * self.n)()
        self.keep = []
        for it, L in zip(self.host, layers):
            assert L["part"].dtype == torch.float32 and L["part"].numel() >= L["K"] * L["N"]
            for f in ("x", "dz", "part", "colpart"):
                t = L.get(f)
                self.keep.append(t)
                setattr(it, f, t.data_ptr() if t is not None else None)
            it.M, it.K, it.N = int(L["M"]), int(L["K"]), int(L["N"])

    def run(self, stream=None):
        _chk(_lib.urso_dense_wgrad_multi(self.n, self.host, self.dt, stream_ptr(stream)), "urso_dense_wgrad_multi")


def bucket_round_ef(g, resid, c, stream=None):
    """urso_bucket_round_ef: c = bf16(g + resid), resid = (g + resid) - float(c), one pass (g is only read)."""
    assert g.dtype == torch.float32 and resid.dtype == torch.float32 and c.dtype == torch.bfloat16 and g.numel() == resid.numel() == c.numel()
    _chk(_lib.urso_bucket_round_ef(g.numel(), ptr(g), ptr(resid), ptr(c), stream_ptr(stream)), "urso_bucket_round_ef")


def bucket_expand_bf16(c, g, stream=None):
    """urso_bucket_expand_bf16: g = float(c)."""
    assert g.dtype == torch.float32 and c.dtype == torch.bfloat16 and g.numel() == c.numel()
    _chk(_lib.urso_bucket_expand_bf16(g.numel(), ptr(c), ptr(g), stream_ptr(stream)), "urso_bucket_expand_bf16")


def conv_winograd_ws_bytes(g, dt):
    return int(_lib.urso_conv_winograd_ws_bytes(C.byref(g), dt))


def conv_winograd_fwd(g, dt, flags, src, wgt, bias, dst, ws, stream=None):
    """urso_conv_winograd_fwd: Winograd F(2x2, 3x3) evaluation of a 3x3 / stride-1 / pad-1 forward conv (opt-in; slower than the direct kernels)."""
    _chk(_lib.urso_conv_winograd_fwd(C.byref(g), dt, flags, ptr(src), ptr(wgt), ptr(bias), ptr(dst), ptr(ws), ws.numel() * ws.element_size(),
                                     stream_ptr(stream)), "urso_conv_winograd_fwd")


def conv_igemm_ws_bytes(g, dt):
    return int(_lib.urso_conv_igemm_ws_bytes(C.byref(g), dt))


def conv_igemm_ws(g, dt, flags, src, wgt, bias, add, mask, dst, ws, stream=None):
    _chk(_lib.urso_conv_igemm_ws(C.byref(g), dt, flags, ptr(src), ptr(wgt), ptr(bias), ptr(add), ptr(mask), ptr(dst),
                                 ptr(ws), ws.numel() * ws.element_size() if ws is not None else 0, stream_ptr(stream)),
         "urso_conv_igemm_ws")


def conv_igemm_bits_ok(g, dt, flags, ws_bytes=0):
    return bool(_lib.urso_conv_igemm_bits_ok(C.byref(g), dt, flags, ws_bytes))


def conv_igemm_halo_ws_bytes():
    """Hand-over workspace of the halo-tile kernel's stream-K schedule; its first 4 KiB (flags) must be zero on entry (left zero)."""
    return int(_lib.urso_conv_igemm_halo_ws_bytes())


def conv_igemm_halo_ok(g, dt, flags, has_add=False):
    return bool(_lib.urso_conv_igemm_halo_ok(C.byref(g), dt, flags, int(bool(has_add))))


def conv_igemm_algorithmic(g, dt, flags, has_add=False, has_mask=False):
    """(FLOPs, bytes) the launch profiler records for a urso_conv_igemm_ex launch (host arithmetic)."""
    fl, by = C.c_double(0), C.c_double(0)
    _chk(_lib.urso_conv_igemm_algorithmic(C.byref(g), dt, flags, int(bool(has_add)), int(bool(has_mask)), C.byref(fl), C.byref(by)), "urso_conv_igemm_algorithmic")
    return float(fl.value), float(by.value)


def conv_igemm_halo2_shape(g, dt, flags, has_add=False, has_ws=False):
    """10 * MI + NJ of the whole-tile halo kernel (conv_halo2.hip) for this layer, 0 when conv_halo.hip keeps it."""
    return int(_lib.urso_conv_igemm_halo2_shape(C.byref(g), dt, flags, int(bool(has_add)), int(bool(has_ws))))


def conv_igemm_ex(g, dt, flags, src, wgt, bias, add, mask, dst, bits_out=None, ws=None, stream=None):
    _chk(_lib.urso_conv_igemm_ex(C.byref(g), dt, flags, ptr(src), ptr(wgt), ptr(bias), ptr(add), ptr(mask), ptr(dst), ptr(bits_out),
                                 ptr(ws), (ws.numel() * ws.element_size()) if ws is not None else 0, stream_ptr(stream)), "urso_conv_igemm_ex")


def conv_pointwise2_ok(B, OH, OW, C0, C1, N, dt, flags):
    return bool(_lib.urso_conv_pointwise2_ok(B, OH, OW, C0, C1, N, dt, flags))


def conv_pointwise2(B, OH, OW, C0, C1, N, dt, flags, src0, wgt0, src1, wgt1, bias, mask, dst, bits_out=None, stream=None):
    """dst = epilogue(src0 . wgt0^T + src1 . wgt1^T + bias): two pointwise layers over the same pixels in one launch (include/ursonet_hip.h)."""
    _chk(_lib.urso_conv_pointwise2(B, OH, OW, C0, C1, N, dt, flags, ptr(src0), ptr(wgt0), ptr(src1), ptr(wgt1), ptr(bias), ptr(mask), ptr(dst),
                                   ptr(bits_out), stream_ptr(stream)), "urso_conv_pointwise2")


def conv_wgrad_ws_bytes(g, dt):
    return int(_lib.urso_conv_wgrad_ws_bytes(C.byref(g), dt))


def conv_wgrad(g, dt, x, dz, ws, dw_raw, colsum, stream=None):
    _chk(_lib.urso_conv_wgrad(C.byref(g), dt, ptr(x), ptr(dz), ptr(ws), ws.numel() * ws.element_size(), ptr(dw_raw),
                              ptr(colsum), stream_ptr(stream)), "urso_conv_wgrad")


def conv_wgrad_splits(g, dt):
    return int(_lib.urso_conv_wgrad_splits(C.byref(g), dt))


def conv_wgrad_partial(g, dt, x, dz, ws, stream=None):
    _chk(_lib.urso_conv_wgrad_partial(C.byref(g), dt, ptr(x), ptr(dz), ptr(ws), ws.numel() * ws.element_size(), stream_ptr(stream)),
         "urso_conv_wgrad_partial")


def param_desc_init(d, KH, KW, Cin, N, npad, splits, eps, weight_decay):
    _chk(_lib.urso_param_desc_init(C.byref(d), KH, KW, Cin, N, npad, splits, eps, weight_decay), "urso_param_desc_init")


class ParamBatch(object):
    """A device copy of a ParamDesc array plus per-(phase, layer subset) block maps; run(phase, key) is one launch."""

    def __init__(self, descs, device):
        self.n = len(descs)
        self.host = (ParamDesc * self.n)(*descs)
        raw = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8)
        self.dev = raw.to(device)
        self.maps = {}

    def plan(self, phase, key, layer_ids):
        ids = (C.c_int32 * len(layer_ids))(*layer_ids)
        nb = _lib.urso_param_batch_plan(phase, self.host, ids, len(layer_ids), None, 0)
        if nb < 0:
            raise UrsoHipError("urso_param_batch_plan: " + last_error())
        buf = (C.c_int32 * (2 * max(nb, 1)))()
        _lib.urso_param_batch_plan(phase, self.host, ids, len(layer_ids), buf, nb)
        t = torch.frombuffer(bytearray(bytes(buf)), dtype=torch.int32).to(self.dev.device)
        self.maps[(phase, key)] = (t, nb)
        return nb

    def run(self, phase, key, dt, stream=None, sqpart=None, ls=None):
        """sqpart (fp32, >= the phase's block count; FINALIZE phases): every block also leaves the sum of squares of what it stored there.
        ls (the loss-scale state; FINALIZE phases): the raw gradients are unscaled as they are read (urso_param_batch_run_ls)."""
        t, nb = self.maps[(phase, key)]
        if nb and ls is not None and phase in (PB_FINALIZE_MAT, PB_FINALIZE_VEC):
            assert sqpart is None or (sqpart.dtype == torch.float32 and sqpart.numel() >= nb)
            _chk(_lib.urso_param_batch_run_ls(phase, dt, ptr(self.dev), ptr(t), nb, ptr(sqpart), _ls_ptr(ls), stream_ptr(stream)),
                 "urso_param_batch_run_ls")
        elif nb and sqpart is not None:
            assert sqpart.dtype == torch.float32 and sqpart.numel() >= nb
            _chk(_lib.urso_param_batch_run_sq(phase, dt, ptr(self.dev), ptr(t), nb, ptr(sqpart), stream_ptr(stream)), "urso_param_batch_run_sq")
        elif nb:
            _chk(_lib.urso_param_batch_run(phase, dt, ptr(self.dev), ptr(t), nb, stream_ptr(stream)), "urso_param_batch_run")

    def nblocks(self, phase, key):
        return self.maps[(phase, key)][1]


def conv_wgrad_pair_splits(g0, g1, dt):
    """(splits0, splits1) of urso_conv_wgrad_partial2 for two 3x3 layers of conv_hwgrad.hip, or None when they do not pair."""
    a, b = C.c_int(0), C.c_int(0)
    ok = _lib.urso_conv_wgrad_pair_splits(C.byref(g0), C.byref(g1), dt, C.byref(a), C.byref(b))
    return (a.value, b.value) if ok else None


def conv_wgrad_partial2(g0, g1, dt, x0, dz0, ws0, x1, dz1, ws1, stream=None):
    _chk(_lib.urso_conv_wgrad_partial2(C.byref(g0), C.byref(g1), dt, ptr(x0), ptr(dz0), ptr(ws0), ws0.numel() * ws0.element_size(),
                                       ptr(x1), ptr(dz1), ptr(ws1), ws1.numel() * ws1.element_size(), stream_ptr(stream)), "urso_conv_wgrad_partial2")


class WgradItem(C.Structure):
    """urso_wgrad_item (include/ursonet_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("dz", C.c_void_p), ("part", C.c_void_p), ("colpart", C.c_void_p), ("g", ConvGeom),
                ("M", C.c_int32), ("ktiles", C.c_int32), ("ntiles", C.c_int32), ("splits", C.c_int32), ("m_per_split", C.c_int32),
                ("mode", C.c_int32), ("fill", C.c_int32)]


def wgrad_group_fits(g, dt):
    return bool(_lib.urso_wgrad_group_fits(C.byref(g), dt))


class WgradGroup(object):
    """The weight gradients of several 16-bit layers in one launch (urso_wgrad_group_plan / _run).

    geoms: the layers' forward geometries.  After construction .splits[i] holds each layer's partial count and .fill the fraction of
    the resident block slots the plan keeps busy (.nblocks == 0: the group does not fit one residency); bind() takes the operand /
    workspace tensors (partials laid out as urso_conv_wgrad_partial does)."""

    def __init__(self, geoms, dt):
        self.n, self.dt = len(geoms), dt
        self.host = (WgradItem * self.n)()
        for it, g in zip(self.host, geoms):
            C.memmove(C.byref(it.g), C.byref(g), C.sizeof(ConvGeom))
        nb = _lib.urso_wgrad_group_plan(self.n, self.host, dt, None, 0)
        if nb < 0:
            raise UrsoHipError("urso_wgrad_group_plan: " + last_error())
        self.nblocks = nb
        self.splits = [int(it.splits) for it in self.host] if nb else []
        self.fill = self.host[0].fill / 1000.0 if nb else 0.0     # work / (resident slots x the longest block)
        self.dev = self.map = None

    def bind(self, xs, dzs, wss, device):
        buf = (C.c_int32 * (2 * self.nblocks))()
        if _lib.urso_wgrad_group_plan(self.n, self.host, self.dt, buf, self.nblocks) != self.nblocks:
            raise UrsoHipError("urso_wgrad_group_plan: " + last_error())
        for it, x, dz, ws in zip(self.host, xs, dzs, wss):
            n_part = it.splits * (it.g.KH * it.g.KW * it.g.C * it.g.N + WGRAD_PART_PAD)
            if ws.numel() * ws.element_size() < 4 * (n_part + it.splits * it.g.N):
                raise UrsoHipError("WgradGroup.bind: workspace too small")
            it.x, it.dz, it.part, it.colpart = x.data_ptr(), dz.data_ptr(), ws.data_ptr(), ws.data_ptr() + 4 * n_part
        self.keep = (list(xs), list(dzs), list(wss))
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)
        self.map = torch.frombuffer(bytearray(bytes(buf)), dtype=torch.int32).to(device)

    def run(self, stream=None):
        _chk(_lib.urso_wgrad_group_run(self.dt, ptr(self.dev), C.cast(self.host, C.c_void_p), self.n, ptr(self.map), self.nblocks,
                                       stream_ptr(stream)), "urso_wgrad_group_run")


def bn_ws_bytes(M, N):
    return int(_lib.urso_bn_ws_bytes(M, N))


def bn_batch_stats(M, N, dt, z, ws, mean, var, mmean, mvar, momentum, eps, stream=None):
    _chk(_lib.urso_bn_batch_stats(M, N, dt, ptr(z), ptr(ws), ws.numel() * ws.element_size(), ptr(mean), ptr(var), ptr(mmean), ptr(mvar),
                                  momentum, eps, stream_ptr(stream)), "urso_bn_batch_stats")


def bn_apply(M, N, dt, z, mean, var, gamma, beta, eps, res, relu, y, stream=None):
    _chk(_lib.urso_bn_apply(M, N, dt, ptr(z), ptr(mean), ptr(var), ptr(gamma), ptr(beta), eps, ptr(res), int(relu), ptr(y), stream_ptr(stream)),
         "urso_bn_apply")


def _ls_ptr(ls):
    """Device pointer of a loss-scale state buffer (ursonet_amd/loss_scale.py: FIELDS fp32 values)."""
    assert ls.dtype == torch.float32 and ls.numel() >= 8
    return ptr(ls)


def bn_backward(M, N, dt, g, z, mean, var, gamma, eps, ws, dbeta, dgamma, bn_trainable, gbeta, ggamma, dz, stream=None, ls=None):
    if ls is not None:
        _chk(_lib.urso_bn_backward_ls(M, N, dt, ptr(g), ptr(z), ptr(mean), ptr(var), ptr(gamma), eps, ptr(ws), ws.numel() * ws.element_size(),
                                      ptr(dbeta), ptr(dgamma), int(bn_trainable), ptr(gbeta), ptr(ggamma), ptr(dz), _ls_ptr(ls), stream_ptr(stream)),
             "urso_bn_backward_ls")
        return
    _chk(_lib.urso_bn_backward(M, N, dt, ptr(g), ptr(z), ptr(mean), ptr(var), ptr(gamma), eps, ptr(ws), ws.numel() * ws.element_size(),
                               ptr(dbeta), ptr(dgamma), int(bn_trainable), ptr(gbeta), ptr(ggamma), ptr(dz), stream_ptr(stream)), "urso_bn_backward")


def conv_weight_prep(KH, KW, Cin, N, npad, dt, w, b, gamma, beta, mean, var, eps, wf, wd, biasf, scale, stream=None):
    _chk(_lib.urso_conv_weight_prep(KH, KW, Cin, N, npad, dt, ptr(w), ptr(b), ptr(gamma), ptr(beta), ptr(mean), ptr(var),
                                    eps, ptr(wf), ptr(wd), ptr(biasf), ptr(scale), stream_ptr(stream)),
         "urso_conv_weight_prep")


def stem_weight_pack(N, dt, w, b, gamma, beta, mean, var, eps, wf, biasf, scale, stream=None):
    _chk(_lib.urso_stem_weight_pack(N, dt, ptr(w), ptr(b), ptr(gamma), ptr(beta), ptr(mean), ptr(var), eps, ptr(wf),
                                    ptr(biasf), ptr(scale), stream_ptr(stream)), "urso_stem_weight_pack")


def stem_wgrad_unpack(N, dw_packed, dw_raw, stream=None):
    _chk(_lib.urso_stem_wgrad_unpack(N, ptr(dw_packed), ptr(dw_raw), stream_ptr(stream)), "urso_stem_wgrad_unpack")


def param_grad_finalize_ws_bytes(K, N):
    return int(_lib.urso_param_grad_finalize_ws_bytes(K, N))


def param_grad_finalize(K, N, ldn, dw_raw, colsum, w, b, gamma, mean, var, eps, wd, trainable, bn_trainable,
                        gw, gb, ggamma, gbeta, ws, stream=None):
    _chk(_lib.urso_param_grad_finalize(K, N, ldn, ptr(dw_raw), ptr(colsum), ptr(w), ptr(b), ptr(gamma), ptr(mean),
                                       ptr(var), eps, wd, int(trainable), int(bn_trainable), ptr(gw), ptr(gb),
                                       ptr(ggamma), ptr(gbeta), ptr(ws), ws.numel() * ws.element_size(),
                                       stream_ptr(stream)), "urso_param_grad_finalize")


def param_grad_finalize_sq_slots(K, N):
    return int(_lib.urso_param_grad_finalize_sq_slots(K, N))


def param_grad_finalize_sq(K, N, ldn, dw_raw, colsum, w, b, gamma, mean, var, eps, wd, trainable, bn_trainable,
                           gw, gb, ggamma, gbeta, ws, sqpart, stream=None):
    assert sqpart.dtype == torch.float32 and sqpart.numel() >= param_grad_finalize_sq_slots(K, N)
    _chk(_lib.urso_param_grad_finalize_sq(K, N, ldn, ptr(dw_raw), ptr(colsum), ptr(w), ptr(b), ptr(gamma), ptr(mean),
                                          ptr(var), eps, wd, int(trainable), int(bn_trainable), ptr(gw), ptr(gb),
                                          ptr(ggamma), ptr(gbeta), ptr(ws), ws.numel() * ws.element_size(), ptr(sqpart),
                                          stream_ptr(stream)), "urso_param_grad_finalize_sq")


def param_grad_finalize_ls(K, N, ldn, dw_raw, colsum, w, b, gamma, mean, var, eps, wd, trainable, bn_trainable,
                           gw, gb, ggamma, gbeta, ws, sqpart, ls, stream=None):
    """The loss-scaled per-layer finalisation; sqpart = None: no squared-norm slots (urso_param_grad_finalize's launches)."""
    assert sqpart is None or (sqpart.dtype == torch.float32 and sqpart.numel() >= param_grad_finalize_sq_slots(K, N))
    _chk(_lib.urso_param_grad_finalize_ls(K, N, ldn, ptr(dw_raw), ptr(colsum), ptr(w), ptr(b), ptr(gamma), ptr(mean),
                                          ptr(var), eps, wd, int(trainable), int(bn_trainable), ptr(gw), ptr(gb),
                                          ptr(ggamma), ptr(gbeta), ptr(ws), ws.numel() * ws.element_size(), ptr(sqpart), _ls_ptr(ls),
                                          stream_ptr(stream)), "urso_param_grad_finalize_ls")


def sqnorm_final(parts, out, stream=None):
    """urso_sqnorm_final: out[0] = sum of parts (the slots the *_sq finalisation launches wrote), in index order."""
    assert parts.dtype == torch.float32 and out.dtype == torch.float32
    _chk(_lib.urso_sqnorm_final(parts.numel(), ptr(parts), ptr(out), stream_ptr(stream)), "urso_sqnorm_final")


def mold_images(B, H, W, src, mean3, dt, dst, stream=None):
    is_u8 = 1 if src.dtype == torch.uint8 else 0
    assert is_u8 or src.dtype == torch.float32
    _chk(_lib.urso_mold_images(B, H, W, is_u8, ptr(src), ptr(mean3), dt, ptr(dst), stream_ptr(stream)), "urso_mold_images")


def maxpool_fwd(B, H, W, Cc, dt, x, y, argmax, stream=None):
    _chk(_lib.urso_maxpool3x3s2_fwd(B, H, W, Cc, dt, ptr(x), ptr(y), ptr(argmax), stream_ptr(stream)), "urso_maxpool3x3s2_fwd")


def maxpool_bwd(B, H, W, Cc, dt, y, dy, argmax, relu_mask, dx, stream=None):
    _chk(_lib.urso_maxpool3x3s2_bwd(B, H, W, Cc, dt, ptr(y), ptr(dy), ptr(argmax), int(relu_mask), ptr(dx),
                                    stream_ptr(stream)), "urso_maxpool3x3s2_bwd")


def _lw_ptrs(lw):
    """lw = (s, ds): one-element fp32 device tensors, the trainable log-variance of a loss and its gradient slot (ds None: s is frozen)."""
    s, ds = lw
    assert s.dtype == torch.float32 and s.numel() == 1 and (ds is None or (ds.dtype == torch.float32 and ds.numel() == 1))
    return ptr(s), ptr(ds)


def softmax_xent(B, K, logits, labels, weight, relu_mask, dt, loss, dz, row_ws, stream=None, ls=None, lw=None):
    """ls (here and in rel_l2 / absdot / mse): the loss-scale state buffer -- the gradient is multiplied by its scale in front of the
    rounding to dt (the *_ls entry points); None: the plain entry point.
    lw (here and in rel_l2 / absdot) = (s, ds): the learnable-loss-weight form of liburso_ext.so (the *_lw entry points; ls may be set too)."""
    if lw is not None:
        _chk(side_lib("ext").urso_softmax_xent_fwd_bwd_lw(B, K, ptr(logits), ptr(labels), weight, int(relu_mask), dt, ptr(loss), ptr(dz), ptr(row_ws),
                                                    *_lw_ptrs(lw), _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)),
             "urso_softmax_xent_fwd_bwd_lw")
        return
    if ls is not None:
        _chk(_lib.urso_softmax_xent_fwd_bwd_ls(B, K, ptr(logits), ptr(labels), weight, int(relu_mask), dt, ptr(loss), ptr(dz),
                                               ptr(row_ws), _ls_ptr(ls), stream_ptr(stream)), "urso_softmax_xent_fwd_bwd_ls")
        return
    _chk(_lib.urso_softmax_xent_fwd_bwd(B, K, ptr(logits), ptr(labels), weight, int(relu_mask), dt, ptr(loss), ptr(dz),
                                        ptr(row_ws), stream_ptr(stream)), "urso_softmax_xent_fwd_bwd")


def rel_l2_norms(B, D, ld, gt, pred, norms, stream=None):
    _chk(_lib.urso_rel_l2_norms(B, D, ld, ptr(gt), ptr(pred), ptr(norms), stream_ptr(stream)), "urso_rel_l2_norms")


def rel_l2_from_norms(B, D, ld, gt, pred, weight, gscale, dt, norms, loss, dpred, stream=None):
    _chk(_lib.urso_rel_l2_from_norms(B, D, ld, ptr(gt), ptr(pred), weight, ptr(gscale), dt, ptr(norms), ptr(loss), ptr(dpred),
                                     stream_ptr(stream)), "urso_rel_l2_from_norms")


def rel_l2(B, D, ld, gt, pred, weight, dt, loss, dpred, norms=None, stream=None, ls=None, lw=None):
    if lw is not None:
        _chk(side_lib("ext").urso_rel_l2_fwd_bwd_lw(B, D, ld, ptr(gt), ptr(pred), weight, dt, ptr(loss), ptr(dpred), ptr(norms), *_lw_ptrs(lw),
                                              _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)), "urso_rel_l2_fwd_bwd_lw")
        return
    if ls is not None:
        _chk(_lib.urso_rel_l2_fwd_bwd_ls(B, D, ld, ptr(gt), ptr(pred), weight, dt, ptr(loss), ptr(dpred), ptr(norms), _ls_ptr(ls),
                                         stream_ptr(stream)), "urso_rel_l2_fwd_bwd_ls")
        return
    _chk(_lib.urso_rel_l2_fwd_bwd(B, D, ld, ptr(gt), ptr(pred), weight, dt, ptr(loss), ptr(dpred), ptr(norms),
                                  stream_ptr(stream)), "urso_rel_l2_fwd_bwd")


def absdot(B, D, ld, normalize, gt, x, weight, dt, q, loss, dx, stream=None, ls=None, lw=None):
    if lw is not None:
        _chk(side_lib("ext").urso_absdot_fwd_bwd_lw(B, D, ld, int(normalize), ptr(gt), ptr(x), weight, dt, ptr(q), ptr(loss), ptr(dx), *_lw_ptrs(lw),
                                              _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)), "urso_absdot_fwd_bwd_lw")
        return
    if ls is not None:
        _chk(_lib.urso_absdot_fwd_bwd_ls(B, D, ld, int(normalize), ptr(gt), ptr(x), weight, dt, ptr(q), ptr(loss), ptr(dx), _ls_ptr(ls),
                                         stream_ptr(stream)), "urso_absdot_fwd_bwd_ls")
        return
    _chk(_lib.urso_absdot_fwd_bwd(B, D, ld, int(normalize), ptr(gt), ptr(x), weight, dt, ptr(q), ptr(loss), ptr(dx),
                                  stream_ptr(stream)), "urso_absdot_fwd_bwd")


def mse(B, D, ld, gt, pred, weight, dt, loss, dpred, stream=None, ls=None):
    if ls is not None:
        _chk(_lib.urso_mse_fwd_bwd_ls(B, D, ld, ptr(gt), ptr(pred), weight, dt, ptr(loss), ptr(dpred), _ls_ptr(ls), stream_ptr(stream)),
             "urso_mse_fwd_bwd_ls")
        return
    _chk(_lib.urso_mse_fwd_bwd(B, D, ld, ptr(gt), ptr(pred), weight, dt, ptr(loss), ptr(dpred), stream_ptr(stream)),
         "urso_mse_fwd_bwd")


def sqnorm_ws_bytes(n):
    return int(_lib.urso_sqnorm_ws_bytes(n))


def sqnorm(n, g, ws, out, stream=None):
    _chk(_lib.urso_sqnorm(n, ptr(g), ptr(ws), ws.numel() * ws.element_size(), ptr(out), stream_ptr(stream)), "urso_sqnorm")


def sgd_momentum_clip(n, w, g, v, hyper, normsq, stream=None, ls=None):
    """ls (here and in adam_amsgrad_clip): the loss-scaled form -- a step whose squared norm is not finite changes nothing."""
    if ls is not None:
        _chk(_lib.urso_sgd_momentum_clip_ls(n, ptr(w), ptr(g), ptr(v), ptr(hyper), ptr(normsq), _ls_ptr(ls), stream_ptr(stream)),
             "urso_sgd_momentum_clip_ls")
        return
    _chk(_lib.urso_sgd_momentum_clip(n, ptr(w), ptr(g), ptr(v), ptr(hyper), ptr(normsq), stream_ptr(stream)),
         "urso_sgd_momentum_clip")


def loss_scale_update(state, normsq, stream=None):
    """urso_loss_scale_update: the rule of ursonet_amd.loss_scale.next_state on the device, after the optimizer of the step."""
    _chk(_lib.urso_loss_scale_update(_ls_ptr(state), ptr(normsq), stream_ptr(stream)), "urso_loss_scale_update")


def ema_update(n, w, ema, state, stream=None, ls=None):
    """urso_ema_update (liburso_ext.so): ema += (1 - d) (w - ema) over n fp32 elements with d = state[EMA_NEXT_DECAY], then the state advances
    (ursonet_amd.weight_ema.update32 / next_state on the device).  ls: the loss-scale state; a step it marks as skipped changes nothing."""
    assert w.dtype == torch.float32 and ema.dtype == torch.float32 and state.dtype == torch.float32 and state.numel() >= EMA_FIELDS
    assert 0 <= n <= min(w.numel(), ema.numel())
    _chk(side_lib("ext").urso_ema_update(n, ptr(w), ptr(ema), ptr(state), _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)),
         "urso_ema_update")


def ema_swap(n, a, b, stream=None):
    """urso_ema_swap (liburso_ext.so): exchange the bit patterns of the first n elements of two 4-byte-element buffers in place."""
    assert a.element_size() == 4 and b.element_size() == 4 and 0 <= n <= min(a.numel(), b.numel())
    _chk(side_lib("ext").urso_ema_swap(n, ptr(a), ptr(b), stream_ptr(stream)), "urso_ema_swap")


def grad_accum_parts(n):
    """urso_grad_accum_parts (liburso_ext.so): the slots urso_grad_accum_close writes for n elements (its block count; needs no GPU)."""
    return int(side_lib("ext").urso_grad_accum_parts(int(n)))


def sam_ascend(n, w, g, w0, state, stream=None):
    """urso_sam_ascend (liburso_train.so): w0 = w (the bits) and, where state's normsq is finite and > 0, w = w + s g over n fp32 elements
    with s = rho / (sqrtf(normsq) + eps); scale, applied and the counts go into state (ursonet_amd.sam.ascend32 / ascend_state32)."""
    assert all(x.dtype == torch.float32 for x in (w, g, w0, state)) and state.numel() >= SAM_STATE
    assert 0 <= n <= min(w.numel(), g.numel(), w0.numel())
    _chk(side_lib("train").urso_sam_ascend(n, ptr(w), ptr(g), ptr(w0), ptr(state), stream_ptr(stream)), "urso_sam_ascend")


def sam_descend(n, w, w0, stream=None):
    """urso_sam_descend (liburso_train.so): w = w0, the bits, over n 4-byte elements."""
    assert w.element_size() == 4 and w0.element_size() == 4 and 0 <= n <= min(w.numel(), w0.numel())
    _chk(side_lib("train").urso_sam_descend(n, ptr(w), ptr(w0), stream_ptr(stream)), "urso_sam_descend")


def sam_settle(state, normsq, guard=True, stream=None):
    """urso_sam_settle (liburso_train.so): a skipped step (guard and a non-finite normsq) takes its ascents out of applied_total; pending = 0
    (ursonet_amd.sam.settle32)."""
    assert state.dtype == torch.float32 and state.numel() >= SAM_STATE and normsq.dtype == torch.float32
    _chk(side_lib("train").urso_sam_settle(ptr(state), ptr(normsq), 1 if guard else 0, stream_ptr(stream)), "urso_sam_settle")


def swa_update(n, w, mean, sq, state, stream=None, ls=None):
    """urso_swa_update (liburso_train.so): on the steps the int32 state collects, w goes into the running mean (and w * w into sq, which may
    be None) over n fp32 elements; then the state advances (ursonet_amd.swa.collect32 / next_state on the device).  ls: the loss-scale
    state; a step it marks as skipped changes nothing."""
    assert w.dtype == torch.float32 and mean.dtype == torch.float32 and (sq is None or sq.dtype == torch.float32)
    assert state.dtype == torch.int32 and state.numel() >= SWA_STATE
    assert 0 <= n <= min(w.numel(), mean.numel()) and (sq is None or n <= sq.numel())
    _chk(side_lib("train").urso_swa_update(n, ptr(w), ptr(mean), ptr(sq) if sq is not None else None, ptr(state),
                                     _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)), "urso_swa_update")


def swag_sample(n, mean, sq, out, s, seed, sample, z_out=None, first=0, stream=None):
    """urso_swag_sample (liburso_train.so): out = mean + (s * sd) * z over n fp32 elements, sd = sqrtf(max(sq - mean * mean, 0)) and z the
    Philox normals of flat-buffer elements first .. first + n - 1 (ursonet_amd.swa.normals / sample32); z_out, when given, receives z."""
    assert all(x is None or x.dtype == torch.float32 for x in (mean, sq, out, z_out))
    assert 0 <= n <= min(x.numel() for x in (mean, sq, out) + ((z_out,) if z_out is not None else ()))
    _chk(side_lib("train").urso_swag_sample(n, int(first), ptr(mean), ptr(sq), ptr(out), ptr(z_out) if z_out is not None else None, float(s),
                                      int(seed), int(sample), stream_ptr(stream)), "urso_swag_sample")


def ens_add(B, n, row0, logits, acc, stat, first, stream=None):
    """urso_ens_add (liburso_train.so): the softmax of the n valid rows of logits (fp32 [B, K] with contiguous rows; a view of the engine's
    output is fine) goes into rows row0 .. of acc (fp64 [rows, K]) and its entropy into stat (fp64 [rows, ENS_STAT]); first overwrites
    (ursonet_amd.ensemble.add64)."""
    assert logits.dtype == torch.float32 and acc.dtype == torch.float64 and stat.dtype == torch.float64
    assert acc.is_contiguous() and stat.is_contiguous() and logits.shape[0] >= B and acc.shape[1] == logits.shape[1] and stat.shape[1] == ENS_STAT
    assert 0 <= n <= B and row0 >= 0 and row0 + n <= min(acc.shape[0], stat.shape[0])
    a = EnsAddArgs()
    a.B, a.n, a.row0, a.K, a.first, a.pad = int(B), int(n), int(row0), int(logits.shape[1]), 1 if first else 0, 0
    a.logits, a.ld = _rows(logits)
    a.acc, a.stat = ptr(acc), ptr(stat)
    _chk(side_lib("train").urso_ens_add(C.byref(a), stream_ptr(stream)), "urso_ens_add")


def ens_settle(n, row0, M, acc, stat, logp, table, stream=None):
    """urso_ens_settle (liburso_train.so): rows row0 .. row0 + n - 1 of acc / stat over M members become logp (fp32 [>= n, K], this chunk's
    rows) and rows row0 .. of table (fp64 [rows, ENS_COLS]) (ursonet_amd.ensemble.settle64)."""
    assert acc.dtype == torch.float64 and stat.dtype == torch.float64 and table.dtype == torch.float64 and logp.dtype == torch.float32
    assert acc.is_contiguous() and stat.is_contiguous() and table.is_contiguous() and logp.is_contiguous()
    assert logp.shape[1] == acc.shape[1] and stat.shape[1] == ENS_STAT and table.shape[1] == ENS_COLS
    assert 0 <= n <= logp.shape[0] and row0 >= 0 and row0 + n <= min(acc.shape[0], stat.shape[0], table.shape[0])
    a = EnsSettleArgs()
    a.n, a.row0, a.K, a.M = int(n), int(row0), int(acc.shape[1]), int(M)
    a.acc, a.stat, a.logp, a.table = ptr(acc), ptr(stat), ptr(logp), ptr(table)
    _chk(side_lib("train").urso_ens_settle(C.byref(a), stream_ptr(stream)), "urso_ens_settle")


def _betas(field, betas):
    J = len(betas)
    assert 1 <= J <= TEMP_MAX_J
    for j in range(TEMP_MAX_J):
        field[j] = float(betas[j]) if j < J else 0.0
    return J


def temp_stats(B, n, row0, betas, logits, target, out, stream=None):
    """urso_temp_stats (liburso_train.so): for the n valid rows of logits and target (fp32 [B, K] with contiguous rows) the fp64 statistics
    {SY, YZ, then LSE, M1, VAR per beta} of the cross-entropy at the 1 .. 8 inverse temperatures `betas` go into rows row0 .. of out
    (fp64 [rows, TEMP_COLS]) (ursonet_amd.calibrate.stats64)."""
    assert logits.dtype == torch.float32 and target.dtype == torch.float32 and out.dtype == torch.float64 and out.is_contiguous()
    assert logits.shape[0] >= B and target.shape[0] >= B and logits.shape[1] == target.shape[1] and out.shape[1] == TEMP_COLS
    assert 0 <= n <= B and row0 >= 0 and row0 + n <= out.shape[0]
    a = TempStatsArgs()
    a.B, a.n, a.row0, a.K = int(B), int(n), int(row0), int(logits.shape[1])
    a.J = _betas(a.beta, betas)
    a.logits, a.ld_z = _rows(logits)
    a.target, a.ld_y = _rows(target)
    a.out = ptr(out)
    _chk(side_lib("train").urso_temp_stats(C.byref(a), stream_ptr(stream)), "urso_temp_stats")


def temp_reduce(N, betas, rows, totals, stream=None):
    """urso_temp_reduce (liburso_train.so): totals[j] = {sum CE, sum g, sum h, rows that are not finite} over rows 0 .. N - 1 of a table of
    temp_stats written with the same betas; totals fp64 [TEMP_MAX_J, TEMP_TOTALS] (ursonet_amd.calibrate.reduce64)."""
    assert rows.dtype == torch.float64 and totals.dtype == torch.float64 and rows.is_contiguous() and totals.is_contiguous()
    assert rows.shape[1] == TEMP_COLS and tuple(totals.shape) == (TEMP_MAX_J, TEMP_TOTALS) and 1 <= N <= rows.shape[0]
    a = TempReduceArgs()
    a.N, a.pad = int(N), 0
    a.J = _betas(a.beta, betas)
    a.rows, a.totals = ptr(rows), ptr(totals)
    _chk(side_lib("train").urso_temp_reduce(C.byref(a), stream_ptr(stream)), "urso_temp_reduce")


def temp_scale(B, n, beta, src, dst, stream=None):
    """urso_temp_scale (liburso_train.so): dst = fl32(src * beta) over the n valid rows of fp32 [B, K] tensors with contiguous rows
    (ursonet_amd.calibrate.scale32)."""
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.shape[1] == dst.shape[1]
    assert 0 <= n <= B and src.shape[0] >= B and dst.shape[0] >= B
    a = TempScaleArgs()
    a.B, a.n, a.K, a.pad, a.beta = int(B), int(n), int(src.shape[1]), 0, float(beta)
    a.in_, a.ld_in = _rows(src)
    a.out, a.ld_out = _rows(dst)
    _chk(side_lib("train").urso_temp_scale(C.byref(a), stream_ptr(stream)), "urso_temp_scale")


def _conf_args(a, B, n, row0, metric, logits, bin_map, est, out):
    """The fields urso_conf_score_args and urso_conf_bound_args share."""
    D = 4 if metric == CONF_ANGLE else 3
    assert metric in (CONF_ANGLE, CONF_EUCLID) and logits.dtype == torch.float32 and logits.shape[0] >= B and 0 <= n <= B and row0 >= 0
    assert bin_map.dtype == (torch.float32 if metric == CONF_ANGLE else torch.float64) and bin_map.is_contiguous()
    assert tuple(bin_map.shape) == (logits.shape[1], D), "the bin map does not fit the logits"
    assert est.dtype == torch.float64 and est.shape[1] == D and row0 + n <= min(est.shape[0], out.shape[0])
    assert out.dtype == torch.float64 and out.is_contiguous() and out.shape[1] == CONF_COLS
    a.B, a.n, a.row0, a.K, a.metric = int(B), int(n), int(row0), int(logits.shape[1]), int(metric)
    a.logits, a.ld_z = _rows(logits)
    a.est, a.ld_est = _rows(est)
    a.map, a.out = ptr(bin_map), ptr(out)
    return a, D


def conf_score(B, n, row0, metric, logits, bin_map, est, ref, out, stream=None):
    """urso_conf_score (liburso_infer.so): for the n valid rows of logits (fp32 [B, K] with contiguous rows) the mass of the bins strictly
    closer to est than the truth is, into rows row0 .. of out (fp64 [rows, CONF_COLS]).  est: fp64 [rows, 4 | 3] with contiguous rows (a
    column slice of a table is fine), row row0 + b for batch row b; ref: fp64 [B, 4 | 3], the truth; bin_map: fp32 [K, 4] (CONF_ANGLE) or
    fp64 [K, 3] (CONF_EUCLID) (ursonet_amd.conformal.score64)."""
    a, D = _conf_args(ConfScoreArgs(), B, n, row0, metric, logits, bin_map, est, out)
    assert ref.dtype == torch.float64 and ref.shape[0] >= B and ref.shape[1] == D
    a.ref, a.ld_ref = _rows(ref)
    a.pad = 0
    _chk(side_lib("infer").urso_conf_score(C.byref(a), stream_ptr(stream)), "urso_conf_score")


def conf_bound(B, n, row0, metric, q, logits, bin_map, est, out, stream=None):
    """urso_conf_bound (liburso_infer.so): for the n valid rows of logits the smallest ball around est that holds more than q of the PMF's
    mass, into rows row0 .. of out (fp64 [rows, CONF_COLS]); arguments as conf_score's, q > 0 (ursonet_amd.conformal.bound64)."""
    a, _D = _conf_args(ConfBoundArgs(), B, n, row0, metric, logits, bin_map, est, out)
    a.q = float(q)
    _chk(side_lib("infer").urso_conf_bound(C.byref(a), stream_ptr(stream)), "urso_conf_bound")


def feat_pool(B, n, row0, grid, act, out, stream=None):
    """urso_feat_pool (liburso_feat.so): the cell means of the n valid batch rows of act ([B, h, w, C] in the engine's dtype, contiguous)
    over the grid (gh, gw) into rows row0 .. of out (fp64 [rows, >= D] with contiguous rows) (ursonet_amd.domain.pool64)."""
    assert act.dim() == 4 and act.is_contiguous() and act.shape[0] >= B and act.dtype in DT_OF_TORCH and 0 <= n <= B and row0 >= 0
    assert out.dtype == torch.float64 and row0 + n <= out.shape[0]
    a = FeatPoolArgs()
    a.B, a.n, a.row0, (a.gh, a.gw), a.dtype = int(B), int(n), int(row0), (int(grid[0]), int(grid[1])), DT_OF_TORCH[act.dtype]
    a.h, a.w, a.C = (int(v) for v in act.shape[1:])
    a.act = ptr(act)
    a.out, a.ld = _rows(out)
    assert out.shape[1] >= a.gh * a.gw * a.C, "the table is narrower than the feature row"
    _chk(side_lib("feat").urso_feat_pool(C.byref(a), stream_ptr(stream)), "urso_feat_pool")


def feat_gram_add(B, n, row0, x, centre, s, g, stream=None):
    """urso_feat_gram_add (liburso_feat.so): rows [row0, row0 + n) of x (fp64 [rows, >= D], contiguous rows), centred on `centre` [D], into
    the sums s [D] and the upper triangle of g (fp64 [D, >= D], contiguous rows) (ursonet_amd.domain.gram_add64)."""
    D = int(s.numel())
    assert all(t.dtype == torch.float64 for t in (x, centre, s, g)) and 0 <= n <= B and row0 >= 0 and row0 + n <= x.shape[0]
    assert centre.numel() == D and x.shape[1] >= D and g.shape[0] >= D and g.shape[1] >= D
    a = FeatGramArgs()
    a.B, a.n, a.row0, a.D, a.pad = int(B), int(n), int(row0), D, 0
    a.x, a.ld_x = _rows(x)
    a.g, a.ld_g = _rows(g)
    a.centre, a.s = ptr(centre), ptr(s)
    _chk(side_lib("feat").urso_feat_gram_add(C.byref(a), stream_ptr(stream)), "urso_feat_gram_add")


def feat_whiten_t(W, device):
    """The storage urso_feat_maha reads: a lower-triangular whitening matrix W [D, D] (host, fp64) transposed, on the device."""
    import numpy as np
    return torch.as_tensor(np.ascontiguousarray(np.asarray(W, dtype=np.float64).T)).to(device).contiguous()


def feat_maha(B, n, row0, x, mean, wt, out, stream=None):
    """urso_feat_maha (liburso_feat.so): the n valid rows of x (fp64 [B, >= D], the batch's feature rows) against mean [D] and wt
    (feat_whiten_t: W transposed, [D, >= D]) into rows row0 .. of out (fp64 [rows, FEAT_COLS]) (ursonet_amd.domain.maha64)."""
    D = int(mean.numel())
    assert all(t.dtype == torch.float64 for t in (x, mean, wt, out)) and 0 <= n <= B and row0 >= 0 and x.shape[0] >= B and x.shape[1] >= D
    assert wt.shape[0] >= D and wt.shape[1] >= D and out.is_contiguous() and out.shape[1] == FEAT_COLS and row0 + n <= out.shape[0]
    a = FeatMahaArgs()
    a.B, a.n, a.row0, a.D, a.pad = int(B), int(n), int(row0), D, 0
    a.x, a.ld_x = _rows(x)
    a.wt, a.ld_w = _rows(wt)
    a.mean, a.out = ptr(mean), ptr(out)
    _chk(side_lib("feat").urso_feat_maha(C.byref(a), stream_ptr(stream)), "urso_feat_maha")


def occl_fill_u8(src, rects, fill, out, n=None, stream=None):
    """urso_occl_fill_u8 (liburso_explain.so): rows 0 .. n - 1 (default: one per rect) of out (uint8 [B, H, W, C], contiguous) become src
    (uint8 [H, W, C], contiguous, outside out) with rect j (int32 [>= n, 4] on the device: y0, x0, y1, x1) painted with fill[:C]; rows >= n
    stay (ursonet_amd.explain.occlude_host)."""
    n = int(rects.shape[0]) if n is None else int(n)
    assert src.dtype == out.dtype == torch.uint8 and rects.dtype == torch.int32 and src.dim() == 3 and out.dim() == 4
    assert tuple(out.shape[1:]) == tuple(src.shape) and rects.dim() == 2 and rects.shape[1] == 4 and 0 <= n <= min(out.shape[0], rects.shape[0])
    a = OcclFillArgs()
    a.B, a.n, (a.H, a.W, a.C) = int(out.shape[0]), n, (int(v) for v in src.shape)
    for c, v in enumerate(list(fill)[:4]):
        a.fill[c] = int(v)
    a.src, a.rects, a.out = ptr(src), ptr(rects), ptr(out)
    _chk(side_lib("explain").urso_occl_fill_u8(C.byref(a), stream_ptr(stream)), "urso_occl_fill_u8")


def occl_score(B, n, row0, dec0, dec, out, ori_z0=None, ori_z=None, loc_z0=None, loc_z=None, stream=None):
    """urso_occl_score (liburso_explain.so): table rows [row0, row0 + n) of dec (fp64 [rows, DEC_COLS]) against the baseline's DEC row dec0
    (fp64 [DEC_COLS]) and, per classification head given, the batch's logits z (fp32 [>= n, >= K], contiguous rows) against the
    baseline's z0 (fp32 [K]) into the same rows of out (fp64 [rows, OCCL_COLS]) (ursonet_amd.explain.score64).  Columns of an absent head
    keep what they held."""
    assert dec0.dtype == dec.dtype == out.dtype == torch.float64 and dec0.numel() == DEC_COLS and dec.shape[1] == DEC_COLS and out.shape[1] == OCCL_COLS
    assert 0 <= n <= B and row0 >= 0 and row0 + n <= min(dec.shape[0], out.shape[0])
    a = OcclScoreArgs()
    a.B, a.n, a.row0 = int(B), int(n), int(row0)
    for head, z0, z in (("ori", ori_z0, ori_z), ("loc", loc_z0, loc_z)):
        assert (z0 is None) == (z is None), "a head is its baseline logits and the batch's"
        K = 0
        if z0 is not None:
            K = int(z0.numel())
            assert z0.dtype == z.dtype == torch.float32 and z.shape[0] >= n and z.shape[1] >= K
        zp, ld = _rows(z)
        setattr(a, head + "_K", K)
        setattr(a, head + "_ld", int(ld))
        setattr(a, head + "_z0", ptr(z0))
        setattr(a, head + "_z", zp)
    a.dec0, a.dec, a.out = ptr(dec0), ptr(dec), ptr(out)
    _chk(side_lib("explain").urso_occl_score(C.byref(a), stream_ptr(stream)), "urso_occl_score")


def occl_splat(scores, cols, rects, window, out, stream=None):
    """urso_occl_splat (liburso_explain.so): the columns `cols` of scores (fp64 [>= P, ld], contiguous rows) of the P patches rects (int32
    [P, 4] on the device) into out (fp64 [M, h, w], contiguous), the maps of the window (y0, x0, y1, x1) (ursonet_amd.explain.splat64)."""
    wy0, wx0, wy1, wx1 = (int(v) for v in window)
    cols = [int(c) for c in cols]
    assert scores.dtype == out.dtype == torch.float64 and rects.dtype == torch.int32 and rects.dim() == 2 and rects.shape[1] == 4
    assert tuple(out.shape) == (len(cols), wy1 - wy0, wx1 - wx0) and scores.shape[0] >= rects.shape[0] and 1 <= len(cols) <= OCCL_MAX_MAPS
    a = OcclSplatArgs()
    a.P, a.M, a.wy0, a.wx0, a.h, a.w = int(rects.shape[0]), len(cols), wy0, wx0, wy1 - wy0, wx1 - wx0
    for m, c in enumerate(cols):
        a.cols[m] = c
    a.scores, a.ld = _rows(scores)
    a.rects, a.out = ptr(rects), ptr(out)
    _chk(side_lib("explain").urso_occl_splat(C.byref(a), stream_ptr(stream)), "urso_occl_splat")


def heat_overlay_u8(heat, lo, scale, lut, alpha, img, stream=None):
    """urso_heat_overlay_u8 (liburso_explain.so): heat (fp64 [h, w], contiguous) through lut (uint8 [256, 3]) onto img (uint8 [h, w, 3], the
    pixels of a row contiguous, any row stride) in place, at weight alpha / 256 (ursonet_amd.explain.overlay_host)."""
    h, w = (int(v) for v in heat.shape)
    assert heat.dtype == torch.float64 and lut.dtype == img.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and tuple(img.shape) == (h, w, 3)
    assert img.is_cuda and img.stride(2) == 1 and img.stride(1) == 3, "expected a device picture whose rows are contiguous"
    a = HeatOverlayArgs()
    a.h, a.w, a.alpha, a.pad, a.ld_img, a.lo, a.scale = h, w, int(alpha), 0, int(img.stride(0)), float(lo), float(scale)
    a.map, a.lut, a.img = ptr(heat), ptr(lut), img.data_ptr()
    _chk(side_lib("explain").urso_heat_overlay_u8(C.byref(a), stream_ptr(stream)), "urso_heat_overlay_u8")


def grad_accum(n, g, acc, first, stream=None):
    """urso_grad_accum (liburso_ext.so): acc = g (first: the bits) or acc += g over n fp32 elements (ursonet_amd.grad_accum.first32 / add32)."""
    assert g.dtype == torch.float32 and acc.dtype == torch.float32 and 0 <= n <= min(g.numel(), acc.numel())
    _chk(side_lib("ext").urso_grad_accum(n, ptr(g), ptr(acc), 1 if first else 0, stream_ptr(stream)), "urso_grad_accum")


def grad_accum_close(n, g, acc, c, sqpart, stream=None):
    """urso_grad_accum_close (liburso_ext.so): g = (acc + g) * c over n fp32 elements (ursonet_amd.grad_accum.close32) and, per block, the
    sum of squares of what it stored into sqpart (grad_accum_parts(n) slots, for sqnorm_final)."""
    assert g.dtype == torch.float32 and acc.dtype == torch.float32 and sqpart.dtype == torch.float32
    assert 0 <= n <= min(g.numel(), acc.numel())
    _chk(side_lib("ext").urso_grad_accum_close(n, ptr(g), ptr(acc), float(c), ptr(sqpart), sqpart.numel(), stream_ptr(stream)),
         "urso_grad_accum_close")


class LarsPlan(object):
    """The tables of the three LARS launches (urso_lars_norms / _trust / _sgd, liburso_ext.so; ursonet_amd/lars.py) for one list of tensors
    [(offset, numel, adapt)] of the flat buffers: the host copies the entry points check, the block map and first-slot table of
    urso_lars_plan, their device copies (uploaded once, here) and the launches' outputs part [NB][2] fp32, trust [T] fp32 and
    stat [T][3] fp64 = (|w|, |g|, q)."""

    def __init__(self, tensors, device):
        self.tensors = [(int(o), int(n), bool(a)) for o, n, a in tensors]
        T = self.T = len(self.tensors)
        self.off_h = (C.c_int64 * max(T, 1))(*[o for o, _, _ in self.tensors])
        self.n_h = (C.c_int64 * max(T, 1))(*[n for _, n, _ in self.tensors])
        lib = side_lib("ext")
        nb = lib.urso_lars_blocks(T, self.n_h)
        _chk(min(nb, 0), "urso_lars_blocks")
        self.nblocks = int(nb)
        blockmap = np.zeros((max(self.nblocks, 1), 2), dtype=np.int32)
        first = np.zeros(T + 1, dtype=np.int32)
        _chk(lib.urso_lars_plan(T, self.n_h, self.nblocks, blockmap.ctypes.data, first.ctypes.data), "urso_lars_plan")
        self.blockmap_h, self.first_h = blockmap[:self.nblocks], first
        tab = np.array([[o, n] for o, n, _ in self.tensors], dtype=np.int64).reshape(T, 2)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.tab = dev(tab) if T else torch.zeros(2, dtype=torch.int64, device=device)
        self.blockmap, self.first = dev(blockmap), dev(first)
        self.adapt = dev(np.array([1 if a else 0 for _, _, a in self.tensors] or [0], dtype=np.int32))
        self.part = torch.zeros(max(self.nblocks, 1), 2, dtype=torch.float32, device=device)
        self.trust = torch.ones(max(T, 1), dtype=torch.float32, device=device)
        self.stat = torch.zeros(max(T, 1), 3, dtype=torch.float64, device=device)

    def norms(self, w, g, stream=None):
        """part[b] = (sum of w^2, sum of g^2) over block b's chunk (ursonet_amd.lars.slot_sums32)."""
        assert w.dtype == torch.float32 and g.dtype == torch.float32
        _chk(side_lib("ext").urso_lars_norms(self.T, self.off_h, self.n_h, ptr(self.tab), ptr(self.blockmap), self.nblocks, ptr(w), ptr(g),
                                       ptr(self.part), stream_ptr(stream)), "urso_lars_norms")

    def trust_ratios(self, hyper, normsq, eta, eps, clip_mode, stream=None, ls=None):
        """trust[t] and stat[t] = (|w|, |g|, q) from the slots (ursonet_amd.lars.norms64 / trust32); ls: the loss-scaled form."""
        _chk(side_lib("ext").urso_lars_trust(self.T, ptr(self.first), ptr(self.adapt), self.nblocks, ptr(self.part), ptr(hyper), ptr(normsq),
                                       float(eta), float(eps), 1 if clip_mode else 0, ptr(self.trust), ptr(self.stat),
                                       _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)), "urso_lars_trust")

    def sgd(self, w, g, v, hyper, normsq, stream=None, ls=None):
        """The update with each tensor's trust (ursonet_amd.lars.update32); ls: the loss-scaled form."""
        assert w.dtype == torch.float32 and g.dtype == torch.float32 and v.dtype == torch.float32
        _chk(side_lib("ext").urso_lars_sgd(self.T, self.off_h, self.n_h, ptr(self.tab), ptr(self.blockmap), self.nblocks, ptr(w), ptr(g), ptr(v),
                                     ptr(self.trust), ptr(hyper), ptr(normsq), _ls_ptr(ls) if ls is not None else None,
                                     stream_ptr(stream)), "urso_lars_sgd")


class BnRecalLayer(C.Structure):
    """urso_bn_recal_layer (include/ursonet_train.h): one BN layer of the recalibration launches."""
    _fields_ = [("bmean", C.c_void_p), ("bvar", C.c_void_p), ("N", C.c_int64), ("M", C.c_int64), ("off_mean", C.c_int64), ("off_var", C.c_int64)]


class BnRecalPlan(object):
    """The table of the two BN recalibration launches (urso_bn_recal_add / _settle, liburso_train.so; ursonet_amd/bn_recal.py) for one list
    of layers [(bmean, bvar, M, off_mean, off_var)] -- float32 device tensors of N batch statistics over M pixels and the offsets of the
    layer's moving_mean / moving_variance slices in a statistics buffer of n_stats floats: the host copy the entry points check, its device
    copy (validated and uploaded once, here, by urso_bn_recal_plan), the float64 accumulator acc [n_stats] in the statistics buffer's layout
    (running mean where moving_mean lies, running m2 where moving_variance lies) and t, the number of batches added since reset()."""

    def __init__(self, layers, n_stats, device):
        self.layers = [(m, v, int(M), int(om), int(ov)) for m, v, M, om, ov in layers]      # (keeps the statistics tensors alive)
        L = self.L = len(self.layers)
        self.n_stats = int(n_stats)
        self.table_h = (BnRecalLayer * max(L, 1))()
        for row, (m, v, M, om, ov) in zip(self.table_h, self.layers):
            assert m.dtype == torch.float32 and v.dtype == torch.float32 and m.numel() == v.numel()
            row.bmean, row.bvar, row.N, row.M, row.off_mean, row.off_var = ptr(m), ptr(v), m.numel(), M, om, ov
        self.table = torch.zeros(max(L, 1) * C.sizeof(BnRecalLayer) // 8, dtype=torch.int64, device=device)
        _chk(side_lib("train").urso_bn_recal_plan(L, C.addressof(self.table_h), self.n_stats, ptr(self.table)), "urso_bn_recal_plan")
        self.acc = torch.zeros(max(self.n_stats, 1), dtype=torch.float64, device=device)
        self.t = 0

    def reset(self):
        """acc = 0, t = 0: nothing pooled."""
        self.acc.zero_()
        self.t = 0

    def add(self, stream=None):
        """One more batch: the layers' bmean / bvar as they are now go into acc (ursonet_amd.bn_recal.pool_add64); t advances."""
        _chk(side_lib("train").urso_bn_recal_add(self.L, C.addressof(self.table_h), ptr(self.table), self.n_stats, ptr(self.acc), self.t,
                                           stream_ptr(stream)), "urso_bn_recal_add")
        self.t += 1

    def settle(self, stats, stream=None):
        """stats[slices] = the pooled float32 statistics (ursonet_amd.bn_recal.pool_settle32); refused before anything was added."""
        assert stats.dtype == torch.float32 and stats.numel() >= self.n_stats
        _chk(side_lib("train").urso_bn_recal_settle(self.L, C.addressof(self.table_h), ptr(self.table), self.n_stats, ptr(self.acc), ptr(stats),
                                              self.t, stream_ptr(stream)), "urso_bn_recal_settle")


class LambPlan(object):
    """The three LAMB launches (urso_lamb_moments / _trust / _apply, liburso_opt.so; ursonet_amd/lamb.py) for one list of tensors
    [(offset, numel, adapt)] of the flat buffers.  The host tables, the block map and their device copies are a LarsPlan's (`tables`: the
    launches share the map of urso_lars_plan); the outputs are this plan's own: part [NB][2] fp32 = (sum w^2, sum r^2), trust [T] fp32,
    stat [T][3] fp64 = (|w|, |r|, q) and state [3] fp32 = {p1, p2, kt}."""

    def __init__(self, tensors, device):
        tb = self.tables = LarsPlan(tensors, device)
        self.tensors, self.T, self.nblocks, self.first_h, self.blockmap_h = tb.tensors, tb.T, tb.nblocks, tb.first_h, tb.blockmap_h
        self.tab, self.blockmap, self.first, self.adapt = tb.tab, tb.blockmap, tb.first, tb.adapt
        self.part, self.trust, self.stat = tb.part, tb.trust, tb.stat          # (allocated there, written by these launches alone)
        self.state = torch.tensor(LAMB_STATE_INIT, dtype=torch.float32, device=device)
        side_lib("opt")                                                            # a missing library is an error here, not at the first step

    def reset(self):
        """state = {1, 1, 0}: before the first step."""
        self.state.copy_(torch.tensor(LAMB_STATE_INIT, dtype=torch.float32))

    def moments(self, w, g, m, v, vhat, hyper, normsq, stream=None, ls=None):
        """The tick, then m, v, vhat and part[b] = (sum of w^2, sum of r^2) over block b's chunk (ursonet_amd.lamb.tick32 / moments32 /
        direction32); ls: the loss-scaled form."""
        assert all(x.dtype == torch.float32 for x in (w, g, m, v, vhat, hyper)) and hyper.numel() >= 8
        tb = self.tables
        _chk(side_lib("opt").urso_lamb_moments(self.T, tb.off_h, tb.n_h, ptr(self.tab), ptr(self.blockmap), self.nblocks, ptr(w), ptr(g), ptr(m),
                                         ptr(v), ptr(vhat), ptr(hyper), ptr(self.state), ptr(normsq), ptr(self.part),
                                         _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)), "urso_lamb_moments")

    def trust_ratios(self, normsq, eta, eps, clip_mode, stream=None, ls=None):
        """trust[t] and stat[t] = (|w|, |r|, q) from the slots (ursonet_amd.lars.norms64, ursonet_amd.lamb.trust32)."""
        _chk(side_lib("opt").urso_lamb_trust(self.T, ptr(self.first), ptr(self.adapt), self.nblocks, ptr(self.part), ptr(normsq), float(eta),
                                       float(eps), 1 if clip_mode else 0, ptr(self.trust), ptr(self.stat),
                                       _ls_ptr(ls) if ls is not None else None, stream_ptr(stream)), "urso_lamb_trust")

    def apply(self, w, m, vhat, hyper, normsq, stream=None, ls=None):
        """w = w - (lr * trust) * r with each tensor's trust (ursonet_amd.lamb.apply32)."""
        assert w.dtype == torch.float32 and m.dtype == torch.float32 and vhat.dtype == torch.float32
        tb = self.tables
        _chk(side_lib("opt").urso_lamb_apply(self.T, tb.off_h, tb.n_h, ptr(self.tab), ptr(self.blockmap), self.nblocks, ptr(w), ptr(m), ptr(vhat),
                                       ptr(self.trust), ptr(hyper), ptr(self.state), ptr(normsq), _ls_ptr(ls) if ls is not None else None,
                                       stream_ptr(stream)), "urso_lamb_apply")


def adam_amsgrad_clip(n, w, g, m, v, vhat, hyper, normsq, stream=None, ls=None):
    if ls is not None:
        _chk(_lib.urso_adam_amsgrad_clip_ls(n, ptr(w), ptr(g), ptr(m), ptr(v), ptr(vhat), ptr(hyper), ptr(normsq), _ls_ptr(ls),
                                            stream_ptr(stream)), "urso_adam_amsgrad_clip_ls")
        return
    _chk(_lib.urso_adam_amsgrad_clip(n, ptr(w), ptr(g), ptr(m), ptr(v), ptr(vhat), ptr(hyper), ptr(normsq), stream_ptr(stream)),
         "urso_adam_amsgrad_clip")


def scale_f32(n, x, s, stream=None):
    _chk(_lib.urso_scale_f32(n, ptr(x), s, stream_ptr(stream)), "urso_scale_f32")


def quat_wavg_decode(B, K, logits, hquat, q, a=None, stream=None):
    _chk(_lib.urso_quat_wavg_decode(B, K, ptr(logits), ptr(hquat), ptr(q), ptr(a), stream_ptr(stream)),
         "urso_quat_wavg_decode")


def quat_gmm_fit(B, K, x, is_pmf, hquat, var, nr_iterations, nr_max_modes, mean, var_out, prior, score, n_modes, stream=None):
    _chk(_lib.urso_quat_gmm_fit(B, K, ptr(x), int(bool(is_pmf)), ptr(hquat), float(var), int(nr_iterations), int(nr_max_modes), ptr(mean),
                                ptr(var_out), ptr(prior), ptr(score), ptr(n_modes), stream_ptr(stream)), "urso_quat_gmm_fit")


def _rows(t):
    """(device pointer, row stride in elements) of a 2-D tensor whose rows are contiguous (None -> (NULL, 0))."""
    if t is None:
        return None, 0
    assert t.is_cuda and t.dim() == 2 and t.stride(1) == 1, "expected a device tensor with contiguous rows"
    return t.data_ptr(), t.stride(0)


def _pose_args(a, B, n, row0, loc_mode, ori_mode, loc, ori, ori2, loc_map, table):
    """The fields urso_pose_eval_args and urso_pose_decode_args share."""
    a.B, a.n, a.row0, a.loc_mode, a.ori_mode = int(B), int(n), int(row0), int(loc_mode), int(ori_mode)
    a.loc, a.loc_ld = _rows(loc)
    a.ori, a.ori_ld = _rows(ori)
    a.ori2, a.loc_map, a.table = _rows(ori2)[0], ptr(loc_map), ptr(table)
    a.loc_map_rows = 0 if loc_map is None else loc_map.shape[0]
    a.loc_bins = loc.shape[1] if loc_mode == EVAL_LOC_CLASS else 0
    return a


def pose_eval(B, n, row0, loc_mode, ori_mode, loc, ori, loc_gt, q_gt, table, ori2=None, loc_map=None, ori_map=None, enc_loc=None,
              enc_ori=None, gmm_mean=None, gmm_nmodes=None, stream=None):
    """urso_pose_eval on one batch: loc / ori / ori2 are fp32 device tensors [B, width] with contiguous rows (views of the engine's
    outputs are fine), the rest contiguous; table is fp64 [rows, EVAL_COLS]."""
    a = _pose_args(PoseEvalArgs(), B, n, row0, loc_mode, ori_mode, loc, ori, ori2, loc_map, table)
    a.ori_map = ptr(ori_map)
    a.ori_map_rows = 0 if ori_map is None else ori_map.shape[0]
    a.ori_bins = 0 if enc_ori is None else enc_ori.shape[1]
    a.enc_loc, a.enc_ori, a.loc_gt, a.q_gt = ptr(enc_loc), ptr(enc_ori), ptr(loc_gt), ptr(q_gt)
    a.gmm_mean, a.gmm_nmodes = ptr(gmm_mean), ptr(gmm_nmodes)
    a.gmm_modes = 0 if gmm_mean is None else gmm_mean.shape[1]
    _chk(_lib.urso_pose_eval(C.byref(a), stream_ptr(stream)), "urso_pose_eval")


def pose_decode(B, n, row0, loc_mode, ori_mode, loc, ori, table, ori2=None, loc_map=None, ori_logits=None, ori_map_rows=0, ori_scatter=None,
                stream=None):
    """urso_pose_decode on one batch (no ground truth): loc / ori / ori2 / ori_logits are fp32 device tensors with contiguous rows,
    ori_scatter is urso_quat_wavg_decode's a_d [B, 16], ori_map_rows the rows of the bin map the logits index; table is fp64
    [rows, DEC_COLS]."""
    a = _pose_args(PoseDecodeArgs(), B, n, row0, loc_mode, ori_mode, loc, ori, ori2, loc_map, table)
    a.ori_logits, a.ori_logits_ld = _rows(ori_logits)
    a.ori_bins = 0 if ori_logits is None else ori_logits.shape[1]
    a.ori_map_rows = int(ori_map_rows)
    a.ori_scatter = ptr(ori_scatter)
    _chk(_lib.urso_pose_decode(C.byref(a), stream_ptr(stream)), "urso_pose_decode")


def pose_fuse_views(B, n, row0, est, r, qr, table, loc_gt=None, q_gt=None, est_view_rows=None, stream=None):
    """urso_pose_fuse_views (liburso_ext.so) on one batch: est is the fp64 device table of the per-view rows, contiguous rows, view v's
    block est_view_rows (default B) rows behind view v - 1's, LOC_EST / Q_EST at urso_pose_decode's columns; r [V,9] and qr [V,4] fp64
    device tensors (ursonet_amd/views.py); loc_gt / q_gt the truth or None; table is fp64 [rows, FUSE_COLS]."""
    assert est.dtype == torch.float64 and r.dtype == torch.float64 and qr.dtype == torch.float64 and table.dtype == torch.float64
    assert r.is_contiguous() and qr.is_contiguous() and table.is_contiguous() and r.shape[0] == qr.shape[0]
    a = PoseFuseViewsArgs()
    a.B, a.n, a.row0, a.V = int(B), int(n), int(row0), int(r.shape[0])
    a.est, a.est_ld = _rows(est)
    a.est_view_rows = int(B if est_view_rows is None else est_view_rows)
    assert est.shape[0] >= (a.V - 1) * a.est_view_rows + a.B and table.shape[0] >= a.row0 + a.n and table.shape[1] == FUSE_COLS
    a.r, a.qr, a.loc_gt, a.q_gt, a.table = ptr(r), ptr(qr), ptr(loc_gt), ptr(q_gt), ptr(table)
    _chk(side_lib("ext").urso_pose_fuse_views(C.byref(a), stream_ptr(stream)), "urso_pose_fuse_views")


def warp_perspective(B, H, W, Cc, interp, src, m, dst, stream=None):
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and m.dtype == torch.float64
    _chk(_lib.urso_warp_perspective(B, H, W, Cc, int(interp), ptr(src), ptr(m), ptr(dst), stream_ptr(stream)), "urso_warp_perspective")


def encode_ori(B, K, q, hquat, redundant, var, out, stream=None):
    assert q.dtype == torch.float64 and redundant.dtype == torch.uint8
    _chk(_lib.urso_encode_ori(B, K, ptr(q), ptr(hquat), ptr(redundant), float(var), ptr(out), stream_ptr(stream)), "urso_encode_ori")


def conv_pair_ok(M, dt, c_narrow, c_wide):
    return bool(_lib.urso_conv_pair_ok(int(M), dt, int(c_narrow), int(c_wide)))


def conv_pair(M, c_narrow, dt, mode, src, w1, bias1, add, bits, mid, w2, bias2, mask2, dst, add_hw=None, stream=None):
    """urso_conv_pair: two chained pointwise layers (c -> 4c (+add) -> c, c = 64 or 128) in one pass; mode 0 forward, 1 backward.
    add_hw = (H, W): `add` is the compact [B, H/2, W/2, 4c] gradient of a dense grid that is zero at odd rows / columns."""
    ah, aw = add_hw if add_hw else (0, 0)
    _chk(_lib.urso_conv_pair(int(M), int(c_narrow), dt, int(mode), ptr(src), ptr(w1), ptr(bias1), ptr(add), ptr(bits), ptr(mid), ptr(w2), ptr(bias2),
                             ptr(mask2), ptr(dst), int(ah), int(aw), stream_ptr(stream)), "urso_conv_pair")


def conv_pair_shortcut(M, dt, src, w1, bias1, xin, ws, bias_s, bits, mid, w2, bias2, dst, stream=None):
    """urso_conv_pair_shortcut: mid = relu(src W1^T + bias1 + xin Ws^T + bias_s), dst = relu(mid W2^T + bias2) (64 / 256 channels)."""
    _chk(_lib.urso_conv_pair_shortcut(int(M), dt, ptr(src), ptr(w1), ptr(bias1), ptr(xin), ptr(ws), ptr(bias_s), ptr(bits), ptr(mid), ptr(w2),
                                      ptr(bias2), ptr(dst), stream_ptr(stream)), "urso_conv_pair_shortcut")


def conv_dgrad_wgrad_pw(M, dt, dz, wd, x, mask_by_x, dx, part, colpart, part_stride, stream=None):
    """urso_conv_dgrad_wgrad_pw: dx = dz Wd^T (optionally masked by x > 0) and the split partials of dW = x^T dz, colsum (64 -> 256 layer)."""
    _chk(_lib.urso_conv_dgrad_wgrad_pw(int(M), dt, ptr(dz), ptr(wd), ptr(x), int(bool(mask_by_x)), ptr(dx), ptr(part), ptr(colpart),
                                       int(part_stride), stream_ptr(stream)), "urso_conv_dgrad_wgrad_pw")


def conv_pair_wgrad_entry(M, dt, src, w1, add, bits, w2, u, dst, ws, xin, mask_by_xin, dxin, part, colpart, part_s, colpart_s, part_stride, stream=None):
    """urso_conv_pair_wgrad_entry: backward pair + weight gradient of the block-closing layer + both gradients of the projection
    shortcut (dxin = mid Ws^T, dWs = xin^T mid); the 256-channel gradient mid never leaves the chip."""
    _chk(_lib.urso_conv_pair_wgrad_entry(int(M), dt, ptr(src), ptr(w1), ptr(add), ptr(bits), ptr(w2), ptr(u), ptr(dst), ptr(ws), ptr(xin), int(bool(mask_by_xin)), ptr(dxin),
                                         ptr(part), ptr(colpart), ptr(part_s), ptr(colpart_s), int(part_stride), stream_ptr(stream)),
         "urso_conv_pair_wgrad_entry")


def stem_conv_pool_ok(g, dt):
    """urso_stem_conv_pool_ok: does the packed stem geometry qualify for the fused conv1 + ReLU + max-pool kernel?"""
    return bool(_lib.urso_stem_conv_pool_ok(C.byref(g), dt))


def stem_conv_pool(g, dt, x, wf, bias, y_pooled, argmax, stream=None):
    """urso_stem_conv_pool: conv1 + ReLU + 3x3/s2 max-pool in one kernel; y_pooled [B][OH/2][OW/2][64], argmax its bytes."""
    _chk(_lib.urso_stem_conv_pool(C.byref(g), dt, ptr(x), ptr(wf), ptr(bias), ptr(y_pooled), ptr(argmax), stream_ptr(stream)), "urso_stem_conv_pool")


def stem_wgrad_pooled(g, dt, x, dpool, argmax, ws, dw_raw, colsum, stream=None):
    """urso_stem_wgrad_pooled: the stem's weight gradient from the max-pool output's gradient + arg-max bytes (no conv1-output gradient)."""
    _chk(_lib.urso_stem_wgrad_pooled(C.byref(g), dt, ptr(x), ptr(dpool), ptr(argmax), ptr(ws), ws.numel() * ws.element_size(), ptr(dw_raw),
                                     ptr(colsum), stream_ptr(stream)), "urso_stem_wgrad_pooled")


def conv_pair_wgrad_splits(M, dt):
    return int(_lib.urso_conv_pair_wgrad_splits(int(M), dt))


def conv_pair_wgrad(M, dt, src, w1, add, bits, mid, w2, u, dst, part, colpart, part_stride, add_hw=None, stream=None):
    """urso_conv_pair_wgrad: the stage-2 backward pair + fp32 partials of dW[64][256] / colsum[256] of the block-closing layer
    (x = u, dz = mid), one partial per block: part[s * part_stride + c * 256 + n], colpart[s * 256 + n]."""
    ah, aw = add_hw if add_hw else (0, 0)
    _chk(_lib.urso_conv_pair_wgrad(int(M), dt, ptr(src), ptr(w1), ptr(add), ptr(bits), ptr(mid), ptr(w2), ptr(u), ptr(dst), int(ah), int(aw),
                                   ptr(part), ptr(colpart), int(part_stride), stream_ptr(stream)), "urso_conv_pair_wgrad")


def conv_pointwise_sampled_ok(g, dt, flags, has_add=False):
    return bool(_lib.urso_conv_pointwise_sampled_ok(C.byref(g), dt, flags, int(bool(has_add))))


def conv_pointwise_sampled(g, dt, flags, src, wgt, bias, add, dst, bits_out, dst_sampled, stream=None):
    """urso_conv_pointwise_sampled: a stage-closing c -> 4c pointwise layer that also writes the even-row / even-column pixels of its output."""
    _chk(_lib.urso_conv_pointwise_sampled(C.byref(g), dt, flags, ptr(src), ptr(wgt), ptr(bias), ptr(add), ptr(dst), ptr(bits_out), ptr(dst_sampled),
                                          stream_ptr(stream)), "urso_conv_pointwise_sampled")


def zero_fill(t, stream=None):
    """urso_zero_fill: t[...] = 0 (16-byte aligned tensor whose size is a multiple of 16 bytes)."""
    _chk(_lib.urso_zero_fill(ptr(t), t.numel() * t.element_size(), stream_ptr(stream)), "urso_zero_fill")


def rows_expand2(B, H, W, row_bytes, src, dst, stream=None):
    """urso_rows_expand2: dst[b, y, x, :] = src[b, y/2, x/2, :] at even (y, x), zero elsewhere."""
    _chk(_lib.urso_rows_expand2(B, H, W, row_bytes, ptr(src), ptr(dst), stream_ptr(stream)), "urso_rows_expand2")


def rows_scatter2(B, H, W, row_bytes, src, dst, stream=None):
    """urso_rows_scatter2: dst[b, 2y, 2x, :] = src[b, y, x, :]; every other pixel of dst is left as it is (cleared once by the caller)."""
    _chk(_lib.urso_rows_scatter2(B, H, W, row_bytes, ptr(src), ptr(dst), stream_ptr(stream)), "urso_rows_scatter2")


def rows_subsample2(B, H, W, row_bytes, src, dst, stream=None):
    """urso_rows_subsample2: dst[b, y/2, x/2, :] = src[b, y, x, :] over per-pixel byte rows (ReLU bit masks)."""
    _chk(_lib.urso_rows_subsample2(B, H, W, row_bytes, ptr(src), ptr(dst), stream_ptr(stream)), "urso_rows_subsample2")


def encode_loc(B, K, loc, hmap, sig2, out, stream=None):
    """urso_encode_loc: loc fp64 [B,3], hmap fp64 [K,3] -> out fp32 [B,K] (utils.encode_loc utils.py:349-396)."""
    _chk(_lib.urso_encode_loc(B, K, ptr(loc), ptr(hmap), float(sig2), ptr(out), stream_ptr(stream)), "urso_encode_loc")


def rgb_to_grey3(B, H, W, src, dst, stream=None):
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8
    _chk(_lib.urso_rgb_to_grey3(B, H, W, ptr(src), ptr(dst), stream_ptr(stream)), "urso_rgb_to_grey3")


def sim2real_op(B, H, W, src, dst, op, par, seed, drop, drop_stride, stream=None):
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and op.dtype == torch.int32 and par.dtype == torch.float32
    assert seed.dtype == torch.int32, "seeds are passed as the bit pattern of uint32 in an int32 tensor"
    _chk(_lib.urso_sim2real_op(B, H, W, ptr(src), ptr(dst), ptr(op), ptr(par), ptr(seed), ptr(drop), int(drop_stride), stream_ptr(stream)),
         "urso_sim2real_op")


def pad_images_u8(B, H, W, Cc, OH, OW, top, left, src, dst, stream=None):
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8
    _chk(_lib.urso_pad_images_u8(B, H, W, Cc, OH, OW, int(top), int(left), ptr(src), ptr(dst), stream_ptr(stream)), "urso_pad_images_u8")


def resize_images_u8(B, H, W, Cc, NH, NW, OH, OW, top, left, ky, ry, kx, rx, y0, fy, x0, fx, trunc_passes, src, dst, stream=None):
    """urso_resize_images_u8: utils.resize_image of a uint8 batch [B,H,W,C] -> [B,OH,OW,C], byte-exact; the tables are device tensors built from
    utils.resize_tables (ky / kx None where the axis does not shrink)."""
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and y0.dtype == torch.int32 and x0.dtype == torch.int32
    assert all(t is None or t.dtype == torch.float64 for t in (ky, kx, fy, fx))
    _chk(_lib.urso_resize_images_u8(B, H, W, Cc, NH, NW, OH, OW, int(top), int(left), ptr(ky), int(ry), ptr(kx), int(rx), ptr(y0), ptr(fy), ptr(x0),
                                    ptr(fx), int(trunc_passes), ptr(src), ptr(dst), stream_ptr(stream)), "urso_resize_images_u8")


def frames_grey_flags_u8(B, HW, src, flags, stream=None):
    """urso_frames_grey_flags_u8: flags[b] (uint8 [B]) = 1 iff frame b of the uint8 batch src [B,HW,3] has R == G == B at every pixel."""
    assert src.dtype == torch.uint8 and flags.dtype == torch.uint8 and src.numel() >= B * HW * 3 and flags.numel() >= B
    _chk(_lib.urso_frames_grey_flags_u8(int(B), int(HW), ptr(src), ptr(flags), stream_ptr(stream)), "urso_frames_grey_flags_u8")


def frames_put_u8(B, HW, src, dst_addr, kind, stream=None):
    """urso_frames_put_u8: frame b of src [B,HW,3] -> device address dst_addr[b] (int64 tensor [B] holding the uint64 addresses); kind
    (uint8 [B]) 0 = channel 0 only, 1 = all three, 2 = skip.  The addresses are ursonet_amd.frame_cache.FrameCache's, nobody else's."""
    assert src.dtype == torch.uint8 and src.numel() >= B * HW * 3
    assert dst_addr.dtype == torch.int64 and dst_addr.numel() >= B and kind.dtype == torch.uint8 and kind.numel() >= B
    _chk(_lib.urso_frames_put_u8(int(B), int(HW), ptr(src), ptr(dst_addr), ptr(kind), stream_ptr(stream)), "urso_frames_put_u8")


def frames_gather_u8(B, HW, src_addr, kind, dst, stream=None):
    """urso_frames_gather_u8: slot b of dst [B,HW,3] <- device address src_addr[b]; kind 0 = grey plane expanded to RGB, 1 = copy, 2 = skip."""
    assert dst.dtype == torch.uint8 and dst.numel() >= B * HW * 3
    assert src_addr.dtype == torch.int64 and src_addr.numel() >= B and kind.dtype == torch.uint8 and kind.numel() >= B
    _chk(_lib.urso_frames_gather_u8(int(B), int(HW), ptr(src_addr), ptr(kind), ptr(dst), stream_ptr(stream)), "urso_frames_gather_u8")


DRAW_SEGMENT, DRAW_DISC, DRAW_MAX_PRIMS, DRAW_PRIM_INTS, DRAW_COORD_MAX = 0, 1, 16, 9, 16384       # include/ursonet_hip.h


def video_prep_u8(B, H, W, crop, pad, grey, src, dst, stream=None):
    """urso_video_prep_u8: crop (top, bottom, left, right) + zero pad + grey mix (three float64 weights) of a uint8 batch [B,H,W,3] ->
    dst [B, H - top - bottom + 2 pad, W - left - right + 2 pad, 3], with the bytes of ursonet_amd.video.VideoPrep.host."""
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8
    top, bottom, left, right = (int(v) for v in crop)
    w0, w1, w2 = (float(v) for v in grey)
    _chk(_lib.urso_video_prep_u8(int(B), int(H), int(W), top, bottom, left, right, int(pad), w0, w1, w2, ptr(src), ptr(dst), stream_ptr(stream)),
         "urso_video_prep_u8")


def draw_prims_u8(B, H, W, prims_host, counts_host, prims, counts, img, stream=None):
    """urso_draw_prims_u8: prims_host int32 ndarray [B,16,9] and counts_host int32 ndarray [B] (C-contiguous) are validated on the host,
    prims / counts are their device copies, img the uint8 batch [B,H,W,3] drawn onto in place."""
    assert prims_host.dtype == "int32" and counts_host.dtype == "int32" and prims_host.flags.c_contiguous and counts_host.flags.c_contiguous
    assert prims_host.shape == (B, DRAW_MAX_PRIMS, DRAW_PRIM_INTS) and counts_host.shape == (B,)
    assert prims.dtype == torch.int32 and counts.dtype == torch.int32 and img.dtype == torch.uint8
    assert prims.numel() == prims_host.size and counts.numel() == B and img.numel() == B * H * W * 3
    _chk(_lib.urso_draw_prims_u8(int(B), int(H), int(W), prims_host.ctypes.data, counts_host.ctypes.data, ptr(prims), ptr(counts), ptr(img),
                                 stream_ptr(stream)), "urso_draw_prims_u8")


def pmf_sheet_shape(n, cell, gap, rows):
    """(SH, SW) of urso_pmf_sheet_u8's picture for `rows` sources (1 or 2)."""
    return rows * n * cell + (rows + 1) * gap, n * n * cell + (n + 1) * gap


def pmf_sheet(B, n, cell, gap, gt, logits, lut, bg, out, scratch=None, stream=None):
    """urso_pmf_sheet_u8: the slice sheet of B orientation PMFs over n^3 bins -> out uint8 [B,SH,SW,3] ((SH, SW) = pmf_sheet_shape).
    gt (a stored PMF) and logits (the head's raw output) are fp32 [B, n^3] device tensors, either may be None; lut uint8 [256,3] on the
    device, bg three bytes.  out needs no alignment (a view into a larger buffer will do) but must be dense.  scratch: uint8, at least
    B * rows * n^3 bytes (allocated here when None).  Nothing is checked here that the library checks: bad arguments raise UrsoHipError
    before any launch."""
    rows = (gt is not None) + (logits is not None)
    K = int(n) ** 3
    assert all(t is None or t.dtype == torch.float32 for t in (gt, logits)) and (lut is None or lut.dtype == torch.uint8)
    assert out is None or out.dtype == torch.uint8
    if 1 <= B <= 65535 and 2 <= n <= 64 and out is not None:             # sizes the library accepts: the buffers must hold them
        if scratch is None:
            scratch = torch.empty(B * max(rows, 1) * K, dtype=torch.uint8, device=out.device)
        assert all(t is None or t.numel() >= B * K for t in (gt, logits)) and (lut is None or lut.numel() == 768)
        assert scratch.dtype == torch.uint8 and scratch.numel() >= B * rows * K
        sh, sw = pmf_sheet_shape(int(n), int(cell), int(gap), rows)
        assert sh * sw * 3 >= 2 ** 31 or out.numel() >= B * sh * sw * 3 or not (1 <= cell <= 64 and 0 <= gap <= 64)
    bg3 = (C.c_ubyte * 3)(*(int(v) & 255 for v in bg))
    _chk(_lib.urso_pmf_sheet_u8(int(B), int(n), int(cell), int(gap), ptr(gt), ptr(logits), ptr(lut), C.cast(bg3, C.c_void_p),
                                ptr(scratch), ptr(out), stream_ptr(stream)), "urso_pmf_sheet_u8")



def prof_enable(on):
    _lib.urso_prof_enable(int(on))


def prof_collect(max_records=65536):
    buf = (ProfRecord * max_records)()
    n = _lib.urso_prof_collect(buf, max_records)
    return [(buf[i].kernel_id, buf[i].ms, buf[i].flops, buf[i].bytes) for i in range(n)]


def prof_collect_ex(max_records=65536):
    """[(kernel_id, ms, flops, bytes, n_launches, symbol)]: symbol = the device symbol of the first kernel the call launched
    (hipKernelNameRefByPtr: what rocprofv3 --kernel-trace prints)."""
    buf = (ProfRecordEx * max_records)()
    n = _lib.urso_prof_collect_ex(buf, max_records)
    return [(buf[i].kernel_id, buf[i].ms, buf[i].flops, buf[i].bytes, buf[i].n_launches, buf[i].symbol.decode(errors="replace")) for i in range(n)]


def prof_collect_l2(max_records=65536):
    """prof_collect_ex with the L2 -> LDS / register bytes of each call appended: [(kernel_id, ms, flops, bytes, n_launches, symbol, l2_bytes)]."""
    buf = (ProfRecordEx * max_records)()
    n = _lib.urso_prof_collect_ex(buf, max_records)
    return [(buf[i].kernel_id, buf[i].ms, buf[i].flops, buf[i].bytes, buf[i].n_launches, buf[i].symbol.decode(errors="replace"), buf[i].l2_bytes)
            for i in range(n)]


COMM_ID_BYTES = 128


def comm_unique_id():
    """urso_comm_unique_id: the 128 bytes rank 0 creates and every rank passes to Comm()."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _chk(_lib.urso_comm_unique_id(C.cast(buf, C.c_void_p)), "urso_comm_unique_id")
    return buf.raw


class Comm(object):
    """urso_comm_*: bucketed gradient averaging over RCCL on the communicator's own stream (include/ursonet_hip.h)."""

    def __init__(self, world, rank, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        h = C.c_void_p()
        self._id = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _chk(_lib.urso_comm_init(C.byref(h), int(world), int(rank), C.cast(self._id, C.c_void_p)), "urso_comm_init")
        self.h, self.world, self.rank = h, int(world), int(rank)

    @classmethod
    def from_torch_group(cls, group=None):
        """One communicator over the ranks of an initialised torch.distributed group (the id travels through that group)."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        t = torch.tensor(list(comm_unique_id()) if rank == 0 else [0] * COMM_ID_BYTES, dtype=torch.uint8, device=dev)
        dist.broadcast(t, src=0, group=group)
        return cls(world, rank, bytes(t.cpu().tolist()))

    def allreduce_bucket(self, t, stream=None):
        """In-place average of tensor t (fp32 / bf16 / fp16, contiguous) after the work already on `stream` (default: current)."""
        _chk(_lib.urso_comm_allreduce_bucket(self.h, ptr(t), t.numel(), DT_OF_TORCH[t.dtype], stream_ptr(stream)), "urso_comm_allreduce_bucket")

    def wait(self, stream=None):
        _chk(_lib.urso_comm_wait(self.h, stream_ptr(stream)), "urso_comm_wait")

    def close(self):
        if self.h:
            _lib.urso_comm_destroy(self.h)
            self.h = None
