"""ctypes binding of libsimt_hip.so (the C ABI declared in include/simt_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails, this raises.
Build it with `python -c "import __graft_entry__ as g; g.build()"` or `simt_amd/csrc/build.sh`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SIMT_LIB_PATH") or os.path.join(_HERE, "libsimt_hip.so")      # SIMT_LIB_PATH: A/B a scratch build (measurements only)

SIMT_F32, SIMT_BF16 = 0, 1
MAX_TAPS = 36
ABI_VERSION = 2          # include/simt_hip.h SIMT_ABI_VERSION
QMAX = 40
CONF_BINS = 256          # include/simt_hip.h SIMT_CONF_BINS: confidence bins per class of simt_pseudo_conf*_u8

c_p = C.c_void_p
i32 = C.c_int32
f32 = C.c_float


class ConvDesc(C.Structure):
    _fields_ = [("x", c_p), ("w", c_p), ("y", c_p), ("bias", c_p), ("res", c_p), ("stats", c_p),
                ("B", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Ho", i32), ("Wo", i32), ("Cout", i32),
                ("Npad", i32), ("Nstore", i32), ("ldy", i32), ("ldr", i32), ("stride", i32), ("ntaps", i32),
                ("relu", i32), ("dtype_in", i32), ("dtype_out", i32), ("tile_n", i32),
                ("dy", C.c_int16 * MAX_TAPS), ("dx", C.c_int16 * MAX_TAPS), ("mask", c_p), ("ldm", i32),
                ("res_bits", c_p), ("bnr_y", c_p), ("bnr_mean", c_p), ("bnr_rstd", c_p), ("bnr_scale", c_p), ("bnr_shift", c_p),
                ("bnr_bits", c_p), ("bnr_part", c_p), ("bnr_mode", i32), ("bnr_ld", i32), ("w_frag", c_p), ("fbn", c_p),
                ("cu_budget", i32), ("reserved_", i32), ("in_scale", c_p), ("in_shift", c_p), ("in_out", c_p)]


FBN_BAR_WORDS = 144
FBN_ERR_WORD = 136


class FbnDesc(C.Structure):
    """simt_fbn_desc (include/simt_hip.h): the train-mode BatchNorm behind a conv, fused into the producing launch."""
    _fields_ = [("mode", i32), ("ldo", i32), ("out", c_p), ("work", c_p), ("gamma", c_p), ("beta", c_p),
                ("running_mean", c_p), ("running_var", c_p), ("momentum", f32), ("eps", f32),
                ("mean", c_p), ("rstd", c_p), ("scale", c_p), ("shift", c_p), ("coef", c_p), ("dgamma", c_p), ("dbeta", c_p),
                ("err", c_p)]


class WgradDesc(C.Structure):
    _fields_ = [("dy", c_p), ("x", c_p), ("slab", c_p),
                ("B", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Ho", i32), ("Wo", i32), ("Cd", i32), ("ldd", i32),
                ("stride", i32), ("ntaps", i32), ("nsplit", i32), ("dtype", i32),
                ("dy_", C.c_int16 * MAX_TAPS), ("dx_", C.c_int16 * MAX_TAPS)]


class WgradReduceJob(C.Structure):
    """simt_wgrad_reduce_job (include/simt_hip.h)."""
    _fields_ = [("slab", c_p), ("dst", c_p), ("nsplit", i32), ("Cd", i32), ("Ktot", i32), ("Cin", i32), ("co_off", i32),
                ("tap_off", i32), ("Cout", i32), ("RS", i32), ("accumulate", i32), ("block0", i32)]


class BnBwdDesc(C.Structure):
    _fields_ = [("dz", c_p), ("z", c_p), ("y", c_p), ("mean", c_p), ("rstd", c_p), ("scale", c_p), ("shift", c_p),
                ("y2", c_p), ("mean2", c_p), ("rstd2", c_p), ("scale2", c_p), ("part", c_p), ("coef", c_p),
                ("dy", c_p), ("dy2", c_p), ("gout", c_p), ("M", C.c_int64), ("C", i32), ("mask_mode", i32),
                ("dtype", i32), ("dgamma", c_p), ("dbeta", c_p), ("dgamma2", c_p), ("dbeta2", c_p), ("reduce_done_nblk", i32)]


class HeadDesc(C.Structure):
    _fields_ = [("pred1", c_p), ("pred2", c_p), ("fixp", c_p), ("label", c_p), ("T1", c_p), ("T2", c_p),
                ("part", c_p), ("keys", c_p), ("hout", c_p), ("g1", c_p), ("dpred1_f32", c_p), ("dpred2_f32", c_p),
                ("dpred1_t", c_p), ("dpred2_t", c_p),
                ("B", i32), ("h", i32), ("w", i32), ("H", i32), ("W", i32), ("C", i32), ("Q", i32), ("ldp", i32),
                ("ldf", i32), ("QP", i32), ("ld_f32", i32), ("ld_t", i32), ("grad_dtype", i32),
                ("th_high", f32), ("th_low", f32), ("lambda_seg", f32), ("lambda_place", f32), ("gscale", f32), ("mode", i32),
                ("single", i32), ("up_half_pixel", i32), ("fix_logits", i32), ("conf_out", c_p), ("label_ws", c_p)]


class StemDesc(C.Structure):
    """simt_stem_desc: the direct 7x7 stem convolution for up to two weight sets."""
    _fields_ = [("x", c_p), ("B", i32), ("H", i32), ("W", i32), ("Ho", i32), ("Wo", i32), ("nsets", i32),
                ("w", c_p * 2), ("y", c_p * 2), ("bias", c_p * 2), ("relu", i32 * 2), ("stats", c_p * 2)]


class NtmInnerDesc(C.Structure):
    _fields_ = [("ntm", c_p * 2), ("w", c_p * 2), ("ntm_grad", c_p * 2), ("w_m", c_p * 2), ("w_v", c_p * 2),
                ("T_out", c_p * 2), ("class_dist", c_p),
                ("Q", i32), ("C", i32), ("steps", i32), ("step0", i32),
                ("lr", f32), ("beta1", f32), ("beta2", f32), ("eps", f32), ("single", i32), ("skip_if", c_p)]


class NtmPostDesc(C.Structure):
    _fields_ = [("ntm", c_p * 2), ("w", c_p * 2), ("ntm_grad", c_p * 2), ("class_dist", c_p), ("hout", c_p),
                ("lout", c_p), ("Q", i32), ("C", i32),
                ("lambda_seg", f32), ("lambda_convex", f32), ("lambda_volume", f32), ("lambda_anchor", f32),
                ("gscale", f32), ("single", i32)]


class TapDesc(C.Structure):
    _fields_ = [("src", c_p), ("bias", c_p), ("dst", c_p),
                ("B", i32), ("H", i32), ("W", i32), ("Q", i32), ("QP", i32), ("lds", i32), ("ldd", i32), ("ntaps", i32),
                ("dy", C.c_int16 * MAX_TAPS), ("dx", C.c_int16 * MAX_TAPS)]


class SgdDesc(C.Structure):
    _fields_ = [("segs", c_p), ("chunks", c_p), ("nchunks", i32), ("chunk", i32), ("lr", f32 * 4), ("wd", f32 * 4),
                ("momentum", f32), ("dampening", f32), ("first_step", i32), ("skip_if", c_p)]


class AdamwDesc(C.Structure):
    """simt_adamw_desc (include/simt_hip.h): the multi-tensor AdamW launch."""
    _fields_ = [("segs", c_p), ("chunks", c_p), ("nchunks", i32), ("chunk", i32), ("step_size", f32 * 4), ("decay", f32 * 4),
                ("beta1", f32), ("beta2", f32), ("omb1", f32), ("omb2", f32), ("bc2s", f32), ("eps", f32), ("first_step", i32),
                ("skip_if", c_p)]


GATHER_MAX = 64          # include/simt_hip.h SIMT_GATHER_MAX


class GatherDesc(C.Structure):
    """simt_gather_desc (include/simt_hip.h): one batch of dataset-cache slots -> network input."""
    _fields_ = [("img", c_p * GATHER_MAX), ("lab", c_p * GATHER_MAX), ("mirror", C.c_uint8 * GATHER_MAX), ("x", c_p), ("lab_out", c_p),
                ("B", i32), ("h", i32), ("w", i32), ("mean", f32 * 3)]


SCALE_CROP_MAX = 64      # include/simt_hip.h SIMT_SCALE_CROP_MAX
SCALE_CROP_CHOICES = 16  # SIMT_SCALE_CROP_CHOICES
SCALE_CROP_LDS_MAX = 65536


class ScaleCropChoice(C.Structure):
    """simt_scale_crop_choice (include/simt_hip.h): one scale's sizes and the offsets of its six tables."""
    _fields_ = [("ws", i32), ("hs", i32), ("ksx", i32), ("ksy", i32), ("bounds_x", i32), ("coef_x", i32), ("bounds_y", i32),
                ("coef_y", i32), ("xtab", i32), ("ytab", i32)]


class ScaleCropDesc(C.Structure):
    """simt_scale_crop_desc (include/simt_hip.h): one batch of source frames -> scaled, cropped network input."""
    _fields_ = [("img", c_p * SCALE_CROP_MAX), ("lab", c_p * SCALE_CROP_MAX), ("ox", i32 * SCALE_CROP_MAX), ("oy", i32 * SCALE_CROP_MAX),
                ("choice", C.c_uint8 * SCALE_CROP_MAX), ("mirror", C.c_uint8 * SCALE_CROP_MAX), ("c", ScaleCropChoice * SCALE_CROP_CHOICES),
                ("tables", c_p), ("x", c_p), ("lab_out", c_p),
                ("B", i32), ("Hs", i32), ("Ws", i32), ("h", i32), ("w", i32), ("n_choices", i32), ("max_rows", i32), ("n_tables", i32),
                ("mean", f32 * 3)]


RARE_CROP_MAX = 16       # include/simt_hip.h SIMT_RARE_CROP_MAX
RARE_CROP_CANDS = 16     # SIMT_RARE_CROP_CANDS
RARE_CROP_PARTS = 16     # SIMT_RARE_CROP_PARTS


class RareCropDesc(C.Structure):
    """simt_rare_crop_desc (include/simt_hip.h): one batch of source frames and K candidate windows per item -> counts, pick, crop."""
    _fields_ = [("img", c_p * RARE_CROP_MAX), ("lab", c_p * RARE_CROP_MAX),
                ("cand_ox", (i32 * RARE_CROP_CANDS) * RARE_CROP_MAX), ("cand_oy", (i32 * RARE_CROP_CANDS) * RARE_CROP_MAX),
                ("cand_choice", (C.c_uint8 * RARE_CROP_CANDS) * RARE_CROP_MAX), ("mirror", C.c_uint8 * RARE_CROP_MAX),
                ("cls", C.c_uint8 * RARE_CROP_MAX), ("c", ScaleCropChoice * SCALE_CROP_CHOICES),
                ("tables", c_p), ("x", c_p), ("lab_out", c_p), ("parts", c_p), ("win", c_p),
                ("B", i32), ("Hs", i32), ("Ws", i32), ("h", i32), ("w", i32), ("n_choices", i32), ("max_rows", i32), ("n_tables", i32),
                ("K", i32), ("min_count", i32), ("mean", f32 * 3)]


CLASS_MIX_MAX = 32       # include/simt_hip.h SIMT_CLASS_MIX_MAX
CLASS_MIX_CLASSES = 32   # SIMT_CLASS_MIX_CLASSES
CLASS_MIX_PARTS = 64     # SIMT_CLASS_MIX_PARTS


class ClassMixDesc(C.Structure):
    """simt_class_mix_desc (include/simt_hip.h): one finished batch -> the class-mixed batch."""
    _fields_ = [("x", c_p), ("lab", c_p), ("x_out", c_p), ("lab_out", c_p), ("part", c_p),
                ("B", i32), ("h", i32), ("w", i32), ("n_classes", i32),
                ("partner", C.c_uint8 * CLASS_MIX_MAX), ("apply", C.c_uint8 * CLASS_MIX_MAX),
                ("rank", (C.c_uint8 * CLASS_MIX_CLASSES) * CLASS_MIX_MAX)]


ONLINE_LABEL_MAX_PARTS = 1024      # include/simt_hip.h SIMT_ONLINE_LABEL_MAX_PARTS


class ClassMixU8Desc(C.Structure):
    """simt_class_mix_u8_desc (include/simt_hip.h): a batch, its byte labels and their presence words -> the mixed batch and int64 labels."""
    _fields_ = [("x", c_p), ("lab8", c_p), ("x_out", c_p), ("lab_out", c_p), ("part", c_p),
                ("B", i32), ("h", i32), ("w", i32), ("n_classes", i32), ("rows", i32),
                ("partner", C.c_uint8 * CLASS_MIX_MAX), ("apply", C.c_uint8 * CLASS_MIX_MAX),
                ("rank", (C.c_uint8 * CLASS_MIX_CLASSES) * CLASS_MIX_MAX)]


HEAD_WEIGHTS_MAX = 64    # include/simt_hip.h SIMT_HEAD_WEIGHTS_MAX: the longest weight table of simt_head_*_weighted_n


class HeadEntropy(C.Structure):
    """simt_head_entropy (include/simt_hip.h): the weight and the exponent of the robust entropy term of simt_head_*_entropy."""
    _fields_ = [("lambda_ent", f32), ("eta", f32)]


class HeadUncertainty(C.Structure):
    """simt_head_uncertainty (include/simt_hip.h): the weight of the two KL regularisers of simt_head_*_uncertain."""
    _fields_ = [("lambda_kl", f32)]


class SourceMixDesc(C.Structure):
    """simt_source_mix_desc (include/simt_hip.h): a labelled source batch, a target batch and its teacher's byte labels -> the mixed batch."""
    _fields_ = [("xs", c_p), ("labs", c_p), ("part_s", c_p), ("xt", c_p), ("lab8", c_p), ("x_out", c_p), ("lab_out", c_p),
                ("B", i32), ("h", i32), ("w", i32), ("n_classes", i32),
                ("apply", C.c_uint8 * CLASS_MIX_MAX), ("rank", (C.c_uint8 * CLASS_MIX_CLASSES) * CLASS_MIX_MAX)]


PHOTOMETRIC_MAX = 32     # include/simt_hip.h SIMT_PHOTOMETRIC_MAX
PHOTOMETRIC_PARTS = 64   # SIMT_PHOTOMETRIC_PARTS


class PhotometricDesc(C.Structure):
    """simt_photometric_desc (include/simt_hip.h): one finished batch -> the colour-jittered, blurred batch."""
    _fields_ = [("x", c_p), ("x_out", c_p), ("part", c_p), ("inv", C.c_double),
                ("B", i32), ("h", i32), ("w", i32), ("mean", f32 * 3),
                ("fb", f32 * PHOTOMETRIC_MAX), ("fc", f32 * PHOTOMETRIC_MAX), ("omfc", f32 * PHOTOMETRIC_MAX),
                ("A", (f32 * 9) * PHOTOMETRIC_MAX), ("wk", (f32 * 6) * PHOTOMETRIC_MAX),
                ("jit", C.c_uint8 * PHOTOMETRIC_MAX), ("blur", C.c_uint8 * PHOTOMETRIC_MAX)]


PATCH_MASK_MAX = 16      # include/simt_hip.h SIMT_PATCH_MASK_MAX
PATCH_MASK_GRID = 32     # SIMT_PATCH_MASK_GRID


class PatchMaskDesc(C.Structure):
    """simt_patch_mask_desc (include/simt_hip.h): one finished batch -> the batch with the patches its row words name blanked."""
    _fields_ = [("x", c_p), ("x_out", c_p), ("B", i32), ("h", i32), ("w", i32), ("patch", i32),
                ("rows", (C.c_uint32 * PATCH_MASK_GRID) * PATCH_MASK_MAX)]


class EmaDesc(C.Structure):
    """simt_ema_desc (include/simt_hip.h): one weight-EMA update over a segment table, e <- e + omd * (w - e)."""
    _fields_ = [("segs", c_p), ("chunks", c_p), ("nchunks", i32), ("chunk", i32), ("omd", f32), ("skip_if", c_p)]


class BnFoldSeg(C.Structure):
    """simt_bn_fold_seg (include/simt_hip.h): one BatchNorm of a simt_bn_fold_multi launch."""
    _fields_ = [("gamma", c_p), ("beta", c_p), ("running_mean", c_p), ("running_var", c_p), ("scale", c_p), ("shift", c_p),
                ("C", i32), ("reserved_", i32)]


# the `segs` records of SgdDesc, AdamwDesc, EmaDesc and BnFoldDesc for simt_amd/multi_tensor.py, which builds the tables (csrc asserts the sizes)
SGD_SEG = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("mult", "<i4"), ("group", "<i4")])
ADAMW_SEG = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("pad", "<i4")])
EMA_SEG = np.dtype([("w", "<u8"), ("e", "<u8"), ("n", "<i8")])
BN_FOLD_SEG = np.dtype(BnFoldSeg)
assert (SGD_SEG.itemsize, ADAMW_SEG.itemsize, EMA_SEG.itemsize, BN_FOLD_SEG.itemsize) == (40, 48, 24, 56)


class BnFoldDesc(C.Structure):
    """simt_bn_fold_desc (include/simt_hip.h): every eval-mode BatchNorm fold of a plan in one launch; `segs` on the device, `segs_host` the
    same records in host memory (the refusals are decided on them)."""
    _fields_ = [("segs", c_p), ("segs_host", C.POINTER(BnFoldSeg)), ("chunks", c_p), ("nsegs", i32), ("nchunks", i32), ("chunk", i32),
                ("eps", f32)]


class OnlineLabelDesc(C.Structure):
    """simt_online_label_desc (include/simt_hip.h): a teacher's low-res map -> the int64 labels the head kernels read, and their counts."""
    _fields_ = [("fix", c_p), ("label", c_p), ("counts", c_p), ("B", i32), ("h", i32), ("w", i32), ("ld", i32), ("H", i32), ("W", i32),
                ("C", i32), ("family", i32), ("threshold", f32)]


class OnlineLabelCbDesc(C.Structure):
    """simt_online_label_cb_desc (include/simt_hip.h): simt_online_label with per-class thresholds read from device memory, and the
    confidence histogram of the same pass."""
    _fields_ = [("fix", c_p), ("label", c_p), ("counts", c_p), ("hist", c_p), ("thr", c_p), ("B", i32), ("h", i32), ("w", i32), ("ld", i32),
                ("H", i32), ("W", i32), ("C", i32), ("family", i32)]


class OnlineLabelU8Desc(C.Structure):
    """simt_online_label_u8_desc (include/simt_hip.h): simt_online_label with byte labels and the per-item class-presence words."""
    _fields_ = [("fix", c_p), ("lab8", c_p), ("counts", c_p), ("part", c_p), ("B", i32), ("h", i32), ("w", i32), ("ld", i32), ("H", i32),
                ("W", i32), ("C", i32), ("family", i32), ("threshold", f32)]


class OnlineLabelCbU8Desc(C.Structure):
    """simt_online_label_cb_u8_desc (include/simt_hip.h): simt_online_label_cb with byte labels and the presence words."""
    _fields_ = [("fix", c_p), ("lab8", c_p), ("counts", c_p), ("hist", c_p), ("thr", c_p), ("part", c_p), ("B", i32), ("h", i32), ("w", i32),
                ("ld", i32), ("H", i32), ("W", i32), ("C", i32), ("family", i32)]


class OnlineLabelWDesc(C.Structure):
    """simt_online_label_w_desc (include/simt_hip.h): simt_online_label that keeps every arg-max and counts the confident pixels per item."""
    _fields_ = [("fix", c_p), ("label", c_p), ("counts", c_p), ("conf_part", c_p), ("B", i32), ("h", i32), ("w", i32), ("ld", i32), ("H", i32),
                ("W", i32), ("C", i32), ("family", i32), ("threshold", f32)]


class OnlineLabelWU8Desc(C.Structure):
    """simt_online_label_w_u8_desc (include/simt_hip.h): the same with byte labels and the presence words."""
    _fields_ = [("fix", c_p), ("lab8", c_p), ("counts", c_p), ("part", c_p), ("conf_part", c_p), ("B", i32), ("h", i32), ("w", i32), ("ld", i32),
                ("H", i32), ("W", i32), ("C", i32), ("family", i32), ("threshold", f32)]


LABEL_QUALITY_MODES = {"item": 0, "batch": 1}      # simt_label_quality_desc.mode


class LabelQualityDesc(C.Structure):
    """simt_label_quality_desc (include/simt_hip.h): the per-item counts of confident pixels -> the weights q[B]."""
    _fields_ = [("conf_part", c_p), ("q", c_p), ("B", i32), ("rows", i32), ("H", i32), ("W", i32), ("mode", i32)]


class ClassThresholdsDesc(C.Structure):
    """simt_class_thresholds_desc (include/simt_hip.h): the histogram -> the batch thresholds, folded into the device thresholds; hist zeroed."""
    _fields_ = [("hist", c_p), ("thr", c_p), ("t_out", c_p), ("drop", C.c_double), ("C", i32), ("cap", f32), ("omd", f32)]


TTA_MAX = 8             # include/simt_hip.h SIMT_TTA_MAX


class TtaTerm(C.Structure):
    """simt_tta_term (include/simt_hip.h): one forward's low-res map of a test-time-augmentation label launch."""
    _fields_ = [("l", c_p), ("h", i32), ("w", i32), ("ld", i32), ("hi", i32), ("wi", i32), ("flip", i32)]


class TtaDesc(C.Structure):
    """simt_tta_desc (include/simt_hip.h)."""
    _fields_ = [("t", TtaTerm * TTA_MAX), ("n", i32), ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("mode", i32), ("threshold", f32),
                ("thr", c_p), ("pred", c_p), ("out", c_p), ("counts", c_p), ("hist", c_p)]


class FeatDistMaskDesc(C.Structure):
    """simt_feat_dist_mask_desc (include/simt_hip.h): int64 labels -> the byte map of the kept feature cells and their count per workgroup."""
    _fields_ = [("label", c_p), ("mask", c_p), ("part", c_p), ("classes", C.c_uint64), ("B", i32), ("H", i32), ("W", i32), ("h", i32), ("w", i32),
                ("min_ratio", f32)]


class FeatDistDesc(C.Structure):
    """simt_feat_dist_desc (include/simt_hip.h): two layer-4 maps and the mask -> distances, their gradient (the seed) and three scalars."""
    _fields_ = [("fs", c_p), ("fi", c_p), ("mask", c_p), ("kept_part", c_p), ("seed", c_p), ("d", c_p), ("part", c_p), ("out", c_p),
                ("lam", C.c_double), ("M", C.c_int64), ("C", i32), ("ld", i32), ("dtype", i32), ("n_kept_part", i32), ("lam_g", f32),
                ("reserved_", i32)]


FDA_MAX_ITEMS = 32       # include/simt_hip.h SIMT_FDA_MAX_ITEMS
FDA_MAX_BAND = 64        # SIMT_FDA_MAX_BAND


class FdaDesc(C.Structure):
    """simt_fda_desc (include/simt_hip.h): a source batch and a target batch -> the source batch with the target's low-band amplitudes."""
    _fields_ = [("xs", c_p), ("xt", c_p), ("x_out", c_p), ("tw_h", c_p), ("tw_w", c_p), ("work", c_p),
                ("B", i32), ("h", i32), ("w", i32), ("b", i32), ("mean", f32 * 3), ("reserved_", i32)]


PROTO_MAX_CLASSES = 64  # include/simt_hip.h SIMT_PROTO_MAX_CLASSES
PROTO_MAX_DIM = 4096    # SIMT_PROTO_MAX_DIM


class ProtoRectifyDesc(C.Structure):
    """simt_proto_rectify_desc (include/simt_hip.h): the teacher's features, its output and the prototypes -> the rectified map, byte labels
    at feature resolution and the count of moved cells per workgroup."""
    _fields_ = [("F", c_p), ("P", c_p), ("out", c_p), ("eta", c_p), ("n", c_p), ("lab", c_p), ("changed_part", c_p), ("M", C.c_int64),
                ("D", i32), ("ldF", i32), ("C", i32), ("ldp", i32), ("dtype", i32), ("family", i32), ("temp", f32), ("thr", f32)]


class ProtoAccDesc(C.Structure):
    """simt_proto_acc_desc (include/simt_hip.h): the features and the byte labels -> per-part class sums and counts in the workspace."""
    _fields_ = [("F", c_p), ("lab", c_p), ("ws", c_p), ("M", C.c_int64), ("D", i32), ("ldF", i32), ("C", i32), ("dtype", i32)]


class ProtoUpdateDesc(C.Structure):
    """simt_proto_update_desc (include/simt_hip.h): the workspace -> the prototypes' moving average and their update counts."""
    _fields_ = [("ws", c_p), ("eta", c_p), ("n", c_p), ("M", C.c_int64), ("D", i32), ("C", i32), ("momentum", C.c_double)]


class CellLabelsDesc(C.Structure):
    """simt_cell_labels_desc (include/simt_hip.h): int64 labels -> one byte label per feature cell and the count of seen-class cells per workgroup."""
    _fields_ = [("label", c_p), ("lab", c_p), ("part", c_p), ("n", c_p), ("B", i32), ("H", i32), ("W", i32), ("h", i32), ("w", i32), ("C", i32),
                ("min_ratio", f32), ("reserved_", i32)]


class ProtoContrastDesc(C.Structure):
    """simt_proto_contrast_desc (include/simt_hip.h): the student's layer-4 map, the cell labels and the prototypes -> the losses, their gradient
    (the seed) and three scalars."""
    _fields_ = [("fs", c_p), ("lab", c_p), ("eta", c_p), ("n", c_p), ("phat", c_p), ("hdr", c_p), ("seed", c_p), ("d", c_p), ("part", c_p),
                ("out", c_p), ("lam", C.c_double), ("M", C.c_int64), ("D", i32), ("C", i32), ("dtype", i32), ("temp", f32), ("lam_g", f32),
                ("reserved_", i32)]


# name -> (restype, argtypes); every symbol include/simt_hip.h declares
_L = C.c_long
_I = C.c_int
SIGNATURES = {
    "simt_last_error": (C.c_char_p, []),
    "simt_abi_version": (_I, []),
    "simt_conv_fprop": (_I, [C.POINTER(ConvDesc), c_p]),
    "simt_stem7_tiles": (_I, [_I, _I, _I]),
    "simt_stem7_pack": (_I, [c_p, c_p, c_p, c_p]),
    "simt_stem7_fwd": (_I, [C.POINTER(StemDesc), c_p]),
    "simt_stem7_wgrad_workgroups": (_I, [_I, _I, _I]),
    "simt_stem7_wgrad": (_I, [c_p, c_p, c_p, c_p, _I, _I, _I, _I, _I, c_p]),
    "simt_conv_mtiles": (_I, [C.POINTER(ConvDesc)]),
    "simt_conv_inbn_ok": (_I, [C.POINTER(ConvDesc)]),
    "simt_conv_fprop_pair": (_I, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), c_p]),
    "simt_conv_pair_fused": (_I, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "simt_conv_fbn_ok": (_I, [C.POINTER(ConvDesc)]),
    "simt_conv_epilogue_flavour": (_I, [C.POINTER(ConvDesc)]),
    "simt_conv_fbn_words": (_L, [C.POINTER(ConvDesc)]),
    "simt_conv_wants_frag": (_I, [C.POINTER(ConvDesc)]),
    "simt_conv_variant": (_I, [C.POINTER(ConvDesc), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "simt_conv_wgrad": (_I, [C.POINTER(WgradDesc), c_p]),
    "simt_wgrad_reduce": (_I, [c_p, c_p, _I, _I, _I, _I, _I, _I, _I, _I, _I, c_p]),
    "simt_conv_wgrad_multi_ok": (_I, [C.POINTER(WgradDesc)]),
    "simt_conv_wgrad_multi_bytes": (_I, []),
    "simt_conv_wgrad_multi_prepare": (_I, [C.POINTER(WgradDesc), _I, c_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "simt_conv_wgrad_multi": (_I, [c_p, _I, _I, _I, _I, c_p]),
    "simt_conv_wgrad_tile_co": (_I, [C.POINTER(WgradDesc)]),
    "simt_wgrad_reduce_multi": (_I, [c_p, _I, _I, c_p]),
    "simt_wgrad_reduce_blocks": (_I, [_I, _I, _I]),
    "simt_pack_weight": (_I, [c_p, c_p, _I, _I, _I, _I, _I, _L, _I, _I, c_p, _I, c_p]),
    "simt_pack_weight_multi": (_I, [c_p, c_p, _I, _I, c_p]),
    "simt_bn_fold": (_I, [c_p, c_p, c_p, c_p, f32, c_p, c_p, _I, c_p]),
    "simt_bn_finalize": (_I, [c_p, _I, _I, _L, c_p, c_p, c_p, c_p, f32, f32, c_p, c_p, c_p, c_p, c_p]),
    "simt_bn_apply": (_I, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, _L, _I, _I, _I, c_p]),
    "simt_bn_apply_bits": (_I, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, _L, _I, _I, _I, c_p]),
    "simt_bn_bwd_nblk": (_I, [_L, _I]),
    "simt_bn_bwd": (_I, [C.POINTER(BnBwdDesc), c_p]),
    "simt_im2col_stem": (_I, [c_p, c_p, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, c_p]),
    "simt_bn_relu_maxpool": (_I, [c_p, c_p, c_p, c_p, c_p, _I, _I, _I, _I, _I, _I, _I, c_p]),
    "simt_maxpool_bwd": (_I, [c_p, c_p, c_p, _I, _I, _I, _I, _I, _I, _I, c_p]),
    "simt_scatter_stride": (_I, [c_p, c_p, _I, _I, _I, _I, _I, _I, _I, _I, c_p]),
    "simt_colsum": (_I, [c_p, c_p, _L, _I, _I, _I, _I, c_p]),
    "simt_maxpool2": (_I, [c_p, c_p, c_p, _I, _I, _I, _I, _I, c_p]),
    "simt_maxpool2_bwd": (_I, [c_p, c_p, c_p, c_p, _I, _I, _I, _I, _I, c_p]),
    "simt_colsum_wide": (_I, [c_p, c_p, _L, _I, _I, _I, c_p]),
    "simt_head_nblk": (_I, [_I, _I, _I]),
    "simt_head_part_floats": (_I, [_I, _I]),
    "simt_head_hout_floats": (_I, [_I, _I]),
    "simt_head_keys_count": (_I, []),
    "simt_softmax_rows": (_I, [c_p, _I, c_p, _I, _L, _I, c_p]),
    "simt_head_loss": (_I, [C.POINTER(HeadDesc), c_p]),
    "simt_head_grad": (_I, [C.POINTER(HeadDesc), c_p]),
    "simt_head_loss_views": (_I, [C.POINTER(HeadDesc), c_p, c_p]),
    "simt_head_grad_views": (_I, [C.POINTER(HeadDesc), c_p, c_p]),
    "simt_ntm_inner_loop": (_I, [C.POINTER(NtmInnerDesc), c_p]),
    "simt_ntm_post": (_I, [C.POINTER(NtmPostDesc), c_p]),
    "simt_sig_ntm": (_I, [c_p, c_p, c_p, c_p, c_p, _I, _I, c_p]),
    "simt_sig_w": (_I, [c_p, c_p, c_p, c_p, _I, c_p]),
    "simt_adam_step": (_I, [c_p, c_p, c_p, c_p, _L, f32, f32, f32, f32, _I, c_p]),
    "simt_adam_step_guarded": (_I, [c_p, c_p, c_p, c_p, _L, f32, f32, f32, f32, _I, c_p, c_p]),
    "simt_sgd_multi": (_I, [C.POINTER(SgdDesc), c_p]),
    "simt_adamw_multi": (_I, [C.POINTER(AdamwDesc), c_p]),
    "simt_event_create": (_I, [C.POINTER(c_p), _I]),
    "simt_event_destroy": (_I, [c_p]),
    "simt_event_record": (_I, [c_p, c_p]),
    "simt_stream_wait_event": (_I, [c_p, c_p]),
    "simt_vec_acc": (_I, [c_p, c_p, _I, _I, c_p]),
    "simt_tap_gather_sum": (_I, [C.POINTER(TapDesc), c_p]),
    "simt_tap_scatter": (_I, [C.POINTER(TapDesc), c_p]),
    "simt_wgrad_reduce_exp": (_I, [c_p, c_p, _I, _I, _I, _I, _I, _I, _I, _I, c_p]),
    "simt_upsample_sum_argmax": (_I, [c_p, _I, _I, _I, c_p, _I, _I, _I, _I, _I, _I, _I, c_p, c_p]),
    "simt_confusion_hist": (_I, [c_p, c_p, _L, _I, c_p, c_p]),
    "simt_upsample2_sum_argmax": (_I, [c_p, _I, _I, _I, _I, _I, c_p, _I, _I, _I, _I, _I, _I, _I, _I, _I, c_p, c_p]),
    "simt_pseudo_label_u8": (_I, [c_p, _I, _I, _I, c_p, _I, _I, _I, _I, _I, _I, _I, _I, f32, c_p, c_p, c_p]),
    "simt_pseudo_label2_u8": (_I, [c_p, _I, _I, _I, _I, _I, c_p, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, f32, c_p, c_p, c_p]),
    "simt_pseudo_conf_u8": (_I, [c_p, _I, _I, _I, _I, _I, _I, _I, c_p, c_p, c_p, c_p, c_p]),
    "simt_pseudo_conf2_u8": (_I, [c_p, _I, _I, _I, _I, _I, _I, _I, _I, _I, c_p, c_p, c_p, c_p, c_p]),
    "simt_online_label": (_I, [C.POINTER(OnlineLabelDesc), c_p]),
    "simt_online_label_cb": (_I, [C.POINTER(OnlineLabelCbDesc), c_p]),
    "simt_class_thresholds": (_I, [C.POINTER(ClassThresholdsDesc), c_p]),
    "simt_online_label_parts": (_I, [C.POINTER(OnlineLabelU8Desc)]),
    "simt_online_label_u8": (_I, [C.POINTER(OnlineLabelU8Desc), c_p]),
    "simt_online_label_cb_u8": (_I, [C.POINTER(OnlineLabelCbU8Desc), c_p]),
    "simt_tta_label": (_I, [C.POINTER(TtaDesc), c_p]),
    "simt_upsample_nchw": (_I, [c_p, _I, _I, _I, _I, _I, _I, _I, _I, c_p, c_p]),
    "simt_upsample_nchw_bwd": (_I, [c_p, _I, _I, _I, _I, _I, _I, _I, _I, c_p, _I, c_p, c_p]),
    "simt_loss_ws_bytes": (_I, []),
    "simt_ce2d_fwd": (_I, [c_p, c_p, c_p, _I, _I, _I, _I, _I, _I, c_p, c_p, c_p]),
    "simt_ce2d_bwd": (_I, [c_p, c_p, c_p, _I, _I, _I, _I, _I, _I, c_p, c_p, c_p, c_p]),
    "simt_entropy2d": (_I, [c_p, _I, _I, _I, _I, c_p, c_p, c_p, c_p, c_p]),
    "simt_hist2d_u8": (_I, [c_p, c_p, _L, _I, _I, c_p, c_p, c_p]),
    "simt_resample_u8": (_I, [c_p, c_p, _I, _I, _I, _I, _I, _I, c_p, c_p, _I, c_p]),
    "simt_image_to_input": (_I, [c_p, c_p, _I, _I, _I, f32, f32, f32, _I, c_p]),
    "simt_label_nearest": (_I, [c_p, c_p, _I, _I, _I, _I, _I, c_p, c_p, _I, c_p]),
    "simt_label_nearest_u8": (_I, [c_p, c_p, _I, _I, _I, _I, _I, c_p, c_p, c_p]),
    "simt_cache_gather": (_I, [C.POINTER(GatherDesc), c_p]),
    "simt_scale_crop_lds_bytes": (_L, [C.POINTER(ScaleCropDesc)]),
    "simt_scale_crop": (_I, [C.POINTER(ScaleCropDesc), c_p]),
    "simt_label_presence": (_I, [c_p, _I, _L, _I, c_p, c_p]),
    "simt_class_mix": (_I, [C.POINTER(ClassMixDesc), c_p]),
    "simt_class_mix_items": (_I, [C.POINTER(ClassMixDesc), c_p, c_p]),
    "simt_class_mix_u8": (_I, [C.POINTER(ClassMixU8Desc), c_p]),
    "simt_grey_mean_parts": (_I, [C.POINTER(PhotometricDesc), c_p]),
    "simt_photometric": (_I, [C.POINTER(PhotometricDesc), c_p]),
    "simt_ema_multi": (_I, [C.POINTER(EmaDesc), c_p]),
    "simt_bn_fold_multi": (_I, [C.POINTER(BnFoldDesc), c_p]),
    "simt_patch_mask": (_I, [C.POINTER(PatchMaskDesc), c_p]),
    "simt_online_label_w": (_I, [C.POINTER(OnlineLabelWDesc), c_p]),
    "simt_online_label_w_u8": (_I, [C.POINTER(OnlineLabelWU8Desc), c_p]),
    "simt_label_quality": (_I, [C.POINTER(LabelQualityDesc), c_p]),
    "simt_head_loss_weighted": (_I, [C.POINTER(HeadDesc), c_p, c_p, c_p]),
    "simt_head_grad_weighted": (_I, [C.POINTER(HeadDesc), c_p, c_p, c_p]),
    "simt_class_mix_u8_items": (_I, [C.POINTER(ClassMixU8Desc), c_p, c_p]),
    "simt_source_mix": (_I, [C.POINTER(SourceMixDesc), c_p]),
    "simt_source_mix_items": (_I, [C.POINTER(SourceMixDesc), c_p, c_p]),
    "simt_head_loss_weighted_n": (_I, [C.POINTER(HeadDesc), c_p, C.c_int, c_p, c_p]),
    "simt_head_grad_weighted_n": (_I, [C.POINTER(HeadDesc), c_p, C.c_int, c_p, c_p]),
    "simt_head_loss_entropy": (_I, [C.POINTER(HeadDesc), c_p, C.c_int, c_p, C.POINTER(HeadEntropy), c_p]),
    "simt_head_grad_entropy": (_I, [C.POINTER(HeadDesc), c_p, C.c_int, c_p, C.POINTER(HeadEntropy), c_p]),
    "simt_head_loss_uncertain": (_I, [C.POINTER(HeadDesc), c_p, C.c_int, c_p, C.POINTER(HeadUncertainty), c_p]),
    "simt_head_grad_uncertain": (_I, [C.POINTER(HeadDesc), c_p, C.c_int, c_p, C.POINTER(HeadUncertainty), c_p]),
    "simt_rare_crop_counts": (_I, [C.POINTER(RareCropDesc), c_p]),
    "simt_rare_crop_pick": (_I, [C.POINTER(RareCropDesc), c_p]),
    "simt_scale_crop_win": (_I, [C.POINTER(RareCropDesc), c_p]),
    "simt_feat_dist_mask_parts": (_I, [_I, _I, _I]),
    "simt_feat_dist_parts": (_I, [_L]),
    "simt_feat_dist_mask": (_I, [C.POINTER(FeatDistMaskDesc), c_p]),
    "simt_feat_dist": (_I, [C.POINTER(FeatDistDesc), c_p]),
    "simt_feat_dist_finalize": (_I, [C.POINTER(FeatDistDesc), c_p]),
    "simt_fda_workspace_bytes": (_L, [_I, _I, _I, _I]),
    "simt_fda_transfer": (_I, [C.POINTER(FdaDesc), c_p]),
    "simt_proto_parts": (_I, [_L]),
    "simt_proto_ws_floats": (_L, [_L, _I, _I]),
    "simt_proto_rectify": (_I, [C.POINTER(ProtoRectifyDesc), c_p]),
    "simt_proto_accumulate": (_I, [C.POINTER(ProtoAccDesc), c_p]),
    "simt_proto_update": (_I, [C.POINTER(ProtoUpdateDesc), c_p]),
    "simt_cell_labels_parts": (_I, [_I, _I, _I]),
    "simt_proto_contrast_parts": (_I, [_L]),
    "simt_proto_contrast_phat_floats": (_L, [_I, _I]),
    "simt_cell_labels": (_I, [C.POINTER(CellLabelsDesc), c_p]),
    "simt_proto_contrast_prep": (_I, [C.POINTER(ProtoContrastDesc), c_p]),
    "simt_proto_contrast": (_I, [C.POINTER(ProtoContrastDesc), c_p]),
    "simt_proto_contrast_finalize": (_I, [C.POINTER(ProtoContrastDesc), c_p]),
}

_lib = None


class SimtHipError(RuntimeError):
    pass


def load():
    """Load libsimt_hip.so and bind every declared symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SimtHipError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Run `python -c 'import __graft_entry__ as g; g.build()'`.")
    # PyTorch-ROCm ships its own libamdhip64 (same soname); it must be mapped first so that this library binds to
    # the SAME HIP runtime instance that owns torch's streams and allocations (two runtimes in one process cannot
    # share stream handles: launches fail with "no ROCm-capable device").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:      # a library built before the symbol was added (the ABI version only counts layout changes)
            raise SimtHipError(f"{LIB_PATH} does not export {name}: it was built from older sources, rebuild it "
                               "(python -c 'import __graft_entry__ as g; g.build()')") from None
        fn.restype = res
        fn.argtypes = args
    if lib.simt_abi_version() != ABI_VERSION:      # a stale libsimt_hip.so reads past the end of the shorter descriptors it was built for
        raise SimtHipError(f"{LIB_PATH} has ABI version {lib.simt_abi_version()}, these bindings need {ABI_VERSION}: rebuild it "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().simt_last_error()
        raise SimtHipError(f"libsimt_hip call failed (code {rc}): {msg.decode() if msg else '?'}")


def call(name, *args):
    check(getattr(load(), name)(*args))
