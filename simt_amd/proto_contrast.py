"""Prototype contrastive loss on the student's layer-4 features (SePiCo, Xie et al., TPAMI'23; the second half of ProDA; keywords
`proto_contrast` / `proto_contrast_temp` / `proto_contrast_min_ratio` of WarmupTrainer, tool flags --proto-contrast / --proto-contrast-temp /
--proto-contrast-min-ratio).

Every other rule of the warm-up stage acts on the labels or on the logits; this one shapes the student's FEATURES.  With `proto_contrast=lambda`
every pass of a micro-batch -- the source pass of `online_source` and the target pass -- adds

    lambda * (1 / N) * sum over valid cells m of  -log softmax_seen( cos(f_m, eta_c) / T )[y_m]

f_m the student's layer-4 output row, eta_c the running class prototypes of `proto_denoise` (the keyword needs it; `proto_denoise=1e30`
leaves the labels all but untouched for a user who wants the contrast alone), y_m the class that fills the cell's window of `self.label` -- ground
truth, teacher labels, mixed labels or weighted mode's arg-max, as the pass holds them -- to `proto_contrast_min_ratio`.  The softmax runs over the
SEEN classes (a prototype exists) only; a cell is valid when it has a label whose class is seen; N, the number of valid cells, is rank-local as in
7.22.  Fewer than two seen classes, or N == 0: the term and its gradient are exactly 0 -- the very first micro-batch is the trainer without the
keyword apart from the seeded launch.  include/simt_hip.h states the contract; tests/_proto_contrast_ref.py restates it.  Per pass, on the main
stream, behind the point where `self.label` is final and in front of `plan.backward()`:

  1. `simt_cell_labels`: one byte label per layer-4 cell,
  2. `simt_proto_contrast_prep`: the normalised prototypes, the seen set and N,
  3. `simt_proto_contrast`: the losses and their gradient into EVERY row of `plan.feat_seed`, the `res` of the layer-4 head's input-gradient
     launch (TrunkPlan(feat_grad_seed=True), the route of 7.22), so the term reaches the trunk weights through the ordinary backward launches
     and the heads get none,
  4. `simt_proto_contrast_finalize`: three scalars; then `plan.use_feat_seed(True)`.

The keyword is refused beside `feat_dist` (both would write `feat_seed` in the source pass).  `losses()` gains `proto_contrast` (lambda * mean
loss of the last target pass, unscaled by iter_size like `feat_dist`), `proto_contrast_cells` (its N) and, with `online_source`,
`source_proto_contrast`; `total` keeps its meaning.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .feat_dist import DEFAULT_MIN_RATIO

DEFAULT_LAMBDA = 0.1           # conventional InfoNCE values, chosen here: NOT checked against SePiCo's published configuration
DEFAULT_TEMP = 0.1
MAX_CLASSES = L.PROTO_MAX_CLASSES
MAX_DIM = L.PROTO_MAX_DIM


def check_proto_contrast(proto_contrast, proto_contrast_temp, proto_contrast_min_ratio, proto_denoise, feat_dist, num_classes=None):
    """The three keywords -> (lambda | None, T, ratio); `proto_denoise` is check_proto's first value, `feat_dist` check_feat_dist's.  ValueError
    that starts with the keyword that does not fit.  lambda None: off (the other two must then be None: they would change nothing)."""
    if proto_contrast is None:
        for name, v in (("proto_contrast_temp", proto_contrast_temp), ("proto_contrast_min_ratio", proto_contrast_min_ratio)):
            if v is not None:
                raise ValueError(f"{name} needs proto_contrast: it belongs to the prototype contrastive term, and this trainer computes none")
        return None, None, None
    what = "expected the weight of the prototype contrastive term, a finite lambda >= 0"
    try:
        lam = float(proto_contrast)
    except (TypeError, ValueError):
        raise ValueError(f"proto_contrast {proto_contrast!r}: {what}") from None
    if isinstance(proto_contrast, bool) or not (0.0 <= lam < math.inf):          # (a NaN fails both comparisons)
        raise ValueError(f"proto_contrast {proto_contrast!r}: {what}")
    if proto_denoise is None:
        raise ValueError("proto_contrast needs proto_denoise: the prototypes are proto_denoise's (and hence online_labels'), and this trainer keeps "
                         "none (proto_denoise=1e30 leaves the labels all but untouched)")
    if feat_dist is not None:
        raise ValueError("proto_contrast with feat_dist: both write the gradient seed of layer 4's output in the source pass, and an accumulating "
                         "seed is not built")
    if num_classes is not None and not 2 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"proto_contrast with num_classes = {num_classes}: the launches take 2 to {MAX_CLASSES} classes")
    what = "expected the temperature of the cosine logits, a finite T > 0"
    if proto_contrast_temp is None:
        temp = DEFAULT_TEMP
    else:
        try:
            temp = float(proto_contrast_temp)
        except (TypeError, ValueError):
            raise ValueError(f"proto_contrast_temp {proto_contrast_temp!r}: {what}") from None
        if isinstance(proto_contrast_temp, bool) or not (1.0e-30 <= temp <= 3.0e38):          # (the launch takes a finite float32 > 0)
            raise ValueError(f"proto_contrast_temp {proto_contrast_temp!r}: {what}")
    what = "expected the share of a cell's label window one class must fill, 0.5 < R <= 1"
    if proto_contrast_min_ratio is None:
        ratio = DEFAULT_MIN_RATIO
    else:
        try:
            ratio = float(proto_contrast_min_ratio)
        except (TypeError, ValueError):
            raise ValueError(f"proto_contrast_min_ratio {proto_contrast_min_ratio!r}: {what}") from None
        if isinstance(proto_contrast_min_ratio, bool) or not (0.5 < ratio <= 1.0) or not (0.5 < float(np.float32(ratio)) <= 1.0):
            raise ValueError(f"proto_contrast_min_ratio {proto_contrast_min_ratio!r}: {what}")
    return lam, temp, ratio


def fill_cell_labels(label, lab, part, n, B, H, W, h, w, Cn, ratio):
    """simt_cell_labels_desc over device tensors (n None: every labelled cell counts)."""
    d = L.CellLabelsDesc()
    d.label, d.lab, d.part, d.n = label.data_ptr(), lab.data_ptr(), part.data_ptr(), None if n is None else n.data_ptr()
    d.B, d.H, d.W, d.h, d.w, d.C, d.min_ratio = B, H, W, h, w, Cn, ratio
    return d


def fill_contrast(fs, lab, eta, n, phat, hdr, seed, d_out, part, out, M, D, Cn, dtype, lam, temp, gscale):
    """simt_proto_contrast_desc over device tensors: the one descriptor of prep, the main launch and finalize."""
    d = L.ProtoContrastDesc()
    d.fs, d.lab, d.eta, d.n, d.phat, d.hdr = fs.data_ptr(), lab.data_ptr(), eta.data_ptr(), n.data_ptr(), phat.data_ptr(), hdr.data_ptr()
    d.seed, d.d, d.part, d.out = seed.data_ptr(), d_out.data_ptr(), part.data_ptr(), out.data_ptr()
    d.lam, d.M, d.D, d.C, d.dtype, d.temp = lam, M, D, Cn, ops.dt_code(dtype), temp
    d.lam_g = lam * gscale          # (float)(lambda * gscale), gscale as in the head descriptor
    return d


class ProtoContrastMixin:
    """The prototype contrastive term of WarmupTrainer: the buffers and descriptors of the four launches, the per-pass calls, the read-out."""

    def _init_proto_contrast(self, lam, temp, ratio):
        """lam None: off -- no buffer, no launch.  Behind the student's plan (built with feat_grad_seed=True), `self.label` and _init_proto."""
        self.proto_contrast = lam
        if lam is None:
            return
        self.proto_contrast_temp, self.proto_contrast_min_ratio = float(temp), float(ratio)
        dev, f32, plan = self.dev, torch.float32, self.plan
        fs = plan.block_io[-1]["z"]
        h, w = plan.feat_hw
        M, D = fs.shape
        assert M == self.B * h * w and fs.is_contiguous() and plan.feat_seed is not None and plan.feat_seed.shape == fs.shape
        if tuple(self.proto_eta.shape) != (self.C, D):
            raise ValueError(f"proto_contrast: the student's layer-4 output has {D} channels, the prototypes {self.proto_eta.shape[1]}")
        lib = L.load()
        n_lab, n_part, words = lib.simt_cell_labels_parts(self.B, h, w), lib.simt_proto_contrast_parts(M), lib.simt_proto_contrast_phat_floats(self.C, D)
        if n_lab < 1 or n_part < 1 or words < 1:
            raise L.SimtHipError(f"simt_cell_labels_parts / simt_proto_contrast_parts / _phat_floats: {n_lab} / {n_part} / {words} for B = {self.B}, "
                                 f"{h} x {w}, C = {self.C}, D = {D}")
        self.pc_lab = torch.zeros(M, device=dev, dtype=torch.uint8)
        self.pc_lab_part = torch.zeros(n_lab, device=dev, dtype=torch.int32)      # every word is written by every cell-label launch
        self.pc_phat = torch.zeros(words, device=dev, dtype=f32)                  # every word is written by every prep launch
        self.pc_hdr = torch.zeros(4, device=dev, dtype=torch.int32)
        self.pc_d = torch.zeros(M, device=dev, dtype=f32)
        self.pc_part = torch.zeros(n_part, device=dev, dtype=f32)
        self.pc_out = torch.zeros(3, device=dev, dtype=f32)
        self.pc_source_out = torch.zeros(3, device=dev, dtype=f32)                # the source pass's scalars (online_source), copied behind its finalize
        self.pc_lab_desc = fill_cell_labels(self.label, self.pc_lab, self.pc_lab_part, self.proto_n, self.B, self.H, self.W, h, w, self.C, ratio)
        self.pc_desc = fill_contrast(fs, self.pc_lab, self.proto_eta, self.proto_n, self.pc_phat, self.pc_hdr, plan.feat_seed, self.pc_d,
                                     self.pc_part, self.pc_out, M, D, self.C, self.dtype, lam, temp, 1.0 / self.hp.iter_size)

    def _pc_launches(self, st, source=False):
        """Main stream, behind the student's forward (stream order) and the point where `self.label` is final, in front of plan.backward(): the
        cell labels, the normalised prototypes, the losses with their gradient into `plan.feat_seed`, the three scalars; then the seeded launch
        is switched on.  Ordering of `proto_eta` / `proto_n`, whose one writer is the teacher's `simt_proto_update`:
          source pass (source=True): the launches lie in front of the event the teacher's forward of THIS micro-batch waits for (`_teacher_input`
          records it behind them, or `_mixed_batch` runs the teacher behind them on this stream), so they read the prototypes BEFORE this
          micro-batch's update;
          target pass: they lie behind the main stream's wait for the teacher's event (`_teacher_labels`), so they read the prototypes AFTER it;
          the next update waits for an event recorded behind both readers (the next `_teacher_input`, main stream);
          with online_mix everything is on the main stream.
        `feat_seed`'s reader, the previous pass's backward, joined its side stream before it returned: it lies in front by stream order."""
        L.call("simt_cell_labels", C.byref(self.pc_lab_desc), st)
        L.call("simt_proto_contrast_prep", C.byref(self.pc_desc), st)
        L.call("simt_proto_contrast", C.byref(self.pc_desc), st)
        L.call("simt_proto_contrast_finalize", C.byref(self.pc_desc), st)
        if source:
            self.pc_source_out.copy_(self.pc_out, non_blocking=True)
        self.plan.use_feat_seed(True)

    def _pc_losses(self, out):
        """losses(): adds `proto_contrast`, `proto_contrast_cells` and, with online_source, `source_proto_contrast` (one more device-to-host copy)."""
        if getattr(self, "proto_contrast", None) is not None:
            v = torch.cat([self.pc_out, self.pc_source_out]).cpu().tolist()
            out["proto_contrast"], out["proto_contrast_cells"] = v[0], int(v[2])
            if getattr(self, "online_source", False):
                out["source_proto_contrast"] = v[3]
        return out
