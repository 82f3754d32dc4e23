"""DAFormer's thing-class ImageNet feature distance (Hoyer et al., CVPR'22; keywords `feat_dist` / `feat_dist_state` /
`feat_dist_classes` / `feat_dist_min_ratio` of WarmupTrainer, tool flags --feat-dist / --feat-dist-from / --feat-dist-classes /
--feat-dist-min-ratio).

With `feat_dist=lambda` the pass that trains on ground-truth labels -- the source pass with `online_source`, the only pass without
`online_labels` -- adds

    lambda * mean over kept cells m of || f_student[m, :] - f_imagenet[m, :] ||_2

where f_student is the student's layer-4 output of the train-mode forward, f_imagenet that of a frozen eval-mode trunk of the same
architecture over `feat_dist_state` (ImageNet weights), and a cell of the layer-4 map is kept when one thing class fills at least
`feat_dist_min_ratio` of its label window (include/simt_hip.h states the contract; tests/_feat_dist_ref.py restates it).  Per labelled pass:

  1. the image goes into the ImageNet plan's input on the main stream, behind the copy into the student's, and an event is recorded,
  2. the student's forward is enqueued (the critical path goes first, as in OnlineLabelMixin._teacher_labels),
  3. the ImageNet forward runs on the side stream behind the event; the main stream waits for it,
  4. `simt_feat_dist_mask`, `simt_feat_dist` and `simt_feat_dist_finalize` run on the main stream in front of `plan.backward()`: the second
     writes every row of `plan.feat_seed`, the `res` of the layer-4 head's input-gradient launch (TrunkPlan(feat_grad_seed=True)), so the
     term's gradient reaches the trunk weights through the ordinary backward launches and the heads get none.

The target pass under `online_source` runs with `plan.use_feat_seed(False)`: the parent's launch, nothing paid.  The ImageNet parameters are
not part of the EMA, `state_dict()` or the optimiser.  `losses()` gains `feat_dist` (lambda * mean distance, unscaled by iter_size like the
head's own terms) and `feat_dist_cells` (N of the last micro-batch); `total` keeps its meaning.  N is rank-local under data parallelism: every
rank's term is the mean over ITS kept cells, and the gradients are averaged by the existing exchange.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .engine import TrunkPlan, side_stream
from .train_state import state_sha256

DEFAULT_LAMBDA = 0.005                                   # DAFormer's imnet_feature_dist_lambda
DEFAULT_MIN_RATIO = 0.75                                 # DAFormer's imnet_feature_dist_scale_min_ratio
DEFAULT_CLASSES = (6, 7, 11, 12, 13, 14, 15, 16, 17, 18)      # DAFormer's thing classes of the 19 Cityscapes train ids
MAX_CLASSES = 64                                         # the thing set is a 64-bit word


def class_word(classes):
    """The thing set as the 64-bit word of simt_feat_dist_mask_desc.classes."""
    w = 0
    for c in classes:
        w |= 1 << int(c)
    return w


def check_feat_dist(feat_dist, feat_dist_state, feat_dist_classes, feat_dist_min_ratio, tau, source, num_classes):
    """The four keywords -> (lambda | None, classes (sorted tuple), min_ratio); `tau` is check_settings' first value, `source` check_source's.
    ValueError that starts with the keyword that does not fit."""
    if feat_dist is None:
        for name, v in (("feat_dist_state", feat_dist_state), ("feat_dist_classes", feat_dist_classes), ("feat_dist_min_ratio", feat_dist_min_ratio)):
            if v is not None:
                raise ValueError(f"{name} needs feat_dist: it belongs to the feature distance, and this trainer computes none")
        return None, None, None
    what = "expected the weight of the feature distance, a finite lambda >= 0"
    try:
        lam = float(feat_dist)
    except (TypeError, ValueError):
        raise ValueError(f"feat_dist {feat_dist!r}: {what}") from None
    if isinstance(feat_dist, bool) or not (0.0 <= lam < math.inf):
        raise ValueError(f"feat_dist {feat_dist!r}: {what}")
    if tau is not None and not source:
        raise ValueError("feat_dist with online_labels needs online_source: the mask is made of ground-truth labels, and a trainer that trains on a "
                         "teacher's labels alone has none")
    if not isinstance(feat_dist_state, dict) or not feat_dist_state:
        raise ValueError("feat_dist_state is required with feat_dist: the state dict of the frozen ImageNet trunk (simt_amd.pretrained.imagenet_trunk)")
    if feat_dist_classes is None:
        if num_classes != 19:
            raise ValueError(f"feat_dist_classes is required with num_classes = {num_classes}: the default is DAFormer's thing set of the 19 Cityscapes classes")
        classes = DEFAULT_CLASSES
    else:
        try:
            classes = tuple(sorted(int(c) for c in feat_dist_classes))
            exact = all(not isinstance(c, bool) and int(c) == c for c in feat_dist_classes)
        except (TypeError, ValueError):
            raise ValueError(f"feat_dist_classes {feat_dist_classes!r}: expected a list of class ids") from None
        top = min(num_classes, MAX_CLASSES)
        if not exact or not classes or len(set(classes)) != len(classes) or classes[0] < 0 or classes[-1] >= top:
            raise ValueError(f"feat_dist_classes {feat_dist_classes!r}: expected distinct class ids in [0, {top})")
    what = "expected the share of a cell's label window one thing class must fill, 0.5 < R <= 1"
    if feat_dist_min_ratio is None:
        ratio = DEFAULT_MIN_RATIO
    else:
        try:
            ratio = float(feat_dist_min_ratio)
        except (TypeError, ValueError):
            raise ValueError(f"feat_dist_min_ratio {feat_dist_min_ratio!r}: {what}") from None
        if isinstance(feat_dist_min_ratio, bool) or not (0.5 < ratio <= 1.0) or not (0.5 < float(np.float32(ratio)) <= 1.0):
            raise ValueError(f"feat_dist_min_ratio {feat_dist_min_ratio!r}: {what}")
    return lam, classes, ratio


class FeatDistMixin:
    """The feature distance of WarmupTrainer: the ImageNet plan, the buffers and descriptors of the three launches, the per-pass calls."""

    def _init_feat_dist(self, lam, classes, ratio, imnet_state, plan_kw):
        """lam None: off -- no plan, no buffer, no launch.  Behind the student's plan (built with feat_grad_seed=True) and `self.label`."""
        self.feat_dist = lam
        if lam is None:
            return
        dev, f32 = self.dev, torch.float32
        self.feat_dist_classes, self.feat_dist_min_ratio = tuple(classes), float(ratio)
        # a frozen copy: no optimiser, no EMA and no state_dict() ever sees it; a train state carries its SHA-256 only (train_state.py)
        self.imnet_params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in imnet_state.items()}
        self.feat_dist_sha256 = state_sha256(self.imnet_params)
        self.imnet = TrunkPlan(self.imnet_params, self.B, self.H, self.W, [], dtype=self.dtype, train=False, stem_from=None, **plan_kw)
        plan = self.plan
        fs, fi = plan.block_io[-1]["z"], self.imnet.block_io[-1]["z"]
        h, w = plan.feat_hw
        M, Cf = fs.shape
        assert fi.shape == fs.shape and M == self.B * h * w and plan.feat_seed is not None and plan.feat_seed.shape == fs.shape
        lib = L.load()
        n_mask = lib.simt_feat_dist_mask_parts(self.B, h, w)
        n_part = lib.simt_feat_dist_parts(M)
        if n_mask < 1 or n_part < 1:
            raise L.SimtHipError(f"simt_feat_dist_mask_parts: {n_mask} for B = {self.B}, {h} x {w}")
        self.fd_mask = torch.zeros(M, device=dev, dtype=torch.uint8)
        self.fd_kept_part = torch.zeros(n_mask, device=dev, dtype=torch.int32)      # every word is written by every mask launch
        self.fd_d = torch.zeros(M, device=dev, dtype=f32)
        self.fd_part = torch.zeros(n_part, device=dev, dtype=f32)
        self.fd_out = torch.zeros(3, device=dev, dtype=f32)
        m = L.FeatDistMaskDesc()
        m.label, m.mask, m.part, m.classes = self.label.data_ptr(), self.fd_mask.data_ptr(), self.fd_kept_part.data_ptr(), class_word(classes)
        m.B, m.H, m.W, m.h, m.w, m.min_ratio = self.B, self.H, self.W, h, w, ratio
        d = L.FeatDistDesc()
        d.fs, d.fi, d.mask, d.kept_part = fs.data_ptr(), fi.data_ptr(), self.fd_mask.data_ptr(), self.fd_kept_part.data_ptr()
        d.seed, d.d, d.part, d.out = plan.feat_seed.data_ptr(), self.fd_d.data_ptr(), self.fd_part.data_ptr(), self.fd_out.data_ptr()
        d.lam, d.M, d.C, d.ld, d.dtype, d.n_kept_part = lam, M, Cf, Cf, ops.dt_code(self.dtype), n_mask
        d.lam_g = lam * (1.0 / self.hp.iter_size)          # (float)(lambda * gscale), gscale as in the head descriptor
        self.fd_mask_desc, self.fd_desc = m, d

    def _fd_input(self):
        """Main stream, behind the copy of the labelled image into `plan.x_in`: the same image into the ImageNet plan's input, then the event
        its forward waits for.  Behind everything the previous pass enqueued on the main stream -- its simt_feat_dist launch, the one reader
        of the ImageNet feature map, among it: the side stream's next ImageNet forward waits for this event, so it cannot overwrite that map
        (nor any ping-pong buffer of the eval plan) while the launch still reads it (WAR)."""
        self.imnet.x_in.copy_(self.plan.x_in, non_blocking=True)
        ev_in = torch.cuda.Event()
        ev_in.record(torch.cuda.current_stream())
        return ev_in

    def _fd_forward(self, ev_in):
        """The ImageNet forward on the side stream, beside the student's forward (already enqueued on the main stream); the main stream then
        waits for it.  The next copy into `imnet.x_in` (main stream) lies behind that wait: the forward that read the input is complete."""
        main, side = torch.cuda.current_stream(), side_stream(self.dev)
        with torch.cuda.stream(side):
            side.wait_event(ev_in)
            self.imnet.fwd_list.run()
            ev_f = torch.cuda.Event()
            ev_f.record(side)
        main.wait_event(ev_f)

    def _fd_launches(self, st):
        """Main stream, behind the student's forward (stream order), the ImageNet forward (the wait of _fd_forward) and the label copy, in
        front of plan.backward(): the mask of the labels, the distances with their gradient into `plan.feat_seed`, the three scalars.  The
        previous pass's backward, the reader of `feat_seed`, joined the side stream before it returned: every reader lies in front."""
        L.call("simt_feat_dist_mask", C.byref(self.fd_mask_desc), st)
        L.call("simt_feat_dist", C.byref(self.fd_desc), st)
        L.call("simt_feat_dist_finalize", C.byref(self.fd_desc), st)

    def _fd_losses(self, out):
        """losses(): adds `feat_dist` and `feat_dist_cells` (one more device-to-host copy of three floats)."""
        if getattr(self, "feat_dist", None) is not None:
            v = self.fd_out.cpu().tolist()
            out["feat_dist"], out["feat_dist_cells"] = v[0], int(v[2])
        return out
