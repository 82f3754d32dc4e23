"""One SimT training iteration on gfx950: the seam the reference lacks (its loss body is inline in
tools/trainV2_simt.py:308-436).  `SimTTrainer.step(image, label, it)` runs, on the current HIP stream and without a
host sync:

  1. the 10-step W inner loop incl. Adam and the gradient leak into NTM      (trainV2_simt.py:326-339)  simt_ntm_inner_loop
  2. the frozen model forward (eval BN folded) -> low-res posterior          (:351-354)               TrunkPlan(train=False)
  3. the trainable forward (train-mode BN, frozen affine)                     (:370)                   TrunkPlan(train=True)
  4. the fused head: upsample + softmax + every loss term + anchors           (:354-409)               simt_head_loss
     Convex / Volume / Anchor + total + d/dNTM                                (:412-424)               simt_ntm_post
     d/d(low-res logits)                                                      (:428)                   simt_head_grad
  5. the trunk backward (dgrad + wgrad + BN backward)                         (:428)                   TrunkPlan.backward
  6. [DP] RCCL all-reduce (mean) of the flat gradient buffer and of dNTM      (new capability)
  7. SGD with duplicate-listing semantics + Adam on NTM1/NTM2                 (:434-436)               simt_sgd_multi / simt_adam_step
     (optimizer="adamw": simt_adamw_multi in the place of simt_sgd_multi, every tensor once -- simt_amd/optimizer.py)

All state lives on the device; scalars are read back only when the caller asks (`losses()`).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import trace
from .ema import EmaMixin
from .ema_teacher import TeacherMixin
from .engine import LaunchList, TrunkPlan, multi_heads, side_stream
from .feat_dist import FeatDistMixin, check_feat_dist
from .optimizer import DEFAULT_BETAS, DEFAULT_EPS, DEFAULT_WARMUP_RATIO, OptimizerMixin
from .online_labels import (DEFAULT_ENTROPY_ETA, OnlineLabelMixin, check_balanced, check_entropy, check_mix, check_settings, check_source,
                            check_uncertainty, check_weighted)
from .proto import DEFAULT_MOMENTUM as DEFAULT_PROTO_MOMENTUM, check_proto
from .proto_contrast import ProtoContrastMixin, check_proto_contrast
from .train_state import TrainStateMixin, state_sha256


class Hyper:
    """Hyper-parameters of tools/trainV2_simt.py:34-70 (flag defaults) / sh_simt.sh:16."""

    def __init__(self, num_classes=19, open_classes=15, th_high=0.8, th_low=0.2, lambda_seg=0.1, lambda_place=0.1,
                 lambda_convex=0.5, lambda_volume=0.1, lambda_anchor=0.5, iter_size=1, lr=2.5e-4, lr_T=2.5e-4,
                 momentum=0.9, weight_decay=5e-4, power=0.9, num_steps=250000, skip_unapplied_grads=False):
        # skip_unapplied_grads: stop the backward at the input of layer3.  The reference's autograd also produces the gradients of
        # conv1 / layer1 / layer2, which its SGD never lists (model/deeplab_multi.py:194-237) and zero_grad() discards; with this
        # switch they are not computed -- identical parameter trajectory and losses, less work.  Off by default (and in bench.py):
        # the default does everything the reference's iteration does.
        self.__dict__.update(locals())
        del self.__dict__["self"]


def lr_poly(base_lr, it, max_iter, power):
    return base_lr * ((1 - float(it) / max_iter) ** power)            # trainV2_simt.py:174-175


def lr_at(base, it, max_iter, power, warmup=0, warmup_ratio=1e-6):
    """The model's learning rate at iteration `it`: `lr_poly`, and over the first `warmup` iterations its "linear" warm-up (DAFormer's
    schedule) -- the poly value times a factor that rises from `warmup_ratio` at it = 0 to 1 at it = warmup.  warmup = 0 returns
    lr_poly's float itself.  lr_T (NTM Adam, the inner W loop) is not warmed up: it stays lr_poly."""
    lr = lr_poly(base, it, max_iter, power)
    if warmup and it < warmup:
        lr = lr * (1 - (1 - float(it) / warmup) * (1 - warmup_ratio))
    return lr


def optim_listing(names, layers_root=("layer3", "layer4"), head_prefixes=("layer5", "layer6", "layer5_1", "layer6_1")):
    """Multiplicity of each tensor in ResNetMulti.optim_parameters (model/deeplab_multi.py:194-237).

    get_1x_lr_params_NOscale walks `for j in layer.modules(): for k in j.parameters()` -- every sub-module yields the
    parameters of its whole subtree, so a tensor is listed once per ancestor module inside the layer (the layer
    itself, its Bottleneck, the leaf; plus the `downsample` Sequential for its members).  group 0 = those, group 1
    (10x lr) = the heads, listed once."""
    g0, g1 = {}, {}
    for n in names:
        root = n.split(".")[0]
        if root in layers_root:
            depth = len(n.split(".")) - 1          # layer3.0.conv1.weight -> 3 ancestors; downsample.0.weight -> 4
            g0[n] = depth
        elif root in head_prefixes:
            g1[n] = 1
    return g0, g1


def sgd_listing(names, roots=("layer3", "layer4")):
    """`optim_listing` as the [(name, mult, group)] of OptimizerMixin._build_sgd: group 0, then group 1."""
    return [(n, mult, group) for group, listing in enumerate(optim_listing(names, layers_root=roots)) for n, mult in listing.items()]


def check_views(tr, teacher_image, fix_item, n):
    """The weak-view arguments of a SimT trainer's step() as two lists of n = iter_size entries (None where absent); ValueError when they do
    not fit the trainer's `teacher_view`."""
    if not tr.teacher_view:
        if teacher_image is not None or fix_item is not None:
            raise ValueError("step(): teacher_image / fix_item need a trainer built with teacher_view=True")
        return [None] * n, [None] * n
    if teacher_image is None:
        raise ValueError("step(): this trainer was built with teacher_view=True and needs teacher_image (the frozen model's view)")
    teachers = list(teacher_image) if isinstance(teacher_image, (list, tuple)) else [teacher_image]
    maps = list(fix_item) if isinstance(fix_item, (list, tuple)) else [fix_item] * (n if fix_item is None else 1)
    if len(teachers) != n or len(maps) != n:
        raise ValueError(f"step() needs {n} teacher_image(s) and fix_item(s) (hp.iter_size), got {len(teachers)} and {len(maps)}")
    for t in teachers:
        if tuple(t.shape) != (tr.B, 3, tr.H, tr.W):
            raise ValueError(f"teacher_image of shape {tuple(t.shape)}, expected {(tr.B, 3, tr.H, tr.W)}")
    for m in maps:
        if m is not None and (tuple(m.shape) != (tr.B, tr.H, tr.W) or m.dtype != torch.uint8):
            raise ValueError(f"fix_item of shape {tuple(m.shape)} and dtype {m.dtype}, expected {(tr.B, tr.H, tr.W)} uint8")
    return teachers, maps


class SimTTrainer(TrainStateMixin, EmaMixin, TeacherMixin, OptimizerMixin):
    def __init__(self, state, fixed_state, ntm1, ntm2, hp, class_dist, B, H, W, *, dtype=torch.bfloat16, device="cuda:0",
                 openset=True, process_group=None, w_init=None, layers=None, ema_decay=None, ema_teacher_every=None, teacher_view=False,
                 optimizer="sgd", adam_betas=DEFAULT_BETAS, adam_eps=DEFAULT_EPS, lr_warmup=0, lr_warmup_ratio=DEFAULT_WARMUP_RATIO):
        """optimizer="adamw" (simt_amd/optimizer.py): simt_adamw_multi in the place of simt_sgd_multi, every applied tensor listed
        once, with adam_betas and adam_eps; lr_warmup=N: the model's learning rate rises linearly over the first N iterations (`lr_at`), lr_T
        does not.  The defaults are the trainer it was.
        teacher_view=True (the weak-view teacher): the frozen model reads an image of its own -- `step(..., teacher_image=...)`,
        the weak view -- through its own one-set stem launch, and the head reads each pixel's frozen operand from the item `fix_item` names
        (simt_head_loss_views / simt_head_grad_views).  False: one image for both networks, as the reference feeds them."""
        self.hp, self.B, self.H, self.W, self.dtype = hp, B, H, W, dtype
        self.teacher_view = bool(teacher_view)
        dev = self.dev = torch.device(device)
        self.pg = process_group
        Cn, K = hp.num_classes, hp.open_classes
        self.C, self.Q = Cn, Cn + K
        f32 = torch.float32
        self.params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
        self.fixed_params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone()
                             for k, v in fixed_state.items()}
        self.frozen_sha256 = state_sha256(self.fixed_params)      # a train state is refused beside another frozen model (train_state.py)
        kw = {"layers": layers} if layers is not None else {}
        self.plan = TrunkPlan(self.params, B, H, W, multi_heads(Cn, K, openset), dtype=dtype, train=True,
                              grads_from_layer=3 if getattr(hp, "skip_unapplied_grads", False) else 0,
                              data_parallel=process_group is not None, **kw)
        # the frozen model sees the same image: it reuses the trainable plan's stem im2col matrix (one im2col per micro-batch)
        # (teacher_view: it sees another one -- no stem_from: its own x_in and its own stem launch, the first of its forward, on the side stream)
        self.fixed = TrunkPlan(self.fixed_params, B, H, W, multi_heads(Cn, 0, False), dtype=dtype, train=False,
                               stem_from=None if self.teacher_view else self.plan,
                               data_parallel=process_group is not None, **kw)      # (same CU budget = same tile lists as the trainable plan)
        # item 0 of the trainable forward feeds BOTH nets: the direct stem launch with the frozen net as its second weight set (bf16), or the im2col
        # (teacher_view: the trainable net alone, one weight set)
        assert self.plan.fwd_list.items[0].tag in ("simt_stem7_fwd", "simt_im2col_stem")
        assert self.plan.fwd_list.items[0].tag == "simt_im2col_stem" or self.plan.stem_desc.nsets == (1 if self.teacher_view else 2)
        assert not self.teacher_view or self.fixed.fwd_list.items[0].tag == self.plan.fwd_list.items[0].tag
        self._fwd_rest = LaunchList()
        self._fwd_rest.items = self.plan.fwd_list.items[1:]
        h, w = self.plan.heads[1].h, self.plan.heads[1].w
        self.h, self.w = h, w
        Q = self.Q
        # ---- NTM / W state (model/deeplab_multi.py:244-286)
        self.ntm = [ntm1.detach().to(dev, f32).clone(), ntm2.detach().to(dev, f32).clone()]
        # ONE allocation [16 scalars (lout) | dNTM1 | dNTM2]: under data parallelism its tail from lout[12] on (the bad-label count, three unused
        # slots, both NTM gradients) is ONE contiguous collective at the end of the exchange (it used to be two)
        self._xchg = torch.zeros(16 + 2 * Q * Cn, device=dev)
        self._ntm_grad_flat = self._xchg[16:].view(2, Q, Cn)
        self.ntm_grad = [self._ntm_grad_flat[0], self._ntm_grad_flat[1]]
        self.ntm_m = [torch.zeros(Q, Cn, device=dev) for _ in range(2)]
        self.ntm_v = [torch.zeros(Q, Cn, device=dev) for _ in range(2)]
        wi = w_init if w_init is not None else torch.full((Q, Q), 1.0 / (Q - 1.0))
        self.wraw = [wi.detach().to(dev, f32).clone() for _ in range(2)]
        self.w_m = [torch.zeros(Q, Q, device=dev) for _ in range(2)]
        self.w_v = [torch.zeros(Q, Q, device=dev) for _ in range(2)]
        self.T = [torch.zeros(Q, Cn, device=dev) for _ in range(2)]
        self.cd = torch.as_tensor(np.asarray(class_dist), dtype=f32).to(dev)
        self.inner_steps = 10
        # ---- head workspaces
        lib = L.load()
        self.nblk = lib.simt_head_nblk(B, H, W)
        self.part = torch.zeros(self.nblk, lib.simt_head_part_floats(Q, Cn), device=dev)
        self.keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
        self.hout = torch.zeros(lib.simt_head_hout_floats(Q, Cn), device=dev)
        self.lout = self._xchg[:16]
        self._bad_reported = 0                     # out-of-range labels already raised for (host side; the device counter is never reset)
        self.QP = ops.round_up(Q, 8)
        self.g1 = torch.zeros(2, B, H, w, self.QP, device=dev)
        self.ldf = self.fixed.ldp["x2"]
        self.fixp = torch.zeros(B * h * w, self.ldf, device=dev)
        self.label = torch.zeros(B, H, W, device=dev, dtype=torch.int64)
        hd = L.HeadDesc()
        p1, p2 = self.plan.out["x1"], self.plan.out["x2"]
        hd.pred1, hd.pred2, hd.fixp, hd.label = p1.data_ptr(), p2.data_ptr(), self.fixp.data_ptr(), self.label.data_ptr()
        hd.T1, hd.T2 = self.T[0].data_ptr(), self.T[1].data_ptr()
        hd.part, hd.keys, hd.hout, hd.g1 = self.part.data_ptr(), self.keys.data_ptr(), self.hout.data_ptr(), self.g1.data_ptr()
        hd.dpred1_f32, hd.dpred2_f32 = None, None
        d1, d2 = self.plan.dlogits["x1"], self.plan.dlogits["x2"]
        hd.dpred1_t, hd.dpred2_t = d1.data_ptr(), d2.data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Cn, Q
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t = self.plan.ldp["x1"], self.ldf, self.QP, 0, d1.shape[1]
        hd.grad_dtype = ops.dt_code(dtype)
        hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place = hp.th_high, hp.th_low, hp.lambda_seg, hp.lambda_place
        hd.gscale = 1.0 / hp.iter_size
        # per-pixel Conf_label_target of the last (micro-)batch (trainV2_simt.py:357-362,387-393), 255 = none: 1 byte per pixel
        self.conf_label = torch.full((B, H, W), 255, device=dev, dtype=torch.uint8)
        hd.conf_out = self.conf_label.data_ptr()
        self._label_ws = torch.full((B, H, W), 255, device=dev, dtype=torch.uint8)          # checked noisy labels, loss pass -> gradient pass
        hd.label_ws = self._label_ws.data_ptr()
        self.head_desc = hd
        # teacher_view: the item of the frozen map each pixel reads (simt_class_mix_items' map), resident; a step without a map reads no map
        self.fix_item = torch.zeros(B, H, W, device=dev, dtype=torch.uint8) if self.teacher_view else None
        self._fix_item_ptr = None
        # ---- NTM descriptors
        ni = L.NtmInnerDesc()
        for k in range(2):
            ni.ntm[k], ni.w[k], ni.ntm_grad[k] = self.ntm[k].data_ptr(), self.wraw[k].data_ptr(), self.ntm_grad[k].data_ptr()
            ni.w_m[k], ni.w_v[k], ni.T_out[k] = self.w_m[k].data_ptr(), self.w_v[k].data_ptr(), self.T[k].data_ptr()
        ni.class_dist, ni.Q, ni.C, ni.steps = self.cd.data_ptr(), Q, Cn, self.inner_steps
        ni.beta1, ni.beta2, ni.eps = 0.9, 0.999, 1e-8
        # every optimiser launch is guarded by the plan's sticky fused-BatchNorm error word (engine.TrunkPlan.fbn_error): once a fused launch has
        # given up polling, SGD, both Adams and the W inner loop change nothing -- a state_dict saved after losses() raised holds the last good state
        self._skip_word = getattr(self.plan, "fbn_err", None)
        if self._skip_word is not None:
            ni.skip_if = self._skip_word.data_ptr()
        self.inner_desc = ni
        npd = L.NtmPostDesc()
        for k in range(2):
            npd.ntm[k], npd.w[k], npd.ntm_grad[k] = self.ntm[k].data_ptr(), self.wraw[k].data_ptr(), self.ntm_grad[k].data_ptr()
        npd.class_dist, npd.hout, npd.lout, npd.Q, npd.C = self.cd.data_ptr(), self.hout.data_ptr(), self.lout.data_ptr(), Q, Cn
        npd.lambda_seg, npd.lambda_convex, npd.lambda_volume = hp.lambda_seg, hp.lambda_convex, hp.lambda_volume
        npd.lambda_anchor, npd.gscale = hp.lambda_anchor, 1.0 / hp.iter_size
        self.post_desc = npd
        # ---- SGD segments (duplicate listings replayed in registers)
        self._build_sgd(sgd_listing(self.plan.grads.keys()))
        self._init_optimizer(optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio)
        self.it_done = 0
        self._init_ema(ema_decay)          # ema_decay=None: no shadow, no launch (simt_amd/ema.py)
        self._init_teacher(ema_teacher_every)      # None: the frozen model never moves (simt_amd/ema_teacher.py)
        # ---- early optimiser step: the gradients SGD applies (layer3, layer4, heads) are final long before the backward has walked
        # through layer2 / layer1 / the stem (whose gradients this stage computes but never applies), so SGD and the re-pack of the
        # updated weights run on the side stream from that point on instead of after the backward (0.7 ms of exclusive tail).
        applied = [n for n in self.sgd_names if self.plan.grad_ready.get(n, 0) > 0]
        self._ev_post = None
        self._early_cut = max(self.plan.grad_ready[n] for n in applied) if applied else None
        if self._early_cut is not None:
            # The block that produced the last applied weight gradient lists its wgrads BEFORE its input-gradient convs
            # (engine._build_backward), and those convs read the packed operands of conv1 / downsample that the early re-pack
            # overwrites: fire at the first hook point at or after the END of that block, so that the event the side stream waits
            # for covers them (WAR).  If the block has no input gradient (nothing below it is differentiated) the cut stands.
            blk = min((m for m in self.plan.bwd_marks.values() if m[1] >= self._early_cut), key=lambda m: m[1], default=None)
            if blk is not None and blk[3] is not None:
                later = [c for c in sorted(set(self.plan.grad_ready.values())) if c >= blk[1]]
                self._early_cut = later[0] if later else None
        self._early_sgd = (os.environ.get("SIMT_EARLY_SGD", "1") != "0" and self._early_cut is not None
                           and hp.iter_size == 1 and self._early_cut < len(self.plan.bwd_list.items))
        self._pack_applied = self.plan.pack_subset(self.sgd_names) if self._early_sgd else None
        # ---- data parallel: bucketed mean all-reduce overlapped with backward
        self._grad_acc = torch.zeros_like(self.plan.flat_grad) if hp.iter_size > 1 else None
        self.reducer = None
        if self.pg is not None:
            from .dp import BucketReducer, make_buckets
            order, sizes, end = self.exchange_table()
            be = int(float(os.environ.get("SIMT_DP_BUCKET_MB", "0")) * (1 << 18)) or self.BUCKET_ELEMS      # (MB of fp32 per all-reduce; default 32)
            buckets = make_buckets(order, sizes, self.plan.grad_ready, bucket_elems=be)
            # the bad-label count (lout[12], accumulated by simt_ntm_post) rides in the same exchange: after the mean every rank holds
            # total / world, so losses() needs no collective of its own and every rank raises in the same call
            self.reducer = BucketReducer(self.plan.flat_grad[:end], buckets, group=self.pg, extra=[self._xchg[12:]])
            self.reducer.total_launches = len(self.plan.bwd_list.items)

    BUCKET_ELEMS = 8 << 20      # 32 MB of fp32 per all-reduce: few large messages for xGMI rings (dp.py)

    def exchange_table(self):
        """(order, sizes, end): the gradients the data-parallel exchange carries, in flat-buffer order, their padded spans in elements and
        the length of the prefix of `plan.flat_grad` they form.  Only gradients the optimiser APPLIES cross xGMI: layer3, layer4
        and the heads = the head of the flat buffer (169 of 180 MB).  conv1 / layer1 / layer2 gradients are computed like the reference
        computes them (unless skip_unapplied_grads) but the SimT stage's SGD never lists them (model/deeplab_multi.py:194-237): they stay
        rank-local.  (tests/golden/g16_dp_bucket_table.json is this table for BASELINE configs[1..2], profiles/tools/dump_bucket_table.py.)"""
        sizes = {n: k for n, (_o, k) in self.plan.grad_offsets.items()}
        applied = set(self.sgd_names)
        order = [n for n in self.plan.grad_order if n in applied and self.plan.grad_ready.get(n, 0) > 0]
        assert order == self.plan.grad_order[:len(order)], "applied gradients must form a prefix of the flat buffer"
        return order, sizes, sum(sizes[n] for n in order)

    # ------------------------------------------------------------------ one iteration
    def _micro_batch(self, image, label, st, teacher_image=None, fix_item=None):
        """Steps 2-5 of the iteration for one micro-batch: both forwards, fused head, NTM terms, backward."""
        self.plan.x_in.copy_(image, non_blocking=True)
        self.label.copy_(label, non_blocking=True)
        if self.teacher_view:      # the weak view and its map: main stream, in front of ev_in (the frozen forward waits for it)
            self.fixed.x_in.copy_(teacher_image, non_blocking=True)
            self._fix_item_ptr = None
            if fix_item is not None:
                self.fix_item.copy_(fix_item, non_blocking=True)
                self._fix_item_ptr = self.fix_item.data_ptr()
        # the stem launch (first launch of the trainable forward: direct conv of both nets, or the im2col they share) feeds BOTH nets: run it before forking
        head = self.plan.fwd_list.items[0]
        rc = head.fn(*head.args, st)
        if rc != 0:
            L.check(rc)
        # 2. frozen model -> low-res posterior, on the side stream: its eval-mode convs share the CUs with the HBM-bound BatchNorm passes of the
        #    trainable forward (3.) instead of running before it.  The host enqueues ~350 launches per forward at ~5 us each: the trainable
        #    forward (critical path) goes first -- enqueued second, its first conv reached the GPU 3.6 ms into the step (rocprofv3 kernel trace).
        #    Measured, bit-identical and removed: other enqueue orders of the two forwards (neutral to +1.9 ms), one launch per layer for both
        #    networks (+1.3 ms: it gives up the two-stream overlap), hipGraphs of the forwards and stream priorities (neutral).
        main = torch.cuda.current_stream()
        side = side_stream(self.dev)
        ev_in = torch.cuda.Event()
        ev_in.record(main)
        with trace.range("forward"):
            self._fwd_rest.run()               # 3. trainable forward (its stem launch already ran above)
        with torch.cuda.stream(side), trace.range("frozen-forward"):
            side.wait_event(ev_in)
            self.fixed.forward()
            ops.softmax_rows(self.fixed.out["x2"], self.ldf, self.fixp, self.ldf, self.B * self.h * self.w, self.C)
            ev_fix = torch.cuda.Event()
            ev_fix.record(side)
        main.wait_event(ev_fix)
        # 4. fused head + NTM regularisers + gradients of the low-res logits (every term scaled by 1 / iter_size, :427;
        #    the NTM gradients accumulate on top of the inner loop's leak and of earlier micro-batches)
        #    The regularisers only feed the Adam step and the loss read-out: they run on the side stream (idle between the frozen forward
        #    and the first weight gradients) beside the head's gradient pass instead of in front of it (a 100 us single-block kernel).
        if self._ev_post is not None:
            main.wait_event(self._ev_post)     # an earlier micro-batch's regularisers still read the head's outputs
        with trace.range("head"):
            L.call("simt_head_loss_views", C.byref(self.head_desc), self._fix_item_ptr, st)
            ev_loss = torch.cuda.Event()
            ev_loss.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ev_loss)
                L.call("simt_ntm_post", C.byref(self.post_desc), side.cuda_stream)
                self._ev_post = torch.cuda.Event()
                self._ev_post.record(side)
            L.call("simt_head_grad_views", C.byref(self.head_desc), self._fix_item_ptr, st)

    def step(self, image, label, it=None, teacher_image=None, fix_item=None):
        """image [B,3,H,W] fp32 (device or host), label [B,H,W] int64 -- or, with hp.iter_size > 1 (gradient accumulation,
        trainV2_simt.py:341-432), sequences of iter_size micro-batches.  Returns the device tensor `lout`
        (total, loss_p1, loss_p2, loss_y1, loss_y2, Place, Convex, Volume, Anchor, vol_ok, ...) of the last micro-batch.
        teacher_view=True: teacher_image (required) is the frozen model's image, fix_item ([B,H,W] uint8 or None) the item of the frozen
        map each pixel reads; sequences like image when hp.iter_size > 1."""
        hp = self.hp
        teachers, maps = check_views(self, teacher_image, fix_item, hp.iter_size)
        it = self.it_done if it is None else it
        lr = lr_at(hp.lr, it, hp.num_steps, hp.power, self.lr_warmup, self.lr_warmup_ratio)
        lr_T = lr_poly(hp.lr_T, it, hp.num_steps, hp.power)      # (not warmed up: DESIGN 7.23)
        st = ops.stream_ptr()
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        labels = list(label) if isinstance(label, (list, tuple)) else [label]
        if len(images) != hp.iter_size or len(labels) != hp.iter_size:
            raise ValueError(f"step() needs {hp.iter_size} micro-batch(es) (hp.iter_size), got {len(images)}")
        # 1. inner W loop (NTM grads start from zero each iteration: optimizer_t*.zero_grad(), :314-318)
        # It only feeds the head (T, W) and the Adam step: it runs on the side stream, ahead of the frozen model's forward, instead
        # of in front of the trainable forward (150 us of a single-block kernel off the critical path).
        main, side = torch.cuda.current_stream(), side_stream(self.dev)
        ev0 = torch.cuda.Event()
        ev0.record(main)                       # the previous step's Adam / head kernels (main stream) come first
        with torch.cuda.stream(side):
            side.wait_event(ev0)
            self._ntm_grad_flat.zero_()
            ni = self.inner_desc
            ni.step0, ni.lr = self.inner_steps * self.it_done, lr_T
            L.call("simt_ntm_inner_loop", C.byref(ni), side.cuda_stream)
        flat = self.plan.flat_grad
        for mi, (img, lab) in enumerate(zip(images, labels)):
            last = mi == hp.iter_size - 1
            self._micro_batch(img, lab, st, teachers[mi], maps[mi])
            # 5. trunk backward (+ 6. data-parallel mean of the gradients, bucket by bucket, on a side stream)
            if self._early_sgd:            # (with a reducer: the exchange completes on the side stream too, ahead of its SGD)
                with trace.range("backward (+ exchange + early optimiser step)"):
                    self._backward_early_sgd(lr, st)
                continue
            if self.reducer is not None and hp.iter_size == 1:
                self.reducer.start()
                with trace.range("backward (+ bucketed exchange)"):
                    self.plan.backward(hook=self.reducer.ready_upto)
                torch.cuda.current_stream().wait_event(self._ev_post)      # the NTM gradients it exchanges last (side stream)
                with trace.range("exchange (flush + wait)"):
                    self.reducer.finish()
                continue
            with trace.range("backward"):
                self.plan.backward()
            if hp.iter_size > 1:      # loss.backward() accumulates into .grad (:428): keep the running sum beside the plan's buffer
                if mi == 0:
                    self._grad_acc.copy_(flat)
                elif not last:
                    L.call("simt_vec_acc", self._grad_acc.data_ptr(), flat.data_ptr(), flat.numel(), 1, st)
                else:
                    L.call("simt_vec_acc", flat.data_ptr(), self._grad_acc.data_ptr(), flat.numel(), 1, st)
                    if self.reducer is not None:   # one exchange of the accumulated gradient (no overlap with backward)
                        torch.cuda.current_stream().wait_event(self._ev_post)
                        self.reducer.start()
                        self.reducer.finish()
        # 7. optimisers
        if not self._early_sgd:
            with trace.range("optimiser"):
                self._sgd(lr, st)
        torch.cuda.current_stream().wait_event(self._ev_post)      # regularisers (side stream): NTM gradients and the losses are final
        for k in range(2):
            ops.adam_step(self.ntm[k], self.ntm_grad[k], self.ntm_m[k], self.ntm_v[k], lr=lr_T, step=self.it_done + 1, skip_if=self._skip_word)
        if not self._early_sgd:
            self.plan.repack()
            if self.ema is not None:
                # behind the re-pack on the main stream: in order after this step's forward (running statistics) and SGD launch, and in front
                # of everything the next step enqueues (its side-stream work waits for an event the main stream records first: ev0)
                self.ema.update(st)
                # the EMA teacher's refresh (simt_amd/ema_teacher.py), if this update made one due, directly behind it on the main stream:
                #   behind this step's frozen forward and softmax_rows (side stream): the main stream waited for ev_fix in front of the head;
                #   in front of the next step's stem launch (main stream, reads the frozen plan's w7 and bn1 shift): stream order;
                #   in front of the next step's frozen forward (side stream): it waits for ev0 / ev_in, which the main stream records first.
                # Once per optimiser step: this point is behind the last micro-batch.
                self._teacher_follows(st)
        self.it_done += 1
        return self.lout

    def _sgd(self, lr, st):
        self._optim_step(lr, st)      # simt_sgd_multi, or simt_adamw_multi in its place (simt_amd/optimizer.py)

    def _backward_early_sgd(self, lr, st):
        """Backward with the SGD step and the re-pack of the updated layers enqueued on the side stream once the block that produced
        the last applied gradient has been enqueued COMPLETELY (its input-gradient convs read the packed weights the re-pack
        overwrites; `_early_cut` is the first hook point at or after that block's end).  The side stream first waits for the main
        stream's launches up to that point; the list's final join makes the main stream wait for all of it."""
        main, side = torch.cuda.current_stream(), side_stream(self.dev)
        done = [False]
        red = self.reducer
        if red is not None:
            red.start()

        def hook(n, ev):
            if red is not None and not done[0]:
                red.ready_upto(n, ev)      # data parallel: the buckets whose gradients are final start their all-reduce
            if done[0] or n < self._early_cut:
                return
            done[0] = True
            ev_main = torch.cuda.Event()
            ev_main.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ev_main)
                if red is not None:
                    # last buckets + NTM gradients, then THIS stream waits for the exchange: the main stream keeps walking through
                    # layer2 / layer1 / the stem (rank-local gradients) while the mean gradients arrive and are applied
                    red.finish()
                self._sgd(lr, side.cuda_stream)
                self._pack_applied.run()
                if self.ema is not None:
                    # behind the re-pack the next forward waits for.  The side stream waited for ev_main (the whole forward: this step's
                    # running statistics) and has just run SGD; the backward list's final join makes the main stream wait for the side
                    # stream, so the launch is complete before the next step writes a master
                    self.ema.update(side.cuda_stream)
                    # the EMA teacher's refresh, if due, directly behind it on the SIDE stream:
                    #   behind this step's frozen forward and softmax_rows: they ran on this stream earlier in the step (stream order);
                    #   behind this step's stem launch, the one main-stream reader of the frozen plan's operands: the side stream waited
                    #   for ev_main, recorded on the main stream after it;
                    #   in front of the next step's frozen forward: stream order;
                    #   in front of the next step's stem launch (main stream): the backward list's final join makes the main stream wait
                    #   for the side stream after this hook has enqueued.
                    self._teacher_follows(side.cuda_stream)
        self.plan.backward(hook=hook)
        assert done[0]

    def state_dict(self):
        """Host copy of the trainable model's state (the reference's `model.state_dict()` of :449,461): every key, NCHW fp32, with
        `num_batches_tracked` = number of train-mode forwards so far (nn.BatchNorm2d bumps it once per forward)."""
        sd = {}
        for k, v in self.params.items():
            sd[k] = (v.detach().cpu() if not k.endswith("num_batches_tracked") else
                     torch.tensor(int(v.item()) + self._nbt_steps(k), dtype=torch.long))
        return sd

    def timed_lists(self):
        """The launch lists of one iteration for per-kernel timing (bench.py): frozen forward, trainable forward, backward."""
        return [self.fixed.fwd_list, self.plan.fwd_list, self.plan.bwd_list]

    def losses(self):
        """Host copy of the scalars of the last step.  Synchronises the device; LOCAL (no collective: under data parallelism the
        bad-label count travels with the gradient exchange, so a rank may call this alone, e.g. rank 0 for logging -- but a rank that
        raises alone leaves its peers blocked in their next all-reduce, so training loops call it on every rank at the same iterations).
        Raises ValueError for labels outside [0, C) other than 255 seen in ANY micro-batch on ANY rank since the last call
        (utils/loss.py:36 raises at once), RuntimeError if a fused BatchNorm launch timed out (TrunkPlan.fbn_error)."""
        v = self.lout.cpu().tolist()                  # ONE device-to-host copy: the scalars and the bad-label count (lout[12])
        self.plan.raise_on_fbn_error()
        # accumulated by simt_ntm_post over every micro-batch since the last call; data parallel: the exchange leaves total / world on every rank
        # (the counter is cumulative and never reset on the device: a local reset by one rank would turn the next mean into a fraction on all)
        bad = int(round(v[12] * (self.reducer.world if self.reducer is not None else 1))) - self._bad_reported
        self._bad_reported += max(bad, 0)
        if bad > 0:      # utils/loss.py:36 / nn.CrossEntropyLoss raise on such a target; the kernels skip the pixel and count it
            raise ValueError(f"{bad} label value(s) outside [0, {self.hp.num_classes}) that are not the ignore value 255")
        keys = ["total", "loss_p1", "loss_p2", "loss_y1", "loss_y2", "place", "convex", "volume", "anchor", "vol_ok"]
        return dict(zip(keys, v))


def accumulate_pass(tr, k, n, st):
    """Behind the backward of pass k of n > 1 passes into one gradient of a warm-up trainer (hp.iter_size micro-batches; with online_source
    two passes each): the first pass starts the sum in `tr._grad_acc`, the ones between add to it, the last adds the sum to its
    own gradient, where the optimiser reads it -- and under data parallelism the one exchange starts there."""
    flat = tr.plan.flat_grad
    if tr._grad_acc is None:
        tr._grad_acc = torch.zeros_like(flat)
    if k == 0:
        tr._grad_acc.copy_(flat)
    elif k < n - 1:
        L.call("simt_vec_acc", tr._grad_acc.data_ptr(), flat.data_ptr(), flat.numel(), 1, st)
    else:
        L.call("simt_vec_acc", flat.data_ptr(), tr._grad_acc.data_ptr(), flat.numel(), 1, st)
        if tr.reducer is not None:
            tr.reducer.start()
            tr.reducer.finish()


class WarmupTrainer(TrainStateMixin, EmaMixin, OnlineLabelMixin, FeatDistMixin, ProtoContrastMixin, OptimizerMixin):
    """The warm-up stage of the reference (tools/trainV1_warmup.py:156-256) on gfx950: DeeplabMulti(num_classes) without
    open-set heads, loss = CE(up(pred2), label) + lambda_seg * CE(up(pred1), label) with ignore_index 255 (:217-224), SGD over
    conv1 ... layer4 with the duplicate listings of `optim_parameters(args, warmup=True)` + heads at 10x lr (:192-193).
    Same engine as SimTTrainer: TrunkPlan forward/backward, the fused head kernels in mode 1, simt_sgd_multi."""

    def __init__(self, state, hp, B, H, W, *, dtype=torch.bfloat16, device="cuda:0", process_group=None, layers=None, ema_decay=None,
                 online_labels=None, online_labels_every=None, online_labels_balanced=None, online_labels_momentum=None,
                 online_mix=None, online_mix_seed=0, online_labels_weighted=None, online_source=None,
                 feat_dist=None, feat_dist_state=None, feat_dist_classes=None, feat_dist_min_ratio=None,
                 optimizer="sgd", adam_betas=DEFAULT_BETAS, adam_eps=DEFAULT_EPS, lr_warmup=0, lr_warmup_ratio=DEFAULT_WARMUP_RATIO,
                 entropy_min=None, entropy_eta=DEFAULT_ENTROPY_ETA, entropy_after=0, proto_denoise=None, proto_momentum=DEFAULT_PROTO_MOMENTUM,
                 proto_contrast=None, proto_contrast_temp=None, proto_contrast_min_ratio=None, uncertainty_rectify=None):
        """optimizer / adam_betas / adam_eps / lr_warmup / lr_warmup_ratio: as for SimTTrainer; the defaults are the trainer it was.
        online_labels=tau in [0, 1) (simt_amd/online_labels.py): the labels of every micro-batch come from a teacher -- a
        closed-set eval-mode plan over a copy of `state`, with an input and a stem launch of its own -- kept where its confidence is > tau;
        online_labels_every=N (needs ema_decay): that teacher follows the weight EMA behind every N-th update.  None: the trainer it was.
        online_labels_balanced=P in (0, 1] (needs online_labels): one threshold per class, kept on the device -- it starts at tau and
        every micro-batch moves it towards the value that keeps the share P of that class's pixels, never above tau, with momentum
        online_labels_momentum=M in [0, 1) (default 0.9).  None: the one threshold tau.
        online_mix=P in (0, 1] (needs online_labels, 2 <= B <= 32, num_classes <= 32): ClassMix by the teacher's labels, behind
        the teacher and in front of the student's forward -- with probability P item i receives, image and label, the pixels of half of the
        classes the teacher found in item (i + 1) % B.  The draws are those of simt_amd.data.class_mix (`generator(online_mix_seed, rank)`,
        one `draw_batch` per micro-batch).  `labelled` and `label_thresholds` stay statistics of the teacher's labels BEFORE the mix, as the
        label launch counts them.  None: the trainer it was -- no buffer, no launch, no draw.
        online_labels_weighted="batch" | "item" (needs online_labels, not with online_labels_balanced, B <= 32): the rule of DACS /
        DAFormer / MIC -- the student trains on the teacher's arg-max at EVERY pixel and each pixel's cross-entropy is multiplied by q, the share
        of the micro-batch's ("batch", the published rule) or of its item's ("item") pixels whose confidence is above online_labels; the
        threshold deletes nothing.  With online_mix in "item" mode a pasted pixel carries its partner's q.  `labelled` keeps its meaning (the
        share of confident pixels); `losses()` gains `label_quality`.  None: the trainer it was.
        online_source=True (needs online_labels): the published DACS step -- every micro-batch is two passes into one gradient,
        supervised cross-entropy on a labelled source pair (`step(source_image=, source_label=)`), then the target pass above; with
        online_mix the mix pastes half of SOURCE item i's classes, image and ground truth, onto target item i (simt_source_mix), and with
        online_labels_weighted a pasted pixel has weight 1.  `losses()` gains `source_seg1` / `source_seg2`.  None / False: the trainer it was.
        feat_dist=lambda >= 0 (simt_amd/feat_dist.py; needs feat_dist_state, and with online_labels also online_source): DAFormer's
        thing-class ImageNet feature distance -- the pass with ground-truth labels (the source pass; without online_labels the only pass) adds
        lambda * the mean L2 distance between the student's layer-4 output and that of a frozen eval-mode trunk over `feat_dist_state`, over the
        cells one class of `feat_dist_classes` (default: DAFormer's ten thing classes of the 19) fills to `feat_dist_min_ratio` (default 0.75);
        its gradient enters the backward at layer 4's output.  `losses()` gains `feat_dist` / `feat_dist_cells`.  None: the trainer it was.
        entropy_min=lambda > 0 (needs online_labels): FDA's robust entropy term on the target pass, inside the fused head -- every
        pixel, labelled or not, adds lambda * (e^2 + 1e-8)^entropy_eta / (B H W) with e its softmax entropy / ln(C) (entropy_eta = 2: FDA's
        penalty; 0.5: ADVENT's MinEnt), from iteration entropy_after on (FDA's switch2entropy); the source pass of online_source never carries
        it.  `losses()` gains `entropy1` / `entropy2` while it is on.  None: the trainer it was.
        proto_denoise=temp > 0 (simt_amd/proto.py; needs online_labels): ProDA's prototype weights -- the teacher's low-res posterior
        is weighed by softmax(-(d - d_min) / temp), d the distance of the cell's layer-4 feature to running class prototypes (momentum
        proto_momentum, default 0.9999), in front of the label launch of every mode; a batch is labelled with the prototypes of the batches
        before it.  `losses()` gains `proto_seen` / `proto_changed`.  None: the trainer it was.
        proto_contrast=lambda >= 0 (simt_amd/proto_contrast.py; needs proto_denoise, refused with feat_dist): the prototype contrastive
        term of SePiCo / ProDA -- every pass adds lambda * the mean over the valid layer-4 cells of -log softmax_seen(cos(f, eta_c) / T)[y], f the
        STUDENT's layer-4 output, eta the prototypes of proto_denoise, y the class that fills the cell's window of the pass's labels to
        proto_contrast_min_ratio (default 0.75), T = proto_contrast_temp (default 0.1); its gradient enters the backward at layer 4's output.
        proto_denoise=1e30 leaves the labels all but untouched for a user who wants the contrast alone.  `losses()` gains `proto_contrast` /
        `proto_contrast_cells` (and `source_proto_contrast` with online_source).  None: the trainer it was.
        uncertainty_rectify=lambda_kl >= 0 (with or without online_labels, refused beside entropy_min): Zheng & Yang's rectification
        of noisy pseudo labels, inside the fused head -- D_k, the KL divergence of head k from the other head at a pixel, is the label's
        uncertainty: the pixel's cross-entropy is multiplied by exp(-D_k) and lambda_kl * mean(D_k) is added, for both heads, the gradient flowing
        through both arguments.  It applies to every pass whose labels are not ground truth (the only pass without online_source, the target pass
        with it), with the weights and the map of the launches it replaces.  `losses()` gains `uncertainty1/2` and `rectify1/2`, and
        `loss_seg1/2` are the rectified cross-entropies.  None: the trainer it was."""
        tau, every = check_settings(online_labels, online_labels_every, ema_decay)
        balanced = check_balanced(online_labels_balanced, online_labels_momentum, tau, hp.num_classes)
        mix = check_mix(online_mix, online_mix_seed, tau, B, hp.num_classes)
        weighted = check_weighted(online_labels_weighted, tau, balanced[0], B)
        source = check_source(online_source, tau)
        entropy = check_entropy(entropy_min, entropy_eta, entropy_after, tau)
        uncertain = check_uncertainty(uncertainty_rectify, entropy[0])
        fd = check_feat_dist(feat_dist, feat_dist_state, feat_dist_classes, feat_dist_min_ratio, tau, source, hp.num_classes)
        proto = check_proto(proto_denoise, proto_momentum, tau, hp.num_classes)
        pc = check_proto_contrast(proto_contrast, proto_contrast_temp, proto_contrast_min_ratio, proto[0], fd[0], hp.num_classes)
        self.hp, self.B, self.H, self.W, self.dtype = hp, B, H, W, dtype
        dev = self.dev = torch.device(device)
        self.pg = process_group
        Cn = self.C = hp.num_classes
        f32 = torch.float32
        self.params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
        kw = {"layers": layers} if layers is not None else {}
        if fd[0] is not None or pc[0] is not None:      # (only then: without the keyword the plan is built by the call it always was)
            kw["feat_grad_seed"] = True
        self.plan = TrunkPlan(self.params, B, H, W, multi_heads(Cn, 0, False), dtype=dtype, train=True,
                              data_parallel=process_group is not None, **kw)
        kw.pop("feat_grad_seed", None)
        h, w = self.h, self.w = self.plan.heads[1].h, self.plan.heads[1].w
        if tau is not None:      # the teacher: the frozen plan of SimTTrainer(teacher_view=True) -- stem_from=None: its own x_in and stem launch
            self.fixed_params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
            self.frozen_sha256 = state_sha256(self.fixed_params)      # a train state is refused beside another start model (train_state.py)
            self.fixed = TrunkPlan(self.fixed_params, B, H, W, multi_heads(Cn, 0, False), dtype=dtype, train=False, stem_from=None,
                                   data_parallel=process_group is not None, **kw)
            self._fix_fwd = self.fixed.fwd_list
        lib = L.load()
        self.part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Cn, Cn), device=dev)
        self.keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
        self.hout = torch.zeros(lib.simt_head_hout_floats(Cn, Cn), device=dev)
        # labels outside [0, C) other than 255, ACCUMULATED over every micro-batch of every step until losses() reads and clears it (hout[15]
        # itself is overwritten by each head launch; nn.CrossEntropyLoss(ignore_index=255) raises on the first one, trainV1_warmup.py:217-224)
        self.bad_labels = torch.zeros(1, device=dev)
        self._bad_reported = 0
        self.QP = ops.round_up(Cn, 8)
        self.g1 = torch.zeros(2, B, H, w, self.QP, device=dev)
        self.label = torch.zeros(B, H, W, device=dev, dtype=torch.int64)
        hd = L.HeadDesc()
        d1, d2 = self.plan.dlogits["x1"], self.plan.dlogits["x2"]
        hd.pred1, hd.pred2, hd.fixp, hd.label = self.plan.out["x1"].data_ptr(), self.plan.out["x2"].data_ptr(), None, self.label.data_ptr()
        hd.T1, hd.T2 = None, None
        hd.part, hd.keys, hd.hout, hd.g1 = self.part.data_ptr(), self.keys.data_ptr(), self.hout.data_ptr(), self.g1.data_ptr()
        hd.dpred1_f32, hd.dpred2_f32, hd.dpred1_t, hd.dpred2_t = None, None, d1.data_ptr(), d2.data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Cn, Cn
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t = self.plan.ldp["x1"], self.plan.ldp["x1"], self.QP, 0, d1.shape[1]
        hd.grad_dtype = ops.dt_code(dtype)
        hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, hp.lambda_seg, 0.0, 1.0 / hp.iter_size
        hd.mode = 1
        self.head_desc = hd
        self._build_sgd(sgd_listing(self.plan.grads.keys(), roots=("conv1", "layer1", "layer2", "layer3", "layer4")))
        self._init_optimizer(optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio)
        self.it_done = 0
        self._init_ema(ema_decay)
        fix = (self.fixed.out["x2"], self.fixed.ldp["x2"]) if tau is not None else (None, 0)
        self._init_online(tau, every, *fix, 0, balanced)      # (family 0: the posterior is resampled align_corners=True)
        self._init_mix(mix)
        self._init_weighted(weighted)
        self._init_source(source)
        self._init_entropy(entropy)
        self._init_uncertainty(uncertain)
        # the input of the teacher's layer-4 classifier -- the last block's output, which no later launch of the eval plan overwrites
        self._init_proto(proto, next(hd for hd in self.fixed.heads if hd.name == "x2").feat if proto[0] is not None else None)
        self._init_feat_dist(*fd, feat_dist_state, dict(kw, data_parallel=process_group is not None))
        self._init_proto_contrast(*pc)
        self.reducer = None
        if self.pg is not None:
            from .dp import BucketReducer, make_buckets
            sizes = {n: k for n, (_o, k) in self.plan.grad_offsets.items()}
            buckets = make_buckets(self.plan.grad_order, sizes, self.plan.grad_ready, bucket_elems=8 << 20)
            self.reducer = BucketReducer(self.plan.flat_grad, buckets, group=self.pg, extra=[self.bad_labels])
        self._grad_acc = None

    def step(self, image, label=None, it=None, teacher_image=None, source_image=None, source_label=None):
        """One micro-batch, or sequences of hp.iter_size micro-batches (trainV1_warmup.py:212-231: loss / iter_size,
        gradients accumulated, one optimiser step).  Built with online_labels: `label` must be None (the labels come from the teacher),
        teacher_image is the teacher's view (None: it sees `image`); sequences like image when hp.iter_size > 1.  Built with online_source:
        source_image [B,3,H,W] / source_label [B,H,W] int64 are the labelled source pair of every micro-batch (sequences likewise); refused
        without the keyword."""
        hp = self.hp
        it = self.it_done if it is None else it
        lr = lr_at(hp.lr, it, hp.num_steps, hp.power, self.lr_warmup, self.lr_warmup_ratio)
        st = ops.stream_ptr()
        self._entropy_at(it)      # whether this iteration's target passes carry the entropy term (entropy_after)
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        labels, teachers = self._views(label, teacher_image, hp.iter_size)
        src_images, src_labels = self._sources(source_image, source_label, hp.iter_size)
        if len(images) != hp.iter_size or len(labels) != hp.iter_size:
            raise ValueError(f"step() needs {hp.iter_size} micro-batch(es) (hp.iter_size), got {len(images)}")
        # passes into the one gradient: a micro-batch is one, with online_source two (the source pass, then the target pass)
        per = 2 if self.online_source else 1
        n_pass = hp.iter_size * per
        for mi, (img, lab) in enumerate(zip(images, labels)):
            if self.online_source:      # pass a: supervised cross-entropy on the source pair, the plain head launches, into the same gradient
                self._source_input(src_images[mi], src_labels[mi])
                if self.feat_dist is not None:      # the ImageNet forward beside the student's, the term's gradient into this backward
                    ev_fd = self._fd_input()
                self.plan.forward()
                if self.feat_dist is not None:
                    self._fd_forward(ev_fd)
                L.call("simt_head_loss", C.byref(self.head_desc), st)
                L.call("simt_vec_acc", self.bad_labels.data_ptr(), self.hout.data_ptr() + 4 * 15, 1, 1, st)      # the source labels count too
                self._source_kept()
                L.call("simt_head_grad", C.byref(self.head_desc), st)
                if self.feat_dist is not None:
                    self._fd_launches(st)
                    self.plan.use_feat_seed(True)
                if self.proto_contrast is not None:      # the source pass's term, on the prototypes before this micro-batch's update
                    self._pc_launches(st, source=True)
                self.plan.backward()
                accumulate_pass(self, mi * per, n_pass, st)
            if self.online_mix is not None:      # the mix writes plan.x_in and self.label itself, behind the teacher (main stream): no input copy
                self._mixed_batch(img, teachers[mi])
                self.plan.forward()
            elif self.online_labels is None:
                self.plan.x_in.copy_(img, non_blocking=True)
                self.label.copy_(lab, non_blocking=True)
                if self.feat_dist is not None:      # the only pass has the ground truth
                    ev_fd = self._fd_input()
                self.plan.forward()
                if self.feat_dist is not None:
                    self._fd_forward(ev_fd)
            else:          # the teacher writes self.label on the side stream, beside the student's forward; the main stream waits for it here
                self.plan.x_in.copy_(img, non_blocking=True)
                ev_in = self._teacher_input(img, teachers[mi])
                self.plan.forward()
                self._teacher_labels(ev_in)
            self._head_loss(st)          # simt_head_loss; with online_labels_weighted its weighted form (OnlineLabelMixin)
            L.call("simt_vec_acc", self.bad_labels.data_ptr(), self.hout.data_ptr() + 4 * 15, 1, 1, st)      # every micro-batch counts
            self._head_grad(st)
            if self.feat_dist is not None:
                if self.online_labels is None:
                    self._fd_launches(st)
                else:      # the target pass under online_source: the seed-less launch, the parent's (the descriptor is read at every launch)
                    self.plan.use_feat_seed(False)
            if self.proto_contrast is not None:      # `self.label` is final (teacher labels, the mix), the teacher's event is waited for
                self._pc_launches(st)
            if self.reducer is not None and n_pass == 1:
                self.reducer.start()
                self.plan.backward(hook=self.reducer.ready_upto)
                self.reducer.finish()
                continue
            self.plan.backward()
            if n_pass > 1:      # the accumulation of hp.iter_size > 1, over passes (accumulate_pass); the exchange behind the last
                accumulate_pass(self, mi * per + per - 1, n_pass, st)
        self._optim_step(lr, st)      # simt_sgd_multi, or simt_adamw_multi in its place (simt_amd/optimizer.py)
        self.plan.repack()
        if self.ema is not None:
            self.ema.update(st)          # main stream, behind SGD and the re-pack, in front of the next step's forward
            # online_labels_every: the teacher's refresh, if this update made one due, directly behind it on the main stream:
            #   behind this step's teacher forward, softmax_rows and label launch (side stream): the main stream waited for their event in
            #   front of simt_head_loss (_teacher_labels);
            #   in front of the next step's teacher forward (side stream): it waits for ev_in, which the main stream records behind this point
            #   (_teacher_input); no main-stream launch reads the teacher plan's operands.
            #   With online_mix the teacher's forward, the label launch and the mix run on the MAIN stream (_mixed_batch): this step's lie in
            #   front of this point and the next step's behind it by stream order alone.
            # Once per optimiser step: this point is behind the last micro-batch.
            self._teacher_follows(st)
        self.it_done += 1
        return self.hout

    def state_dict(self):
        sd = {}
        for k, v in self.params.items():
            sd[k] = (v.detach().cpu() if not k.endswith("num_batches_tracked") else
                     torch.tensor(int(v.item()) + self._nbt_steps(k), dtype=torch.long))
        return sd

    def losses(self):
        """Host copy of the last micro-batch's scalars; local (see SimTTrainer.losses).  The bad-label count covers EVERY micro-batch of every
        step since the last call (a device-side accumulator; under data parallelism it rides in the gradient exchange)."""
        v = torch.cat([self.hout[:16], self.bad_labels]).cpu().tolist()
        self.plan.raise_on_fbn_error()
        bad = int(round(v[16] * (self.reducer.world if self.reducer is not None else 1))) - self._bad_reported      # cumulative, never reset on the device
        self._bad_reported += max(bad, 0)
        if bad > 0:      # nn.CrossEntropyLoss(ignore_index=255) raises on such a target (trainV1_warmup.py:217-224)
            raise ValueError(f"{bad} label value(s) outside [0, {self.hp.num_classes}) that are not the ignore value 255")
        # `loss = loss / args.iter_size` (trainV1_warmup.py:227): the reported total is the scaled one, like SimTTrainer's
        return self._pc_losses(self._fd_losses(self._uncertainty_losses(
            self._labelled({"total": v[14] / self.hp.iter_size, "loss_seg1": v[0], "loss_seg2": v[1]}))))
