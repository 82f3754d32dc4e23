"""SimT training iteration over a ONE-OUTPUT model on gfx950: DeepLabv3 (model/deeplabv3.py, BASELINE configs[3]) and DeepLab-VGG16
(model/deeplab_vgg.py, configs[4]).

The reference has exactly one SimT loop (tools/trainV2_simt.py:308-436), written for the two-output DeeplabMulti; no script trains
these two model files.  The iteration run here is that loop with every auxiliary-head object removed (pred1, NTM1, NTM_W1 and the
lambda_seg-weighted terms they feed), i.e. term by term the reference's code applied to the model's single output:

    total = Place(pred) + CE(pred, Conf) + NLL(log(softmax(pred) @ T), noisy label)
            + lambda_convex * (-||W T||^2) + lambda_volume * log sqrt|det T^T T| + lambda_anchor * Anchor(T)

(oracle: `oracle.simt_oracle.simt_losses_single`, tied to the golden-pinned two-head restatement by an identity test).  Model facts
that matter to the fused head kernel (csrc/head_loss.hip, simt_head_desc.single / up_half_pixel / fix_logits):
  * DeepLabv3 upsamples INSIDE the model with F.interpolate(bilinear), align_corners=False (deeplabv3.py:137); the script's
    interp_target on the full-resolution tensor is then the identity, and the frozen model's posterior is
    softmax(upsample(logits)).  The kernel consumes the low-res logits and applies the half-pixel taps itself; the 210 MB
    full-resolution logits tensor and its adjoint are never written.
  * DeeplabVGG returns low-res logits; interp_target (align_corners=True) and softmax-then-upsample as for DeepLab-v2.
Optimiser: the model's own optim_parameters (deeplabv3.py:139-166: layer3 at lr, ASSP + classifiers at 10 lr, each tensor listed
once; deeplab_vgg.py:53-54: every parameter, one group), SGD momentum / weight decay as in trainV2_simt.py:296-297; Adam on NTM.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ema import EmaMixin
from .ema_teacher import TeacherMixin
from .engine import LaunchList, side_stream
from .online_labels import (DEFAULT_ENTROPY_ETA, OnlineLabelMixin, check_balanced, check_entropy, check_mix, check_settings, check_source,
                            check_weighted)
from .proto import DEFAULT_MOMENTUM as DEFAULT_PROTO_MOMENTUM, check_proto
from .optimizer import DEFAULT_BETAS, DEFAULT_EPS, DEFAULT_WARMUP_RATIO, OptimizerMixin
from .step import accumulate_pass, check_views, lr_at, lr_poly
from .train_state import TrainStateMixin, state_sha256


class SimTSingleTrainer(TrainStateMixin, EmaMixin, TeacherMixin, OptimizerMixin):
    def __init__(self, model, state, fixed_state, ntm, hp, class_dist, B, H, W, *, dtype=torch.bfloat16, device="cuda:0",
                 process_group=None, arch=None, ema_decay=None, ema_teacher_every=None, teacher_view=False,
                 optimizer="sgd", adam_betas=DEFAULT_BETAS, adam_eps=DEFAULT_EPS, lr_warmup=0, lr_warmup_ratio=DEFAULT_WARMUP_RATIO):
        """optimizer / adam_betas / adam_eps / lr_warmup / lr_warmup_ratio: as for step.SimTTrainer; the BatchNorm gamma and beta
        this trainer trains go without weight decay under "adamw".  The defaults are the trainer it was.
        model: "v3" | "vgg".  state: the trainable model's state_dict tensors (DeepLabv3(nc, openc, openset=True) /
        DeeplabVGG(nc + openc)); fixed_state: the frozen model's (nc outputs).  arch: plan keyword arguments (reduced depths / widths
        for tests): v3 -> layers, width, assp_ch; vgg -> vgg_layers.  teacher_view: as for SimTTrainer (the frozen plan has an input of its
        own here already: the weak view is copied into it instead of the trainable plan's image)."""
        assert model in ("v3", "vgg")
        self.model, self.hp, self.B, self.H, self.W, self.dtype = model, hp, B, H, W, dtype
        self.teacher_view = bool(teacher_view)
        dev = self.dev = torch.device(device)
        self.pg = process_group
        Cn, K = hp.num_classes, hp.open_classes
        self.C, self.Q = Cn, Cn + K
        Q = self.Q
        f32 = torch.float32
        conv = lambda d: {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in d.items()}
        self.params, self.fixed_params = conv(state), conv(fixed_state)
        self.frozen_sha256 = state_sha256(self.fixed_params)      # a train state is refused beside another frozen model (train_state.py)
        arch = dict(arch or {})
        if model == "v3":
            from .engine_v3 import V3Plan
            self.plan = V3Plan(self.params, B, H, W, Cn, K, True, dtype=dtype, train=True, data_parallel=process_group is not None, **arch)
            self.fixed = V3Plan(self.fixed_params, B, H, W, Cn, 0, False, dtype=dtype, train=False, **arch)
            # the in-model upsample (last forward launch) and its adjoint (first backward launch) are fused into the head kernel
            assert self.plan.fwd_list.items[-1].tag == "simt_upsample_nchw" and self.fixed.fwd_list.items[-1].tag == "simt_upsample_nchw"
            self._fwd, self._fix_fwd, self._bwd = LaunchList(), LaunchList(), LaunchList()
            self._fwd.items = self.plan.fwd_list.items[:-1]
            self._fix_fwd.items = self.fixed.fwd_list.items[:-1]
            i0 = next(i for i, it in enumerate(self.plan.bwd_list.items) if it.tag == "simt_upsample_nchw_bwd")
            self._bwd.items = self.plan.bwd_list.items[:i0] + self.plan.bwd_list.items[i0 + 1:]
            (h, w) = self.plan.feat_hw
            self.pred, self.ldp = self.plan.logits, self.plan.ldq
            self.fix_logits_t, self.ldf = self.fixed.logits, self.fixed.ldq
            dl = self.plan.dlogits["x"]
            half, fix_logits = 1, 1
        else:
            from .engine_vgg import VggPlan
            self.plan = VggPlan(self.params, B, H, W, Q, dtype=dtype, train=True, data_parallel=process_group is not None, **arch)
            self.fixed = VggPlan(self.fixed_params, B, H, W, Cn, dtype=dtype, train=False, **arch)
            self._fwd, self._fix_fwd, self._bwd = self.plan.fwd_list, self.fixed.fwd_list, self.plan.bwd_list
            h, w = self.plan.heads[0].h, self.plan.heads[0].w
            self.pred, self.ldp = self.plan.out["x"], self.plan.ldp["x"]
            self.fix_logits_t, self.ldf = self.fixed.out["x"], self.fixed.ldp["x"]
            dl = self.plan.dlogits["x"]
            half, fix_logits = 0, 0
        self.h, self.w = h, w
        self.grad_ready = self.plan.grad_ready
        # ---- NTM / W (index [1] of the two-slot descriptors; slot [0] = the auxiliary head, absent here)
        self.ntm = ntm.detach().to(dev, f32).clone()
        self._xchg = torch.zeros(16 + Q * Cn, device=dev)      # [lout | dNTM]: lout[12:] + dNTM is ONE collective under data parallelism (step.py)
        self.ntm_grad = self._xchg[16:].view(Q, Cn)
        self.ntm_m, self.ntm_v = torch.zeros(Q, Cn, device=dev), torch.zeros(Q, Cn, device=dev)
        self.wraw = torch.full((Q, Q), 1.0 / (Q - 1.0), device=dev)
        self.w_m, self.w_v = torch.zeros(Q, Q, device=dev), torch.zeros(Q, Q, device=dev)
        self.T = torch.zeros(Q, Cn, device=dev)
        self.cd = torch.as_tensor(np.asarray(class_dist), dtype=f32).to(dev)
        self.inner_steps = 10
        lib = L.load()
        self.part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Cn), device=dev)
        self.keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
        self.hout = torch.zeros(lib.simt_head_hout_floats(Q, Cn), device=dev)
        self.lout = self._xchg[:16]
        self._bad_reported = 0
        self.QP = ops.round_up(Q, 8)
        self.g1 = torch.zeros(2, B, H, w, self.QP, device=dev)
        self.fixp = self.fix_logits_t if fix_logits else torch.zeros(B * h * w, self.ldf, device=dev)
        self.label = torch.zeros(B, H, W, device=dev, dtype=torch.int64)
        hd = L.HeadDesc()
        hd.pred1, hd.pred2, hd.fixp, hd.label = None, self.pred.data_ptr(), self.fixp.data_ptr(), self.label.data_ptr()
        hd.T1, hd.T2 = None, self.T.data_ptr()
        hd.part, hd.keys, hd.hout, hd.g1 = self.part.data_ptr(), self.keys.data_ptr(), self.hout.data_ptr(), self.g1.data_ptr()
        hd.dpred1_f32, hd.dpred2_f32, hd.dpred1_t, hd.dpred2_t = None, None, None, dl.data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Cn, Q
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t = self.ldp, self.ldf, self.QP, 0, dl.shape[1]
        hd.grad_dtype = ops.dt_code(dtype)
        hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place = hp.th_high, hp.th_low, 0.0, hp.lambda_place
        hd.gscale, hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1.0 / hp.iter_size, 0, 1, half, fix_logits
        self.conf_label = torch.full((B, H, W), 255, device=dev, dtype=torch.uint8)      # per-pixel Conf_label_target, 255 = none
        hd.conf_out = self.conf_label.data_ptr()
        self._label_ws = torch.full((B, H, W), 255, device=dev, dtype=torch.uint8)          # checked noisy labels, loss pass -> gradient pass
        hd.label_ws = self._label_ws.data_ptr()
        self.head_desc = hd
        self.fix_item = torch.zeros(B, H, W, device=dev, dtype=torch.uint8) if self.teacher_view else None      # (step.SimTTrainer)
        ni = L.NtmInnerDesc()
        ni.ntm[1], ni.w[1], ni.ntm_grad[1] = self.ntm.data_ptr(), self.wraw.data_ptr(), self.ntm_grad.data_ptr()
        ni.w_m[1], ni.w_v[1], ni.T_out[1] = self.w_m.data_ptr(), self.w_v.data_ptr(), self.T.data_ptr()
        ni.class_dist, ni.Q, ni.C, ni.steps, ni.single = self.cd.data_ptr(), Q, Cn, self.inner_steps, 1
        ni.beta1, ni.beta2, ni.eps = 0.9, 0.999, 1e-8
        # every optimiser launch is guarded by the plan's sticky fused-BatchNorm error word (engine.TrunkPlan.fbn_error): once a fused launch has
        # given up polling, SGD, both Adams and the W inner loop change nothing -- a state_dict saved after losses() raised holds the last good state
        self._skip_word = getattr(self.plan, "fbn_err", None)
        if self._skip_word is not None:
            ni.skip_if = self._skip_word.data_ptr()
        self.inner_desc = ni
        npd = L.NtmPostDesc()
        npd.ntm[1], npd.w[1], npd.ntm_grad[1] = self.ntm.data_ptr(), self.wraw.data_ptr(), self.ntm_grad.data_ptr()
        npd.class_dist, npd.hout, npd.lout, npd.Q, npd.C = self.cd.data_ptr(), self.hout.data_ptr(), self.lout.data_ptr(), Q, Cn
        npd.lambda_seg, npd.lambda_convex, npd.lambda_volume = 0.0, hp.lambda_convex, hp.lambda_volume
        npd.lambda_anchor, npd.gscale, npd.single = hp.lambda_anchor, 1.0 / hp.iter_size, 1
        self.post_desc = npd
        self._build_sgd([(n, 1, group) for group, names in enumerate(self.optim_groups()) for n in names])      # every tensor listed once
        self._init_optimizer(optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio)
        self.it_done = 0
        self._init_ema(ema_decay)          # ema_decay=None: no shadow, no launch (simt_amd/ema.py)
        # None: the frozen model never moves (simt_amd/ema_teacher.py).  DeeplabVGG has ONE classifier of Cn + K rows: the frozen model's Cn rows
        # follow the leading Cn rows of its shadow
        self._init_teacher(ema_teacher_every, prefix_rows=K if model == "vgg" else 0)
        self.reducer = None
        if self.pg is not None:
            from .dp import BucketReducer, make_buckets
            sizes = {n: k for n, (_o, k) in self.plan.grad_offsets.items()}
            buckets = make_buckets(self.plan.grad_order, sizes, self.plan.grad_ready, bucket_elems=8 << 20)
            self.reducer = BucketReducer(self.plan.flat_grad, buckets, group=self.pg, extra=[self._xchg[12:]])

    # ------------------------------------------------------------------ optimiser
    def optim_groups(self):
        """(group 0 names, group 1 names) per the model's optim_parameters; only tensors that receive a gradient are kept."""
        names = [n for n in self.plan.grads if self.plan.grad_ready.get(n, 0) > 0]
        if self.model == "v3":
            g0 = [n for n in names if n.startswith("resnet.resnet_50.layer3.")]
            g1 = [n for n in names if n.startswith(("assp.", "conv.", "conv_1."))]
            return g0, g1
        return names, []

    # ------------------------------------------------------------------ one iteration
    def step(self, image, label, it=None, teacher_image=None, fix_item=None):
        hp = self.hp
        assert hp.iter_size == 1, "gradient accumulation is implemented for the DeepLab-v2 trainer only"
        (teacher_image,), (fix_item,) = check_views(self, teacher_image, fix_item, 1)
        it = self.it_done if it is None else it
        lr = lr_at(hp.lr, it, hp.num_steps, hp.power, self.lr_warmup, self.lr_warmup_ratio)
        lr_T = lr_poly(hp.lr_T, it, hp.num_steps, hp.power)      # (not warmed up: DESIGN 7.23)
        st = ops.stream_ptr()
        main, side = torch.cuda.current_stream(), side_stream(self.dev)
        ev0 = torch.cuda.Event()
        ev0.record(main)
        self.plan.x_in.copy_(image, non_blocking=True)
        self.label.copy_(label, non_blocking=True)
        item_ptr = None
        if self.teacher_view:      # the weak view and its map: main stream, in front of ev_in
            self.fixed.x_in.copy_(teacher_image, non_blocking=True)
            if fix_item is not None:
                self.fix_item.copy_(fix_item, non_blocking=True)
                item_ptr = self.fix_item.data_ptr()
        ev_in = torch.cuda.Event()
        ev_in.record(main)
        with torch.cuda.stream(side):
            # W inner loop (T, W for the head; its leak into dNTM) and the frozen model's forward, beside the trainable forward
            side.wait_event(ev0)
            self.ntm_grad.zero_()
            ni = self.inner_desc
            ni.step0, ni.lr = self.inner_steps * self.it_done, lr_T
            L.call("simt_ntm_inner_loop", C.byref(ni), side.cuda_stream)
            side.wait_event(ev_in)
            if not self.teacher_view:
                self.fixed.x_in.copy_(self.plan.x_in, non_blocking=True)
            self._fix_fwd.run()
            if not self.head_desc.fix_logits:
                ops.softmax_rows(self.fix_logits_t, self.ldf, self.fixp, self.ldf, self.B * self.h * self.w, self.C)
            ev_fix = torch.cuda.Event()
            ev_fix.record(side)
        self._fwd.run()
        main.wait_event(ev_fix)
        L.call("simt_head_loss_views", C.byref(self.head_desc), item_ptr, st)
        ev_loss = torch.cuda.Event()
        ev_loss.record(main)
        with torch.cuda.stream(side):          # the regularisers only feed Adam and the loss read-out: beside the head's gradient pass
            side.wait_event(ev_loss)
            L.call("simt_ntm_post", C.byref(self.post_desc), side.cuda_stream)
            ev_post = torch.cuda.Event()
            ev_post.record(side)
        L.call("simt_head_grad_views", C.byref(self.head_desc), item_ptr, st)
        if self.reducer is not None:
            self.reducer.start()
            self._bwd.run()
            main.wait_event(ev_post)           # the NTM gradients it exchanges (side stream)
            self.reducer.finish()
        else:
            self._bwd.run()
        self._optim_step(lr, st)      # simt_sgd_multi, or simt_adamw_multi in its place (simt_amd/optimizer.py)
        main.wait_event(ev_post)
        ops.adam_step(self.ntm, self.ntm_grad, self.ntm_m, self.ntm_v, lr=lr_T, step=self.it_done + 1, skip_if=self._skip_word)
        self.plan.repack()
        if self.ema is not None:
            self.ema.update(st)          # main stream, behind SGD and the re-pack; the next step's side-stream work waits for ev0 (main) first
            # the EMA teacher's refresh, if due, directly behind it on the main stream: behind this step's frozen forward (side stream; the main
            # stream waited for ev_fix in front of the head) and in front of the next one (the side stream waits for ev0, recorded on the main
            # stream at the start of the next step); no main-stream launch reads the frozen plan's operands
            self._teacher_follows(st)
        self.it_done += 1
        return self.lout

    def state_dict(self):
        """Host copy of the trainable model's state, the counterpart of SimTTrainer.state_dict: every key the trainer was given, fp32 (int64
        for `num_batches_tracked`).  Trained tensors and running statistics are the current ones; keys the plan never touches (DeepLabv3's
        layer4 / fc, DeeplabVGG's classifier branches 2 and 3) come back as given.  `num_batches_tracked` grows by the number of steps
        taken for the BatchNorms that run (nn.BatchNorm2d bumps it once per train-mode forward; DeepLabv3._dead_bns: not layer4's)."""
        sd = {}
        for k, v in self.params.items():
            if k.endswith(".num_batches_tracked"):
                sd[k] = torch.tensor(int(v.item()) + self._nbt_steps(k), dtype=torch.long)
            else:
                sd[k] = v.detach().cpu()
        return sd

    def timed_lists(self):
        return [self._fix_fwd, self._fwd, self._bwd]

    def losses(self):
        """Local (no collective): see SimTTrainer.losses."""
        v = self.lout.cpu().tolist()                  # ONE device-to-host copy: the scalars and the bad-label count (lout[12])
        self.plan.raise_on_fbn_error()
        # accumulated by simt_ntm_post since the last call; data parallel: the gradient exchange leaves total / world on every rank
        bad = int(round(v[12] * (self.reducer.world if self.reducer is not None else 1))) - self._bad_reported      # cumulative, never reset on the device
        self._bad_reported += max(bad, 0)
        if bad > 0:      # the reference's nll_loss raises on such a target; the kernels skip the pixel and count it
            raise ValueError(f"{bad} label value(s) outside [0, {self.hp.num_classes}) that are not the ignore value 255")
        return {"total": v[0], "loss_p": v[2], "loss_y": v[4], "place": v[5], "convex": v[6], "volume": v[7], "anchor": v[8],
                "vol_ok": v[9]}


class WarmupSingleTrainer(TrainStateMixin, EmaMixin, OnlineLabelMixin, OptimizerMixin):
    """The warm-up stage (tools/trainV1_warmup.py:156-256) over a ONE-OUTPUT model: DeepLabv3(nc) or DeeplabVGG(nc), trained by cross-entropy
    on the pseudo labels, loss = CE(interp_target(model(x)), label) with ignore_index 255 (:212-231 without the auxiliary head; for
    DeepLabv3 interp_target is the identity behind the in-model upsample), / iter_size with the gradients accumulated over hp.iter_size
    micro-batches and one SGD step.  The checkpoint it writes is what the SimT stage restores (trainV2_simt --model DeepLabv3 | DeepLabVGG).
    Engine: the plans of SimTSingleTrainer, the fused head kernels in their one-head warm-up flavour (simt_head_desc single = 1, mode = 1),
    the model's own optim_parameters through SimTSingleTrainer.optim_groups, OptimizerMixin._build_sgd, simt_sgd_multi."""

    def __init__(self, model, state, hp, B, H, W, *, dtype=torch.bfloat16, device="cuda:0", process_group=None, arch=None, ema_decay=None,
                 online_labels=None, online_labels_every=None, online_labels_balanced=None, online_labels_momentum=None,
                 online_mix=None, online_mix_seed=0, online_labels_weighted=None, online_source=None,
                 feat_dist=None, feat_dist_state=None, feat_dist_classes=None, feat_dist_min_ratio=None,
                 optimizer="sgd", adam_betas=DEFAULT_BETAS, adam_eps=DEFAULT_EPS, lr_warmup=0, lr_warmup_ratio=DEFAULT_WARMUP_RATIO,
                 entropy_min=None, entropy_eta=DEFAULT_ENTROPY_ETA, entropy_after=0, proto_denoise=None, proto_momentum=DEFAULT_PROTO_MOMENTUM,
                 proto_contrast=None, proto_contrast_temp=None, proto_contrast_min_ratio=None, uncertainty_rectify=None):
        """model: "v3" | "vgg".  state: the model's state_dict tensors (DeepLabv3(nc) / DeeplabVGG(nc), nc = hp.num_classes).  arch: plan
        keyword arguments, as for SimTSingleTrainer.  optimizer / adam_betas / adam_eps / lr_warmup / lr_warmup_ratio: as for SimTSingleTrainer
        (DESIGN 7.23).  online_labels / online_labels_every / online_labels_balanced /
        online_labels_momentum: as for step.WarmupTrainer; the
        teacher is the frozen plan of SimTSingleTrainer (DeepLabv3: without its last launch, the in-model upsample).  online_mix /
        online_mix_seed: ClassMix by the teacher's labels, as for step.WarmupTrainer; `labelled` and `label_thresholds` stay
        statistics of the teacher's labels before the mix.  online_labels_weighted: the quality weights of DACS, as for step.WarmupTrainer
        (DESIGN 7.19).  online_source: a labelled source pair in every micro-batch, as for step.WarmupTrainer.
        feat_dist*: refused -- the ImageNet feature distance is built for DeepLab-v2 (step.WarmupTrainer) only.
        entropy_min / entropy_eta / entropy_after: the entropy term of the target pass, as for step.WarmupTrainer (one head:
        `entropy2` only).  proto_denoise / proto_momentum: ProDA's prototype weights in front of the label launch, as for step.WarmupTrainer
        (DESIGN 7.26); the features are the trunk output the ASSP reads (DeepLabv3) or fc7's output (DeepLab-VGG16).
        proto_contrast*: refused -- the prototype contrastive term needs the seeded backward of DeepLab-v2 (step.WarmupTrainer).
        uncertainty_rectify: refused -- the uncertainty is the KL divergence between DeepLab-v2's two heads, and this model has one."""
        assert model in ("v3", "vgg")
        if uncertainty_rectify is not None:
            raise ValueError("uncertainty_rectify: the label uncertainty is the KL divergence between the two classifier heads of DeepLab-v2 "
                             "(WarmupTrainer); DeepLabv3 and DeepLab-VGG16 (WarmupSingleTrainer) have one head (DESIGN 7.28)")
        for name, v in (("proto_contrast", proto_contrast), ("proto_contrast_temp", proto_contrast_temp), ("proto_contrast_min_ratio", proto_contrast_min_ratio)):
            if v is not None:
                raise ValueError(f"{name}: the prototype contrastive term is built for DeepLab-v2 (WarmupTrainer) only; DeepLabv3 and DeepLab-VGG16 "
                                 "(WarmupSingleTrainer) have no seeded backward (DESIGN 7.27, not built)")
        for name, v in (("feat_dist", feat_dist), ("feat_dist_state", feat_dist_state), ("feat_dist_classes", feat_dist_classes),
                        ("feat_dist_min_ratio", feat_dist_min_ratio)):
            if v is not None:
                raise ValueError(f"{name}: the ImageNet feature distance is built for DeepLab-v2 (WarmupTrainer) only; DeepLabv3 and DeepLab-VGG16 "
                                 "(WarmupSingleTrainer) have no seeded backward and no head-less eval plan yet (DESIGN 7.22, not built)")
        tau, every = check_settings(online_labels, online_labels_every, ema_decay)
        balanced = check_balanced(online_labels_balanced, online_labels_momentum, tau, hp.num_classes)
        mix = check_mix(online_mix, online_mix_seed, tau, B, hp.num_classes)
        weighted = check_weighted(online_labels_weighted, tau, balanced[0], B)
        source = check_source(online_source, tau)
        entropy = check_entropy(entropy_min, entropy_eta, entropy_after, tau)
        proto = check_proto(proto_denoise, proto_momentum, tau, hp.num_classes)
        self.model, self.hp, self.B, self.H, self.W, self.dtype = model, hp, B, H, W, dtype
        dev = self.dev = torch.device(device)
        self.pg = process_group
        Cn = self.C = hp.num_classes
        f32 = torch.float32
        self.params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
        arch = dict(arch or {})
        dp = process_group is not None
        if model == "v3":
            from .engine_v3 import V3Plan
            self.plan = V3Plan(self.params, B, H, W, Cn, 0, False, dtype=dtype, train=True, data_parallel=dp, **arch)
            # the in-model upsample and its adjoint are fused into the head kernel, as in SimTSingleTrainer
            assert self.plan.fwd_list.items[-1].tag == "simt_upsample_nchw"
            self._fwd, self._bwd = LaunchList(), LaunchList()
            self._fwd.items = self.plan.fwd_list.items[:-1]
            i0 = next(i for i, it in enumerate(self.plan.bwd_list.items) if it.tag == "simt_upsample_nchw_bwd")
            self._bwd.items = self.plan.bwd_list.items[:i0] + self.plan.bwd_list.items[i0 + 1:]
            h, w = self.plan.feat_hw
            self.pred, self.ldp = self.plan.logits, self.plan.ldq
            half = 1
        else:
            from .engine_vgg import VggPlan
            self.plan = VggPlan(self.params, B, H, W, Cn, dtype=dtype, train=True, data_parallel=dp, **arch)
            self._fwd, self._bwd = self.plan.fwd_list, self.plan.bwd_list
            h, w = self.plan.heads[0].h, self.plan.heads[0].w
            self.pred, self.ldp = self.plan.out["x"], self.plan.ldp["x"]
            half = 0
        self.h, self.w = h, w
        fix_out, ldf = None, 0
        if tau is not None:      # the teacher: a second plan over a copy of the start state, as SimTSingleTrainer builds its frozen one
            self.fixed_params = {k: v.detach().to(dev, f32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
            self.frozen_sha256 = state_sha256(self.fixed_params)      # a train state is refused beside another start model (train_state.py)
            if model == "v3":
                self.fixed = V3Plan(self.fixed_params, B, H, W, Cn, 0, False, dtype=dtype, train=False, **arch)
                assert self.fixed.fwd_list.items[-1].tag == "simt_upsample_nchw"      # the label kernel resamples the low-res logits itself
                self._fix_fwd = LaunchList()
                self._fix_fwd.items = self.fixed.fwd_list.items[:-1]
                fix_out, ldf = self.fixed.logits, self.fixed.ldq
            else:
                self.fixed = VggPlan(self.fixed_params, B, H, W, Cn, dtype=dtype, train=False, **arch)
                self._fix_fwd = self.fixed.fwd_list
                fix_out, ldf = self.fixed.out["x"], self.fixed.ldp["x"]
        dl = self.plan.dlogits["x"]
        lib = L.load()
        self.part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Cn, Cn), device=dev)
        self.keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
        self.hout = torch.zeros(lib.simt_head_hout_floats(Cn, Cn), device=dev)
        # labels outside [0, C) other than 255, accumulated over every micro-batch of every step (hout[15] is per launch; see WarmupTrainer)
        self.bad_labels = torch.zeros(1, device=dev)
        self._bad_reported = 0
        self.QP = ops.round_up(Cn, 8)
        self.g1 = torch.zeros(2, B, H, w, self.QP, device=dev)          # the head-1 half is never written (single = 1)
        self.label = torch.zeros(B, H, W, device=dev, dtype=torch.int64)
        hd = L.HeadDesc()
        hd.pred1, hd.pred2, hd.fixp, hd.label = None, self.pred.data_ptr(), None, self.label.data_ptr()
        hd.T1, hd.T2 = None, None
        hd.part, hd.keys, hd.hout, hd.g1 = self.part.data_ptr(), self.keys.data_ptr(), self.hout.data_ptr(), self.g1.data_ptr()
        hd.dpred1_f32, hd.dpred2_f32, hd.dpred1_t, hd.dpred2_t = None, None, None, dl.data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Cn, Cn
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t = self.ldp, self.ldp, self.QP, 0, dl.shape[1]
        hd.grad_dtype = ops.dt_code(dtype)
        hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, 0.0, 0.0, 1.0 / hp.iter_size
        hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1, 1, half, 0
        self.head_desc = hd
        self._build_sgd([(n, 1, group) for group, names in enumerate(self.optim_groups()) for n in names])      # every tensor listed once
        self._init_optimizer(optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio)
        self.it_done = 0
        self._init_ema(ema_decay)
        self._init_online(tau, every, fix_out, ldf, half, balanced)      # (family 1 = the half-pixel model, DeepLabv3)
        self._init_mix(mix)
        self._init_weighted(weighted)
        self._init_source(source)
        self._init_entropy(entropy)
        # the input of the teacher's main classifier; neither eval plan recycles it (every activation is a buffer of its own)
        self._init_proto(proto, None if proto[0] is None else self.fixed.feat if model == "v3" else self.fixed.heads[0].feat)
        self.reducer = None
        if self.pg is not None:
            from .dp import BucketReducer, make_buckets
            sizes = {n: k for n, (_o, k) in self.plan.grad_offsets.items()}
            buckets = make_buckets(self.plan.grad_order, sizes, self.plan.grad_ready, bucket_elems=8 << 20)
            self.reducer = BucketReducer(self.plan.flat_grad, buckets, group=self.pg, extra=[self.bad_labels])
        self._grad_acc = None

    optim_groups = SimTSingleTrainer.optim_groups

    def step(self, image, label=None, it=None, teacher_image=None, source_image=None, source_label=None):
        """One micro-batch, or sequences of hp.iter_size micro-batches (trainV1_warmup.py:212-231: loss / iter_size, gradients accumulated,
        one optimiser step; under data parallelism one exchange of the accumulated gradient).  Built with online_labels: `label` must be
        None, teacher_image is the teacher's view (None: it sees `image`), as for step.WarmupTrainer.  Built with online_source:
        source_image / source_label are the labelled source pair of every micro-batch, as for step.WarmupTrainer."""
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
                self._fwd.run()
                L.call("simt_head_loss", C.byref(self.head_desc), st)
                L.call("simt_vec_acc", self.bad_labels.data_ptr(), self.hout.data_ptr() + 4 * 15, 1, 1, st)      # the source labels count too
                self._source_kept()
                L.call("simt_head_grad", C.byref(self.head_desc), st)
                self._bwd.run()
                accumulate_pass(self, mi * per, n_pass, st)
            if self.online_mix is not None:      # the mix writes plan.x_in and self.label itself, behind the teacher (main stream): no input copy
                self._mixed_batch(img, teachers[mi])
                self._fwd.run()
            elif self.online_labels is None:
                self.plan.x_in.copy_(img, non_blocking=True)
                self.label.copy_(lab, non_blocking=True)
                self._fwd.run()
            else:          # the teacher writes self.label on the side stream, beside the student's forward; the main stream waits for it here
                self.plan.x_in.copy_(img, non_blocking=True)
                ev_in = self._teacher_input(img, teachers[mi])
                self._fwd.run()
                self._teacher_labels(ev_in)
            self._head_loss(st)          # simt_head_loss; with online_labels_weighted its weighted form (OnlineLabelMixin)
            L.call("simt_vec_acc", self.bad_labels.data_ptr(), self.hout.data_ptr() + 4 * 15, 1, 1, st)      # every micro-batch counts
            self._head_grad(st)
            if self.reducer is not None and n_pass == 1:
                self.reducer.start()
                self._bwd.run()
                self.reducer.finish()
                continue
            self._bwd.run()
            if n_pass > 1:      # the accumulation of hp.iter_size > 1, over passes (step.accumulate_pass); the exchange behind the last
                accumulate_pass(self, mi * per + per - 1, n_pass, st)
        self._optim_step(lr, st)      # simt_sgd_multi, or simt_adamw_multi in its place (simt_amd/optimizer.py)
        self.plan.repack()
        if self.ema is not None:
            self.ema.update(st)          # main stream, behind SGD and the re-pack, in front of the next step's forward
            # online_labels_every: the teacher's refresh, if due, directly behind it on the main stream: behind this step's teacher forward and
            # label launch (side stream; the main stream waited for their event in front of simt_head_loss) and in front of the next ones
            # (the side stream waits for ev_in, recorded on the main stream behind this point); as in step.WarmupTrainer.  With online_mix
            # the teacher's launches and the mix run on the main stream (_mixed_batch): stream order alone
            self._teacher_follows(st)
        self.it_done += 1
        return self.hout

    def state_dict(self):
        """Every key the trainer was given, fp32 (int64 for `num_batches_tracked`); loads strict=True into DeepLabv3(nc) / DeeplabVGG(nc).
        `num_batches_tracked` grows by steps x iter_size for the BatchNorms that run (see SimTSingleTrainer.state_dict)."""
        sd = {}
        for k, v in self.params.items():
            if k.endswith(".num_batches_tracked"):
                sd[k] = torch.tensor(int(v.item()) + self._nbt_steps(k), dtype=torch.long)
            else:
                sd[k] = v.detach().cpu()
        return sd

    def timed_lists(self):
        return [self._fwd, self._bwd]

    def losses(self):
        """Host copy of the last micro-batch's loss; local (see SimTTrainer.losses).  Raises ValueError for labels outside [0, C) other than
        255 seen in any micro-batch (on any rank) since the last call, RuntimeError if a fused BatchNorm launch gave up (TrunkPlan.fbn_error)."""
        v = torch.cat([self.hout[:16], self.bad_labels]).cpu().tolist()
        self.plan.raise_on_fbn_error()
        bad = int(round(v[16] * (self.reducer.world if self.reducer is not None else 1))) - self._bad_reported      # cumulative, never reset on the device
        self._bad_reported += max(bad, 0)
        if bad > 0:      # nn.CrossEntropyLoss(ignore_index=255) raises on such a target (trainV1_warmup.py:217-224)
            raise ValueError(f"{bad} label value(s) outside [0, {self.hp.num_classes}) that are not the ignore value 255")
        # `loss = loss / args.iter_size` (trainV1_warmup.py:227): the reported total is the scaled one, like WarmupTrainer's
        return self._labelled({"total": v[14] / self.hp.iter_size, "loss_seg": v[1]})
