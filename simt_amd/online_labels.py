"""Online labels: the warm-up trainers train on a teacher's labels (keywords `online_labels` / `online_labels_every`, tool flags
--online-labels / --online-labels-every).

Without this module the warm-up stage needs a label PNG per image (tools/make_pseudo_labels.py).  With `online_labels=tau` the trainer keeps a
second, closed-set eval-mode plan over a copy of the state it was given -- the TEACHER, built as the SimT trainers build their frozen model --
and every micro-batch

  1. the teacher's forward runs on the side stream beside the student's (the event pattern of SimTTrainer._micro_batch),
  2. family 0 (DeepLab-v2, VGG16): `simt_softmax_rows` of its low-res logits,
  3. ONE `simt_online_label` launch (csrc/label_sweep.hip) writes the int64 labels straight into `trainer.label`, the buffer the head
     descriptor already points at -- arg-max where the resampled posterior's maximum is > tau, 255 elsewhere; the label rule and the
     source of the export's confidence mode -- and adds the labels' counts to `label_counts`,
  4. the main stream waits for that launch in front of `simt_head_loss`; everything behind it is the step without the keyword.

There is no host label and no widening copy.  The teacher sees `teacher_image` (the weak view) when one is passed, else the student's image.
With `online_labels_every=N` (needs `ema_decay`) the teacher follows the weight EMA: `TeacherRefresh` / `TeacherMixin` of
simt_amd/ema_teacher.py as they are, directly behind `ema.update()`; without N it never moves.

`losses()` gains `labelled`: the share of pixels that received a label since the previous call -- the host diffs the cumulative device counts,
as it does for the bad-label counter.  Rank-local under data parallelism.

Class-balanced (keywords `online_labels_balanced=P` / `online_labels_momentum=M`, flags --online-labels-balanced /
--online-labels-momentum): one threshold PER CLASS, kept on the device.  `label_thr[C]` starts at tau; step 3 becomes `simt_online_label_cb`
(label = arg where conf >= thr[arg], and the [C][256] histogram of the confidences in the same pass) followed by `simt_class_thresholds` on the
same stream: per class the threshold that keeps the share P of THIS batch's pixels (`class_thresholds` of tools/make_pseudo_labels.py, capped
at tau), folded into the state with momentum M, and the histogram zeroed.  A batch is therefore labelled with the thresholds of the batches
before it (IAST's ordering), and nothing waits for the host.  `balanced_update` below restates the second launch in numpy.  `losses()` gains
`label_thresholds`.  Rank-local, as `labelled` is.

ClassMix behind the teacher (keywords `online_mix=P` / `online_mix_seed=S`, flag --online-mix): the student's forward then depends
on the labels, so the whole micro-batch runs on the main stream (`_mixed_batch`): teacher forward, step 2, the `_u8` flavour of step 3's launch --
the labels as BYTES plus the per-item class-presence words of the same pass -- and `simt_class_mix_u8`, which selects from the caller's image
and those bytes straight into the student's input and `trainer.label` (int64); there is no input copy and no staging pair.  The draws are the
loader's (`simt_amd.data.class_mix`: `generator(S, rank)`, one `draw_batch` per micro-batch).  `labelled` and `label_thresholds` stay statistics
of the teacher's labels BEFORE the mix.

Quality weights (keyword `online_labels_weighted="batch" | "item"`, flag --online-labels-weighted): the rule of DACS / DAFormer /
MIC.  The threshold deletes no pixel: step 3 becomes `simt_online_label_w` (`_w_u8` with the mix) -- the arg-max at EVERY pixel, the counts of
the launch it replaces (`labelled` keeps its meaning: the share of confident pixels) and the per-item numbers of confident pixels -- followed
by `simt_label_quality` on the same stream: q[B], the share of confident pixels of the micro-batch ("batch": one scalar, the published rule)
or of every item ("item").  The head launches become `simt_head_loss_weighted` / `simt_head_grad_weighted`: every pixel's cross-entropy
times its item's q, still divided by the number of labelled pixels.  With `online_mix` in "item" mode the mix is `simt_class_mix_u8_items`
and the head reads a pasted pixel's weight from its partner's entry through that map; in "batch" mode all entries are equal and there is
no map.  `label_quality` below restates the second launch in numpy.  `losses()` gains `label_quality`, the weights of the last micro-batch.
Rank-local, as `labelled` is.  Not with `online_labels_balanced` in this version.

A labelled source batch in the same step (keyword `online_source=True`, flag --online-source): the published DACS step.  Every
micro-batch is TWO passes into one gradient, through the accumulation path `iter_size > 1` uses (the head's gscale stays 1 / iter_size: the
two losses are summed).  Pass a: `source_image` / `source_label` into the plan's input and `trainer.label`, forward, the plain
`simt_head_loss` / `simt_head_grad`, backward; two floats of `hout` are kept by a device copy (`source_seg1` / `source_seg2` of `losses()`).
Pass b: the target micro-batch as above.  With `online_mix` the mix of pass b is the cross-domain one: `simt_label_presence` of the source
labels and `simt_source_mix` paste half of source item i's classes -- image and GROUND TRUTH -- onto target item i; with
`online_labels_weighted` (either mode) it is `simt_source_mix_items`, and the head launches become `simt_head_loss_weighted_n` /
`simt_head_grad_weighted_n` over a [2B] table whose entries B .. 2B-1 are 1.0f: a pasted pixel has weight 1, a target pixel its q.

Entropy minimisation on the target pass (keywords `entropy_min=lambda` / `entropy_eta` / `entropy_after=N`, flags --entropy-min /
--entropy-eta / --entropy-after): FDA's robust entropy term (eta = 2) or ADVENT's MinEnt (eta = 0.5) on EVERY pixel of the target pass, label or
not, inside the fused head: from iteration N on the target pass's head launches are `simt_head_loss_entropy` / `simt_head_grad_entropy` with
the weights the launches they replace would take -- none (NULL: the plain and the class-balanced trainers), q[B], or the [2B] table.  Before N,
and in the source pass of `online_source` at every iteration, the launches are the ones above.  `losses()` gains `entropy1` / `entropy2`
(`hout[2]`, `hout[3]`; the one-output models: `entropy2` only) while the term is on.  Nothing new is exchanged under data parallelism.

Uncertainty rectification (keyword `uncertainty_rectify=lambda_kl`, flag --uncertainty-rectify; DeepLab-v2's two heads only): Zheng &
Yang's rule for noisy pseudo labels -- the per-pixel KL divergence between the two heads' predictions is the label's uncertainty, a pixel's
cross-entropy is multiplied by exp(-KL) and lambda_kl * the mean KL is added.  Every pass whose labels are not ground truth (the only pass
without `online_source`, with or without `online_labels`; the target pass with it) launches `simt_head_loss_uncertain` /
`simt_head_grad_uncertain` with the weights and the map of the launches they replace; the source pass keeps the plain launches.  `losses()`
gains `uncertainty1/2` (`hout[2]`, `hout[3]`) and `rectify1/2` (`hout[4]`, `hout[5]`).  Refused beside `entropy_min`.  Nothing new is exchanged.

Prototype weights in front of every label launch (keywords `proto_denoise=temp` / `proto_momentum=M`, flags --proto-denoise /
--proto-momentum; simt_amd/proto.py): behind step 2 three launches weigh the teacher's low-res output by the distance of every cell's feature
to running class prototypes, into a map of the same layout; the label launches of every mode above read that map instead -- their
descriptors are re-pointed once -- and nothing else changes.  `losses()` gains `proto_seen` / `proto_changed`.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops
from .data import class_mix
from .ema_teacher import TeacherMixin, check_every
from .engine import side_stream
from .proto import ProtoMixin

DEFAULT_THRESHOLD = 0.968      # DACS / DAFormer
DEFAULT_PORTION = 0.5          # BDL's label generator keeps the more confident half of every class
DEFAULT_MOMENTUM = 0.9         # IAST's exponential average of the per-class thresholds
MAX_BALANCED_CLASSES = 64      # CONF_MAX_C of csrc/label_sweep.hip: the confidence histogram lives in LDS
WEIGHTED_MODES = ("batch", "item")      # online_labels_weighted; simt_label_quality_desc.mode through _lib.LABEL_QUALITY_MODES
MAX_WEIGHTED_ITEMS = 32        # SIMT_CLASS_MIX_MAX: one LDS word per item in the label launch, a byte per pixel in the item map
DEFAULT_ENTROPY_LAMBDA = 0.005 # FDA's --entW
DEFAULT_ENTROPY_ETA = 2.0      # FDA's --ita (Charbonnier penalty); 0.5: ADVENT's MinEnt up to sqrt(eps) = 1e-4


def check_threshold(tau):
    """-> float(tau); ValueError naming `online_labels` unless 0 <= tau < 1 (a NaN is refused)."""
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"online_labels {tau!r}: expected a confidence threshold in [0, 1)") from None
    if isinstance(tau, bool) or not (0.0 <= t < 1.0):
        raise ValueError(f"online_labels {tau!r}: expected a confidence threshold in [0, 1)")
    return t


def check_settings(online_labels, online_labels_every, ema_decay):
    """The two keywords of the warm-up trainers -> (tau | None, N | None); ValueError naming the keyword that does not fit."""
    tau = None if online_labels is None else check_threshold(online_labels)
    if online_labels_every is None:
        return tau, None
    try:
        every = check_every(online_labels_every)
    except ValueError:
        raise ValueError(f"online_labels_every {online_labels_every!r}: expected an integer >= 1") from None
    if tau is None:
        raise ValueError("online_labels_every needs online_labels: it moves the teacher that makes the labels, and this trainer has none")
    if ema_decay is None:
        raise ValueError("online_labels_every needs ema_decay: the teacher follows the weight EMA, and this trainer keeps none")
    return tau, every


def check_balanced(online_labels_balanced, online_labels_momentum, tau, num_classes):
    """The two keywords of the class-balanced thresholds -> (P | None, M | None); `tau` is check_settings' first value.  ValueError that
    starts with the keyword that does not fit."""
    if online_labels_balanced is None:
        if online_labels_momentum is not None:
            raise ValueError("online_labels_momentum needs online_labels_balanced: it averages the per-class thresholds, and this trainer keeps none")
        return None, None
    what = "expected the share of every class's pixels to keep, 0 < P <= 1"
    try:
        p = float(online_labels_balanced)
    except (TypeError, ValueError):
        raise ValueError(f"online_labels_balanced {online_labels_balanced!r}: {what}") from None
    if isinstance(online_labels_balanced, bool) or not (0.0 < p <= 1.0):
        raise ValueError(f"online_labels_balanced {online_labels_balanced!r}: {what}")
    if tau is None:
        raise ValueError("online_labels_balanced needs online_labels: it balances the teacher's labels, and this trainer has no teacher")
    if num_classes > MAX_BALANCED_CLASSES:
        raise ValueError(f"online_labels_balanced with num_classes = {num_classes}: the confidence histogram holds at most {MAX_BALANCED_CLASSES} classes")
    if online_labels_momentum is None:
        return p, DEFAULT_MOMENTUM
    what = "expected the thresholds' momentum, 0 <= M < 1"
    try:
        m = float(online_labels_momentum)
    except (TypeError, ValueError):
        raise ValueError(f"online_labels_momentum {online_labels_momentum!r}: {what}") from None
    if isinstance(online_labels_momentum, bool) or not (0.0 <= m < 1.0):
        raise ValueError(f"online_labels_momentum {online_labels_momentum!r}: {what}")
    return p, m


def check_mix(online_mix, online_mix_seed, tau, batch_size, num_classes):
    """The two keywords of the mix behind the teacher -> (P | None, S); `tau` is check_settings' first value.  ValueError that
    starts with the keyword that does not fit."""
    seed = 0 if online_mix_seed is None else online_mix_seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError(f"online_mix_seed {online_mix_seed!r}: expected a non-negative integer (the seed of the mix's own generator)")
    if online_mix is None:
        if seed != 0:
            raise ValueError("online_mix_seed needs online_mix: it seeds the mix's draws, and this trainer mixes nothing")
        return None, 0
    what = "expected the probability that an item receives its neighbour's classes, 0 < P <= 1"
    try:
        p = float(online_mix)
    except (TypeError, ValueError):
        raise ValueError(f"online_mix {online_mix!r}: {what}") from None
    if isinstance(online_mix, bool) or not (0.0 < p <= 1.0):          # (a NaN fails both comparisons)
        raise ValueError(f"online_mix {online_mix!r}: {what}")
    if tau is None:
        raise ValueError("online_mix needs online_labels: it mixes by the teacher's labels, and this trainer has no teacher")
    if not 2 <= batch_size <= class_mix.MAX_ITEMS:
        raise ValueError(f"online_mix with a batch of {batch_size}: items are mixed with their neighbour in the batch, 2 to {class_mix.MAX_ITEMS} of them")
    if not 1 <= num_classes <= class_mix.MAX_CLASSES:
        raise ValueError(f"online_mix with num_classes = {num_classes}: the presence word holds 1 to {class_mix.MAX_CLASSES} classes")
    return p, int(seed)


def check_weighted(online_labels_weighted, tau, balanced, batch_size):
    """The keyword of the quality weights -> "batch" | "item" | None; `tau` is check_settings' first value, `balanced`
    check_balanced's first.  ValueError that starts with the keyword."""
    mode = online_labels_weighted
    if mode is None:
        return None
    if not isinstance(mode, str) or mode not in WEIGHTED_MODES:
        raise ValueError(f"online_labels_weighted {mode!r}: expected \"batch\" (one weight for the micro-batch, the rule of DACS) or \"item\" "
                         "(one weight per image)")
    if tau is None:
        raise ValueError("online_labels_weighted needs online_labels: it weighs the teacher's labels, and this trainer has no teacher")
    if balanced is not None:
        raise ValueError("online_labels_weighted cannot be combined with online_labels_balanced in this version: the weight is the share of "
                         "pixels above the ONE threshold, and the per-class thresholds have no such share yet")
    if not 1 <= batch_size <= MAX_WEIGHTED_ITEMS:
        raise ValueError(f"online_labels_weighted with a batch of {batch_size}: the label launch counts at most {MAX_WEIGHTED_ITEMS} items")
    return mode


def check_source(online_source, tau):
    """The keyword of the source batch -> bool; `tau` is check_settings' first value.  ValueError that starts with the keyword."""
    if online_source is None:
        return False
    if not isinstance(online_source, (bool, np.bool_)):
        raise ValueError(f"online_source {online_source!r}: expected True (a labelled source batch in every optimiser step) or False")
    if online_source and tau is None:
        raise ValueError("online_source needs online_labels: the source batch is trained beside a target batch that a teacher labels, and "
                         "this trainer has no teacher")
    return bool(online_source)


def check_uncertainty(uncertainty_rectify, entropy):
    """The keyword of the uncertainty rectification -> lambda_kl | None (off); `entropy` is check_entropy's lambda (None: off).
    ValueError that starts with the keyword.  0 is allowed: the rectified cross-entropy without the KL regulariser."""
    if uncertainty_rectify is None:
        return None
    what = "expected the weight of the two-head KL regulariser, a finite lambda_kl >= 0 (None: no rectification)"
    try:
        lam = float(uncertainty_rectify)
    except (TypeError, ValueError):
        raise ValueError(f"uncertainty_rectify {uncertainty_rectify!r}: {what}") from None
    if isinstance(uncertainty_rectify, bool) or not (0.0 <= lam <= 3.0e38):          # (a NaN fails both comparisons; the launch takes a float32)
        raise ValueError(f"uncertainty_rectify {uncertainty_rectify!r}: {what}")
    if entropy is not None:
        raise ValueError("uncertainty_rectify beside entropy_min is not built: one flavour of the fused head would have to carry both terms")
    return lam


def check_entropy(entropy_min, entropy_eta, entropy_after, tau):
    """The three keywords of the entropy term -> (lambda | None, eta, N); `tau` is check_settings' first value.  ValueError
    that starts with the keyword that does not fit.  lambda None: off (eta and N must then be their defaults: they would change nothing)."""
    eta = DEFAULT_ENTROPY_ETA if entropy_eta is None else entropy_eta
    after = 0 if entropy_after is None else entropy_after
    what = "expected the exponent of the penalty (e^2 + 1e-8)^eta, a finite eta > 0"
    try:
        e = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"entropy_eta {entropy_eta!r}: {what}") from None
    if isinstance(eta, bool) or not (1.0e-38 <= e <= 3.0e38):          # (a NaN fails both comparisons; the launch takes a finite float32 > 0)
        raise ValueError(f"entropy_eta {entropy_eta!r}: {what}")
    if isinstance(after, bool) or not isinstance(after, (int, np.integer)) or after < 0:
        raise ValueError(f"entropy_after {entropy_after!r}: expected the first iteration that carries the term, an integer >= 0")
    if entropy_min is None:
        if e != DEFAULT_ENTROPY_ETA:
            raise ValueError("entropy_eta needs entropy_min: it shapes the entropy term, and this trainer has none")
        if after != 0:
            raise ValueError("entropy_after needs entropy_min: it switches the entropy term on, and this trainer has none")
        return None, DEFAULT_ENTROPY_ETA, 0
    what = "expected the weight of the entropy term, a finite lambda > 0 (None: no term)"
    try:
        lam = float(entropy_min)
    except (TypeError, ValueError):
        raise ValueError(f"entropy_min {entropy_min!r}: {what}") from None
    if isinstance(entropy_min, bool) or not (1.0e-38 <= lam <= 3.0e38):          # (likewise)
        raise ValueError(f"entropy_min {entropy_min!r}: {what}")
    if tau is None:
        raise ValueError("entropy_min needs online_labels: the term is a loss on an UNLABELLED target pass, and without a teacher the only pass "
                         "of this trainer has ground truth")
    return lam, e, int(after)


def label_quality(n, N, mode):
    """`simt_label_quality` in numpy -> float32 [B].  n: the number of confident pixels of every item (integers), N = H * W.  "item":
    q[b] = float32(float64(n_b) / float64(N)); "batch": every entry float32(float64(sum n) / float64(B * N)).  Integer sums, one
    conversion, one division, one rounding."""
    n = [int(v) for v in np.asarray(n).reshape(-1)]
    if mode not in WEIGHTED_MODES:
        raise ValueError(f"label_quality mode {mode!r}: expected one of {WEIGHTED_MODES}")
    if mode == "item":
        return np.array([np.float32(np.float64(v) / np.float64(int(N))) for v in n], dtype=np.float32)
    return np.full(len(n), np.float32(np.float64(sum(n)) / np.float64(len(n) * int(N))), dtype=np.float32)


def balanced_update(thr, hist, P, T, M):
    """`simt_class_thresholds` in numpy (steps 3 and 4 of DESIGN 7.17) -> (the new thresholds, the batch thresholds t), float32 [C] each.

    t = class_thresholds(hist, P, cap=T); for every class with a pixel in `hist`: thr + omd * (t - thr) with omd = float32(1 - M), each of
    the three float32 operations rounded on its own (the form csrc/ema.hip pins); a class without pixels keeps its threshold."""
    from .tools.make_pseudo_labels import class_thresholds
    hist = np.asarray(hist)
    thr = np.asarray(thr, dtype=np.float32)
    t = class_thresholds(hist, P, cap=T)
    omd = np.float32(1.0 - M)
    diff = (t - thr).astype(np.float32)
    step = (omd * diff).astype(np.float32)
    moved = (thr + step).astype(np.float32)
    seen = hist.astype(np.int64).sum(axis=1) > 0
    return np.where(seen, moved, thr).astype(np.float32), t


def labelled_share(counts, reported):
    """counts: the cumulative [C+1] label counts (classes, then the 255s); reported: [labelled, pixels] already handed out.  -> (share of the
    pixels counted since that received a label -- 0.0 when none were counted --, the new `reported`)."""
    kept, total = int(sum(counts[:-1])), int(sum(counts))
    d_kept, d_total = kept - int(reported[0]), total - int(reported[1])
    return (d_kept / d_total if d_total > 0 else 0.0), [kept, total]


class OnlineLabelMixin(TeacherMixin, ProtoMixin):
    """The teacher's side of WarmupTrainer and WarmupSingleTrainer.  The trainer builds `fixed_params`, `fixed` (the eval-mode plan), `_fix_fwd`
    (its forward launches) and names the teacher's low-res output; this class owns the per-step launches, the counts and the read-out."""

    def _init_online(self, tau, every, fix_out, ldf, family, balanced=(None, None)):
        """tau / every: check_settings' pair (tau None: off -- no buffer, no launch).  balanced: check_balanced's pair (P None: one threshold).  fix_out: the teacher's low-res logits [B*h*w][ldf];
        family: 0 = probabilities resampled align_corners=True (DeepLab-v2, VGG16), 1 = logits resampled half-pixel (DeepLabv3)."""
        self.online_labels, self.teacher = tau, None
        self.online_labels_balanced, self.online_labels_momentum = balanced
        if tau is None:
            return
        dev = self.dev
        self._fix_out, self.ldf, self._family = fix_out, ldf, family
        # family 0: the low-res posterior (simt_softmax_rows of the logits); family 1 reads the logits themselves
        self.fixp = fix_out if family else torch.zeros(self.B * self.h * self.w, ldf, device=dev)
        self.label_counts = torch.zeros(self.C + 1, device=dev, dtype=torch.int64)      # cumulative, never reset on the device
        self._counts_reported = [0, 0]
        d = L.OnlineLabelDesc()
        d.fix, d.label, d.counts = self.fixp.data_ptr(), self.label.data_ptr(), self.label_counts.data_ptr()
        d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = self.B, self.h, self.w, ldf, self.H, self.W, self.C, family, tau
        self.online_desc = d
        if self.online_labels_balanced is not None:
            self._init_balanced(d)
        self._init_teacher(every)          # None: the teacher stays at the start weights (simt_amd/ema_teacher.py)

    def _init_balanced(self, one):
        """The per-class thresholds (start: tau everywhere), the histogram the two launches share (zero between micro-batches) and their
        descriptors; `one` is the descriptor of simt_online_label, whose geometry they take."""
        P, M, dev = self.online_labels_balanced, self.online_labels_momentum, self.dev
        self.label_thr = torch.full((self.C,), self.online_labels, device=dev, dtype=torch.float32)
        self.label_hist = torch.zeros(self.C, L.CONF_BINS, device=dev, dtype=torch.int64)
        d = L.OnlineLabelCbDesc()
        d.fix, d.label, d.counts, d.hist, d.thr = one.fix, one.label, one.counts, self.label_hist.data_ptr(), self.label_thr.data_ptr()
        d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family = one.B, one.h, one.w, one.ld, one.H, one.W, one.C, one.family
        t = L.ClassThresholdsDesc()
        t.hist, t.thr, t.t_out = self.label_hist.data_ptr(), self.label_thr.data_ptr(), None
        t.drop, t.C, t.cap, t.omd = 1.0 - P, self.C, self.online_labels, 1.0 - M      # (ctypes rounds cap and omd to float32)
        self.online_cb_desc, self.thresholds_desc = d, t

    def _init_mix(self, mix):
        """mix: check_mix's pair (P None: off -- no buffer, no launch, no draw).  Behind _init_online.  The byte labels, the presence words
        of the label launch, the `_u8` descriptors (the geometry of the int64 ones) and the mix's descriptor, whose outputs are the student
        plan's input and `self.label`: the buffers the forward and the head kernels already read."""
        self.online_mix, self.online_mix_seed = mix
        if self.online_mix is None:
            return
        dev, one = self.dev, self.online_desc
        rank = 0
        if getattr(self, "pg", None) is not None:
            import torch.distributed as dist
            rank = dist.get_rank(self.pg)
        self._mix_rng = class_mix.generator(self.online_mix_seed, rank)      # the loader's ClassMix contract: a generator of the mix's own
        self.lab8 = torch.zeros(self.B, self.H, self.W, device=dev, dtype=torch.uint8)
        d = L.OnlineLabelU8Desc()
        d.fix, d.lab8, d.counts = one.fix, self.lab8.data_ptr(), one.counts
        d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = one.B, one.h, one.w, one.ld, one.H, one.W, one.C, one.family, one.threshold
        rows = L.load().simt_online_label_parts(C.byref(d))
        if rows < 1:
            raise L.SimtHipError(f"simt_online_label_parts: {rows} for B = {self.B}, {self.H} x {self.W}")
        self.mix_part = torch.zeros(self.B, rows, device=dev, dtype=torch.int32)      # every word is written by every label launch
        d.part = self.mix_part.data_ptr()
        self.online_u8_desc = d
        if self.online_labels_balanced is not None:
            cb, e = self.online_cb_desc, L.OnlineLabelCbU8Desc()
            e.fix, e.lab8, e.counts, e.hist, e.thr, e.part = cb.fix, d.lab8, cb.counts, cb.hist, cb.thr, d.part
            e.B, e.h, e.w, e.ld, e.H, e.W, e.C, e.family = cb.B, cb.h, cb.w, cb.ld, cb.H, cb.W, cb.C, cb.family
            self.online_cb_u8_desc = e
        m = L.ClassMixU8Desc()
        m.lab8, m.x_out, m.lab_out, m.part = d.lab8, self.plan.x_in.data_ptr(), self.label.data_ptr(), d.part
        m.B, m.h, m.w, m.n_classes, m.rows = self.B, self.H, self.W, self.C, rows
        for i in range(self.B):
            m.partner[i] = (i + 1) % self.B
        self.mix_desc = m
        self._mix_stage = None             # for an image the launch cannot read where it lies; allocated on first need

    def _init_weighted(self, mode):
        """mode: check_weighted's value (None: off -- no buffer, no launch).  Behind _init_online and _init_mix.  The per-item counts of
        confident pixels, the weights, the `_w` descriptor that replaces the label launch's (the geometry of the one it replaces) and, with
        the mix in "item" mode, the item map the mix writes and the head reads."""
        self.online_labels_weighted = mode
        if mode is None:
            return
        dev, one = self.dev, self.online_desc
        probe = L.OnlineLabelU8Desc()
        probe.B, probe.H, probe.W, probe.family = one.B, one.H, one.W, one.family
        rows = L.load().simt_online_label_parts(C.byref(probe))
        if rows < 1:
            raise L.SimtHipError(f"simt_online_label_parts: {rows} for B = {self.B}, {self.H} x {self.W}")
        self.conf_part = torch.zeros(self.B, rows, device=dev, dtype=torch.int32)      # every word is written by every label launch
        self.label_q = torch.zeros(self.B, device=dev, dtype=torch.float32)
        if self.online_mix is None:
            d = L.OnlineLabelWDesc()
            d.fix, d.label, d.counts, d.conf_part = one.fix, one.label, one.counts, self.conf_part.data_ptr()
        else:
            u = self.online_u8_desc
            d = L.OnlineLabelWU8Desc()
            d.fix, d.lab8, d.counts, d.part, d.conf_part = u.fix, u.lab8, u.counts, u.part, self.conf_part.data_ptr()
        d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = one.B, one.h, one.w, one.ld, one.H, one.W, one.C, one.family, one.threshold
        self.online_w_desc = d
        q = L.LabelQualityDesc()
        q.conf_part, q.q, q.B, q.rows, q.H, q.W, q.mode = self.conf_part.data_ptr(), self.label_q.data_ptr(), self.B, rows, self.H, self.W, \
            L.LABEL_QUALITY_MODES[mode]
        self.quality_desc = q
        # "batch": all entries are equal, so a pasted pixel's weight is its own item's and no map is needed
        self.w_item = torch.zeros(self.B, self.H, self.W, device=dev, dtype=torch.uint8) if (self.online_mix is not None and mode == "item") else None

    def _init_source(self, on):
        """on: check_source's value (False: off -- no buffer, no launch).  Behind _init_online, _init_mix and _init_weighted.  The two
        kept floats of the source pass; with the mix the presence words of the source labels and the descriptor of simt_source_mix, whose
        outputs are the mix's -- the source pair itself is read where the caller left it, or from a staging pair allocated on first need
        (`_source_input`); with the quality weights also the [2B] table -- q in 0 .. B-1 (`label_q` becomes a
        view of it, so simt_label_quality writes there), 1.0f behind, written once -- and the item map in either mode."""
        self.online_source = bool(on)
        if not on:
            return
        dev, B = self.dev, self.B
        self.source_hout = torch.zeros(2, device=dev)
        if self.online_mix is None:
            return
        self.src_x = self.src_lab = None      # the source pair as the mix reads it: set per micro-batch by _source_input
        self._src_stage = [None, None]        # for a pair the launch cannot read where it lies; allocated on first need
        self.src_part = torch.zeros(B, L.CLASS_MIX_PARTS, device=dev, dtype=torch.int32)      # every word is written by every presence launch
        m = L.SourceMixDesc()
        m.part_s, m.lab8 = self.src_part.data_ptr(), self.lab8.data_ptr()
        m.x_out, m.lab_out = self.plan.x_in.data_ptr(), self.label.data_ptr()
        m.B, m.h, m.w, m.n_classes = B, self.H, self.W, self.C
        self.source_mix_desc = m
        if self.online_labels_weighted is not None:
            table = torch.ones(2 * B, device=dev, dtype=torch.float32)
            table[:B] = self.label_q
            self.label_w, self.label_q = table, table[:B]
            self.quality_desc.q = self.label_q.data_ptr()
            if self.w_item is None:        # "batch": the entries 0 .. B-1 are equal, but a pasted pixel reads entry B + i
                self.w_item = torch.zeros(B, self.H, self.W, device=dev, dtype=torch.uint8)

    def _init_entropy(self, entropy):
        """entropy: check_entropy's triple (lambda None: off -- nothing kept, every launch the one it was).  Behind _init_online."""
        self.entropy_min, self.entropy_eta, self.entropy_after = entropy
        self._entropy_on, self._entropy_it = False, None
        if self.entropy_min is not None:
            self.entropy_rec = L.HeadEntropy(self.entropy_min, self.entropy_eta)

    def _entropy_at(self, it):
        """step(): whether the target pass of iteration `it` carries the term (FDA's switch2entropy); kept for the launches and losses()."""
        self._entropy_it = int(it)
        self._entropy_on = getattr(self, "entropy_min", None) is not None and int(it) >= self.entropy_after
        return self._entropy_on

    def _entropy_reported(self):
        """losses(): whether the last step carried the term (a trainer resumed and not yet stepped: the step before `it_done`)."""
        if getattr(self, "entropy_min", None) is None:
            return False
        it = self._entropy_it if self._entropy_it is not None else self.it_done - 1
        return it >= self.entropy_after and self.it_done > 0

    def _init_uncertainty(self, lambda_kl):
        """lambda_kl: check_uncertainty's value (None: off -- nothing kept, every launch the one it was).  Behind _init_entropy."""
        self.uncertainty_rectify = lambda_kl
        if lambda_kl is not None:
            if self.head_desc.single:
                raise ValueError("uncertainty_rectify needs two heads: the uncertainty is the KL divergence between them")
            self.uncertainty_rec = L.HeadUncertainty(lambda_kl)

    def _uncertainty_losses(self, out):
        """losses(): with uncertainty_rectify adds K_k (`uncertainty1/2`) and the mean rectification weight (`rectify1/2`) of the last micro-batch's
        pass on labels that are not ground truth; `loss_seg1/2` are then the rectified cross-entropies R_k."""
        if getattr(self, "uncertainty_rectify", None) is not None and self.it_done > 0:
            out["uncertainty1"], out["uncertainty2"], out["rectify1"], out["rectify2"] = self.hout[2:6].cpu().tolist()
        return out

    def _weight_args(self):
        """The (w, nw, map) triple of the entropy and the uncertainty launches: the table the weighted launches of this trainer read, or (NULL, 0, NULL)."""
        if getattr(self, "online_labels_weighted", None) is None:
            return None, 0, None
        if self._source_table():
            return self.label_w.data_ptr(), 2 * self.B, self.w_item.data_ptr()
        return self.label_q.data_ptr(), self.B, None if self.w_item is None else self.w_item.data_ptr()

    def _source_table(self):
        """True when the weighted head launches read the [2B] table through the source mix's item map."""
        return getattr(self, "online_source", False) and self.online_mix is not None

    def _head_loss(self, st):
        """simt_head_loss of the micro-batch, or its weighted form (the map: the mix's item map in "item" mode, else NULL; with
        online_source and the mix the [2B] table and the source mix's map).  At an iteration that carries the entropy term (_entropy_at):
        simt_head_loss_entropy with the same weights."""
        if getattr(self, "uncertainty_rectify", None) is not None:      # DESIGN 7.28 (refused beside entropy_min)
            w, nw, item = self._weight_args()
            L.call("simt_head_loss_uncertain", C.byref(self.head_desc), w, nw, item, C.byref(self.uncertainty_rec), st)
        elif getattr(self, "_entropy_on", False):
            w, nw, item = self._weight_args()
            L.call("simt_head_loss_entropy", C.byref(self.head_desc), w, nw, item, C.byref(self.entropy_rec), st)
        elif getattr(self, "online_labels_weighted", None) is None:
            L.call("simt_head_loss", C.byref(self.head_desc), st)
        elif self._source_table():
            L.call("simt_head_loss_weighted_n", C.byref(self.head_desc), self.label_w.data_ptr(), 2 * self.B, self.w_item.data_ptr(), st)
        else:
            L.call("simt_head_loss_weighted", C.byref(self.head_desc), self.label_q.data_ptr(),
                   None if self.w_item is None else self.w_item.data_ptr(), st)

    def _head_grad(self, st):
        if getattr(self, "uncertainty_rectify", None) is not None:
            w, nw, item = self._weight_args()
            L.call("simt_head_grad_uncertain", C.byref(self.head_desc), w, nw, item, C.byref(self.uncertainty_rec), st)
        elif getattr(self, "_entropy_on", False):
            w, nw, item = self._weight_args()
            L.call("simt_head_grad_entropy", C.byref(self.head_desc), w, nw, item, C.byref(self.entropy_rec), st)
        elif getattr(self, "online_labels_weighted", None) is None:
            L.call("simt_head_grad", C.byref(self.head_desc), st)
        elif self._source_table():
            L.call("simt_head_grad_weighted_n", C.byref(self.head_desc), self.label_w.data_ptr(), 2 * self.B, self.w_item.data_ptr(), st)
        else:
            L.call("simt_head_grad_weighted", C.byref(self.head_desc), self.label_q.data_ptr(),
                   None if self.w_item is None else self.w_item.data_ptr(), st)

    def _sources(self, source_image, source_label, n):
        """step()'s `source_image` / `source_label` as lists of n = iter_size entries; ValueError when they do not fit the trainer."""
        if not getattr(self, "online_source", False):
            if source_image is not None or source_label is not None:
                raise ValueError("step(): source_image / source_label need a trainer built with online_source=True (this one has no source pass)")
            return [None] * n, [None] * n
        if source_image is None or source_label is None:
            raise ValueError("step(): this trainer was built with online_source and needs source_image and source_label")
        imgs = list(source_image) if isinstance(source_image, (list, tuple)) else [source_image]
        labs = list(source_label) if isinstance(source_label, (list, tuple)) else [source_label]
        if len(imgs) != n or len(labs) != n:
            raise ValueError(f"step() needs {n} source_image(s) and source_label(s) (hp.iter_size), got {len(imgs)} and {len(labs)}")
        for x, l in zip(imgs, labs):
            if tuple(x.shape) != (self.B, 3, self.H, self.W):
                raise ValueError(f"source_image of shape {tuple(x.shape)}, expected {(self.B, 3, self.H, self.W)}")
            if tuple(l.shape) != (self.B, self.H, self.W):
                raise ValueError(f"source_label of shape {tuple(l.shape)}, expected {(self.B, self.H, self.W)}")
        return imgs, labs

    def _readable(self, t, dtype, out):
        """True when a launch can read the caller's tensor where it lies: contiguous, of `dtype`, on this device, at a 16-byte base, and not
        the buffer `out` that the launch writes."""
        return (t.device == out.device and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.data_ptr() != out.data_ptr())

    def _source_input(self, source_image, source_label):
        """Pass a's input, main stream: the source pair into `plan.x_in` and `self.label`.  Behind everything the previous pass enqueued on
        the main stream (its head kernels read `label`, its stem weight gradient `plan.x_in`): the write-after-read ordering of the input
        copy.  With the mix, pass b's simt_label_presence and simt_source_mix read the pair again (`src_x`, `src_lab`): the caller's
        tensors themselves where they are contiguous fp32 / int64 tensors of this device at a 16-byte base (`_mix_source`'s test on the
        target side; step() holds them until it returns), else copies in a staging pair of the trainer's own."""
        if self.online_mix is not None:
            pair = []
            for k, (t, dtype, out) in enumerate(((source_image, torch.float32, self.plan.x_in), (source_label, torch.int64, self.label))):
                if not self._readable(t, dtype, out):
                    if self._src_stage[k] is None:
                        self._src_stage[k] = torch.empty_like(out)
                    self._src_stage[k].copy_(t, non_blocking=True)
                    t = self._src_stage[k]
                pair.append(t)
            source_image, source_label = self.src_x, self.src_lab = pair
        self.plan.x_in.copy_(source_image, non_blocking=True)
        self.label.copy_(source_label, non_blocking=True)

    def _source_kept(self):
        """Behind pass a's simt_head_loss, main stream: its two losses, kept for losses() (pass b's launch overwrites `hout`)."""
        self.source_hout.copy_(self.hout[:2], non_blocking=True)

    def _mix_source(self, image):
        """The student's image as simt_class_mix_u8 reads it: the caller's tensor where it is a contiguous fp32 tensor of this device at a
        16-byte base (and not the plan's input itself, which the launch writes), else a copy in a staging buffer of the trainer's own."""
        if tuple(image.shape) != (self.B, 3, self.H, self.W):
            raise ValueError(f"image of shape {tuple(image.shape)}, expected {(self.B, 3, self.H, self.W)}")
        if (image.device == self.plan.x_in.device and image.dtype == torch.float32 and image.is_contiguous() and image.data_ptr() % 16 == 0
                and image.data_ptr() != self.plan.x_in.data_ptr()):
            return image
        if self._mix_stage is None:
            self._mix_stage = torch.empty_like(self.plan.x_in)
        self._mix_stage.copy_(image, non_blocking=True)
        return self._mix_stage

    def _mixed_batch(self, image, teacher_image):
        """One micro-batch with online_mix, ALL on the main stream, in front of the student's forward, which now depends on
        the labels: the teacher's input, its forward, the posterior (family 0), the `_u8` label launch (+ simt_class_thresholds when
        balanced), then simt_class_mix_u8 from the caller's image into `plan.x_in` and `self.label`.  No host synchronisation; the draws
        are host values in the descriptor.  Ordering, all by stream order:
          the previous micro-batch's head kernels (they read `label`), stem weight gradient (it reads `plan.x_in`; the backward joins its
          side stream before it returns) and optimiser come first -- the write-after-read ordering the input copy had;
          an EMA-teacher refresh (`_teacher_follows`, main stream, behind the update) lies behind this step's teacher forward and in front
          of the next one, which runs on the same stream.
        With online_source this is pass b and the mix is simt_label_presence(src_lab) + simt_source_mix: pass a -- its input
        copies (a staging copy of the source pair among them, when one is needed), its forward, head kernels and backward -- lies in
        front of all of this on the same stream, so the source pair is complete and nothing of pass a still reads `plan.x_in` or `label`
        when the mix writes them."""
        st = ops.stream_ptr()
        x = self._mix_source(image)
        self.fixed.x_in.copy_(image if teacher_image is None else teacher_image, non_blocking=True)
        self._fix_fwd.run()
        if not self._family:
            ops.softmax_rows(self._fix_out, self.ldf, self.fixp, self.ldf, self.B * self.h * self.w, self.C)
        self._proto_launches(st)      # with proto_denoise the label launches below read the rectified map
        if getattr(self, "online_labels_weighted", None) is not None:      # every arg-max, the counts at tau, the weights
            L.call("simt_online_label_w_u8", C.byref(self.online_w_desc), st)
            L.call("simt_label_quality", C.byref(self.quality_desc), st)
        elif self.online_labels_balanced is None:
            L.call("simt_online_label_u8", C.byref(self.online_u8_desc), st)
        else:
            L.call("simt_online_label_cb_u8", C.byref(self.online_cb_u8_desc), st)
            L.call("simt_class_thresholds", C.byref(self.thresholds_desc), st)
        apply, rank = class_mix.draw_batch(self._mix_rng, self.B, self.C, self.online_mix)      # one call per micro-batch, in order
        source = getattr(self, "online_source", False)
        m = self.source_mix_desc if source else self.mix_desc
        table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
        table[:self.B, :self.C] = rank
        C.memmove(m.rank, table.ctypes.data, table.nbytes)
        for i in range(self.B):
            m.apply[i] = 1 if apply[i] else 0
        if source:      # the pasted side is source item i (`src_x`, `src_lab`: what pass a trained on), image and ground truth
            m.xs, m.labs, m.xt = self.src_x.data_ptr(), self.src_lab.data_ptr(), x.data_ptr()
            L.call("simt_label_presence", self.src_lab.data_ptr(), self.B, self.H * self.W, self.C, self.src_part.data_ptr(), st)
            if getattr(self, "online_labels_weighted", None) is not None:      # either mode: a pasted pixel reads entry B + i, 1.0f
                L.call("simt_source_mix_items", C.byref(m), self.w_item.data_ptr(), st)
            else:
                L.call("simt_source_mix", C.byref(m), st)
            return
        m.x = x.data_ptr()
        if getattr(self, "w_item", None) is not None:      # "item" weights: the head reads a pasted pixel's weight from its partner's entry
            L.call("simt_class_mix_u8_items", C.byref(m), self.w_item.data_ptr(), st)
        else:
            L.call("simt_class_mix_u8", C.byref(m), st)

    def _views(self, label, teacher_image, n):
        """step()'s `label` / `teacher_image` as lists of n = iter_size entries; ValueError when they do not fit the trainer."""
        if self.online_labels is None:
            if teacher_image is not None:
                raise ValueError("step(): teacher_image needs a trainer built with online_labels (this one trains on the labels it is given)")
            if label is None:
                raise ValueError("step(): this trainer was built without online_labels and needs a label")
            return list(label) if isinstance(label, (list, tuple)) else [label], [None] * n
        if label is not None and not (isinstance(label, (list, tuple)) and all(l is None for l in label)):
            raise ValueError("step(): this trainer was built with online_labels: the labels come from the teacher, pass label=None")
        if teacher_image is None:
            return [None] * n, [None] * n
        teachers = list(teacher_image) if isinstance(teacher_image, (list, tuple)) else [teacher_image]
        if len(teachers) != n:
            raise ValueError(f"step() needs {n} teacher_image(s) (hp.iter_size), got {len(teachers)}")
        for t in teachers:
            if tuple(t.shape) != (self.B, 3, self.H, self.W):
                raise ValueError(f"teacher_image of shape {tuple(t.shape)}, expected {(self.B, 3, self.H, self.W)}")
        return [None] * n, teachers

    def _teacher_input(self, image, teacher_image):
        """Main stream, behind the copy of the student's image: the teacher's input, then the event its forward waits for.  Recorded behind
        everything the previous (micro-)batch enqueued on the main stream: its head kernels, which read `label`, come first (WAR)."""
        self.fixed.x_in.copy_(image if teacher_image is None else teacher_image, non_blocking=True)
        ev_in = torch.cuda.Event()
        ev_in.record(torch.cuda.current_stream())
        return ev_in

    def _teacher_labels(self, ev_in):
        """The teacher's forward, the posterior and the label launch on the side stream, beside the student's forward (already enqueued on
        the main stream: the critical path goes first, as in SimTTrainer._micro_batch); the main stream then waits for the labels."""
        main, side = torch.cuda.current_stream(), side_stream(self.dev)
        with torch.cuda.stream(side):
            side.wait_event(ev_in)
            self._fix_fwd.run()
            if not self._family:
                ops.softmax_rows(self._fix_out, self.ldf, self.fixp, self.ldf, self.B * self.h * self.w, self.C)
            self._proto_launches(side.cuda_stream)      # with proto_denoise the label launches below read the rectified map
            if getattr(self, "online_labels_weighted", None) is not None:      # (the main stream waits for both below)
                L.call("simt_online_label_w", C.byref(self.online_w_desc), side.cuda_stream)
                L.call("simt_label_quality", C.byref(self.quality_desc), side.cuda_stream)
            elif self.online_labels_balanced is None:
                L.call("simt_online_label", C.byref(self.online_desc), side.cuda_stream)
            else:          # label with the thresholds as they stand and count; then move them and zero the histogram
                L.call("simt_online_label_cb", C.byref(self.online_cb_desc), side.cuda_stream)
                L.call("simt_class_thresholds", C.byref(self.thresholds_desc), side.cuda_stream)
            ev_lab = torch.cuda.Event()
            ev_lab.record(side)
        main.wait_event(ev_lab)

    def _labelled(self, out):
        """losses(): adds `labelled` to `out` (one more device-to-host copy: int64 counts do not ride in the float scalars)."""
        if self.online_labels is not None:
            out["labelled"], self._counts_reported = labelled_share(self.label_counts.cpu().tolist(), self._counts_reported)
            if getattr(self, "online_labels_balanced", None) is not None:
                out["label_thresholds"] = self.label_thr.cpu().tolist()
            if getattr(self, "online_labels_weighted", None) is not None:      # the weights of the last micro-batch
                out["label_quality"] = self.label_q.cpu().tolist()
            if getattr(self, "online_source", False):      # the source pass of the last micro-batch
                out["source_seg1"], out["source_seg2"] = self.source_hout.cpu().tolist()
            if self._entropy_reported():      # the target pass of the last micro-batch
                e1, e2 = self.hout[2:4].cpu().tolist()
                if not self.head_desc.single:
                    out["entropy1"] = e1
                out["entropy2"] = e2
            self._proto_losses(out)      # proto_seen / proto_changed of the last micro-batch
        return out
