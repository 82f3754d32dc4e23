"""Online labels: the warm-up trainers train on a teacher's labels (keywords `online_labels` / `online_labels_every`, tool flags
--online-labels / --online-labels-every).

Without this module the warm-up stage needs a label PNG per image (tools/make_pseudo_labels.py).  With `online_labels=tau` the trainer keeps a
second, closed-set eval-mode plan over a copy of the state it was given -- the TEACHER, built as the SimT trainers build their frozen model --
and every micro-batch

  1. the teacher's forward runs on the side stream beside the student's (the event pattern of SimTTrainer._micro_batch),
  2. family 0 (DeepLab-v2, VGG16): `simt_softmax_rows` of its low-res logits,
  3. ONE `simt_online_label` launch (csrc/eval_metric.hip) writes the int64 labels straight into `trainer.label`, the buffer the head
     descriptor already points at -- arg-max where the resampled posterior's maximum is > tau, 255 elsewhere; the label rule and the device
     functions of the export kernels' confidence mode -- and adds the labels' counts to `label_counts`,
  4. the main stream waits for that launch in front of `simt_head_loss`; everything behind it is the step without the keyword.

There is no host label and no widening copy.  The teacher sees `teacher_image` (the weak view) when one is passed, else the student's image.
With `online_labels_every=N` (needs `ema_decay`) the teacher follows the weight EMA: `TeacherRefresh` / `TeacherMixin` of
simt_amd/ema_teacher.py as they are, directly behind `ema.update()`; without N it never moves.

`losses()` gains `labelled`: the share of pixels that received a label since the previous call -- the host diffs the cumulative device counts,
as it does for the bad-label counter.  Rank-local under data parallelism.
"""
import ctypes as C

import torch

from . import _lib as L
from . import ops
from .ema_teacher import TeacherMixin, check_every
from .engine import side_stream

DEFAULT_THRESHOLD = 0.968      # DACS / DAFormer


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


def labelled_share(counts, reported):
    """counts: the cumulative [C+1] label counts (classes, then the 255s); reported: [labelled, pixels] already handed out.  -> (share of the
    pixels counted since that received a label -- 0.0 when none were counted --, the new `reported`)."""
    kept, total = int(sum(counts[:-1])), int(sum(counts))
    d_kept, d_total = kept - int(reported[0]), total - int(reported[1])
    return (d_kept / d_total if d_total > 0 else 0.0), [kept, total]


class OnlineLabelMixin(TeacherMixin):
    """The teacher's side of WarmupTrainer and WarmupSingleTrainer.  The trainer builds `fixed_params`, `fixed` (the eval-mode plan), `_fix_fwd`
    (its forward launches) and names the teacher's low-res output; this class owns the per-step launches, the counts and the read-out."""

    def _init_online(self, tau, every, fix_out, ldf, family):
        """tau / every: check_settings' pair (tau None: off -- no buffer, no launch).  fix_out: the teacher's low-res logits [B*h*w][ldf];
        family: 0 = probabilities resampled align_corners=True (DeepLab-v2, VGG16), 1 = logits resampled half-pixel (DeepLabv3)."""
        self.online_labels, self.teacher = tau, None
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
        self._init_teacher(every)          # None: the teacher stays at the start weights (simt_amd/ema_teacher.py)

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
            L.call("simt_online_label", C.byref(self.online_desc), side.cuda_stream)
            ev_lab = torch.cuda.Event()
            ev_lab.record(side)
        main.wait_event(ev_lab)

    def _labelled(self, out):
        """losses(): adds `labelled` to `out` (one more device-to-host copy: int64 counts do not ride in the float scalars)."""
        if self.online_labels is not None:
            out["labelled"], self._counts_reported = labelled_share(self.label_counts.cpu().tolist(), self._counts_reported)
        return out
