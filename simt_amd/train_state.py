"""The train-state file: everything a training run needs to be CONTINUED, not just re-started.

A snapshot written by the tools holds `state_dict()` only.  What the next step also depends on lives in the trainer: the SGD momentum
buffers, both noise-transition matrices with their Adam moments, the raw W of the inner loop with its moments, the iteration counter
(poly learning rate, Adam bias correction, the inner loop's `step0`) and the cumulative bad-label counter.  `TrainStateMixin` gives the four
trainers `training_state()` / `load_training_state(ts)`; `save` / `load` put that dict, the snapshot rotation's bookkeeping and the loop's
position into ONE file, written through `save_atomic`.  The check of a resume is bitwise: k steps, save, load into a fresh trainer, n - k
steps == n steps (tests/test_gpu_resume.py).

Stored: what is not derived from something else in the dict.  NOT stored: T (the inner loop rewrites it every step), every packed operand
(`plan.repack()` rebuilds them from the masters on load) and the frozen model -- a resumed run is given the same --restore-from and the
SHA-256 of the frozen tensors is compared instead, which keeps the file at weights + momentum.  (With the EMA teacher the frozen model moves: the
file then carries it as it is, beside the unchanged SHA-256 of the model the run started beside.)
"""
import hashlib
import os

import torch

FORMAT_VERSION = 1

# Hyper fields that change the parameter trajectory: a state is refused by a trainer that differs in one of them.  (`skip_unapplied_grads`
# is not among them: it drops gradients no optimiser applies, the trajectory is the same.)
TRAJECTORY_FIELDS = ("lr", "lr_T", "momentum", "weight_decay", "power", "num_steps", "lambda_seg", "lambda_place", "lambda_convex",
                     "lambda_volume", "lambda_anchor", "th_high", "th_low", "num_classes", "open_classes", "iter_size")
CHECKED_FIELDS = TRAJECTORY_FIELDS + ("B", "H", "W", "dtype", "trainer", "model", "arch", "format_version")
# Checked too, but ABSENT = False: keywords added after format_version 1 that a trainer writes into `hyper` only when they are on, so that the
# states of runs without them stay what they were (teacher_view: the weak-view teacher of the SimT trainers)
SWITCH_FIELDS = ("teacher_view",)
# The same, with VALUES: absent = off, present = the keyword's value, compared as it is (online_labels = tau, online_labels_every = N: the
# warm-up trainers' teacher)
VALUE_FIELDS = ("online_labels", "online_labels_every")
# and the class-balanced thresholds of that teacher's labels (online_labels_balanced = P, online_labels_momentum = M: DESIGN 7.17), compared
# through value_mismatches(..., fields=BALANCE_FIELDS)
BALANCE_FIELDS = ("online_labels_balanced", "online_labels_momentum")
# and the mix behind that teacher (online_mix = P, online_mix_seed = S: DESIGN 7.18), compared through value_mismatches(..., fields=MIX_FIELDS)
MIX_FIELDS = ("online_mix", "online_mix_seed")
# and the quality weights of that teacher's labels (online_labels_weighted = "batch" | "item": DESIGN 7.19), compared through
# value_mismatches(..., fields=WEIGHTED_FIELDS)
WEIGHTED_FIELDS = ("online_labels_weighted",)
# and the labelled source batch trained beside that teacher's labels (online_source = True: DESIGN 7.20), compared through
# value_mismatches(..., fields=SOURCE_FIELDS)
SOURCE_FIELDS = ("online_source",)
# and the ImageNet feature distance (feat_dist = lambda with its classes, ratio and the SHA-256 of the frozen ImageNet trunk: DESIGN 7.22),
# compared through value_mismatches(..., fields=FEAT_DIST_FIELDS)
FEAT_DIST_FIELDS = ("feat_dist", "feat_dist_classes", "feat_dist_min_ratio", "feat_dist_sha256")
# and the optimiser and the learning-rate warm-up: optimizer / adam_betas / adam_eps are written only under "adamw", lr_warmup /
# lr_warmup_ratio only with a warm-up > 0; compared through value_mismatches(..., fields=OPTIMIZER_FIELDS)
OPTIMIZER_FIELDS = ("optimizer", "adam_betas", "adam_eps", "lr_warmup", "lr_warmup_ratio")
# and the entropy term of the target pass (entropy_min = lambda with its exponent and the iteration that switches it on: DESIGN 7.25),
# written only when on; compared through value_mismatches(..., fields=ENTROPY_FIELDS)
ENTROPY_FIELDS = ("entropy_min", "entropy_eta", "entropy_after")
# and the prototype weights on the teacher's labels (proto_denoise = temp, proto_momentum = M: DESIGN 7.26), written only when on; compared
# through value_mismatches(..., fields=PROTO_FIELDS)
PROTO_FIELDS = ("proto_denoise", "proto_momentum")
# and the prototype contrastive term on the student's layer-4 features (proto_contrast = lambda with its temperature and ratio: DESIGN 7.27),
# written only when on; compared through value_mismatches(..., fields=PROTO_CONTRAST_FIELDS).  No accumulator: the term keeps no state of its own.
PROTO_CONTRAST_FIELDS = ("proto_contrast", "proto_contrast_temp", "proto_contrast_min_ratio")
# and the uncertainty rectification (uncertainty_rectify = lambda_kl: DESIGN 7.28), written only when on; compared through
# value_mismatches(..., fields=UNCERTAINTY_FIELDS)
UNCERTAINTY_FIELDS = ("uncertainty_rectify",)
NTM_FIELDS = ("ntm", "ntm_m", "ntm_v", "wraw", "w_m", "w_v")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pure helpers (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def state_sha256(state):
    """SHA-256 over a {name: tensor} dict in sorted key order: name, dtype, shape and bytes of every tensor.  Independent of the dict's
    order and of where the tensors live; one changed element changes it."""
    h = hashlib.sha256()
    for k in sorted(state):
        t = state[k].detach().cpu().contiguous()
        h.update(f"{k}|{t.dtype}|{tuple(t.shape)}|".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _norm(v):
    """Lists and tuples compare equal (a file round trip may turn one into the other)."""
    if isinstance(v, (list, tuple)):
        return tuple(_norm(x) for x in v)
    if isinstance(v, dict):
        return tuple(sorted((k, _norm(x)) for k, x in v.items()))
    return v


def hyper_mismatches(saved, current, fields=CHECKED_FIELDS):
    """Names of the checked fields in which two `hyper` dicts differ, in the order of `fields`.  Fields outside `fields` are ignored."""
    missing = object()
    return [f for f in fields if _norm(saved.get(f, missing)) != _norm(current.get(f, missing))]


def switch_mismatches(saved, current, fields=SWITCH_FIELDS):
    """Names of the switches (absent = off) in which two `hyper` dicts differ."""
    return [f for f in fields if bool(saved.get(f, False)) != bool(current.get(f, False))]


def value_mismatches(saved, current, fields=VALUE_FIELDS):
    """Names of the valued keywords (absent = off) in which two `hyper` dicts differ: added, dropped, or another value."""
    return [f for f in fields if _norm(saved.get(f)) != _norm(current.get(f))]


def optimizer_hyper(optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio):
    """The `hyper` entries of the optimiser keywords, valued fields with absent = off: the optimiser's name, betas and eps only
    under "adamw", the warm-up's length and ratio only when it is > 0 -- nothing at the defaults, so such a dict stays what it was."""
    hy = {}
    if optimizer == "adamw":
        hy.update(optimizer="adamw", adam_betas=[float(b) for b in adam_betas], adam_eps=float(adam_eps))
    if lr_warmup:
        hy.update(lr_warmup=int(lr_warmup), lr_warmup_ratio=float(lr_warmup_ratio))
    return hy


def save_atomic(obj, path):
    """torch.save to a temporary name, then os.replace: a crash or a full disk during the save leaves the previous file intact."""
    tmp = path + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def save(path, trainer_state, keeper_state=None, loop_state=None):
    """ONE file: the trainer's `training_state()`, `SnapshotKeeper.state()` and what the loop itself must find unchanged (the tools: world
    size, seed, data, class prior).  Atomic: a crash during the write leaves the previous file intact (a stale `<path>.tmp` may remain;
    `load` never reads it)."""
    save_atomic({"format_version": FORMAT_VERSION, "trainer": trainer_state, "keeper": keeper_state, "loop": loop_state or {}}, path)


def load(path):
    """-> (trainer_state, keeper_state, loop_state).  ValueError if `path` is not a train-state file of this format version."""
    obj = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(obj, dict) or "trainer" not in obj or "format_version" not in obj:
        raise ValueError(f"{path!r} is not a train-state file (a snapshot holds the model only: pass it to --restore-from)")
    if obj["format_version"] != FORMAT_VERSION:
        raise ValueError(f"{path!r}: train-state format_version {obj['format_version']}, this build reads {FORMAT_VERSION}")
    return obj["trainer"], obj.get("keeper"), obj.get("loop") or {}


def transition_parameters(path):
    """The learned noise-transition parameters of a train-state file: {"ntm": ..., "wraw": ...} (lists of two for DeepLab, single tensors
    for the one-output models).  No snapshot holds them; T itself is sig_NTM(ntm) times the class prior (model/deeplab_multi.py:255-261)."""
    ts, _k, _l = load(path)
    if "ntm" not in ts:
        raise ValueError(f"{path!r} is the state of a {ts['hyper'].get('trainer')}: the warm-up stage learns no transition matrix")
    return {"ntm": ts["ntm"], "wraw": ts["wraw"]}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the trainers' side
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _host(v):
    return [t.detach().cpu() for t in v] if isinstance(v, list) else v.detach().cpu()


def _arch(tr):
    plan = tr.plan
    if hasattr(plan, "v3_layers"):
        return {"layers": list(plan.v3_layers), "width": plan.width, "assp_ch": plan.assp_ch}
    if hasattr(plan, "vgg_layers"):
        return {"vgg_layers": [list(l) for l in plan.vgg_layers]}
    return {"layers": list(plan.layers)}


class TrainStateMixin:
    """`training_state()` / `load_training_state()` of SimTTrainer, WarmupTrainer, SimTSingleTrainer and WarmupSingleTrainer."""

    def _hyper_state(self):
        hy = {k: v for k, v in self.hp.__dict__.items() if isinstance(v, (bool, int, float, str))}
        hy.update(B=self.B, H=self.H, W=self.W, dtype={torch.bfloat16: "bf16", torch.float32: "f32"}[self.dtype],
                  trainer=type(self).__name__, model=getattr(self, "model", "v2"), arch=_arch(self), format_version=FORMAT_VERSION)
        if getattr(self, "teacher_view", False):      # (absent = False: a state from before the keyword loads into a trainer without it)
            hy["teacher_view"] = True
        if getattr(self, "online_labels", None) is not None:      # (absent = off: the states of trainers without the keyword stay what they were)
            hy["online_labels"] = float(self.online_labels)
            if self.teacher is not None:
                hy["online_labels_every"] = int(self.teacher.every)
            if getattr(self, "online_labels_balanced", None) is not None:
                hy["online_labels_balanced"] = float(self.online_labels_balanced)
                hy["online_labels_momentum"] = float(self.online_labels_momentum)
            if getattr(self, "online_mix", None) is not None:
                hy["online_mix"] = float(self.online_mix)
                hy["online_mix_seed"] = int(self.online_mix_seed)
            if getattr(self, "online_labels_weighted", None) is not None:
                hy["online_labels_weighted"] = str(self.online_labels_weighted)
            if getattr(self, "online_source", False):
                hy["online_source"] = True
            if getattr(self, "entropy_min", None) is not None:
                hy.update(entropy_min=float(self.entropy_min), entropy_eta=float(self.entropy_eta), entropy_after=int(self.entropy_after))
            if getattr(self, "proto_denoise", None) is not None:
                hy.update(proto_denoise=float(self.proto_denoise), proto_momentum=float(self.proto_momentum))
            if getattr(self, "proto_contrast", None) is not None:
                hy.update(proto_contrast=float(self.proto_contrast), proto_contrast_temp=float(self.proto_contrast_temp),
                          proto_contrast_min_ratio=float(self.proto_contrast_min_ratio))
        if getattr(self, "uncertainty_rectify", None) is not None:      # (with or without online_labels; absent = off)
            hy["uncertainty_rectify"] = float(self.uncertainty_rectify)
        if getattr(self, "feat_dist", None) is not None:      # (absent = off, like the keywords above)
            hy.update(feat_dist=float(self.feat_dist), feat_dist_classes=[int(c) for c in self.feat_dist_classes],
                      feat_dist_min_ratio=float(self.feat_dist_min_ratio), feat_dist_sha256=self.feat_dist_sha256)
        hy.update(optimizer_hyper(getattr(self, "optimizer", "sgd"), getattr(self, "adam_betas", None), getattr(self, "adam_eps", None),
                                  getattr(self, "lr_warmup", 0), getattr(self, "lr_warmup_ratio", None)))
        return hy

    def _nbt_steps(self, key):
        """What state_dict() adds to the `num_batches_tracked` the trainer was given: the train-mode forwards of that BatchNorm so far.  Every
        BatchNorm of DeepLab-v2 runs; of DeepLabv3 those of the plan (not layer4's: DeepLabv3._dead_bns); DeepLab-VGG16 has none.  With
        `online_source` a micro-batch is two train-mode forwards, the source pass and the target pass."""
        model = getattr(self, "model", "v2")
        live = model == "v2" or (model == "v3" and key[:-len(".num_batches_tracked")] in self.plan.bn)
        return self.it_done * self.hp.iter_size * (2 if getattr(self, "online_source", False) else 1) if live else 0

    def training_state(self):
        """Everything the next `step()` depends on, as a plain dict of host tensors and Python scalars: `model` (= state_dict()),
        `momentum`, the NTM / W tensors with their Adam moments (SimT trainers), `it_done`, the device-side accumulators that outlive a step
        and reach `losses()` (the scalars of the last step with the cumulative bad-label count, and its host twin `bad_reported`), `hyper`
        and (SimT trainers) `frozen_sha256`; with a weight EMA (`ema_decay`, simt_amd/ema.py) also `ema` = {decay, updates, shadow} -- the key is
        absent without one, and `load_training_state` refuses a state whose `ema` does not fit the trainer's; with the EMA teacher
        (`ema_teacher_every`, simt_amd/ema_teacher.py) also `teacher` = {every, refreshes, params}: the frozen model as the last refresh left it
        (`frozen_sha256` stays the hash of the model the run started beside), refused likewise when the keyword is dropped, added or N differs.
        The warm-up trainers' online labels (`online_labels`, simt_amd/online_labels.py): `hyper` carries tau and N only when on, `frozen_sha256`
        is that of the start model, a moving teacher travels as the same `teacher` entry, and `accumulators` gains the cumulative label counts
        with their host twin; without the keyword the dict is what it was.  With `online_labels_balanced` `hyper` also carries P and M
        and `accumulators` the per-class thresholds (`label_thresholds`); their histogram is zero between steps and is not stored.  With
        `online_mix` `hyper` also carries P and S and the dict gains `mix_rng`, the `bit_generator.state` of the mix's generator:
        the resumed run draws what the uninterrupted one draws.  With `online_labels_weighted` `hyper` also carries the mode and
        `accumulators` the last micro-batch's weights (`label_quality`); without the keyword the dict is what it was.  With `online_source`
         `hyper` also carries `online_source: True` and `accumulators` the two kept losses of the last source pass (`source_hout`).
        With `optimizer="adamw"` the dict gains `momentum2` (Adam's second moment; `momentum` is its first) and `hyper` the
        optimiser's name, betas and eps; with `lr_warmup` > 0 `hyper` carries it and its ratio.  Without the keywords the dict is what it was.
        With `feat_dist` `hyper` also carries lambda, the classes, the ratio and `feat_dist_sha256` -- the hash of the frozen
        ImageNet trunk, which is not stored -- and `accumulators` the three scalars of the last labelled pass (`feat_dist_out`).
        With `entropy_min` `hyper` also carries lambda, eta and the iteration that switches the term on; nothing else is kept (the
        term's two scalars ride in `hout`).
        With `uncertainty_rectify` `hyper` also carries lambda_kl; nothing else is kept (the four scalars ride in `hout`).
        With `proto_denoise` `hyper` also carries temp and M and `accumulators` the prototypes, their update counts and the
        moved-cell counts of the last micro-batch (`proto_eta`, `proto_n`, `proto_changed_part`); without the keyword the dict is what it was.
        Synchronises the device.  Derived state (T, packed operands) and the frozen weights are not
        stored.  The one other device word `losses()` reads, the plan's sticky fused-BatchNorm error word, is not carried but CHECKED: while
        it is set the optimiser launches skip their updates yet `it_done` goes on counting, so what the trainer holds is no state of the
        run -- RuntimeError (`TrunkPlan.raise_on_fbn_error`), no dict, and a file written earlier stays the last good state.  Data parallel: every rank holds the same parameters, momentum and NTM state after the exchange, so rank 0's dict is THE
        state and every rank loads it; the rank-local BatchNorm running statistics of ranks >= 1 are not preserved."""
        torch.cuda.synchronize(self.dev)
        self.plan.raise_on_fbn_error()
        ts = {"model": self.state_dict(), "momentum": {n: t.detach().cpu() for n, t in self.mom.items()}, "it_done": int(self.it_done),
              "bad_reported": int(self._bad_reported), "hyper": self._hyper_state()}
        if getattr(self, "optimizer", "sgd") == "adamw":      # Adam's second moment (its first is `momentum`); absent under SGD
            ts["momentum2"] = {n: t.detach().cpu() for n, t in self.mom2.items()}
        for f in NTM_FIELDS:
            if hasattr(self, f):
                ts[f] = _host(getattr(self, f))
        if hasattr(self, "frozen_sha256"):
            ts["frozen_sha256"] = self.frozen_sha256
        if hasattr(self, "lout"):
            ts["accumulators"] = {"lout": self.lout.detach().cpu()}
        else:      # the warm-up trainers: the head's scalars (overwritten by every launch) and the bad-label accumulator beside them
            ts["accumulators"] = {"hout": self.hout[:16].detach().cpu(), "bad_labels": self.bad_labels.detach().cpu()}
            if getattr(self, "online_labels", None) is not None:      # the cumulative label counts and their host twin: `labelled` resumes exactly
                ts["accumulators"].update(label_counts=self.label_counts.detach().cpu(), counts_reported=[int(c) for c in self._counts_reported])
                if getattr(self, "online_labels_balanced", None) is not None:
                    ts["accumulators"]["label_thresholds"] = self.label_thr.detach().cpu()
                if getattr(self, "online_labels_weighted", None) is not None:      # the last micro-batch's weights: `label_quality` resumes exactly
                    ts["accumulators"]["label_quality"] = self.label_q.detach().cpu()
                if getattr(self, "online_source", False):      # the last source pass's losses: `source_seg1` / `source_seg2` resume exactly
                    ts["accumulators"]["source_hout"] = self.source_hout.detach().cpu()
                if getattr(self, "proto_denoise", None) is not None:      # the prototypes: the next micro-batch is labelled with them
                    ts["accumulators"].update(proto_eta=self.proto_eta.detach().cpu(), proto_n=self.proto_n.detach().cpu(),
                                              proto_changed_part=self.proto_changed_part.detach().cpu())
        if getattr(self, "feat_dist", None) is not None:      # the last labelled pass's three scalars: `feat_dist` / `feat_dist_cells` resume exactly
            ts["accumulators"]["feat_dist_out"] = self.fd_out.detach().cpu()
        if getattr(self, "online_mix", None) is not None:      # the position of the mix's own generator (numpy's plain dict of Python ints)
            ts["mix_rng"] = self._mix_rng.bit_generator.state
        if getattr(self, "ema", None) is not None:      # the weight EMA (simt_amd/ema.py): decay, update count, shadow; absent without one
            ts["ema"] = self.ema.state()
        if getattr(self, "teacher", None) is not None:      # the EMA teacher (simt_amd/ema_teacher.py): every, refresh count, the frozen model as it is now
            ts["teacher"] = self.teacher.state()
        return ts

    def load_training_state(self, ts):
        """Continue where `ts` (a `training_state()` dict, e.g. of `train_state.load`) was taken: the next `step()` computes, bit for bit,
        what the trainer that wrote it would have computed.  The trainer must have been constructed like that one -- same geometry, dtype,
        model / arch, hyper-parameters and frozen model; which weights it was given does not matter, they are replaced.  ValueError,
        naming what differs, otherwise; nothing has been changed then.  Every packed operand is rebuilt from the loaded masters
        (`plan.repack()`).  `state_dict()` afterwards reports the `num_batches_tracked` an uninterrupted run reports (the steps taken are
        counted once).  Data parallel: every rank loads the same dict (see training_state)."""
        bad = (hyper_mismatches(ts["hyper"], self._hyper_state()) + switch_mismatches(ts["hyper"], self._hyper_state()) +
               value_mismatches(ts["hyper"], self._hyper_state()) + value_mismatches(ts["hyper"], self._hyper_state(), fields=BALANCE_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=MIX_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=WEIGHTED_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=SOURCE_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=FEAT_DIST_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=OPTIMIZER_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=ENTROPY_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=UNCERTAINTY_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=PROTO_FIELDS) +
               value_mismatches(ts["hyper"], self._hyper_state(), fields=PROTO_CONTRAST_FIELDS))
        if bad:
            mine = self._hyper_state()
            raise ValueError("the train state was written by a different run: " +
                             ", ".join(f"{f} (state: {ts['hyper'].get(f)!r}, this trainer: {mine.get(f)!r})" for f in bad))
        if hasattr(self, "frozen_sha256") and ts.get("frozen_sha256") != self.frozen_sha256:
            raise ValueError(f"frozen_sha256 differs: the train state was written beside another frozen model (state: {ts.get('frozen_sha256')}, "
                             f"this trainer: {self.frozen_sha256}); give the resumed run the same --restore-from")
        if getattr(self, "online_mix", None) is not None and "mix_rng" not in ts:
            raise ValueError("mix_rng: the train state carries no generator state for online_mix")
        from .ema import state_mismatch
        why = state_mismatch(getattr(self, "ema", None), ts.get("ema"))
        if why:
            raise ValueError(why)
        from .ema_teacher import state_mismatch as teacher_mismatch
        why = teacher_mismatch(getattr(self, "teacher", None), ts.get("teacher"))
        if why:
            raise ValueError(why)
        problems = []
        moments2 = [("momentum2", ts.get("momentum2", {}), self.mom2)] if getattr(self, "optimizer", "sgd") == "adamw" else []
        for what, theirs, mine in [("momentum", ts["momentum"], self.mom), ("model", ts["model"], self.params)] + moments2:
            for n in mine:
                if n not in theirs:
                    problems.append(f"{what} {n}: missing")
                elif tuple(theirs[n].shape) != tuple(mine[n].shape):
                    problems.append(f"{what} {n}: shape {tuple(theirs[n].shape)}, expected {tuple(mine[n].shape)}")
            problems += [f"{what} {n}: unknown to this trainer" for n in theirs if n not in mine]
        for f in NTM_FIELDS:
            if hasattr(self, f):
                mine, theirs = getattr(self, f), ts.get(f)
                pairs = list(zip(mine, theirs)) if isinstance(mine, list) and isinstance(theirs, list) and len(mine) == len(theirs) else \
                    [(mine, theirs)] if torch.is_tensor(mine) and torch.is_tensor(theirs) else None
                if pairs is None or any(tuple(a.shape) != tuple(b.shape) for a, b in pairs):
                    problems.append(f"{f}: missing or of another shape")
        if problems:
            raise ValueError("the train state does not fit this trainer: " + "; ".join(problems[:8]) +
                             (f" (and {len(problems) - 8} more)" if len(problems) > 8 else ""))
        it_done = int(ts["it_done"])
        self.it_done = it_done
        for k, p in self.params.items():
            if k.endswith("num_batches_tracked"):
                p.fill_(int(ts["model"][k]) - self._nbt_steps(k))       # state_dict() adds the steps taken: count them once
            else:
                p.copy_(ts["model"][k])
        for n, buf in self.mom.items():
            buf.copy_(ts["momentum"][n])
        if moments2:
            for n, buf in self.mom2.items():
                buf.copy_(ts["momentum2"][n])
        for f in NTM_FIELDS:
            if hasattr(self, f):
                mine, theirs = getattr(self, f), ts[f]
                for a, b in (zip(mine, theirs) if isinstance(mine, list) else [(mine, theirs)]):
                    a.copy_(b)
        acc = ts["accumulators"]
        if hasattr(self, "lout"):
            self.lout.copy_(acc["lout"])
        else:
            self.hout[:16].copy_(acc["hout"])
            self.bad_labels.copy_(acc["bad_labels"])
            if getattr(self, "online_labels", None) is not None:
                self.label_counts.copy_(acc["label_counts"])
                self._counts_reported = [int(c) for c in acc["counts_reported"]]
                if getattr(self, "online_labels_balanced", None) is not None:
                    self.label_thr.copy_(acc["label_thresholds"])
                if getattr(self, "online_labels_weighted", None) is not None:
                    self.label_q.copy_(acc["label_quality"])
                if getattr(self, "online_source", False):
                    self.source_hout.copy_(acc["source_hout"])
                if getattr(self, "proto_denoise", None) is not None:
                    self.proto_eta.copy_(acc["proto_eta"])
                    self.proto_n.copy_(acc["proto_n"])
                    self.proto_changed_part.copy_(acc["proto_changed_part"])
        if getattr(self, "feat_dist", None) is not None:
            self.fd_out.copy_(acc["feat_dist_out"])
        self._bad_reported = int(ts["bad_reported"])
        if getattr(self, "online_mix", None) is not None:
            self._mix_rng.bit_generator.state = ts["mix_rng"]
        if getattr(self, "ema", None) is not None:
            self.ema.load_state(ts["ema"])
        if getattr(self, "teacher", None) is not None:      # the frozen model as the saved run's last refresh left it; its plan is re-packed
            self.teacher.load_state(ts["teacher"])
        self.plan.repack()
        torch.cuda.synchronize(self.dev)

