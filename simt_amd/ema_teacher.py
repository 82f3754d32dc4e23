"""The EMA teacher: the SimT stage's frozen model follows the weight EMA (keyword `ema_teacher_every`, tool flag --ema-teacher).

The frozen model's low-res posterior decides which pixels get a confidence label.  Without this module it is loaded once and never changes.
With `ema_teacher_every=N` the trainer REFRESHES it behind every EMA update that brings `ema.updates` to a multiple of N: the frozen model's
floating tensors become bit copies of their shadows (simt_amd/ema.py) and the frozen plan's operands are re-derived from them.  A refresh is a
fixed launch list, built once by the constructor and replayed on the stream the EMA update ran on, directly behind it:

  1. ONE `simt_ema_multi` launch with omd = 1 (its word-copy flavour) over a table shadow -> `fixed_params`, every floating tensor of the frozen
     model, with the EMA's `skip_if` word: while the plan's sticky fused-BatchNorm error word is set the copy changes nothing and the frozen
     model stays the last good teacher (the launches behind it then re-derive the operands they already hold).  `num_batches_tracked` is not
     touched.
  2. ONE `simt_bn_fold_multi` launch (csrc/bn_fold_multi.hip) over every BatchNorm fold of the frozen plan -- bit for bit the plan's own
     `simt_bn_fold` launches, 104 of them for a ResNet-101 trunk.  Not issued where the plan folds nothing (VGG16).
  3. every other entry of the frozen plan's pack list in its original order, weight packs coalesced (`simt_pack_weight_multi`,
     `simt_stem7_pack`, `simt_vec_acc`): the entries `plan.repack()` replays, which read the folded scales of 2.

The frozen model's keys are a subset of the student's: the closed-set heads (`layer5` / `layer6`; DeepLabv3's `conv`) have their shadows, the
open-set modules have no counterpart in the frozen model.  DeepLab-VGG16 has ONE classifier with num_classes + open_classes output rows whose
first num_classes rows are the closed-set classes: there the frozen tensor follows that leading block of its shadow (`prefix_rows`), a
contiguous prefix, so the copy stays a plain segment.

`frozen_sha256` keeps its meaning: the hash of the model the run STARTED beside, taken before any refresh; a resumed run is given the same
--restore-from.  Between two refreshes (N > 1) the teacher is not the current shadow, so the train state carries it:
`teacher = {every, refreshes, params}` (simt_amd/train_state.py).

The host decides when a refresh is due from `ema.updates`, which also counts updates the error word made skip (simt_amd/ema.py): such a state
is refused by `training_state()` and a run continues from the last good train state, whose counts belong to its tensors.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .multi_tensor import CHUNK, Table

FOLD_CHUNK = 256         # channels per workgroup of simt_bn_fold_multi: one per lane


def check_every(every):
    """-> int(every); ValueError unless it is an integer >= 1."""
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or int(every) < 1:
        raise ValueError(f"ema_teacher_every {every!r}: expected an integer >= 1")
    return int(every)


def refresh_due(updates, every):
    """Is a refresh due behind the EMA update that brought the update count to `updates`?  Behind every `every`-th one; never before the first."""
    return int(updates) > 0 and int(updates) % int(every) == 0


def teacher_sources(fixed_shapes, shadow_shapes, prefix_rows=0):
    """Which shadow feeds each floating tensor of the frozen model.  fixed_shapes / shadow_shapes: {key: shape}.  -> ({key: elements copied},
    problems): a key is served by the shadow of the same name and shape, or -- with prefix_rows = K > 0 -- by the first rows of a shadow that has
    exactly K more of them (the one-classifier model); every other key is a problem."""
    served, problems = {}, []
    for k, shp in fixed_shapes.items():
        shp = tuple(shp)
        theirs = shadow_shapes.get(k)
        if theirs is None:
            problems.append(f"{k}: no shadow")
            continue
        theirs = tuple(theirs)
        if theirs == shp or (prefix_rows > 0 and len(shp) >= 1 and theirs[1:] == shp[1:] and theirs[0] == shp[0] + prefix_rows):
            served[k] = int(np.prod(shp, dtype=np.int64))
        else:
            problems.append(f"{k}: shadow of shape {theirs}, frozen tensor of shape {shp}")
    return served, problems


def state_mismatch(teacher, saved):
    """The `teacher` entry of a train state against a trainer's teacher (either may be None): the reason they do not fit, naming the field
    (`ema_teacher`), or None."""
    if teacher is None and saved is None:
        return None
    if teacher is None:
        return (f"ema_teacher: the train state was written with the EMA teacher (every {saved.get('every')!r}), this trainer's frozen model does "
                "not move (pass the same ema_teacher_every / --ema-teacher)")
    if saved is None:
        return (f"ema_teacher: this trainer's frozen model follows the EMA (every {teacher.every!r}), the train state was written with a frozen "
                "model that does not move")
    if int(saved["every"]) != teacher.every:
        return f"ema_teacher every differs (state: {saved['every']!r}, this trainer: {teacher.every!r})"
    theirs, problems = saved["params"], []
    for k, n in teacher.copied.items():
        if k not in theirs:
            problems.append(f"{k}: missing")
        elif tuple(theirs[k].shape) != tuple(teacher.fixed_params[k].shape):
            problems.append(f"{k}: shape {tuple(theirs[k].shape)}, expected {tuple(teacher.fixed_params[k].shape)}")
    problems += [f"{k}: unknown to this trainer" for k in theirs if k not in teacher.copied]
    if problems:
        return "ema_teacher params do not fit this trainer: " + "; ".join(problems[:8]) + (f" (and {len(problems) - 8} more)" if len(problems) > 8 else "")
    return None


class TeacherRefresh:
    def __init__(self, ema, fixed_params, fixed_plan, every, *, prefix_rows=0):
        """ema: the trainer's WeightEma; fixed_params / fixed_plan: the frozen model's device tensors and its eval-mode plan; every: N >= 1;
        prefix_rows: open_classes for the one-classifier model (see the module docstring), 0 otherwise."""
        self.every = check_every(every)
        self.refreshes = 0
        self.ema, self.fixed_params, self.plan = ema, fixed_params, fixed_plan
        floating = {k: v for k, v in fixed_params.items() if v.is_floating_point()}
        self.copied, problems = teacher_sources({k: v.shape for k, v in floating.items()}, {k: v.shape for k, v in ema.shadow.items()},
                                                prefix_rows)
        if problems:
            raise ValueError("ema_teacher_every: floating tensors of the frozen model without a shadow of their shape: " + "; ".join(problems[:8]) +
                             (f" (and {len(problems) - 8} more)" if len(problems) > 8 else ""))
        assert all(v.dtype == torch.float32 and v.is_contiguous() for v in floating.values())
        dev = fixed_plan.dev
        lib = L.load()
        self.launches = []                 # (entry point, arguments without the stream): built once, replayed by run()
        self._keep = []
        # ---- 1. shadow -> fixed_params: the EMA kernel's word copy over a table of its own
        recs = [(ema.shadow[k].data_ptr(), floating[k].data_ptr(), n) for k, n in self.copied.items() if n > 0]
        copy = Table(recs, L.EMA_SEG, "n", CHUNK, dev)
        self.elements = copy.elements
        d = copy.bind(L.EmaDesc(), ema._skip_if)
        d.omd = 1.0
        self.copy_desc = d
        self._keep.append(copy)
        self.launches.append((lib.simt_ema_multi, (C.byref(d),)))
        # ---- 2. every BatchNorm fold of the frozen plan in one launch
        raw = fixed_plan._pack_items_raw
        folds = [it for it in raw if it.fn is lib.simt_bn_fold]
        self.fold_desc = None
        if folds:
            eps = folds[0].args[4]
            assert all(it.args[4] == eps for it in folds)
            fold = Table([it.args[:4] + it.args[5:] for it in folds], L.BN_FOLD_SEG, "C", FOLD_CHUNK, dev)
            host = (L.BnFoldSeg * len(folds)).from_buffer_copy(fold.host)      # the same records in host memory: what the library's refusals read
            fd = fold.bind(L.BnFoldDesc())
            fd.segs_host, fd.nsegs, fd.eps = host, len(folds), eps
            self.fold_desc = fd
            self._keep += [host, fold]
            self.launches.append((lib.simt_bn_fold_multi, (C.byref(fd),)))
        # ---- 3. the rest of the pack list in its original order, packs coalesced: the plan's own coalesced list (engine.LaunchList.coalesce_packs,
        #         device tables included) without its folds.  The folds only read parameters, so running all of them first keeps every
        #         scale in front of the pack that reads it.
        rest = [it for it in fixed_plan.pack_list.items if it.fn is not lib.simt_bn_fold]
        others = lambda items: [(it.fn, it.args) for it in items if it.fn not in (lib.simt_bn_fold, lib.simt_pack_weight, lib.simt_pack_weight_multi)]
        assert others(rest) == others(raw) and all(it.fn is not None and it.stream == 0 for it in rest)
        self.launches += [(it.fn, it.args) for it in rest]

    def run(self, stream):
        """Replay the refresh on `stream` (a raw stream handle)."""
        for fn, args in self.launches:
            rc = fn(*args, stream)
            if rc != 0:
                L.check(rc)
        self.refreshes += 1

    # ------------------------------------------------------------------ train state
    def state(self):
        return {"every": self.every, "refreshes": int(self.refreshes), "params": {k: self.fixed_params[k].detach().cpu() for k in self.copied}}

    def load_state(self, saved):
        for k in self.copied:
            self.fixed_params[k].copy_(saved["params"][k])
        self.refreshes = int(saved["refreshes"])
        self.plan.repack()


class TeacherMixin:
    """`teacher_refreshes`, `teacher_params` and `teacher_state_dict()` of SimTTrainer and SimTSingleTrainer (keyword `ema_teacher_every`; None:
    the frozen model never moves, no launch, no buffer)."""

    def _init_teacher(self, every, prefix_rows=0):
        self.teacher = None
        if every is None:
            return
        every = check_every(every)
        if getattr(self, "ema", None) is None:
            raise ValueError("ema_teacher_every needs ema_decay: the frozen model follows the weight EMA, and this trainer keeps none")
        self.teacher = TeacherRefresh(self.ema, self.fixed_params, self.fixed, every, prefix_rows=prefix_rows)

    def _teacher_follows(self, stream):
        """Called directly behind `ema.update(stream)`: the refresh, on the same stream, if that update made one due."""
        if self.teacher is not None and refresh_due(self.ema.updates, self.teacher.every):
            self.teacher.run(stream)

    def _need_teacher(self):
        if getattr(self, "teacher", None) is None:
            raise RuntimeError(f"this {type(self).__name__} was built without ema_teacher_every: its frozen model does not move")
        return self.teacher

    @property
    def teacher_refreshes(self):
        """Refreshes ENQUEUED so far.  Like `ema_updates` it counts on the host: a refresh issued while the fused-BatchNorm error word was set
        copied nothing (the frozen model kept the last good teacher) and is counted all the same."""
        return self._need_teacher().refreshes

    @property
    def teacher_params(self):
        """The device dict the frozen plan reads (`fixed_params`)."""
        return self._need_teacher().fixed_params

    def teacher_state_dict(self):
        """Host copy of the teacher as it is now: every key of the frozen model; loads strict=True into the closed-set nn.Module."""
        return {k: v.detach().cpu() for k, v in self._need_teacher().fixed_params.items()}
