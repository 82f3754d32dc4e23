"""Exponential moving average of the weights: a shadow model that follows the trainer's masters, one launch per optimiser step.

`WeightEma(params, decay)` keeps one fp32 device tensor per floating tensor of a trainer's `params` -- weights, biases, BatchNorm affine AND
BatchNorm running statistics (timm's ModelEmaV2 semantics: an eval-mode forward of the averaged weights needs statistics that belong to
them) -- initialised as a bit copy.  `update(stream)` is ONE `simt_ema_multi` launch over all of them (csrc/ema.hip), held bit for bit to the
arithmetic contract of include/simt_hip.h: e <- e + omd * (w - e) in float32, three roundings, no FMA.  `num_batches_tracked` (int64) has no
shadow: `params` / `ema_state_dict()` report the live values.

Decay schedule (DAFormer's): the update with 0-based index t uses omd_t = float32(max(1 - D, 1 / (t + 1))), computed in float64 and rounded
once -- update 0 is the copy, the shadow is the plain running mean of the iterates until 1 / (t + 1) falls below 1 - D, the exponential average
from there on.  The update count is state of the EMA (not the trainer's `it_done`) and lives on the host: the launch is given the plan's sticky
fused-BatchNorm error word (`skip_if`) and changes nothing while it is set, which the host cannot see -- so after a step behind which
`losses()` / `training_state()` raise, `updates` has counted launches that skipped.  That state is undefined for the live model too and
`training_state()` refuses to save it; a run continues from the last good train state, which carries the count that belongs to its shadow.

The EMA is a pure observer: it reads the masters and writes only its own tensors; the trained trajectory is bit for bit the one without it.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .multi_tensor import CHUNK, Table


def check_decay(decay):
    """-> float(decay); ValueError unless 0 <= decay < 1."""
    d = float(decay)
    if not (0.0 <= d < 1.0):
        raise ValueError(f"ema decay {decay!r}: expected a value in [0, 1)")
    return d


def omd_schedule(decay, t):
    """1 - decay of the update with 0-based index t, as the float32 the kernel is given: max(1 - D, 1 / (t + 1)) in float64, rounded once."""
    return np.float32(max(1.0 - float(decay), 1.0 / (int(t) + 1.0)))


class WeightEma:
    def __init__(self, params, decay, *, skip_if=None):
        """params: a trainer's {name: device tensor}; decay: D in [0, 1); skip_if: the plan's fused-BatchNorm error word (int64 device tensor)
        or None."""
        self.decay = check_decay(decay)
        self.live = params
        self.updates = 0
        self.shadow = {k: v.detach().clone() for k, v in params.items() if v.is_floating_point()}
        assert all(v.dtype == torch.float32 and v.is_contiguous() and params[k].is_contiguous() for k, v in self.shadow.items())
        recs = [(params[k].data_ptr(), e.data_ptr(), e.numel()) for k, e in self.shadow.items() if e.numel() > 0]
        table = Table(recs, L.EMA_SEG, "n", CHUNK, next(iter(params.values())).device)
        self.segs, self.chunks, self.elements = table.segs, table.chunks, table.elements
        self._skip_if = skip_if
        self.desc = table.bind(L.EmaDesc(), skip_if)

    @property
    def params(self):
        """Device dict with the keys of the live `params`: the shadow for floating tensors, the live tensor itself for the rest
        (`num_batches_tracked`).  `Evaluator.load()` takes it as is."""
        return {k: self.shadow.get(k, v) for k, v in self.live.items()}

    def update(self, stream):
        """One launch on `stream` (a raw stream handle): the shadow moves towards the masters as they are on that stream at this point."""
        self.desc.omd = float(omd_schedule(self.decay, self.updates))
        L.call("simt_ema_multi", C.byref(self.desc), stream)
        self.updates += 1

    # ------------------------------------------------------------------ train state
    def state(self):
        return {"decay": self.decay, "updates": int(self.updates), "shadow": {k: v.detach().cpu() for k, v in self.shadow.items()}}

    def mismatch(self, saved):
        """Why `saved` (a `state()` dict) does not fit this EMA, or None."""
        if float(saved["decay"]) != self.decay:
            return f"ema decay differs (state: {saved['decay']!r}, this trainer: {self.decay!r})"
        theirs, problems = saved["shadow"], []
        for n, e in self.shadow.items():
            if n not in theirs:
                problems.append(f"{n}: missing")
            elif tuple(theirs[n].shape) != tuple(e.shape):
                problems.append(f"{n}: shape {tuple(theirs[n].shape)}, expected {tuple(e.shape)}")
        problems += [f"{n}: unknown to this trainer" for n in theirs if n not in self.shadow]
        if problems:
            return "ema shadow does not fit this trainer: " + "; ".join(problems[:8]) + (f" (and {len(problems) - 8} more)" if len(problems) > 8 else "")
        return None

    def load_state(self, saved):
        for n, e in self.shadow.items():
            e.copy_(saved["shadow"][n])
        self.updates = int(saved["updates"])


def state_mismatch(ema, saved):
    """The `ema` entry of a train state against a trainer's EMA (either may be None): the reason they do not fit, or None."""
    if ema is None and saved is None:
        return None
    if ema is None:
        return (f"ema: the train state was written with a weight EMA (decay {saved.get('decay')!r}), this trainer has none "
                "(pass the same ema_decay / --ema)")
    if saved is None:
        return f"ema: this trainer keeps a weight EMA (decay {ema.decay!r}), the train state was written without one"
    return ema.mismatch(saved)


class EmaMixin:
    """`ema_params`, `ema_state_dict()` and `ema_updates` of the four trainers (keyword `ema_decay`; None: no shadow, no launch)."""

    def _init_ema(self, ema_decay):
        self.ema = None if ema_decay is None else WeightEma(self.params, ema_decay, skip_if=getattr(self.plan, "fbn_err", None))

    def _need_ema(self):
        if getattr(self, "ema", None) is None:
            raise RuntimeError(f"this {type(self).__name__} was built without ema_decay: it keeps no weight EMA")
        return self.ema

    @property
    def ema_params(self):
        return self._need_ema().params

    @property
    def ema_updates(self):
        return self._need_ema().updates

    def ema_state_dict(self):
        """Host copy of the averaged model: the keys, shapes and dtypes of `state_dict()`, floating tensors from the shadow,
        `num_batches_tracked` as `state_dict()` reports it.  Loads strict=True where `state_dict()` does."""
        ema = self._need_ema()
        sd = {}
        for k, v in self.params.items():
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.tensor(int(v.item()) + self._nbt_steps(k), dtype=torch.long)
            else:
                sd[k] = ema.shadow.get(k, v).detach().cpu()
        return sd
