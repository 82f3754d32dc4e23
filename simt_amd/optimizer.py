"""The trainers' optimiser launch: the reference's SGD (simt_sgd_multi, duplicate listings) or AdamW (simt_adamw_multi), DESIGN 7.23.

`optimizer="sgd"` (the default) is the trainer it was: the same descriptor, the same launch, nothing allocated.  `optimizer="adamw"` is the
optimiser DAFormer's hyper-parameters are written for (lr 6e-5, weight decay 0.01, heads at 10x, poly power 1.0, 1500 iterations of linear
warm-up): torch.optim.AdamW's single-tensor update, decoupled weight decay, in ONE launch over a segment table that lists every applied
tensor ONCE -- the reference's duplicate listings are 3-4 sequential SGD updates of one tensor; replayed through Adam they would advance
the step count per listing, so they are not replayed.  The table keeps the groups of the SGD table (0: trunk at lr, 1: heads at 10 x lr) and
adds their twins without weight decay for the BatchNorm gamma and beta a trainer trains (2: trunk, 3: heads; DAFormer's norm_decay_mult = 0).
Biases decay like weights.  m reuses the SGD momentum buffers (`mom`), v is `mom2`: one more fp32 copy of the applied parameters.

The per-step constants are formed here in float64 and rounded once to fp32 (`adamw_constants`), as simt_adam_step_guarded forms its own.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .multi_tensor import CHUNK, Table

OPTIMIZERS = ("sgd", "adamw")
DEFAULT_BETAS = (0.9, 0.999)
DEFAULT_EPS = 1e-8
DEFAULT_WARMUP_RATIO = 1e-6


def check_optimizer(optimizer="sgd", adam_betas=DEFAULT_BETAS, adam_eps=DEFAULT_EPS, lr_warmup=0, lr_warmup_ratio=DEFAULT_WARMUP_RATIO):
    """The five keywords as (optimizer, (beta1, beta2), eps, warm-up iterations, warm-up ratio); ValueError naming the one that does not fit."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer={optimizer!r}: one of {OPTIMIZERS}")
    try:
        b1, b2 = (float(b) for b in adam_betas)
    except (TypeError, ValueError):
        raise ValueError(f"adam_betas={adam_betas!r}: two numbers in [0, 1)") from None
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"adam_betas={adam_betas!r}: two numbers in [0, 1)")
    eps = float(adam_eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"adam_eps={adam_eps!r}: a number > 0")
    if lr_warmup is None or int(lr_warmup) != lr_warmup or lr_warmup < 0:
        raise ValueError(f"lr_warmup={lr_warmup!r}: a number of iterations >= 0")
    ratio = float(lr_warmup_ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"lr_warmup_ratio={lr_warmup_ratio!r}: a number in [0, 1]")
    return optimizer, (b1, b2), eps, int(lr_warmup), ratio


def adamw_constants(lrs, wds, betas, t):
    """The fp32 constants of one simt_adamw_multi launch at step t >= 1, each formed in float64 and rounded once:
    -> (step_size[g] = lr_g / (1 - beta1^t), decay[g] = 1 - lr_g * wd_g, beta1, beta2, 1 - beta1, 1 - beta2, sqrt(1 - beta2^t)).
    The betas enter as the fp32 numbers the kernel multiplies by, so its v recurrence and its bias correction speak of the same beta2."""
    f32 = np.float32
    b1, b2 = float(f32(betas[0])), float(f32(betas[1]))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step_size = [f32(float(lr) / bc1) for lr in lrs]
    decay = [f32(1.0 - float(lr) * float(wd)) for lr, wd in zip(lrs, wds)]
    return step_size, decay, f32(b1), f32(b2), f32(1.0 - b1), f32(1.0 - b2), f32(math.sqrt(bc2))


def adamw_table(recs, chunk=CHUNK):
    """recs: (p, g, m, v device pointers, n, group) per tensor -> (segment bytes as a uint8 array, [(segment, chunk index)])."""
    t = Table(recs, L.ADAMW_SEG, "n", chunk, "cpu")
    return t.host, t.pairs


def is_norm_parameter(name, params):
    """A BatchNorm's gamma or beta: `<module>.weight` / `<module>.bias` of a module that keeps running statistics."""
    mod, _, leaf = name.rpartition(".")
    return leaf in ("weight", "bias") and (mod + ".running_mean") in params


class OptimizerMixin:
    """`_build_sgd`, `_init_optimizer` (behind it) and `_optim_step`, the one optimiser launch of SimTTrainer, WarmupTrainer, SimTSingleTrainer
    and WarmupSingleTrainer.  The trainer provides params, plan.grads, hp, it_done and dev."""

    def _build_sgd(self, listing):
        """listing: [(name, mult, group)] in table order -- the SGD launch replays a tensor's `mult` duplicate listings in registers."""
        self.mom = {n: torch.zeros_like(self.params[n]) for n, _m, _g in listing}
        self.sgd_names = [n for n, _m, _g in listing]
        self.sgd_groups = {n: g for n, _m, g in listing}
        table = Table([(self.params[n].data_ptr(), self.plan.grads[n].data_ptr(), self.mom[n].data_ptr(), self.params[n].numel(), mult, g)
                       for n, mult, g in listing], L.SGD_SEG, "n", CHUNK, self.dev)
        self.sgd_segs, self.sgd_chunks = table.segs, table.chunks
        self.sgd_desc = table.bind(L.SgdDesc(), getattr(self.plan, "fbn_err", None))
        self.sgd_desc.momentum, self.sgd_desc.dampening = self.hp.momentum, 0.0

    def _init_optimizer(self, optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio):
        self.optimizer, self.adam_betas, self.adam_eps, self.lr_warmup, self.lr_warmup_ratio = \
            check_optimizer(optimizer, adam_betas, adam_eps, lr_warmup, lr_warmup_ratio)
        if self.optimizer != "adamw":
            return
        self.mom2 = {n: torch.zeros_like(self.mom[n]) for n in self.sgd_names}
        group = lambda n: self.sgd_groups[n] + (2 if is_norm_parameter(n, self.params) else 0)
        table = Table([(self.params[n].data_ptr(), self.plan.grads[n].data_ptr(), self.mom[n].data_ptr(), self.mom2[n].data_ptr(),
                        self.params[n].numel(), group(n)) for n in self.sgd_names],      # every applied tensor ONCE, whatever the SGD table's `mult` says
                      L.ADAMW_SEG, "n", CHUNK, self.dev)
        self.adamw_segs, self.adamw_chunks = table.segs, table.chunks
        self.adamw_desc = table.bind(L.AdamwDesc(), getattr(self.plan, "fbn_err", None))      # the guard word of the SGD launch
        self.adamw_desc.eps = self.adam_eps

    def _optim_step(self, lr, st):
        """The optimiser launch of this step on stream `st`: group 0 at `lr`, group 1 at 10 x lr (AdamW: 2 and 3 likewise, without decay)."""
        wd = self.hp.weight_decay
        if self.optimizer == "adamw":
            d = self.adamw_desc
            step_size, decay, b1, b2, omb1, omb2, bc2s = adamw_constants((lr, lr * 10.0, lr, lr * 10.0), (wd, wd, 0.0, 0.0), self.adam_betas,
                                                                         self.it_done + 1)
            for i in range(4):
                d.step_size[i], d.decay[i] = step_size[i], decay[i]
            d.beta1, d.beta2, d.omb1, d.omb2, d.bc2s = b1, b2, omb1, omb2, bc2s
            d.first_step = 1 if self.it_done == 0 else 0
            L.call("simt_adamw_multi", C.byref(d), st)
            return
        d = self.sgd_desc
        d.lr[0], d.lr[1] = lr, lr * 10.0
        d.wd[0], d.wd[1] = wd, wd
        d.first_step = 1 if self.it_done == 0 else 0
        L.call("simt_sgd_multi", C.byref(d), st)
