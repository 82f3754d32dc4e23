"""The AdamW restatement (tests/_adamw_ref.py), the learning-rate schedule `lr_at` and the train state's optimiser fields, on the host.

The comparator must reject what it is there to reject (an element 4x its bound away, a dropped decay, swapped betas) before it is trusted to
accept the kernel; it must accept an honest fp32 evaluation of the recurrence, and torch.optim.AdamW itself -- which pins the formula to
torch's and not to a reading of it."""
import numpy as np
import pytest
import torch

import _adamw_ref as ref
from simt_amd import optimizer as opt
from simt_amd import train_state as tsf
from simt_amd.step import lr_at, lr_poly

# betas that ARE fp32 numbers: torch forms 1 - beta from the Python float, the contract from the fp32 beta the kernel multiplies by; for
# such betas the two are the same number, so torch's result is held to the bound with no allowance for a constant's rounding
EXACT_BETAS = (0.875, 0.998046875)
GROUPS = [(6e-5, 0.01), (6e-4, 0.01), (6e-5, 0.0), (6e-4, 0.0)]      # (lr, wd): trunk, heads at 10x, and their twins without decay


def _data(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10.0 ** float(-(k % 3)) for k in range(3)]
    group = torch.arange(n) % 4
    return p0, grads, group


def _run_ref(p0, grads, group, betas, eps, lr_scale=lambda k: 0.7 ** k):
    """Three chained steps of the restatement -> [(p, m, v) per step], and the constants of every step."""
    p, m, v = ref.exact(p0), None, None
    out, consts = [], []
    for k, g in enumerate(grads):
        c = ref.constants([lr * lr_scale(k) for lr, _wd in GROUPS], [wd for _lr, wd in GROUPS], betas, k + 1)
        p, m, v = ref.adamw_ref(p, ref.exact(g), m, v, ref.per_element(c["step_size"], group), ref.per_element(c["decay"], group),
                                c["beta2"], c["omb1"], c["omb2"], c["bc2s"], eps, k == 0)
        out.append((p, m, v))
        consts.append(c)
    return out, consts


def _run_f32(p0, grads, group, consts, eps, drop_decay=False, swap_betas=False):
    p, m, v = p0.numpy().copy(), None, None
    g_idx = group.numpy()
    out = []
    for k, (g, c) in enumerate(zip(grads, consts)):
        decay = np.ones(4, np.float32) if drop_decay else np.array(c["decay"], np.float32)
        b2, o1, o2 = (c["beta1"], c["omb2"], c["omb1"]) if swap_betas else (c["beta2"], c["omb1"], c["omb2"])
        p, m, v = ref.adamw_f32(p, g.numpy(), m, v, np.array(c["step_size"], np.float32)[g_idx], decay[g_idx], b2, o1, o2, c["bc2s"], eps, k == 0)
        out.append((p, m, v))
    return out


def test_comparator_accepts_fp32_numpy_over_three_steps():
    p0, grads, group = _data(4099, 1)
    want, consts = _run_ref(p0, grads, group, (0.9, 0.999), 1e-8)
    got = _run_f32(p0, grads, group, consts, 1e-8)
    worst = 0.0
    for k in range(3):
        for name, a, b in zip("pmv", got[k], want[k]):
            worst = max(worst, ref.ratio(torch.from_numpy(a), b, f"step {k} {name}"))
    print(f"fp32 numpy against the restatement: worst |fp32 - float64| / bound = {worst:.3f} (allowed {ref.SLACK})")
    assert worst > 0.0      # the fp32 evaluation does round: a bound of zero would accept nothing, a ratio of zero would show nothing


def test_comparator_accepts_second_moments_among_the_subnormals():
    """Gradients of 1e-19 (a trunk's far corners hold such): omb2 * g * g is about 1e-41, a subnormal, whose rounding error is half the
    subnormal spacing and not u x its magnitude -- the eta of the restatement.  Without eta the honest fp32 evaluation would be rejected."""
    p0, grads, group = _data(4099, 5)
    grads = [g * 1e-19 for g in grads]
    for g in grads:
        g[::5] = 0.0      # and gradients of exactly zero: v = 0, whose bound is eta alone
    want, consts = _run_ref(p0, grads, group, (0.9, 0.999), 1e-8)
    got = _run_f32(p0, grads, group, consts, 1e-8)
    v = got[0][2]
    assert ((v > 0) & (v < np.float32(2.0 ** -126))).mean() > 0.5, "the case is about subnormal second moments"
    for k in range(3):
        for name, a, b in zip("pmv", got[k], want[k]):
            ref.ratio(torch.from_numpy(a), b, f"step {k} {name}")
    rel_only = ref.V(want[0][2].v, want[0][2].e - ref.ETA * 2)      # the bound of v without the two products' eta
    with pytest.raises(AssertionError, match="x its bound"):
        ref.ratio(torch.from_numpy(v), rel_only, "v without eta")


def test_comparator_rejects_and_names_an_element_4x_its_bound_away():
    p0, grads, group = _data(1031, 2)
    want, consts = _run_ref(p0, grads, group, (0.9, 0.999), 1e-8)
    got = _run_f32(p0, grads, group, consts, 1e-8)
    for name, a, b in zip("pmv", got[2], want[2]):
        red = torch.from_numpy(a.copy())
        idx = 517
        red[idx] = float(b.v[idx] + 4.0 * b.e[idx])
        if float(red[idx]) == float(a[idx]):      # (the push must be visible in fp32, or the case shows nothing)
            pytest.fail(f"{name}: 4x the bound of element {idx} is below fp32 resolution")
        with pytest.raises(AssertionError, match=f"element {idx} "):
            ref.ratio(red, b, f"red {name}")
    nan = torch.from_numpy(got[2][0].copy())
    nan[3] = float("nan")
    with pytest.raises(AssertionError, match="NaN stored"):
        ref.ratio(nan, want[2][0], "nan p")


def test_comparator_rejects_a_dropped_decay_and_swapped_betas():
    p0, grads, group = _data(1031, 3)
    want, consts = _run_ref(p0, grads, group, (0.9, 0.999), 1e-8, lr_scale=lambda k: 100.0)      # (a decay of 1 - 6e-5 is visible at this lr)
    ok = _run_f32(p0, grads, group, consts, 1e-8)
    ref.ratio(torch.from_numpy(ok[0][0]), want[0][0], "p")
    dropped = _run_f32(p0, grads, group, consts, 1e-8, drop_decay=True)
    with pytest.raises(AssertionError, match="x its bound"):
        ref.ratio(torch.from_numpy(dropped[0][0]), want[0][0], "p without decay")
    swapped = _run_f32(p0, grads, group, consts, 1e-8, swap_betas=True)
    for name, a, b in zip("pmv", swapped[1], want[1]):
        with pytest.raises(AssertionError, match="x its bound"):
            ref.ratio(torch.from_numpy(a), b, f"{name} with swapped betas")


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_comparator_accepts_torch_adamw(eps):
    """torch.optim.AdamW (single-tensor path, fp32, CPU) on four groups with different lr and wd, three steps with the lr changing per step."""
    n = 2053
    gen = torch.Generator().manual_seed(4)
    tensors = [torch.randn(n, generator=gen).requires_grad_() for _ in GROUPS]
    p0 = torch.cat([t.detach() for t in tensors])
    group = torch.arange(4).repeat_interleave(n)
    o = torch.optim.AdamW([{"params": [t], "lr": lr, "weight_decay": wd} for t, (lr, wd) in zip(tensors, GROUPS)], betas=EXACT_BETAS, eps=eps,
                          foreach=False)
    p, m, v = ref.exact(p0), None, None
    worst = 0.0
    for k in range(3):
        g = torch.randn(4 * n, generator=gen) * 10.0 ** float(-k)
        lrs = [lr * 0.7 ** k for lr, _wd in GROUPS]
        for t, pg, lr, gi in zip(tensors, o.param_groups, lrs, g.split(n)):
            t.grad = gi.clone()
            pg["lr"] = lr
        o.step()
        c = ref.constants(lrs, [wd for _lr, wd in GROUPS], EXACT_BETAS, k + 1)
        p, m, v = ref.adamw_ref(p, ref.exact(g), m, v, ref.per_element(c["step_size"], group), ref.per_element(c["decay"], group),
                                c["beta2"], c["omb1"], c["omb2"], c["bc2s"], eps, k == 0)
        st = [o.state[t] for t in tensors]
        worst = max(worst, ref.ratio(torch.cat([t.detach() for t in tensors]), p, f"step {k} p"),
                    ref.ratio(torch.cat([s["exp_avg"] for s in st]), m, f"step {k} m"),
                    ref.ratio(torch.cat([s["exp_avg_sq"] for s in st]), v, f"step {k} v"))
    print(f"torch.optim.AdamW against the restatement, eps {eps}: worst ratio {worst:.3f} (allowed {ref.SLACK})")


def test_constants_of_the_package_are_the_contract_s():
    for t in (1, 2, 7, 1500):
        lrs, wds = [lr for lr, _ in GROUPS], [wd for _, wd in GROUPS]
        c = ref.constants(lrs, wds, (0.9, 0.999), t)
        step_size, decay, b1, b2, omb1, omb2, bc2s = opt.adamw_constants(lrs, wds, (0.9, 0.999), t)
        assert [x.tobytes() for x in step_size] == [x.tobytes() for x in c["step_size"]]
        assert [x.tobytes() for x in decay] == [x.tobytes() for x in c["decay"]]
        assert (b1, b2, omb1, omb2, bc2s) == (c["beta1"], c["beta2"], c["omb1"], c["omb2"], c["bc2s"])
    assert c["omb1"] == np.float32(1.0) - np.float32(0.9)      # `1.f - beta` of simt_adam_step: the same fp32 number


def test_lr_at():
    base, n_it, power = 6e-5, 40000, 1.0
    for it in (0, 1, 17, 39999):
        for pw in (0.9, 1.0):
            assert lr_at(base, it, n_it, pw) == lr_poly(base, it, n_it, pw)
            assert lr_at(base, it, n_it, pw, 0, 0.5) == lr_poly(base, it, n_it, pw)
    N, r = 1500, 1e-6
    poly = lambda it: base * (1 - it / n_it) ** power
    assert lr_at(base, 0, n_it, power, N, r) == pytest.approx(base * r, rel=1e-12)                              # it = 0: ratio x base
    assert lr_at(base, 1, n_it, power, N, r) == pytest.approx(poly(1) * (1 - (1499 / 1500) * (1 - r)), rel=1e-12)
    assert lr_at(base, N - 1, n_it, power, N, r) == pytest.approx(poly(N - 1) * (1 - (1 / 1500) * (1 - r)), rel=1e-12)
    assert lr_at(base, N, n_it, power, N, r) == lr_poly(base, N, n_it, power)                                   # the ramp has ended: poly itself
    assert lr_at(base, N + 1, n_it, power, N, r) == lr_poly(base, N + 1, n_it, power)
    ramp = [lr_at(base, it, n_it, power, N, r) for it in range(N + 1)]
    assert all(b > a for a, b in zip(ramp, ramp[1:])), "the ramp rises at every iteration"
    assert lr_at(2.5e-4, 2, 10, 0.9, 4, 0.25) == pytest.approx(2.5e-4 * 0.8 ** 0.9 * (1 - 0.5 * 0.75), rel=1e-12)


def test_check_optimizer():
    assert opt.check_optimizer() == ("sgd", (0.9, 0.999), 1e-8, 0, 1e-6)
    assert opt.check_optimizer("adamw", [0.8, 0.99], 1e-6, 1500, 0.1) == ("adamw", (0.8, 0.99), 1e-6, 1500, 0.1)
    for kw in (dict(optimizer="adam"), dict(adam_betas=(0.9,)), dict(adam_betas=(1.0, 0.999)), dict(adam_betas=(0.9, -0.1)), dict(adam_eps=0.0),
               dict(lr_warmup=-1), dict(lr_warmup=1.5), dict(lr_warmup_ratio=1.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            opt.check_optimizer(**kw)


def test_norm_parameters_and_table():
    params = {"a.conv.weight": 0, "a.bn.weight": 0, "a.bn.bias": 0, "a.bn.running_mean": 0, "a.bn.running_var": 0, "head.bias": 0}
    assert [n for n in params if opt.is_norm_parameter(n, params)] == ["a.bn.weight", "a.bn.bias"]
    segs, chunks = opt.adamw_table([(16, 32, 48, 64, 5, 1), (80, 96, 112, 128, 65537, 3)], chunk=65536)
    assert segs.size == 2 * 48 and chunks == [(0, 0), (1, 0), (1, 1)]
    rec = segs.view(np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("pad", "<i4")]))
    assert rec[1].tolist() == (80, 96, 112, 128, 65537, 3, 0)


def test_train_state_hyper_fields():
    assert tsf.optimizer_hyper("sgd", (0.9, 0.999), 1e-8, 0, 1e-6) == {}      # flags off: nothing is written, the dict is what it was
    on = tsf.optimizer_hyper("adamw", (0.9, 0.999), 1e-8, 4, 1e-6)
    assert on == {"optimizer": "adamw", "adam_betas": [0.9, 0.999], "adam_eps": 1e-8, "lr_warmup": 4, "lr_warmup_ratio": 1e-6}
    assert tsf.optimizer_hyper("sgd", (0.9, 0.999), 1e-8, 4, 0.5) == {"lr_warmup": 4, "lr_warmup_ratio": 0.5}
    assert tsf.optimizer_hyper("adamw", (0.9, 0.999), 1e-8, 0, 1e-6) == {"optimizer": "adamw", "adam_betas": [0.9, 0.999], "adam_eps": 1e-8}
    F = tsf.OPTIMIZER_FIELDS
    assert tsf.value_mismatches(on, {}) == []          # the default fields are the two they were
    assert tsf.value_mismatches(on, dict(on), fields=F) == [] == tsf.value_mismatches({}, {}, fields=F)
    assert tsf.value_mismatches(on, dict(on, adam_betas=(0.9, 0.999)), fields=F) == []      # a file round trip may turn a list into a tuple
    assert tsf.value_mismatches(on, {}, fields=F) == list(F)
    assert tsf.value_mismatches(on, dict(on, adam_betas=[0.9, 0.99]), fields=F) == ["adam_betas"]
    assert tsf.value_mismatches(on, dict(on, adam_eps=1e-6), fields=F) == ["adam_eps"]
    assert tsf.value_mismatches(on, dict(on, lr_warmup=5), fields=F) == ["lr_warmup"]
    assert tsf.value_mismatches(on, dict(on, lr_warmup_ratio=0.1), fields=F) == ["lr_warmup_ratio"]
    off = {k: v for k, v in on.items() if k.startswith("lr_")}
    assert tsf.value_mismatches(on, off, fields=F) == ["optimizer", "adam_betas", "adam_eps"]
