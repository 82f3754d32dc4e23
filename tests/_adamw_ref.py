"""simt_adamw_multi (csrc/optim.hip) restated in float64 with a carried per-element error bound, and the comparator the CPU and
the GPU tests share.  No library: plain torch in float64, on whatever device the data it is given lives on (the trainer tests keep ten
million elements on the device; the CPU tests and the kernel tests work on the host).

The bound is derived, not measured -- the method of tests/test_gpu_optim.py, restated here.  Beside every float64 quantity x the restatement
carries e(x), a bound of |fp32 evaluation - x| (`V`: value, bound), by the standard model of a rounded operation, u = 2^-24:

    r = a (+|-|*) b:   e(r) = prop + u * (|r| + prop)
        prop(a + b) = e(a) + e(b),      prop(a * b) = |a| e(b) + |b| e(a) + e(a) e(b)
    r = a / b:         prop = (|a| e(b) + |b| e(a)) / (|b| (|b| - e(b))),    e(r) = prop + u_div * (|r| + prop)
    r = sqrt(a):       prop = e(a) / (sqrt(a - e(a)) + sqrt(a)),             e(r) = prop + u_sqrt * (|r| + prop)
                       (and never more than sqrt(e(a)): |sqrt(x) - sqrt(y)| <= sqrt(|x - y|), which is the bound where a is zero)

Every fp32 operation adds at most u of the magnitude of its result on top of what its operands carry.  A product or a quotient may also
land among the subnormals (the second moment of a gradient of 1e-21 is 1e-42), where the spacing is 2^-149 whatever the magnitude: such a
result carries up to eta = 2^-150 more (gradual underflow, the standard model's fl(x) = x (1 + d) + eta; sums and differences of fp32 numbers
are exact down there, and sqrt does not underflow), so every product and quotient adds eta.  A multiply-add contracted to one fma
rounds once instead of twice: its error is below the bound of the two operations, so the bound holds contracted or not.  `sqrtf` is
documented at 1 ulp (u_sqrt = 2^-23), the fp32 `/` operator is correctly rounded (u_div = 2^-24; hipcc's default, which the build leaves on).
Constants (step_size, decay, beta2, 1 - beta1, 1 - beta2, sqrt(1 - beta2^t), eps) enter as the fp32 numbers the kernel receives, with no
error of their own.  Steps chain: the bound of step k starts from the bound of step k - 1, the restatement is never re-synchronised with the
evaluation it judges.  A stored element may differ from float64 by at most SLACK = 2 times its bound.

Per element, in torch.optim.AdamW's single-tensor order (group g of the element's tensor):

    p = p * decay[g]                       decoupled weight decay
    m = m + (grad - m) * omb1              first step: m = grad * omb1
    v = v * beta2 + omb2 * grad * grad     first step: v = omb2 * grad * grad
    den = sqrtf(v) / bc2s + eps
    p = p - step_size[g] * (m / den)
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
U_SQRT = 2.0 ** -23      # sqrtf: 1 ulp
U_DIV = 2.0 ** -24       # operator /: correctly rounded
ETA = 2.0 ** -150        # a product or a quotient that underflows: half the spacing of the subnormals
SLACK = 2.0              # a stored element may differ from float64 by at most SLACK x its bound


class V:
    """(float64 value, bound of |fp32 evaluation - value|)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e


def exact(x):
    """fp32 data as the kernel reads it: exact.  Stays on x's device."""
    return V(torch.as_tensor(x).detach().double().flatten())


def const(x, like):
    """One fp32 constant (or a per-element tensor of them, already float64 of fp32 numbers) as the kernel receives it: exact."""
    if torch.is_tensor(x):
        return V(x.double())
    return V(torch.full_like(like.v, float(np.float32(x))))


def _rnd(v, prop, u=U, eta=0.0):
    return V(v, prop + u * (v.abs() + prop) + eta)


def add(a, b):
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e, eta=ETA)


def div(a, b):
    lo = b.v.abs() - b.e
    assert bool((lo > 0).all()), "divisor not bounded away from zero"
    return _rnd(a.v / b.v, (a.v.abs() * b.e + b.v.abs() * a.e) / (b.v.abs() * lo), U_DIV, eta=ETA)


def sqrt(a):
    lo = (a.v - a.e).clamp_min(0.0)
    prop = torch.minimum(a.e / (lo.sqrt() + a.v.sqrt()).clamp_min(1e-300), a.e.sqrt())      # (at a = 0, a gradient of zero: the second form)
    return _rnd(a.v.sqrt(), prop, U_SQRT)


def constants(lrs, wds, betas, t):
    """The fp32 constants of the launch at step t >= 1 as the contract states them: formed in float64, rounded once.  The betas are the fp32
    numbers the kernel multiplies by.  -> dict(step_size=[...], decay=[...], beta1, beta2, omb1, omb2, bc2s) of np.float32."""
    f32 = np.float32
    b1, b2 = float(f32(betas[0])), float(f32(betas[1]))
    return dict(step_size=[f32(float(lr) / (1.0 - b1 ** t)) for lr in lrs],
                decay=[f32(1.0 - float(lr) * float(wd)) for lr, wd in zip(lrs, wds)],
                beta1=f32(b1), beta2=f32(b2), omb1=f32(1.0 - b1), omb2=f32(1.0 - b2), bc2s=f32(math.sqrt(1.0 - b2 ** t)))


def per_element(values, group):
    """The per-group fp32 constants `values` spread over the elements: float64 tensor, values[group[i]]."""
    return torch.tensor([float(x) for x in values], dtype=F64, device=group.device)[group]


def adamw_ref(p, g, m, v, step_size, decay, beta2, omb1, omb2, bc2s, eps, first_step):
    """One launch in float64 with the carried bound, operation by operation in the kernel's order.  p, g, m, v: V; step_size and decay: scalars
    or per-element float64 tensors (per_element); the rest scalars.  first_step: m and v are not read.  -> (p, m, v)."""
    p1 = mul(p, const(decay, p))
    gg = mul(mul(const(omb2, p), g), g)
    if first_step:
        mi = mul(g, const(omb1, p))
        vi = gg
    else:
        mi = add(m, mul(sub(g, m), const(omb1, p)))
        vi = add(mul(v, const(beta2, p)), gg)
    den = add(div(sqrt(vi), const(bc2s, p)), const(eps, p))
    pn = sub(p1, mul(const(step_size, p), div(mi, den)))
    return pn, mi, vi


def adamw_f32(p, g, m, v, step_size, decay, beta2, omb1, omb2, bc2s, eps, first_step):
    """The same recurrence evaluated in fp32 with numpy, every operation rounded (no fma).  Arrays of np.float32; step_size / decay arrays or
    scalars.  -> (p, m, v)."""
    f = np.float32
    step_size, decay = np.asarray(step_size, dtype=f), np.asarray(decay, dtype=f)
    p = p * decay
    if first_step:
        m = g * f(omb1)
        v = f(omb2) * g * g
    else:
        m = m + (g - m) * f(omb1)
        v = v * f(beta2) + f(omb2) * g * g
    den = np.sqrt(v) / f(bc2s) + f(eps)
    p = p - step_size * (m / den)
    assert p.dtype == f and m.dtype == f and v.dtype == f
    return p, m, v


def ratio(got, ref, what):
    """Worst |got - ref.v| / ref.e over the elements; AssertionError naming the worst element when it is above SLACK (or a NaN is stored)."""
    got = torch.as_tensor(got).detach().to(ref.v.device).flatten()
    assert not bool(torch.isnan(got).any()), f"{what}: NaN stored"
    diff = (got.double() - ref.v).abs()
    r = torch.where(ref.e > 0, diff / ref.e.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    worst = int(r.argmax())
    assert float(r[worst]) <= SLACK, (f"{what}: element {worst} is {float(got[worst])!r}, float64 {float(ref.v[worst])!r}: "
                                      f"|difference| {float(diff[worst]):.3e} = {float(r[worst]):.2f} x its bound {float(ref.e[worst]):.3e} (allowed {SLACK})")
    return float(r[worst])
