"""The optimiser kernels, element by element: simt_sgd_multi (csrc/optim.hip) and simt_adam_step / simt_adam_step_guarded (csrc/ntm.hip)
against the same recurrence in float64 on the same fp32 inputs, EVERY element, three steps.

The bound is derived, not measured.  Beside every float64 quantity x the reference carries e(x), a bound of |fp32 evaluation - x|
(`_V`: value, bound), by the standard model of a rounded operation, u = 2^-24:

    r = a (+|-|*) b:   e(r) = prop + u * (|r| + prop)
        prop(a + b) = e(a) + e(b),      prop(a * b) = |a| e(b) + |b| e(a) + e(a) e(b)
    r = a / b:         prop = (|a| e(b) + |b| e(a)) / (|b| (|b| - e(b))),    e(r) = prop + u_div * (|r| + prop)
    r = sqrt(a):       prop = e(a) / (sqrt(a - e(a)) + sqrt(a)),             e(r) = prop + u_sqrt * (|r| + prop)

so every fp32 operation adds at most u of the magnitude of its result on top of what its operands already carry.  A multiply-add contracted
to one fma rounds once instead of twice: its error is below the bound of the two operations, so the bound holds contracted or not.  The
`mult` replays of a duplicate listing and the three steps chain: the bound of step k starts from the bound of step k - 1 (the reference is
never re-synchronised with the device).  Constants (lr, weight decay, momentum, beta, 1 - beta, eps, lr / bias correction) enter as the
fp32 numbers the kernel receives, with no error of their own.

Adam's square root and division: `sqrtf` is documented at 1 ulp (HIP math API, single-precision table: u_sqrt = 2^-23), and the fp32 `/`
operator is correctly rounded (0.5 ulp: u_div = 2^-24) under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, which csrc/build.sh
leaves on.

A stored element may differ from float64 by at most TWICE its bound.  Each test prints the worst ratio |stored - float64| / bound it saw."""
import ctypes as C

import numpy as np
import pytest
import torch

from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -24
U_SQRT = 2.0 ** -23      # sqrtf: 1 ulp (HIP math API)
U_DIV = 2.0 ** -24       # operator /: correctly rounded (hipcc default)
SLACK = 2.0              # a stored element may differ from float64 by at most SLACK x its bound


class _V:
    """(float64 value, bound of |fp32 evaluation - value|)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e


def _c(x, like):
    """An fp32 constant as the kernel receives it: exact."""
    return _V(torch.full_like(like.v, float(np.float32(x))))


def _rnd(v, prop, u=U):
    return _V(v, prop + u * (v.abs() + prop))


def _add(a, b):
    return _rnd(a.v + b.v, a.e + b.e)


def _sub(a, b):
    return _rnd(a.v - b.v, a.e + b.e)


def _mul(a, b):
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def _div(a, b):
    lo = b.v.abs() - b.e
    assert bool((lo > 0).all()), "divisor not bounded away from zero"
    return _rnd(a.v / b.v, (a.v.abs() * b.e + b.v.abs() * a.e) / (b.v.abs() * lo), U_DIV)


def _sqrt(a):
    lo = (a.v - a.e).clamp_min(0.0)
    return _rnd(a.v.sqrt(), a.e / (lo.sqrt() + a.v.sqrt()).clamp_min(1e-300), U_SQRT)


def _where(m, a, b):
    return _V(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e))


def _ratio(got, ref, what):
    """Worst |got - ref.v| / ref.e; asserts it is <= SLACK and names the worst element."""
    diff = (got.double() - ref.v).abs()
    r = torch.where(ref.e > 0, diff / ref.e.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    assert not bool(torch.isnan(got).any()), f"{what}: NaN stored"
    worst = int(r.argmax())
    assert float(r[worst]) <= SLACK, (f"{what}: element {worst} is {float(got[worst])!r}, float64 {float(ref.v[worst])!r}: "
                                      f"|difference| {float(diff[worst]):.3e} = {float(r[worst]):.2f} x its bound {float(ref.e[worst]):.3e} (allowed {SLACK})")
    return float(r[worst])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# simt_sgd_multi
# ---------------------------------------------------------------------------------------------------------------------------------------------
NS = [1, 3, 4, 5, 65535, 65536, 65537, 2 * 65536 + 3]      # chunk edges (chunk = 65536 elements), float4 tails
SEGS = [(n, mult, (i + mult) & 1) for i, n in enumerate(NS) for mult in (1, 2, 3, 4)]      # (n, mult, lr group)
CHUNK = 65536


def _layout(off_bytes):
    """Element offsets of the segments inside one buffer: every segment starts `off_bytes` past a 16-byte boundary, with at least four guard
    elements before it and one after.  -> (starts, total)."""
    starts, cur = [], 0
    for (n, _m, _g) in SEGS:
        s = (cur + 3) // 4 * 4 + 4 + off_bytes // 4
        starts.append(s)
        cur = s + n + 1
    return starts, (cur + 3) // 4 * 4 + 4


class _SgdRun:
    """One set of device buffers (p, g, buf as views into three NaN-filled buffers at the given byte offsets) and the launch descriptor."""

    def __init__(self, dev, offs, p0, momentum):
        self.dev = dev
        self.lay = [_layout(o) for o in offs]
        self.bufs = [torch.full((tot,), float("nan"), device=dev) for (_s, tot) in self.lay]
        for b in self.bufs:
            assert b.data_ptr() % 16 == 0
        self.seg_mask = []
        for (starts, tot) in self.lay:
            m = torch.zeros(tot, dtype=torch.bool)
            for s, (n, _m, _g) in zip(starts, SEGS):
                m[s:s + n] = True
            self.seg_mask.append(m.to(dev))
        self.put(0, p0)
        self.put(2, torch.zeros_like(p0))
        recs = []
        for i, (n, mult, group) in enumerate(SEGS):
            ptrs = [self.bufs[k].data_ptr() + 4 * self.lay[k][0][i] for k in range(3)]
            for k in range(3):
                assert ptrs[k] % 16 == offs[k]
            recs.append((ptrs[0], ptrs[1], ptrs[2], n, mult, group))
        seg_dt = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("mult", "<i4"), ("group", "<i4")])
        self.segs = torch.from_numpy(np.array(recs, dtype=seg_dt).view(np.uint8).copy()).to(dev)
        chunks = [(si, ci) for si, r in enumerate(recs) for ci in range((r[3] + CHUNK - 1) // CHUNK)]
        self.chunks = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self.skip = torch.zeros(1, dtype=torch.int64, device=dev)
        d = L.SgdDesc()
        d.segs, d.chunks, d.nchunks, d.chunk = self.segs.data_ptr(), self.chunks.data_ptr(), len(chunks), CHUNK
        d.momentum, d.dampening = momentum, 0.0
        d.skip_if = self.skip.data_ptr()
        self.d = d

    def put(self, k, flat):
        """flat: the concatenation of every segment's values (host fp32) -> buffer k."""
        self.bufs[k][self.seg_mask[k]] = flat.to(self.dev)

    def get(self, k):
        return self.bufs[k][self.seg_mask[k]].cpu()

    def guards_intact(self):
        return all(bool(torch.isnan(b[~m]).all()) for b, m in zip(self.bufs, self.seg_mask))

    def launch(self, lr, wd, first_step):
        d = self.d
        d.lr[0], d.lr[1], d.wd[0], d.wd[1] = lr[0], lr[1], wd, wd
        d.first_step = first_step
        L.call("simt_sgd_multi", C.byref(d), ops.stream_ptr())
        torch.cuda.synchronize()


def _sgd_ref(p, buf, g, mult, lr, wd, momentum, first_step):
    """One launch of sgd_multi_kernel's `upd` in float64 with the carried bound: the `mult` listings replayed, sharing one momentum buffer."""
    if first_step:
        buf = _V(torch.zeros_like(p.v))
    for r in range(int(mult.max())):
        live = mult > r
        d = _add(g, _mul(_c(wd, p), p)) if wd != 0.0 else g
        if momentum != 0.0:
            nb = d if first_step else _add(_mul(_c(momentum, p), buf), d)      # (1 - dampening) = 1: an exact factor
            buf = _where(live, nb, buf)
            d = nb
        p = _where(live, _sub(p, _mul(_V(lr), d)), p)
    return p, buf


@pytest.mark.parametrize("offs", [(4, 8, 12), (8, 12, 4), (12, 4, 8), (4, 0, 0), (0, 12, 0), (0, 0, 8), (4, 4, 4)],
                         ids=lambda o: "p%d_g%d_buf%d" % o)
@pytest.mark.parametrize("wd,momentum", [(5e-4, 0.9), (0.0, 0.9), (5e-4, 0.0), (0.0, 0.0)])
def test_sgd_multi_every_element_vs_float64(dev, offs, wd, momentum):
    """Three launches (first_step 1, 0, 0; the learning rates of both groups, changing per step) over 32 segments (every n of NS x mult 1..4)
    whose p, g and buf start `offs` bytes past a 16-byte boundary (the scalar path of optim.hip), and the same data in 16-byte aligned buffers
    (the float4 path): every element of p and buf within twice the carried bound (module docstring) of the float64 recurrence, the aligned
    and the unaligned run bit-identical, the NaN guards around every segment intact.  Then the guard word: non-zero -> p and buf bit-identical
    to before, zero again -> they move.  Last, the red case: one element moved by 4x its own bound must fail and be named."""
    gen = torch.Generator().manual_seed(1000 + offs[0] * 64 + offs[1] * 4 + offs[2] // 4 + int(wd > 0) * 7 + int(momentum > 0) * 13)
    ntot = sum(n for n, _m, _g in SEGS)
    p0 = torch.randn(ntot, generator=gen)
    mult = torch.cat([torch.full((n,), m, dtype=torch.int64) for n, m, _g in SEGS])
    group = torch.cat([torch.full((n,), g_, dtype=torch.int64) for n, _m, g_ in SEGS])
    runs = [_SgdRun(dev, offs, p0, momentum), _SgdRun(dev, (0, 0, 0), p0, momentum)]
    p, buf = _V(p0.double()), _V(torch.zeros(ntot, dtype=F64))
    worst = 0.0
    for step in range(3):
        lrs = (0.1 * 0.7 ** step, 1.0 * 0.7 ** step)
        g = torch.randn(ntot, generator=gen)
        lr = torch.where(group == 0, torch.tensor(float(np.float32(lrs[0])), dtype=F64), torch.tensor(float(np.float32(lrs[1])), dtype=F64))
        p, buf = _sgd_ref(p, buf, _V(g.double()), mult, lr, wd, momentum, step == 0)
        for run in runs:
            run.put(1, g)
            run.launch(lrs, wd, 1 if step == 0 else 0)
            assert run.guards_intact(), f"step {step}: a guard element next to a segment was written"
        gp, gb = runs[0].get(0), runs[0].get(2)
        assert torch.equal(gp, runs[1].get(0)), f"step {step}: p differs between the unaligned (scalar) and the aligned (float4) run"
        worst = max(worst, _ratio(gp, p, f"step {step} p"))
        if momentum != 0.0:
            assert torch.equal(gb, runs[1].get(2)), f"step {step}: buf differs between the unaligned and the aligned run"
            worst = max(worst, _ratio(gb, buf, f"step {step} buf"))
        else:
            assert bool((gb == 0).all()), "momentum 0: the buffer is not touched"
    print(f"simt_sgd_multi offs {offs} wd {wd} momentum {momentum}: worst |stored - float64| / bound = {worst:.3f} (allowed {SLACK})")
    # ---- guard word
    run = runs[0]
    before = [b.clone() for b in run.bufs]
    run.skip.fill_(1)
    run.launch((0.1, 1.0), wd, 0)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, run.bufs)), "skip_if non-zero: something moved"
    run.skip.zero_()
    run.launch((0.1, 1.0), wd, 0)
    moved = run.get(0) != before[0][run.seg_mask[0]].cpu()
    assert float(moved.double().mean()) > 0.99, "skip_if zero again: p did not move"
    # ---- red: one element 4x its own bound away must fail, by name
    gp = runs[1].get(0).clone()
    idx = 65535 + 7
    gp[idx] = float(p.v[idx] + 4.0 * p.e[idx])
    with pytest.raises(AssertionError, match=f"element {idx} "):
        _ratio(gp, p, "red p")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# simt_adam_step / simt_adam_step_guarded
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _adam_ref(p, g, m, v, lr, beta1, beta2, eps, step):
    """adam_step_kernel in float64 with the carried bound, operation by operation in the kernel's order."""
    f32 = np.float32
    bc1, bc2 = 1.0 - float(f32(beta1)) ** step, 1.0 - float(f32(beta2)) ** step      # host side, in double (simt_adam_step_guarded)
    step_size, bc2s = f32(float(f32(lr)) / bc1), f32(np.sqrt(bc2))
    omb1, omb2 = f32(1.0) - f32(beta1), f32(1.0) - f32(beta2)                         # `1.f - beta`: one fp32 subtraction, reproduced exactly
    mi = _add(m, _mul(_sub(g, m), _c(omb1, p)))
    vi = _add(_mul(v, _c(beta2, p)), _mul(_mul(_c(omb2, p), g), g))
    den = _add(_div(_sqrt(vi), _c(bc2s, p)), _c(eps, p))
    pn = _sub(p, _mul(_c(step_size, p), _div(mi, den)))
    return pn, mi, vi


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("Q,Cn", [(22, 19), (25, 19), (34, 19)])
def test_adam_step_every_element_vs_float64(dev, Q, Cn, guarded):
    """Steps 1 to 3 of Adam on a Q x C transition matrix: p, m and v of every element within twice the carried bound of the float64 recurrence
    (module docstring; sqrtf 1 ulp, division correctly rounded).  guarded: through ops.adam_step (simt_adam_step_guarded) with the guard word
    0; then word 1 -> nothing moves, word 0 again -> it moves.  Unguarded: simt_adam_step.  Red: one element 4x its bound away fails."""
    gen = torch.Generator().manual_seed(Q * 100 + int(guarded))
    n = Q * Cn
    p0 = torch.randn(Q, Cn, generator=gen) * 2.0
    pd, md, vd = p0.clone().to(dev), torch.zeros(Q, Cn, device=dev), torch.zeros(Q, Cn, device=dev)
    gd = torch.zeros(Q, Cn, device=dev)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    lr, b1, b2, eps = 6e-3, 0.9, 0.999, 1e-8
    p, m, v = _V(p0.double().flatten()), _V(torch.zeros(n, dtype=F64)), _V(torch.zeros(n, dtype=F64))
    worst = 0.0

    def launch(step):
        if guarded:
            ops.adam_step(pd, gd, md, vd, lr=lr, beta1=b1, beta2=b2, eps=eps, step=step, skip_if=word)
        else:
            L.call("simt_adam_step", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lr, b1, b2, eps, step, ops.stream_ptr())
        torch.cuda.synchronize()

    for step in (1, 2, 3):
        g = torch.randn(Q, Cn, generator=gen) * 1e-2
        gd.copy_(g)
        launch(step)
        p, m, v = _adam_ref(p, _V(g.double().flatten()), m, v, lr, b1, b2, eps, step)
        for name, got, ref in (("p", pd, p), ("m", md, m), ("v", vd, v)):
            worst = max(worst, _ratio(got.cpu().flatten(), ref, f"Q{Q} step {step} {name}"))
    print(f"simt_adam_step{'_guarded' if guarded else ''} {Q} x {Cn}: worst |stored - float64| / bound = {worst:.3f} (allowed {SLACK})")
    if guarded:
        before = [t.clone() for t in (pd, md, vd)]
        word.fill_(1)
        launch(4)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, (pd, md, vd))), "guard word non-zero: moved"
        word.zero_()
        launch(4)
        assert float((pd != before[0]).double().mean()) > 0.99 and not torch.equal(md, before[1]) and not torch.equal(vd, before[2])
    red = p.v.clone().float()
    idx = n - 2
    red[idx] = float(p.v[idx] + 4.0 * p.e[idx])
    with pytest.raises(AssertionError, match=f"element {idx} "):
        _ratio(red, p, "red p")
