"""Scale-aware, per-element bar for the gradients of the fused SimT head (simt_head_grad), and the references it is measured against.

`close(a, b, tol)` of the head tests asserts max|a - b| <= tol * (1 + max|b|): for the head's gradients, whose entries shrink like
1 / (B H W), that is an ABSOLUTE bar of `tol` -- at 4 x 768 x 768 nine times the rms of the auxiliary head's gradient.  Here every element of a
gradient tensor g is held against the float64 oracle on its own scale:

    s = |ref64| + rms(ref64)            (an element is a sum of >= 64 pixel terms of either sign: its error scales with rms, not with |ref64| alone)
    e = |g - ref64| / s
    tau = max(4 * q99.9(|ref32 - ref64| / s), 16 * 2^-24)

ref32 is the SAME oracle in fp32 on the same inputs: tau is measured from the references at each geometry, never from the kernel.  The
factor 4 covers the kernel's different summation order over the pixels under a low-res element and its exp2-based exp.

Discrete decisions (confidence thresholds, arg-maxes) may fall differently in fp32 and float64 on a few pixels; each flip moves the low-res
elements under that pixel by 1e-3 .. 1e-1 of s.  The elements where the references themselves disagree (|ref32 - ref64| / s > tau) are the
EXCLUSION set; the kernel may decide a different handful of pixels (GPU-only outliers).  Both are allowed only while
  1. exclusions + outliers are at most CAP = 0.1 % of the tensor, and
  2. each of them still meets the old absolute bar 1e-5 * (1 + max|ref64|)
(3., the per-pixel confidence map equal to the fp32 oracle's, is asserted by the callers).  Every other element must have e <= tau.

bf16 outputs (dpred*_t with grad_dtype = SIMT_BF16), against gscale * ref64:
  * every element outside the allowed set within ONE bf16 ulp (ulp_bf16 of tests/_launch_oracle.py).  The allowed set is the exclusion set
    plus the outliers of the fp32 output OF THE SAME LAUNCH; without that companion nothing but the exclusion set is excused (a bf16 value
    cannot show by itself that a pixel was decided differently).  The ulp is floored at the ulp of max(2^-6, 512 tau) * rms: an fp32 value
    within tau * s of ref64 rounds to within ulp / 2 + tau * s, which is <= one ulp once ulp >= 2 tau rms, i.e. |x| >= 2^8 * 2 tau rms;
  * the share exactly equal to bf16(gscale * ref64) at least the references' own share (bf16(ref32) == bf16(ref64), same elements) minus
    0.5 percentage points (round-to-nearest ties decided by the last fp32 bits);
  * bit for bit the round-to-nearest-even of the fp32 output where the launch wrote both.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _launch_oracle import ulp_bf16
from oracle import simt_oracle as so

BF = torch.bfloat16
F64 = torch.float64
TAU_FLOOR = 16.0 * 2.0 ** -24
CAP = 1e-3                    # exclusions + GPU-only outliers, share of the tensor's elements
OLD_TOL = 1e-5                # the absolute bar every excused element still meets
EXACT_MARGIN = 0.005


def old_close_ok(a, b, tol):
    """The comparison `close` of tests/test_gpu_head_ntm.py / test_gpu_single.py asserts, as a predicate."""
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return (a - b).abs().max().item() <= tol * (1 + b.abs().max().item())


def _d(t):
    t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    return t.detach().double().cpu()


def _quantile(x, q):
    v = x.reshape(-1).sort().values
    return v[min(v.numel() - 1, int(q * (v.numel() - 1) + 0.5))].item()      # nearest rank (torch.quantile caps the size)


def measure(ref64, ref32):
    """-> dict(s, tau, q, excl): per-element scale, threshold, the references' 99.9 % quantile and the exclusion set."""
    r64, r32 = _d(ref64), _d(ref32)
    assert r64.shape == r32.shape
    rms = r64.pow(2).mean().sqrt().item()
    assert rms > 0, "an all-zero reference cannot set a scale"
    s = r64.abs() + rms
    dref = (r32 - r64).abs() / s
    q = _quantile(dref, 0.999)
    tau = max(4.0 * q, TAU_FLOOR)
    return {"s": s, "tau": tau, "q": q, "excl": dref > tau, "rms": rms, "r64": r64, "r32": r32}


def _nan_inf(e):
    return torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)


def _degenerate(g, r64, r32, what):
    """References with NaNs (a loss over zero pixels) or all zero: the NaN pattern / the zeros must be reproduced exactly.
    -> (g, r64, r32) with the NaNs removed, or None when there is nothing left to scale."""
    nan = torch.isnan(r64)
    if bool(nan.any()):
        assert torch.equal(torch.isnan(g), nan) and torch.equal(torch.isnan(r32), nan), f"{what}: NaN pattern differs"
        g, r64, r32 = torch.nan_to_num(g), torch.nan_to_num(r64), torch.nan_to_num(r32)
    if not bool((r64 != 0).any()):
        assert not bool((g != 0).any()), f"{what}: the reference is all zero, the output is not"
        return None
    return g, r64, r32


def grad_bar(got, ref64, ref32, what, gscale=1.0):
    """fp32 gradient `got` (same shape as the references) against gscale * ref64.  AssertionError on a violation, else
    dict(worst: max e / tau over the held elements, worst_any: over all elements, outliers: GPU-only outliers, excluded, tau, q, n, out)."""
    g = _d(got)
    assert g.shape == ref64.shape, (what, g.shape, ref64.shape)
    dg = _degenerate(g, _d(ref64) * gscale, _d(ref32) * gscale, what)
    if dg is None:
        z = torch.zeros_like(g, dtype=torch.bool)
        return {"worst": 0.0, "worst_any": 0.0, "outliers": 0, "excluded": 0, "tau": TAU_FLOOR, "q": 0.0, "n": g.numel(), "out": z, "excl": z}
    g = dg[0]
    m = measure(dg[1], dg[2])
    err = _nan_inf((g - m["r64"]).abs())
    e = err / m["s"]
    out = (e > m["tau"]) & ~m["excl"]
    nex, nout, n = int(m["excl"].sum()), int(out.sum()), g.numel()
    held = ~(out | m["excl"])
    res = {"worst": (e[held].max().item() if bool(held.any()) else 0.0) / m["tau"], "worst_any": e.max().item() / m["tau"],
           "outliers": nout, "excluded": nex, "tau": m["tau"], "q": m["q"], "n": n, "out": out, "excl": m["excl"]}
    first = out.nonzero()[0].tolist() if nout else None
    assert nex + nout <= CAP * n, (f"{what}: {nout} elements beyond tau = {m['tau']:.3e} (worst {res['worst_any']:.1f} x tau, first at {first}) + "
                                   f"{nex} where the references disagree = {(nex + nout) / n:.4%} of {n}, cap {CAP:.1%}")
    old = OLD_TOL * (1 + m["r64"].abs().max().item())
    loose = (out | m["excl"]) & (err > old)
    assert not bool(loose.any()), (f"{what}: {int(loose.sum())} excused elements miss the old absolute bar {old:.3e} "
                                   f"(first at {loose.nonzero()[0].tolist()}, err {err[loose].max().item():.3e})")
    return res


def bf16_bar(got_bf16, ref64, ref32, what, gscale=1.0, got_f32=None):
    """bf16 gradient against gscale * ref64 (see the module docstring).  got_f32: the fp32 output of the same launch (same shape) or None.
    -> dict(exact, exact_ref, worst_ulps, allowed, tau)."""
    assert got_bf16.dtype == BF
    m = measure(_d(ref64) * gscale, _d(ref32) * gscale)
    gb = got_bf16.detach().cpu()
    assert gb.shape == m["r64"].shape, (what, gb.shape, m["r64"].shape)
    allowed = m["excl"].clone()
    if got_f32 is not None:
        g32 = got_f32.detach().float().cpu()
        same = gb.view(torch.int16) == g32.to(BF).view(torch.int16)
        same |= (gb == 0) & (g32.to(BF) == 0)
        assert bool(same.all()), (f"{what}: {int((~same).sum())} bf16 elements are not the round-to-nearest of the fp32 output "
                                  f"(first at {(~same).nonzero()[0].tolist()})")
        allowed |= grad_bar(g32, ref64, ref32, what + " (fp32 companion)", gscale)["out"]
    n = gb.numel()
    assert int(allowed.sum()) <= CAP * n, f"{what}: {int(allowed.sum())} excused elements of {n}, cap {CAP:.1%}"
    err = _nan_inf((gb.double() - m["r64"]).abs())
    ulp = ulp_bf16(m["r64"], max(2.0 ** -6, 512.0 * m["tau"]) * m["rms"])
    ulps = err / ulp
    bad = (ulps > 1.0) & ~allowed
    worst = ulps[~allowed].max().item()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {n} bf16 elements more than one ulp from the float64 gradient (worst {worst:.2f} ulps, "
                                 f"first at {bad.nonzero()[0].tolist()})")
    old = OLD_TOL * (1 + m["r64"].abs().max().item()) + ulp
    loose = allowed & (err > old)
    assert not bool(loose.any()), f"{what}: {int(loose.sum())} excused bf16 elements miss the old absolute bar + one ulp"
    keep = ~allowed
    want = m["r64"].float().to(BF)
    exact = (gb == want)[keep].double().mean().item()
    exact_ref = (m["r32"].float().to(BF) == want)[keep].double().mean().item()
    assert exact >= exact_ref - EXACT_MARGIN, (f"{what}: {exact:.5f} of the elements equal bf16(float64 gradient); the fp32 oracle reaches "
                                               f"{exact_ref:.5f} (margin {EXACT_MARGIN})")
    return {"exact": exact, "exact_ref": exact_ref, "worst_ulps": worst, "allowed": int(allowed.sum()), "tau": m["tau"]}


def report(tag, what, r):
    """One line per tensor for the log (pytest -s) and profiles/head_gradient_bar.txt."""
    if "exact" in r:
        print(f"[head-bar] {tag} {what}: bf16 exact {r['exact']:.5f} (references {r['exact_ref']:.5f}), worst {r['worst_ulps']:.3f} ulp, "
              f"{r['allowed']} excused", flush=True)
    else:
        print(f"[head-bar] {tag} {what}: tau {r['tau']:.3e} (q99.9 {r['q']:.3e}), references' outliers {r['excluded']}, worst e/tau "
              f"{r['worst']:.3f} (any element {r['worst_any']:.2f}), GPU-only outliers {r['outliers']} of {r['n']}", flush=True)


def trainer_form(tag, what, f32_raw, dt_raw, back, Q, QP, ref64, ref32, gscale):
    """One head's outputs of a launch in the form the trainers ask for: f32_raw [M, ld_f32] fp32 and dt_raw [M, ld_t] bf16 (pre-filled with
    SENTINEL), both written by the SAME simt_head_grad; back: raw -> [B, Q, h, w].  The fp32 bar, the bf16 bar (bit-for-bit rounding of the
    fp32 output included), and the pitch columns: [Q, QP) zero, [QP, ld_t) untouched (include/simt_hip.h simt_head_desc.dpred1_t)."""
    from _launch_oracle import SENTINEL
    assert dt_raw.dtype == BF and dt_raw.shape[1] >= QP
    assert bool((dt_raw[:, QP:] == SENTINEL).all()), f"{tag} {what}: pad columns [QP, ld_t) of the bf16 gradient were written"
    assert bool((dt_raw[:, Q:QP] == 0).all()) and bool((f32_raw[:, Q:QP] == 0).all()), f"{tag} {what}: columns [Q, QP) are not zero"
    r32 = grad_bar(back(f32_raw), ref64, ref32, f"{tag} {what} fp32", gscale)
    report(tag, f"{what} fp32 gscale {gscale}", r32)
    rb = bf16_bar(back(dt_raw), ref64, ref32, f"{tag} {what} bf16", gscale, got_f32=back(f32_raw))
    report(tag, f"{what} bf16 gscale {gscale} ld_t {dt_raw.shape[1]}", rb)
    return r32, rb


def half_is_bitwise(tag, what, f32_half, f32_one):
    """gscale enters simt_head_grad once, in the per-term factors gscale * lambda / N (csrc/head_loss.hip): a power of two scales every
    product and sum exactly, so the fp32 output at gscale = 0.5 is 0.5 x the output at gscale = 1 bit for bit."""
    same = (f32_half == 0.5 * f32_one)
    assert bool(same.all()), f"{tag} {what}: {int((~same).sum())} elements at gscale = 0.5 are not half the gscale = 1 output (first at {(~same).nonzero()[0].tolist()})"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the references: oracle/simt_oracle.py in float64 and in fp32 on the same inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def hyper(d, K, Cn=19):
    return so.Hyper(num_classes=Cn, open_classes=K, th_high=float(d["th"][0]), th_low=float(d["th"][1]), lambda_seg=float(d["lambda_seg"]),
                    lambda_place=float(d["lambda_place"]), lambda_convex=float(d["lam"][0]), lambda_volume=float(d["lam"][1]),
                    lambda_anchor=float(d["lam"][2]))


DEFAULT_D = {"lam": np.array([0.5, 0.1, 0.5]), "lr_T": 6e-3, "th": np.array([0.8, 0.2]), "lambda_seg": 0.1, "lambda_place": 0.1}


def two_head_ref(p1, p2, f2, lab, ntm, d, cd, dtype, total_of=None):
    """tests/test_gpu_head_ntm.py's oracle run (inner W loop, simt_losses, backward) in `dtype`: logits, NTMs, W and the class prior cast.
    total_of(out, hp): the scalar to differentiate instead of out["total"] (the mutants of tests/test_head_bar_cpu.py).
    -> dict(dpred1, dpred2, ntm_grad1, ntm_grad2, out; w, m, v: sig_W's raw weights and their Adam moments after the inner loop, two each)."""
    K = int(d["K"]); Cn = cd.numel(); Q = Cn + K
    H, W = lab.shape[1:]
    hp = hyper(d, K, Cn)
    cdt = cd.to(dtype)
    n = [x.to(dtype).clone().requires_grad_(True) for x in ntm]
    wr = [so.w_init(Cn, K).to(dtype).requires_grad_(True) for _ in range(2)]
    z = lambda: torch.zeros(Q, Q, dtype=dtype)
    state = {"step": 0, "m1": z(), "v1": z(), "m2": z(), "v2": z()}
    so.inner_w_loop(n[0], n[1], wr[0], wr[1], state, cdt, hp, float(d["lr_T"]))
    q1, q2 = p1.to(dtype).clone().requires_grad_(True), p2.to(dtype).clone().requires_grad_(True)
    T1, T2 = so.sig_ntm_forward(n[0], cdt, Cn), so.sig_ntm_forward(n[1], cdt, Cn)
    out = so.simt_losses(q1, q2, f2.to(dtype), lab, T1, T2, so.sig_w_forward(wr[0]), so.sig_w_forward(wr[1]), hp, (H, W))
    (out["total"] if total_of is None else total_of(out, hp)).backward()
    return {"dpred1": q1.grad, "dpred2": q2.grad, "ntm_grad1": n[0].grad, "ntm_grad2": n[1].grad,
            "out": {k: v.detach() for k, v in out.items()}, "w": [x.detach() for x in wr], "m": [state["m1"], state["m2"]],
            "v": [state["v1"], state["v2"]]}


def single_ref(pred, fix, lab, ntm, K, half, cd, dtype, d=DEFAULT_D):
    """tests/test_gpu_single.py's oracle run for the one-output models in `dtype`.  half: DeepLabv3 (half-pixel upsample, softmax after the
    upsample); else DeepLab-VGG16 (align_corners=True, softmax before).  -> dict(dpred2, ntm_grad2, out; w, m, v: sig_W's raw weight and its
    Adam moments after the inner loop)."""
    Cn = cd.numel(); Q = Cn + K
    H, W = lab.shape[1:]
    hp = hyper(dict(d, K=K), K, Cn)
    cdt = cd.to(dtype)
    n = ntm.to(dtype).clone().requires_grad_(True)
    wr = so.w_init(Cn, K).to(dtype).requires_grad_(True)
    state = {"step": 0, "m": torch.zeros(Q, Q, dtype=dtype), "v": torch.zeros(Q, Q, dtype=dtype)}
    so.inner_w_loop_single(n, wr, state, cdt, hp, float(d["lr_T"]))
    q = pred.to(dtype).clone().requires_grad_(True)
    fx = fix.to(dtype)
    Tm = so.sig_ntm_forward(n, cdt, Cn)
    if half:
        up, prob = F.interpolate(q, size=(H, W), mode="bilinear"), torch.softmax(F.interpolate(fx, size=(H, W), mode="bilinear"), 1)
    else:
        up, prob = so.upsample(q, (H, W)), so.upsample(torch.softmax(fx, 1), (H, W))
    out = so.simt_losses_single(up, prob, lab, Tm, so.sig_w_forward(wr), hp)
    out["total"].backward()
    return {"dpred2": q.grad, "ntm_grad2": n.grad, "out": {k: v.detach() for k, v in out.items()}, "w": wr.detach(), "m": state["m"], "v": state["v"]}


def warmup_ref(pred1, pred2, lab, lambda_seg, half, dtype):
    """The warm-up stage's loss (mode = 1) in `dtype`: CE(up(pred2)) + lambda_seg * CE(up(pred1)), ignore 255 and every label outside [0, C)
    (the kernel skips and counts those).  pred1 None: the one-output models.  -> dict(dpred1 or None, dpred2, total, l1, l2)."""
    H, W = lab.shape[1:]
    Cn = pred2.shape[1]
    rl = lab.clone()
    rl[(rl >= Cn) | (rl < 0)] = 255
    up = (lambda x: F.interpolate(x, size=(H, W), mode="bilinear")) if half else (lambda x: so.upsample(x, (H, W)))
    q2 = pred2.to(dtype).clone().requires_grad_(True)
    l2 = F.cross_entropy(up(q2), rl, ignore_index=255)
    q1, l1 = None, None
    total = l2
    if pred1 is not None:
        q1 = pred1.to(dtype).clone().requires_grad_(True)
        l1 = F.cross_entropy(up(q1), rl, ignore_index=255)
        total = l2 + lambda_seg * l1
    total.backward()
    return {"dpred1": None if q1 is None else q1.grad, "dpred2": q2.grad, "total": total.detach(), "l1": None if l1 is None else l1.detach(),
            "l2": l2.detach()}


_CACHE = {}


def cached(key, fn):
    """Module-level cache of reference runs: the float64 oracle at 4 x 768 x 768 costs ~15 s, and several parametrizations share one."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def ref_pair(key, fn):
    """(ref64, ref32) of fn(dtype), cached under key."""
    return cached(key, lambda: (fn(F64), fn(torch.float32)))


def head_inputs(geom, K, cd, block=8, Cn=19):
    """The inputs of test_head_bigger_than_one_block_vs_oracle (block=8) / test_head_production_size_vs_oracle (block=16) at
    geom = (B, h, w, H, W): seed 5 for the logits, seed 11 for the labels.  -> (pred1, pred2, fixed2, label, [ntm1, ntm2])."""
    B, h, w, H, W = geom
    Q = Cn + K
    g = torch.Generator().manual_seed(5)
    p1 = torch.randn(B, Q, h, w, generator=g) * 3
    p2 = torch.randn(B, Q, h, w, generator=g) * 3
    f2 = torch.randn(B, Cn, h, w, generator=g) * 4
    _, lab = so.synthetic_batch(B, H, W, cd.numpy(), seed=11, block=block)
    return p1, p2, f2, lab, [so.ntm_init(Cn, K, 1), so.ntm_init(Cn, K, 2)]
