"""References and the per-element bar for the NTM micro-solver (csrc/ntm.hip: simt_ntm_inner_loop, simt_ntm_post, simt_sig_ntm, simt_sig_w).

`close(a, b, tol)` asserts max|a - b| <= tol * (1 + max|b|).  sig_W keeps its diagonal at -1e4, so for W that is an ABSOLUTE bar of 0.1 at
tol = 1e-5 -- the off-diagonal entries start at 1 / (Q - 1) = 0.048 and ten Adam steps move them by at most 0.061: a kernel that never
updated W passes.  exp_avg_sq (largest entry 3e-6) under an absolute 1e-5 is just as free.  Here every element of a tensor g is held against
the float64 oracle on its own scale, like tests/_head_bar.py:

    s = |ref64| + rms(ref64)
    e = |g - ref64| / s
    tau = max(4 * max(|ref32 - ref64| / s), 16 * 2^-24)

ref32 is the SAME reference (oracle/simt_oracle.py) in fp32 on the same inputs: tau comes from the references, never from the kernel.  The
factor 4 covers a different summation order and expf.  NO exclusions and no outliers: these kernels take no per-pixel decisions; their only
discrete choices are the Gauss-Jordan pivot row and the volume guard, and the inputs pin both (tests/test_ntm_ref_cpu.py).

W: the bar holds the off-diagonal entries (rms over them); the diagonal must be exactly what the reference leaves there (-1e4 once a step or
a forward ran).  The diagonals of the Adam moments must equal the reference's exactly (zero when they start at zero: the softmax of -1e4
is exactly 0 in fp32 and in float64, so the diagonal's gradient is).
"""
import contextlib
import functools
import math

import numpy as np
import torch

from oracle import simt_oracle as so

F64 = torch.float64
F32 = torch.float32
TAU_FLOOR = 16.0 * 2.0 ** -24
SCALAR_TOL = 1e-4            # the project's bar for the loss scalars ("loss within 1e-4 fp32")
QMAXH = 40                   # pitch of the `ex` rows in hout (csrc/head_loss.hip QMAX)
REAL_CD = so.load_class_dist()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the bar
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _d(t):
    t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    return t.detach().double().cpu()


def bar(got, ref64, ref32, what, mask=None, golden=None):
    """Every element of `got` (under `mask`, if given) within tau of ref64 on its own scale.  AssertionError on a violation (a NaN / Inf in
    `got` is one), else dict(tau, worst: max e / tau, ref: max |ref32 - ref64| / s, n).
    golden: hold `got` to this fp32 vector of the reference implementation instead, on the same scale s, within 2 tau (it carries an fp32
    error of its own)."""
    g, r64, r32 = _d(got), _d(ref64), _d(ref32)
    assert g.shape == r64.shape == r32.shape, (what, g.shape, r64.shape, r32.shape)
    c = r64 if golden is None else _d(golden)
    assert c.shape == r64.shape
    if mask is not None:
        g, r64, r32, c = g[mask], r64[mask], r32[mask], c[mask]
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{what}: the references are not finite"
    rms = r64.pow(2).mean().sqrt().item() if r64.numel() else 0.0
    if rms == 0.0:             # nothing to set a scale: the zeros must be reproduced exactly (moments that never moved)
        assert not bool((r32 != 0).any()) and not bool((g != 0).any()), f"{what}: the reference is all zero, the output is not"
        return {"tau": TAU_FLOOR, "worst": 0.0, "ref": 0.0, "n": g.numel()}
    s = r64.abs() + rms
    ref = ((r32 - r64).abs() / s).max().item()
    tau = max(4.0 * ref, TAU_FLOOR) * (1.0 if golden is None else 2.0)
    e = (g - c).abs() / s
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    worst = e.max().item()
    assert worst <= tau, (f"{what}: {int((e > tau).sum())} of {e.numel()} elements beyond tau = {tau:.3e} (worst e / tau = {worst / tau:.2f} at flat index "
                          f"{int(e.argmax())}: got {g.flatten()[int(e.argmax())].item():.9e}, expected {c.flatten()[int(e.argmax())].item():.9e})")
    return {"tau": tau, "worst": worst / tau, "ref": ref, "n": g.numel()}


def offdiag(q):
    return ~torch.eye(q, dtype=torch.bool)


def square_bar(got, ref64, ref32, what, golden=None):
    """A Q x Q tensor of sig_W (the raw weight or one of its Adam moments): off-diagonal entries under the bar, the diagonal exactly the
    references' (-1e4 for the weight once a step ran, 0 for moments that started at 0)."""
    g, r64, r32 = _d(got), _d(ref64), _d(ref32)
    assert golden is None or torch.equal(_d(golden).diagonal(), r64.diagonal()), f"{what}: the golden diagonal is not the references'"
    q = g.shape[0]
    dg, d64, d32 = g.diagonal(), r64.diagonal(), r32.diagonal()
    assert torch.equal(d64, d32), f"{what}: the references disagree on the diagonal"
    assert torch.equal(dg, d64), f"{what}: diagonal {dg.tolist()} is not the reference's {d64.tolist()}"
    if q < 2:
        return {"tau": TAU_FLOOR, "worst": 0.0, "ref": 0.0, "n": 0}
    return bar(g, r64, r32, what, mask=offdiag(q), golden=golden)


def report(tag, what, r):
    """One line per tensor for the log (pytest -s) and profiles/ntm_solver_bar.txt."""
    print(f"[ntm-bar] {tag} {what}: tau {r['tau']:.3e} (references {r['ref']:.3e}), worst e/tau {r['worst']:.3f} of {r['n']}", flush=True)


def old_close_ok(a, b, tol):
    """`close` of tests/test_gpu_head_ntm.py / test_gpu_single.py, as a predicate."""
    a, b = _d(a), _d(b)
    return (a - b).abs().max().item() <= tol * (1 + b.abs().max().item())


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def scalars_close(got, ref64, idx, what, tol=SCALAR_TOL):
    """lout slots `idx` within tol * (1 + |ref64|): the existing bar of the loss scalars."""
    g, r = _d(got), _d(ref64)
    for i in idx:
        assert math.isfinite(g[i].item()) and abs(g[i].item() - r[i].item()) <= tol * (1 + abs(r[i].item())), \
            f"{what}: lout[{i}] = {g[i].item():.9e}, float64 {r[i].item():.9e}"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def prior(C, kind="real", seed=0):
    """real: the Cityscapes prior (C = 19 only); softmax: a softmax of randn; zero: the same with one entry exactly 0 (renormalised)."""
    if kind == "real":
        assert C == REAL_CD.numel()
        return REAL_CD.float().clone()
    g = torch.Generator().manual_seed(1000 + 10 * C + seed)
    p = torch.softmax(torch.randn(C, generator=g, dtype=F64), 0)
    if kind == "zero":
        p[C // 2] = 0.0
        p = p / p.sum()
    else:
        assert kind == "softmax"
    return p.float()


def state(Q, C, kind, seed=0):
    """-> dict(ntm, w, m, v: lists of two fp32 tensors, ntm_grad: the non-zero gradient NTM.grad already holds).
    init: ntm_init / w_init / zero moments.  trained: ntm = randn * 3, w = randn (diagonal included: whatever a checkpoint holds), m ~ 1e-3,
    v ~ 1e-6, zero moment diagonals.  saturated: trained, with blocks of ntm at +-30 (sigmoid' = 0 in fp32)."""
    g = torch.Generator().manual_seed(7000 + 100 * Q + C + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    K = Q - C
    if kind == "init":
        ntm = [so.ntm_init(C, K, 1 + seed), so.ntm_init(C, K, 2 + seed)]
        w = [so.w_init(C, K) for _ in range(2)]
        m = [torch.zeros(Q, Q) for _ in range(2)]
        v = [torch.zeros(Q, Q) for _ in range(2)]
    else:
        assert kind in ("trained", "saturated")
        ntm = [rn(Q, C) * 3 for _ in range(2)]
        w = [rn(Q, Q) for _ in range(2)]
        od = offdiag(Q).float()
        m = [rn(Q, Q) * 1e-3 * od for _ in range(2)]
        v = [rn(Q, Q).abs() * 1e-6 * od for _ in range(2)]
        if kind == "saturated":
            for k in range(2):
                ntm[k][: (Q + 1) // 2, : (C + 1) // 2] = 30.0 if k == 0 else -30.0
                ntm[k][Q // 2 + 1:, C // 2 + 1:] = -30.0 if k == 0 else 30.0
    return {"ntm": ntm, "w": w, "m": m, "v": v, "ntm_grad": [rn(Q, C) * 1e-2 for _ in range(2)]}


def synthetic_hout(Q, C, ex="all", seed=0, floats=None):
    """A result block of simt_head_loss without a head launch, in ntm_post_kernel's layout: 16 scalars; A[k] at 16 + k Q C; ex[k] at
    16 + 2 Q C + 40 k; dTy[k] at 16 + 2 Q C + 4 * 40 + k Q C.  ex: all / none / mixed rows exist.  floats: simt_head_hout_floats(Q, C) (the
    rest stays zero).  -> fp32 [floats]"""
    g = torch.Generator().manual_seed(9000 + 100 * Q + C + seed)
    n = 16 + 4 * Q * C + 4 * QMAXH
    h = torch.zeros(n if floats is None else floats)
    assert h.numel() >= n
    h[:16] = torch.rand(16, generator=g) * 3 + 0.1             # loss terms of the head; [15] the count of out-of-range labels
    h[6], h[15] = 1234.0, 3.0
    for k in range(2):
        h[16 + k * Q * C: 16 + (k + 1) * Q * C] = torch.softmax(torch.randn(Q, C, generator=g) * 2, 1).flatten()
        e = {"all": torch.ones(Q), "none": torch.zeros(Q), "mixed": (torch.rand(Q, generator=g) < 0.5).float()}[ex]
        if ex == "mixed":
            e[0], e[Q - 1] = (1.0, 0.0) if k == 0 else (0.0, 1.0)
        h[16 + 2 * Q * C + k * QMAXH: 16 + 2 * Q * C + k * QMAXH + Q] = e
        o = 16 + 2 * Q * C + 4 * QMAXH + k * Q * C
        h[o: o + Q * C] = torch.randn(Q * C, generator=g) * 0.3
    return h


def hout_parts(hout, Q, C):
    """-> (scalars [16], A [2][Q, C], ex [2][Q] bool, dTy [2][Q, C])"""
    qc = Q * C
    A = [hout[16 + k * qc: 16 + (k + 1) * qc].view(Q, C) for k in range(2)]
    ex = [hout[16 + 2 * qc + k * QMAXH: 16 + 2 * qc + k * QMAXH + Q] != 0 for k in range(2)]
    o = 16 + 2 * qc + 4 * QMAXH
    dTy = [hout[o + k * qc: o + (k + 1) * qc].view(Q, C) for k in range(2)]
    return hout[:16], A, ex, dTy


# ---------------------------------------------------------------------------------------------------------------------------------------------
# references: oracle/simt_oracle.py in `dtype`
# ---------------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _patched(**kw):
    old = {k: getattr(so, k) for k in kw}
    try:
        for k, f in kw.items():
            setattr(so, k, f)
        yield
    finally:
        for k, f in old.items():
            setattr(so, k, f)


def inner_ref(dtype, ntm, w, m, v, *, step0, steps, lr, class_dist, C, betas=(0.9, 0.999), eps=1e-8, ntm_grad=None, single=False, adam=None,
              sig_w=None):
    """so.inner_w_loop (single: so.inner_w_loop_single on slot 1) in `dtype` from an arbitrary state.  ntm / w / m / v / ntm_grad: lists of two
    tensors (single: slot 0 is ignored and comes back as None).  adam / sig_w: replacements for so.adam_step_ / so.sig_w_forward (the
    mutants of tests/test_ntm_ref_cpu.py).  -> dict(w, m, v, T, ntm_grad: lists of two)."""
    ks = (1,) if single else (0, 1)
    cd = class_dist.to(dtype)
    n = {k: ntm[k].to(dtype).clone().requires_grad_(True) for k in ks}
    wr = {k: w[k].to(dtype).clone().requires_grad_(True) for k in ks}
    mm = {k: m[k].to(dtype).clone() for k in ks}
    vv = {k: v[k].to(dtype).clone() for k in ks}
    for k in ks:
        if ntm_grad is not None:
            n[k].grad = ntm_grad[k].to(dtype).clone()
    step = functools.partial(so.adam_step_ if adam is None else adam, beta1=betas[0], beta2=betas[1], eps=eps)
    hp = so.Hyper(num_classes=C, open_classes=ntm[1].shape[0] - C)
    with _patched(adam_step_=step, **({} if sig_w is None else {"sig_w_forward": sig_w})):
        if single:
            so.inner_w_loop_single(n[1], wr[1], {"step": step0, "m": mm[1], "v": vv[1]}, cd, hp, lr, steps=steps)
        else:
            so.inner_w_loop(n[0], n[1], wr[0], wr[1], {"step": step0, "m1": mm[0], "v1": vv[0], "m2": mm[1], "v2": vv[1]}, cd, hp, lr, steps=steps)
    out = {"w": [None, None], "m": [None, None], "v": [None, None], "T": [None, None], "ntm_grad": [None, None]}
    for k in ks:
        out["w"][k], out["m"][k], out["v"][k] = wr[k].detach(), mm[k], vv[k]
        out["T"][k] = so.sig_ntm_forward(n[k].detach(), cd, C)
        out["ntm_grad"][k] = torch.zeros_like(n[k].detach()) if n[k].grad is None else n[k].grad
    return out


def post_ref(dtype, ntm, w, hout, *, class_dist, C, lambda_seg, lambdas, gscale=1.0, single=False, ntm_grad=None, lout12=0.0, force_guard=False,
             mutant=None):
    """simt_ntm_post from a synthetic hout, in `dtype`, differentiated by autograd:

        gscale * sum_k [ wy_k <dTy_k, T_k> + lambda_convex convex_k + lambda_volume vol_k + lambda_anchor sum_{j: ex_k[j]} ||T_k[j] - A_k[j]||^2 ]

    T_k = sig_ntm_forward(ntm_k), convex_k = -||sig_w_forward(w_k) T_k||^2, vol_k = log sqrt |det T_k^T T_k|, wy_0 = lambda_seg, wy_1 = 1; the
    volume terms leave value and gradient when their SUM is NaN / Inf (force_guard: or when told to -- float64 does not underflow where fp32
    does).  single: k = 1 only, no lambda_seg terms.  mutant: "vol_while_guarded" keeps the volume gradient under the guard, "anchor_all_rows"
    ignores ex.  -> dict(lout [13] as ntm_post_kernel assembles it, ntm_grad [2], w [2] (diagonal := -1e4), guarded, vol [2])."""
    Q = ntm[1].shape[0]
    ks = (1,) if single else (0, 1)
    lc, lv, la = lambdas
    cd = class_dist.to(dtype)
    o, A, ex, dTy = hout_parts(hout.to(dtype), Q, C)
    n = {k: ntm[k].to(dtype).clone().requires_grad_(True) for k in ks}
    wr = {k: w[k].to(dtype).clone() for k in ks}
    zero = torch.zeros((), dtype=dtype)
    convex, vol, anchor, lin = [zero, zero], [zero, zero], [zero, zero], [zero, zero]
    for k in ks:
        T = so.sig_ntm_forward(n[k], cd, C)
        Wm = so.sig_w_forward(wr[k])
        convex[k] = 0.0 - ((Wm @ T) ** 2).sum()
        vol[k] = torch.log(torch.sqrt(torch.abs(torch.linalg.det(T.t() @ T))))
        rows = torch.ones(Q, dtype=torch.bool) if mutant == "anchor_all_rows" else ex[k]
        anchor[k] = ((T[rows] - A[k][rows]) ** 2).sum()
        lin[k] = (lambda_seg if k == 0 else 1.0) * (dTy[k] * T).sum()
    vsum = vol[0] + vol[1]
    guarded = bool(torch.isinf(vsum) or torch.isnan(vsum)) or force_guard
    vterm = zero if guarded else vsum
    csum, asum = convex[0] + convex[1], anchor[0] + anchor[1]
    diff = lin[0] + lin[1] + lc * csum + lv * (vsum if mutant == "vol_while_guarded" else vterm) + la * asum
    (gscale * diff).backward()
    lseg = 0.0 if single else lambda_seg
    place = lseg * o[2] + o[3]
    target = o[1] + o[5] + lseg * o[0] + lseg * o[4]
    total = place + target + lc * csum + lv * vterm + la * asum
    lout = torch.stack([total * gscale, zero if single else o[0], o[1], zero if single else o[4], o[5], place, csum, vterm, asum,
                        torch.tensor(0.0 if guarded else 1.0, dtype=dtype), vol[0], vol[1], lout12 + o[15]]).detach()
    g0 = [None, None]
    for k in ks:
        g0[k] = n[k].grad if ntm_grad is None else ntm_grad[k].to(dtype) + n[k].grad
    return {"lout": lout, "ntm_grad": g0, "w": [wr.get(0), wr.get(1)], "guarded": guarded, "vol": [v.detach() for v in vol]}


def sig_ntm_ref(dtype, ntm, class_dist, C, dT=None):
    """-> (T, dN or None): simt_sig_ntm's forward and, given dT, its backward."""
    n = ntm.to(dtype).clone().requires_grad_(True)
    T = so.sig_ntm_forward(n, class_dist.to(dtype), C)
    if dT is None:
        return T.detach(), None
    T.backward(dT.to(dtype))
    return T.detach(), n.grad


def sig_w_ref(dtype, w, dW=None):
    """-> (W, dweight or None, the weight after the call: diagonal := -1e4)."""
    wr = w.to(dtype).clone().requires_grad_(True)
    Wm = so.sig_w_forward(wr)
    if dW is None:
        return Wm.detach(), None, wr.detach()
    Wm.backward(dW.to(dtype))
    return Wm.detach(), wr.grad, wr.detach()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Gauss-Jordan in float64, the way ntm_post_kernel walks it: used only to SHOW that an input needs a row swap
# ---------------------------------------------------------------------------------------------------------------------------------------------
def gauss_jordan(G):
    """-> (product of the pivots with the swap sign, G^-1, number of row swaps) by Gauss-Jordan with partial pivoting (first largest |.|)."""
    G = np.array(G, dtype=np.float64)
    c = G.shape[0]
    M = np.concatenate([G, np.eye(c)], 1)
    det, swaps = 1.0, 0
    for p in range(c):
        piv = p + int(np.argmax(np.abs(M[p:, p])))
        if piv != p:
            M[[p, piv]] = M[[piv, p]]
            det, swaps = -det, swaps + 1
        det *= M[p, p]
        M[p] /= M[p, p]
        for r in range(c):
            if r != p:
                M[r] -= M[r, p] * M[p]
    return det, M[:, c:], swaps


def swaps_of(ntm, class_dist, C):
    T = so.sig_ntm_forward(ntm.double(), class_dist.double(), C).numpy()
    return gauss_jordan(T.T @ T)


# the two special inputs of simt_ntm_post (asserted in tests/test_ntm_ref_cpu.py) -------------------------------------------------------------
SWAP_Q, SWAP_SEED = 22, 0


def swap_input(seed=None):
    """class_dist * 8 and NTM = randn * 3 at Q = 22: T^T T is no longer diagonally dominant, the elimination has to swap rows.
    -> (class_dist, [ntm1, ntm2])"""
    g = torch.Generator().manual_seed(31000 + (SWAP_SEED if seed is None else seed))
    return REAL_CD.float() * 8.0, [torch.randn(SWAP_Q, 19, generator=g) * 3 for _ in range(2)]


def guard_input(Q=22, both=True):
    """class_dist * 1e6 with NTM = 0: every row of T is the prior up to 2e-6, det(T^T T) = 1e-205 in float64 and 0 in fp32 -> vol = -inf, the
    guard.  both=False: NTM2 = -30 instead, T2 = [I; prior rows], healthy -- the guard is on the SUM, so both lose the volume gradient.
    -> (class_dist, [ntm1, ntm2])"""
    return REAL_CD.float() * 1e6, [torch.zeros(Q, 19), torch.zeros(Q, 19) if both else torch.full((Q, 19), -30.0)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_ntm_solver.py (tests/test_ntm_ref_cpu.py runs the references on every one of them)
# ---------------------------------------------------------------------------------------------------------------------------------------------
LR_T = 6e-3
LAMBDA_SEG = 0.1
LAMBDAS = {"test": (0.5, 0.1, 0.5), "train": (0.1, 1.0, 1.0)}          # (convex, volume, anchor): the tests' default and the trainers'
# (Q, C, state, step0, steps, single, prior): a subset of the product that takes every value of every dimension, the limits (40, 20), Q == C
# and the smallest matrix with an off-diagonal (3, 2) in both forms
INNER_CASES = [
    (22, 19, "init", 0, 10, 0, "real"),
    (22, 19, "trained", 10, 10, 0, "real"),
    (22, 19, "trained", 10, 0, 0, "real"),
    (25, 19, "trained", 5000, 10, 1, "real"),
    (25, 19, "saturated", 5000, 10, 0, "real"),
    (34, 19, "saturated", 10, 10, 0, "real"),
    (34, 19, "init", 0, 1, 1, "real"),
    (40, 20, "trained", 5000, 10, 0, "softmax"),
    (40, 20, "saturated", 0, 1, 0, "zero"),
    (40, 20, "trained", 0, 0, 1, "softmax"),
    (20, 20, "init", 0, 10, 0, "softmax"),
    (20, 20, "trained", 10, 1, 1, "zero"),
    (3, 2, "trained", 10, 10, 0, "softmax"),
    (3, 2, "init", 0, 10, 1, "softmax"),
]
# (Q, C, state, ex, lambdas, single, prior)
POST_CASES = [
    (22, 19, "init", "all", "test", 0, "real"),
    (22, 19, "trained", "mixed", "train", 0, "real"),
    (22, 19, "trained", "mixed", "test", 1, "real"),
    (25, 19, "saturated", "none", "train", 0, "real"),
    (34, 19, "saturated", "mixed", "test", 0, "real"),
    (34, 19, "init", "all", "train", 1, "real"),
    (40, 20, "trained", "mixed", "train", 0, "softmax"),
    (40, 20, "saturated", "all", "test", 1, "zero"),
    (20, 20, "init", "mixed", "test", 0, "softmax"),
    (20, 20, "trained", "none", "train", 1, "zero"),
    (3, 2, "trained", "mixed", "train", 0, "softmax"),
    (3, 2, "init", "all", "test", 1, "softmax"),
]
LOUT12_BEFORE = 5.0          # what lout[12] holds before the first call: the slot accumulates


def case_id(c):
    return "-".join(str(x) for x in c)


def inner_case(c):
    """-> (state, class_dist, keyword arguments of inner_ref)"""
    Q, C, kind, step0, steps, single, pk = c
    st, cd = state(Q, C, kind), prior(C, pk)
    return st, cd, dict(step0=step0, steps=steps, lr=LR_T, class_dist=cd, C=C, ntm_grad=st["ntm_grad"], single=bool(single))


def inner_refs(c):
    st, cd, kw = inner_case(c)
    return ref_pair(("inner", c), lambda dt: inner_ref(dt, st["ntm"], st["w"], st["m"], st["v"], **kw))


def post_case(c, floats=None, gscale=1.0):
    """-> (state, class_dist, hout, keyword arguments of post_ref)"""
    Q, C, kind, ex, lam, single, pk = c
    st, cd = state(Q, C, kind), prior(C, pk)
    hout = synthetic_hout(Q, C, ex, floats=floats)
    return st, cd, hout, dict(class_dist=cd, C=C, lambda_seg=LAMBDA_SEG, lambdas=LAMBDAS[lam], gscale=gscale, single=bool(single),
                              ntm_grad=st["ntm_grad"], lout12=LOUT12_BEFORE)


def post_refs(c):
    st, cd, hout, kw = post_case(c)
    return ref_pair(("post", c), lambda dt: post_ref(dt, st["ntm"], st["w"], hout, **kw))


def special_post_case(name):
    """swap / guard_both / guard_one at Q = 22: -> (ntm [2], w [2], class_dist, hout, keyword arguments of post_ref, float64 needs force_guard)"""
    cd, ntm = swap_input() if name == "swap" else guard_input(22, both=(name == "guard_both"))
    Q = ntm[0].shape[0]
    w = state(Q, 19, "trained")["w"]
    kw = dict(class_dist=cd, C=19, lambda_seg=LAMBDA_SEG, lambdas=LAMBDAS["train"], gscale=1.0, single=False, ntm_grad=None, lout12=0.0)
    return ntm, w, cd, synthetic_hout(Q, 19, "mixed", seed=5), kw, name != "swap"


def special_post_refs(name):
    """(ref64, ref32); the guard cases: float64 WITH THE GUARD FORCED (it does not underflow), fp32 as it decides by itself."""
    ntm, w, cd, hout, kw, force = special_post_case(name)
    return ref_pair(("post", name), lambda dt: post_ref(dt, ntm, w, hout, force_guard=(force and dt == F64), **kw))


_CACHE = {}


def ref_pair(key, fn):
    """(ref64, ref32) of fn(dtype), computed once per key and shared (never modified by the callers)."""
    if key not in _CACHE:
        _CACHE[key] = (fn(F64), fn(F32))
    return _CACHE[key]
