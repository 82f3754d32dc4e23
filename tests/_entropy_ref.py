"""The warm-up cross-entropy plus the robust entropy term of the target pass (simt_head_loss_entropy / simt_head_grad_entropy)
restated with torch autograd in any dtype, the inputs the CPU and the GPU tests share, and the comparator both use.

    up    = bilinear upsample of the low-res logits (align_corners=True, or the half-pixel default of F.interpolate)
    CE    = tests/_weighted_ref.py's weighted cross-entropy (w None: every weight 1), divided by the number of labelled pixels
    ls    = log_softmax(up);  q = exp(ls);  u = -ls;  H = sum_j q_j u_j;  e = H / ln Q;  t = e^2 + 1e-8;  rho = t^eta
    ent_k = sum over ALL B * H * W pixels of rho / (B * H * W)
    total = CE_2 + lambda_seg * CE_1 + lambda_ent * (ent_2 + lambda_seg * ent_1)

Written from the contract in include/simt_hip.h, not from the kernel: log_softmax, exp, pow and autograd.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _head_bar as hb
import _weighted_ref as wr
from oracle import simt_oracle as so

EPS = 1e-8
# wr.CASES and "wide": Q = 27 > 24 takes the <QMAX, 0, 0> builds, W = 260 > 256 two chunks per row in pass 2, B * H * W = 8 840 is no multiple of 256
CASES = dict(wr.CASES, wide=(2, 5, 9, 17, 260, 27, 27))
MUTANTS = ("no_lnq", "labelled_mean", "no_lambda_seg", "no_chain", "sign")
BLOCK = (slice(1, 3), slice(1, 4))          # the low-res block of item 0 (saturated) and of item 1 (uniform): every case has h, w >= 5


def inputs(case, cd, seed=0):
    """wr.inputs at CASES[case], with one low-res block of item 0 multiplied by 20 (near one-hot: e * e far below eps) and the same block of
    item 1 set to a constant (uniform: e = 1), in both heads.  -> (pred1, pred2, lab, w, w_item)."""
    added = case not in wr.CASES
    if added:
        wr.CASES[case] = CASES[case]
    try:
        p1, p2, lab, wt, item = wr.inputs(case, cd, seed)
    finally:
        if added:
            del wr.CASES[case]
    for p in (p1, p2):
        p[0][:, BLOCK[0], BLOCK[1]] *= 20
        p[1][:, BLOCK[0], BLOCK[1]] = 0.7
    return p1, p2, lab, wt, item


def pixel_weights(w, w_item, B, H, W, dtype):
    """-> [B][H][W] weights: 1 without a table; w[b]; or w[min(w_item, len(w) - 1)] with a map."""
    if w is None:
        assert w_item is None
        return torch.ones(B, H, W, dtype=dtype)
    w = torch.as_tensor(np.asarray(w, dtype=np.float32)).to(dtype)
    if w_item is None:
        return w[:B].view(B, 1, 1).expand(B, H, W)
    return w[torch.as_tensor(np.asarray(w_item)).long().clamp(max=w.numel() - 1)]


def entropy_ref(pred1, pred2, lab, w, w_item, lambda_seg, half, dtype, Cn, lambda_ent, eta, mutant=None):
    """pred1 (None: the one-output models) / pred2: [B][Q][h][w] logits; lab [B][H][W] int64; w None or a table; w_item None or bytes.
    mutant: one of MUTANTS, a planted mistake (tests/test_entropy_cpu.py).
    -> dict(dpred1 | None, dpred2, l1 | None, l2, ent1 | None, ent2, total, N)."""
    assert mutant is None or mutant in MUTANTS
    B, Q = pred2.shape[:2]
    H, W = lab.shape[1:]
    valid = (lab >= 0) & (lab < Cn) & (lab != 255)
    idx = torch.where(valid, lab, torch.zeros_like(lab))
    wp = pixel_weights(w, w_item, B, H, W, dtype) * valid.to(dtype)
    N = valid.sum().to(dtype)
    up = (lambda x: F.interpolate(x, size=(H, W), mode="bilinear")) if half else (lambda x: so.upsample(x, (H, W)))
    lnq = 1.0 if mutant == "no_lnq" else math.log(Q)

    def terms(p):
        ls = torch.log_softmax(up(p), 1)
        ce = (wp * -ls.gather(1, idx[:, None])[:, 0]).sum() / N
        ent = ((ls.exp() * -ls).sum(1)) / lnq
        t = ent * ent + EPS
        rho = t.pow(eta)
        if mutant == "no_chain":          # the chain factor 2 eta e rho / t replaced by 1: the gradient of the plain entropy, the value kept
            rho = rho.detach() + (ent - ent.detach())
        mean = rho[valid].sum() / N if mutant == "labelled_mean" else rho.sum() / (B * H * W)
        return ce, -mean if mutant == "sign" else mean
    q2 = pred2.to(dtype).clone().requires_grad_(True)
    l2, e2 = terms(q2)
    q1, l1, e1 = None, None, None
    total = l2 + lambda_ent * e2
    if pred1 is not None:
        q1 = pred1.to(dtype).clone().requires_grad_(True)
        l1, e1 = terms(q1)
        total = l2 + lambda_seg * l1 + lambda_ent * (e2 + (1.0 if mutant == "no_lambda_seg" else lambda_seg) * e1)
    total.backward()
    det = lambda x: None if x is None else x.detach()          # noqa: E731
    return {"dpred1": None if q1 is None else q1.grad, "dpred2": q2.grad, "l1": det(l1), "l2": det(l2), "ent1": det(e1), "ent2": det(e2),
            "total": det(total), "N": int(valid.sum())}


def analytic_grad(pred, size, half, lambda_ent, eta, dtype=torch.float64):
    """d(lambda_ent * ent) / d(low-res logits) by the formula of include/simt_hip.h, the upsample's adjoint taken by autograd on a LINEAR map:
    d ent / d v_j = (2 eta e rho / t) / ln(Q) * (-q_j (H - u_j)) / (B H W)."""
    B, Q = pred.shape[:2]
    H, W = size
    up = (lambda x: F.interpolate(x, size=(H, W), mode="bilinear")) if half else (lambda x: so.upsample(x, (H, W)))
    p = pred.to(dtype).clone().requires_grad_(True)
    v = up(p)
    with torch.no_grad():
        lse = torch.logsumexp(v, 1, keepdim=True)
        u = lse - v
        q = torch.softmax(v, 1)
        Hp = (q * u).sum(1, keepdim=True)
        e = Hp / math.log(Q)
        t = e * e + EPS
        rho = torch.exp(eta * torch.log(t))
        dv = lambda_ent / (B * H * W) * (2 * eta * e * rho / t) / math.log(Q) * (-q * (Hp - u))
    (v * dv).sum().backward()
    return p.grad


LOSS_TOL = 1e-4          # the project's loss bar: |got - ref64| <= 1e-4 * (1 + |ref64|)


def compare(tag, hout, grads, r64, r32, single):
    """The comparator of the GPU tests: hout[:16] and the fp32 gradients {"dpred2": [B][Q][h][w], "dpred1": ...} of one launch pair against
    the float64 restatement under the loss bar and tests/_head_bar.py's gradient bar (tau from r64 / r32).  AssertionError on a miss."""
    pairs = ((1, "l2"), (3, "ent2"), (14, "total")) + (() if single else ((0, "l1"), (2, "ent1")))
    for i, k in pairs:
        want, got = float(r64[k]), float(hout[i])
        print(f"[entropy] {tag} hout[{i}] = {got!r}, float64 {k} = {want!r}", flush=True)
        assert abs(got - want) <= LOSS_TOL * (1 + abs(want)), (tag, k, got, want)
    assert int(hout[6]) == r64["N"], (tag, float(hout[6]), r64["N"])
    res = {}
    for k in ("dpred2",) + (() if single else ("dpred1",)):
        res[k] = hb.grad_bar(grads[k], r64[k], r32[k], f"{tag} {k} fp32")
        hb.report(tag, f"{k} fp32", res[k])
    return res
