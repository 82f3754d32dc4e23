"""The uncertainty-rectified pseudo-label loss of the two-head warm-up pass (simt_head_loss_uncertain / simt_head_grad_uncertain, DESIGN
7.28; Zheng & Yang, IJCV 2021) restated with torch autograd in any dtype, an analytic gradient by the header's formula, and the comparator
the CPU and the GPU tests share.

    up    = bilinear upsample of the low-res logits (align_corners=True, or the half-pixel default of F.interpolate)
    ls_k  = log_softmax(up(pred_k));  q_k = exp(ls_k);  u_k = -ls_k
    D_k   = KL(q_o || q_k) = sum_j q_o,j (u_k,j - u_o,j)          o the other head; nothing detached, nothing clamped
    R_k   = sum over labelled pixels of w_p exp(-D_k) u_k,label / N          N = labelled pixels
    K_k   = sum over ALL B * H * W pixels of D_k / (B * H * W)
    total = R_2 + lambda_kl K_2 + lambda_seg (R_1 + lambda_kl K_1)

Written from the contract in include/simt_hip.h, not from the kernel: log_softmax, exp and autograd.  The inputs are tests/_entropy_ref.py's.
"""
import torch
import torch.nn.functional as F

import _entropy_ref as er
import _head_bar as hb
from oracle import simt_oracle as so

CASES = er.CASES
inputs = er.inputs
pixel_weights = er.pixel_weights
# (case, half-pixel): the six two-head launches of the GPU tests.  "rows" is a compile-time-count descriptor (22, 19) that the uncertainty
# launches run on the run-time-count build; "wide" has Q = 27 > 24 (the QM = 40 builds), two chunks per row and B * H * W no multiple of 256
HEADS = [("straddle", False), ("straddle", True), ("rows", False), ("rows", True), ("wide", False), ("wide", True)]
HID = lambda c: f"{c[0]}-{'half' if c[1] else 'align'}"          # noqa: E731
MUTANTS = ("kl_swapped", "other_detached", "k_over_n", "no_exp_in_grad", "no_lambda_seg_k1", "c_sign")
LOSS_TOL = er.LOSS_TOL          # the project's loss bar: |got - ref64| <= 1e-4 * (1 + |ref64|)


def _up(half, size):
    return (lambda x: F.interpolate(x, size=size, mode="bilinear")) if half else (lambda x: so.upsample(x, size))


def uncertain_losses(q1, q2, lab, w, w_item, lambda_seg, half, Cn, lambda_kl, mutant=None):
    """The loss on low-res logits q1 / q2 [B][Q][h][w] of any dtype, differentiable in both.  -> dict(total, r1, r2, k1, k2, m1, m2, N)."""
    assert mutant is None or mutant in MUTANTS
    dtype = q2.dtype
    B, Q = q2.shape[:2]
    H, W = lab.shape[1:]
    valid = (lab >= 0) & (lab < Cn) & (lab != 255)
    idx = torch.where(valid, lab, torch.zeros_like(lab))
    wp = pixel_weights(w, w_item, B, H, W, dtype) * valid.to(dtype)
    N = valid.sum().to(dtype)
    up = _up(half, (H, W))
    ls = {1: torch.log_softmax(up(q1), 1), 2: torch.log_softmax(up(q2), 1)}

    def head(k):
        o = 3 - k
        lk, lo = ls[k], ls[o]
        if mutant == "other_detached":
            lo = lo.detach()
        own = 2 * lk.detach() - lk if mutant == "c_sign" else lk          # c_sign: D_k's gradient w.r.t. its own head negated, values kept
        if mutant == "kl_swapped":          # KL(q_k || q_o)
            D = (lk.exp() * (lk - lo)).sum(1)
        else:
            D = (lo.exp() * ((-own) - (-lo))).sum(1)
        rw = torch.exp(-D)
        ul = -lk.gather(1, idx[:, None])[:, 0]
        if mutant == "no_exp_in_grad":          # d/d u_label is 1 and not exp(-D); the value and the gradient through exp(-D) stay
            ce = rw * ul.detach() + (ul - ul.detach())
        else:
            ce = rw * ul
        R = (wp * ce).sum() / N
        K = D[valid].sum() / N if mutant == "k_over_n" else D.sum() / (B * H * W)
        return R, K, (rw.detach() * valid).sum() / N
    r1, k1, m1 = head(1)
    r2, k2, m2 = head(2)
    total = r2 + lambda_kl * k2 + lambda_seg * r1 + (1.0 if mutant == "no_lambda_seg_k1" else lambda_seg) * lambda_kl * k1
    return {"total": total, "r1": r1, "r2": r2, "k1": k1, "k2": k2, "m1": m1, "m2": m2, "N": int(valid.sum())}


def uncertain_ref(pred1, pred2, lab, w, w_item, lambda_seg, half, dtype, Cn, lambda_kl, mutant=None):
    """pred1 / pred2: [B][Q][h][w] logits; lab [B][H][W] int64; w None or a table; w_item None or bytes.  mutant: one of MUTANTS, a planted
    mistake (tests/test_uncertain_cpu.py).
    -> dict(dpred1, dpred2, r1, r2, k1, k2, m1, m2 (the mean rectification weights), total, N)."""
    q1 = pred1.to(dtype).clone().requires_grad_(True)
    q2 = pred2.to(dtype).clone().requires_grad_(True)
    out = uncertain_losses(q1, q2, lab, w, w_item, lambda_seg, half, Cn, lambda_kl, mutant)
    out["total"].backward()
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    return dict(out, dpred1=q1.grad, dpred2=q2.grad)


def analytic_grad(pred1, pred2, lab, w, w_item, lambda_seg, half, Cn, lambda_kl, dtype=torch.float64, gscale=1.0):
    """(dpred1, dpred2) by the formula of include/simt_hip.h, the upsample's adjoint taken by autograd on a LINEAR map:
    G_k,j = gscale { L_k [ a_k (q_k,j - onehot_j) + c_k (q_k,j - q_o,j) ] + L_o c_o q_k,j ((u_o,j - u_k,j) - D_o) },
    a_k = w_p exp(-D_k) / N, c_k = lambda_kl / (B H W) - a_k u_k,label, L_2 = 1, L_1 = lambda_seg."""
    B, Q = pred2.shape[:2]
    H, W = lab.shape[1:]
    valid = (lab >= 0) & (lab < Cn) & (lab != 255)
    idx = torch.where(valid, lab, torch.zeros_like(lab))
    wp = (pixel_weights(w, w_item, B, H, W, dtype) * valid.to(dtype))[:, None]
    N = valid.sum().to(dtype)
    up = _up(half, (H, W))
    p = {1: pred1.to(dtype).clone().requires_grad_(True), 2: pred2.to(dtype).clone().requires_grad_(True)}
    v = {k: up(p[k]) for k in (1, 2)}
    with torch.no_grad():
        u = {k: torch.logsumexp(v[k], 1, keepdim=True) - v[k] for k in (1, 2)}
        q = {k: torch.softmax(v[k], 1) for k in (1, 2)}
        onehot = torch.zeros_like(v[1]).scatter_(1, idx[:, None], 1.0) * valid[:, None].to(dtype)
        lam = {1: lambda_seg, 2: 1.0}
        D = {k: (q[3 - k] * (u[k] - u[3 - k])).sum(1, keepdim=True) for k in (1, 2)}
        a = {k: wp * torch.exp(-D[k]) / N for k in (1, 2)}
        c = {k: lambda_kl / (B * H * W) - a[k] * u[k].gather(1, idx[:, None]) for k in (1, 2)}
        G = {}
        for k in (1, 2):
            o = 3 - k
            G[k] = gscale * (lam[k] * (a[k] * (q[k] - onehot) + c[k] * (q[k] - q[o])) + lam[o] * c[o] * q[k] * ((u[o] - u[k]) - D[o]))
    ((v[1] * G[1]).sum() + (v[2] * G[2]).sum()).backward()
    return p[1].grad, p[2].grad


HOUT_KEYS = ((0, "r1"), (1, "r2"), (2, "k1"), (3, "k2"), (4, "m1"), (5, "m2"), (14, "total"))


def compare(tag, hout, grads, r64, r32):
    """The comparator of the tests: hout[:16] and the fp32 gradients {"dpred1", "dpred2": [B][Q][h][w]} of one launch pair against the
    float64 restatement under the loss bar and tests/_head_bar.py's gradient bar (tau from r64 / r32).  AssertionError on a miss."""
    for i, k in HOUT_KEYS:
        want, got = float(r64[k]), float(hout[i])
        print(f"[uncertain] {tag} hout[{i}] = {got!r}, float64 {k} = {want!r}", flush=True)
        assert abs(got - want) <= LOSS_TOL * (1 + abs(want)), (tag, k, got, want)
    assert int(hout[6]) == r64["N"], (tag, float(hout[6]), r64["N"])
    res = {}
    for k in ("dpred2", "dpred1"):
        res[k] = hb.grad_bar(grads[k], r64[k], r32[k], f"{tag} {k} fp32")
        hb.report(tag, f"{k} fp32", res[k])
    return res


def as_launch(r):
    """A restatement's dict in the form compare() takes a launch in: (hout[:16], grads)."""
    hout = torch.zeros(16, dtype=torch.float64)
    for i, k in HOUT_KEYS:
        hout[i] = float(r[k])
    hout[6] = r["N"]
    return hout, {"dpred1": r["dpred1"], "dpred2": r["dpred2"]}
