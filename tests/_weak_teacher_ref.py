"""The weak-view teacher restated without a GPU: the item map of the mix and the SimT losses when the frozen model's
posterior of pixel p = (b, y, x) is read from item `item[b, y, x]` of the weak view.  The yardstick of tests/test_weak_teacher_cpu.py and
tests/test_gpu_weak_teacher.py.

`item_map` stands on tests/_class_mix_ref.py (sets, `sorted`, boolean masks).  `view_losses` / `view_losses_single` are
oracle.simt_oracle.simt_losses / simt_losses_single line for line, composed of the oracle's own pieces (imported, not copied): the one change
is that `conf0` and `labelC_flat` are gathered per pixel by the item map before anything uses them.  (`anchor_at` is `anchor_loss` itself
unless the caller names the anchor pixels: one line of it restated, for the plateau case it describes.)"""
import numpy as np
import torch
import torch.nn.functional as F

import _class_mix_ref as cm
import _head_bar as hb
from oracle import simt_oracle as so
from oracle.simt_oracle import anchor_loss, confidence_labels, noisy_nll, placeholder_loss


def item_map(lab, partner, apply, rank, n_classes):
    """-> uint8 [B,h,w]: the item each pixel of the mixed batch was taken from: partner[i] where item i takes its partner's pixel, else i."""
    lab = np.asarray(lab)
    B = lab.shape[0]
    out = np.empty(lab.shape, dtype=np.uint8)
    for i in range(B):
        out[i] = i
        if not apply[i]:
            continue
        j = int(partner[i])
        S = cm.chosen(lab[j], rank[i], n_classes)
        valid = (lab[j] >= 0) & (lab[j] < n_classes)
        out[i][valid & np.isin(lab[j], sorted(S))] = j
    return out


def gather_views(conf0, labelC_flat, item):
    """conf0 [B,H,W], labelC_flat [B*H*W, C] (pixel-major, as confidence_labels returns them) read through item [B,H,W]: pixel (b, y, x) takes
    the entries of pixel (item[b, y, x], y, x).  item None: unchanged."""
    if item is None:
        return conf0, labelC_flat
    B, H, W = conf0.shape
    it = torch.as_tensor(np.asarray(item)).long().clamp(max=B - 1)
    assert tuple(it.shape) == (B, H, W)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    src = ((it * H + yy) * W + xx).reshape(-1)
    return conf0.reshape(-1)[src].view(B, H, W), labelC_flat[src]


def anchor_at(pred_up, T, labelC_flat, idx):
    """anchor_loss with the anchor pixels GIVEN (idx [Q], None: the oracle's own first arg-max): where the upsample repeats a low-res row the
    maximum of a channel is a plateau up to rounding, and which of its pixels is first depends on the arithmetic -- a caller that has checked
    that another pixel is an arg-max too evaluates the term there.  The Exist set is the oracle's."""
    a, own, exist = anchor_loss(pred_up, T, labelC_flat)
    if idx is None:
        return a, own, exist
    idx = torch.as_tensor(idx).long()
    return ((T[exist] - labelC_flat[idx][exist]) ** 2).sum(), idx, exist


def view_losses(pred_lr1, pred_lr2, fixed_lr2, label, T1, T2, W1, W2, hp, size, item=None, up=None, prob_up=None, anchor_idx=(None, None)):
    """simt_losses with the frozen posterior gathered by `item`.  up: the upsample of the student's logits (default: the oracle's
    align_corners one); prob_up: the frozen posterior at label resolution when it is not `upsample(softmax(fixed_lr2))` (a model that
    upsamples its logits inside: softmax after the interpolation)."""
    c = hp.num_classes
    up = so.upsample if up is None else up
    if prob_up is None:
        conf0, labelC_flat = confidence_labels(fixed_lr2.detach(), size, hp)
    else:
        conf0, labelC_flat = _conf_of(prob_up.detach(), hp)
    conf0, labelC_flat = gather_views(conf0, labelC_flat, item)
    p1, p2 = up(pred_lr1, size), up(pred_lr2, size)
    a1, idx1, ex1 = anchor_at(p1, T1, labelC_flat, anchor_idx[0])
    a2, idx2, ex2 = anchor_at(p2, T2, labelC_flat, anchor_idx[1])
    anchor = a1 + a2
    pseudo = p2.detach().argmax(1)
    repl = torch.where(pseudo >= c, pseudo, torch.full_like(pseudo, 255))
    conf = torch.where(conf0 == c, repl, conf0)
    loss_p1 = F.cross_entropy(p1, conf, ignore_index=255)
    loss_p2 = F.cross_entropy(p2, conf, ignore_index=255)
    pl1, k1, u1 = placeholder_loss(p1, hp)
    pl2, k2, u2 = placeholder_loss(p2, hp)
    place = hp.lambda_seg * pl1 + pl2
    loss_y1 = noisy_nll(p1, T1, label)
    loss_y2 = noisy_nll(p2, T2, label)
    convex = 0.0 - ((W1 @ T1) ** 2).sum() - ((W2 @ T2) ** 2).sum()
    vol = torch.log(torch.sqrt(torch.abs(torch.linalg.det(T1.t() @ T1)))) + \
        torch.log(torch.sqrt(torch.abs(torch.linalg.det(T2.t() @ T2))))
    if torch.isinf(vol) or torch.isnan(vol):
        vol = 0.0
    target = loss_p2 + loss_y2 + hp.lambda_seg * loss_p1 + hp.lambda_seg * loss_y1
    total = place + target + hp.lambda_convex * convex + hp.lambda_volume * vol + hp.lambda_anchor * anchor
    return {"total": total / hp.iter_size, "loss_p1": loss_p1, "loss_p2": loss_p2, "loss_y1": loss_y1, "loss_y2": loss_y2,
            "place": place, "convex": convex, "volume": vol if torch.is_tensor(vol) else torch.tensor(vol),
            "anchor": anchor, "conf": conf, "conf0": conf0, "anchor_idx1": idx1, "anchor_idx2": idx2,
            "exist1": ex1, "exist2": ex2, "known1": k1, "known2": k2, "unknown1": u1, "unknown2": u2}


def _conf_of(prob_up, hp):
    """simt_losses_single's first four lines: (conf0, labelC_flat) of a posterior at label resolution."""
    c = hp.num_classes
    m, a = prob_up.max(1)
    conf0 = torch.where(m > hp.th_high, a, torch.full_like(a, 255))
    conf0 = torch.where(m < hp.th_low, torch.full_like(a, c), conf0)
    return conf0, prob_up.permute(0, 2, 3, 1).reshape(-1, c)


def view_losses_single(pred_up, prob_up, label, T, W, hp, item=None, anchor_idx=None):
    """simt_losses_single with the frozen posterior gathered by `item`."""
    c = hp.num_classes
    conf0, labelC_flat = gather_views(*_conf_of(prob_up, hp), item)
    anchor, idx, ex = anchor_at(pred_up, T, labelC_flat, anchor_idx)
    pseudo = pred_up.detach().argmax(1)
    repl = torch.where(pseudo >= c, pseudo, torch.full_like(pseudo, 255))
    conf = torch.where(conf0 == c, repl, conf0)
    loss_p = F.cross_entropy(pred_up, conf, ignore_index=255)
    place, known, unknown = placeholder_loss(pred_up, hp)
    loss_y = noisy_nll(pred_up, T, label)
    convex = 0.0 - ((W @ T) ** 2).sum()
    vol = torch.log(torch.sqrt(torch.abs(torch.linalg.det(T.t() @ T))))
    if torch.isinf(vol) or torch.isnan(vol):
        vol = 0.0
    total = place + loss_p + loss_y + hp.lambda_convex * convex + hp.lambda_volume * vol + hp.lambda_anchor * anchor
    return {"total": total / hp.iter_size, "loss_p": loss_p, "loss_y": loss_y, "place": place, "convex": convex,
            "volume": vol if torch.is_tensor(vol) else torch.tensor(vol), "anchor": anchor, "conf": conf, "anchor_idx": idx,
            "exist": ex, "known": known, "unknown": unknown}


def _ups(half):
    if half:
        return lambda x, size: F.interpolate(x, size=size, mode="bilinear")
    return so.upsample


def two_head_view_ref(p1, p2, f2, lab, ntm, d, cd, dtype, item, half=False, fix_logits=False, anchor_idx=(None, None)):
    """_head_bar.two_head_ref through view_losses: the inner W loop, the losses under `item`, backward, in `dtype`.  half / fix_logits: the
    head descriptor's up_half_pixel / fix_logits."""
    K = int(d["K"]); Cn = cd.numel(); Q = Cn + K
    H, W = lab.shape[1:]
    hp = hb.hyper(d, K, Cn)
    cdt = cd.to(dtype)
    n = [x.to(dtype).clone().requires_grad_(True) for x in ntm]
    wr = [so.w_init(Cn, K).to(dtype).requires_grad_(True) for _ in range(2)]
    z = lambda: torch.zeros(Q, Q, dtype=dtype)
    state = {"step": 0, "m1": z(), "v1": z(), "m2": z(), "v2": z()}
    so.inner_w_loop(n[0], n[1], wr[0], wr[1], state, cdt, hp, float(d["lr_T"]))
    q1, q2 = p1.to(dtype).clone().requires_grad_(True), p2.to(dtype).clone().requires_grad_(True)
    T1, T2 = so.sig_ntm_forward(n[0], cdt, Cn), so.sig_ntm_forward(n[1], cdt, Cn)
    up = _ups(half)
    fx = f2.to(dtype)
    prob_up = torch.softmax(up(fx, (H, W)), 1) if fix_logits else up(torch.softmax(fx, 1), (H, W))
    out = view_losses(q1, q2, fx, lab, T1, T2, so.sig_w_forward(wr[0]), so.sig_w_forward(wr[1]), hp, (H, W), item=item, up=up, prob_up=prob_up,
                      anchor_idx=anchor_idx)
    out["total"].backward()
    return {"dpred1": q1.grad, "dpred2": q2.grad, "ntm_grad1": n[0].grad, "ntm_grad2": n[1].grad, "out": {k: v.detach() for k, v in out.items()}}


def single_view_ref(pred, fix, lab, ntm, K, cd, dtype, item, half=False, fix_logits=False, d=hb.DEFAULT_D, anchor_idx=None):
    """_head_bar.single_ref through view_losses_single."""
    Cn = cd.numel(); Q = Cn + K
    H, W = lab.shape[1:]
    hp = hb.hyper(dict(d, K=K), K, Cn)
    cdt = cd.to(dtype)
    n = ntm.to(dtype).clone().requires_grad_(True)
    wr = so.w_init(Cn, K).to(dtype).requires_grad_(True)
    state = {"step": 0, "m": torch.zeros(Q, Q, dtype=dtype), "v": torch.zeros(Q, Q, dtype=dtype)}
    so.inner_w_loop_single(n, wr, state, cdt, hp, float(d["lr_T"]))
    q = pred.to(dtype).clone().requires_grad_(True)
    fx = fix.to(dtype)
    Tm = so.sig_ntm_forward(n, cdt, Cn)
    up = _ups(half)
    prob = torch.softmax(up(fx, (H, W)), 1) if fix_logits else up(torch.softmax(fx, 1), (H, W))
    out = view_losses_single(up(q, (H, W)), prob, lab, Tm, so.sig_w_forward(wr), hp, item=item, anchor_idx=anchor_idx)
    out["total"].backward()
    return {"dpred2": q.grad, "ntm_grad2": n.grad, "out": {k: v.detach() for k, v in out.items()}}
