"""The quality-weighted warm-up cross-entropy (simt_head_loss_weighted / simt_head_grad_weighted) restated with torch autograd in
any dtype, and the inputs the CPU and the GPU tests share.

    up   = bilinear upsample of the low-res logits (align_corners=True, or the half-pixel default of F.interpolate)
    CE_p = -log_softmax(up)[label_p]                     over the pixels whose label is a class (255 and out-of-range labels are skipped)
    w_p  = w[item of p]  or  w[min(w_item[p], B - 1)]    with an item map
    loss_k = sum_p w_p * CE_p / N,   N = the NUMBER of labelled pixels (not the sum of the weights)
    total  = loss_2 + lambda_seg * loss_1

Nothing here is taken from the kernel: the upsample is oracle/simt_oracle.upsample or F.interpolate, the rest three lines of torch.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import simt_oracle as so

F64 = torch.float64

# name -> (B, h, w, H, W, Q, C): CASES["straddle"]: H * W = 16 900 is no multiple of 256 with B = 3 (a 256-pixel group of pass 1 straddles two
# items) and W = 260 > 256 (two chunks per row in pass 2); CASES["rows"]: the compile-time-count build (Q, C) = (22, 19) whose pass 2 takes
# R = 3 image rows per block (head_rows_per_block: 516 % 3 == 0, 2 * 0.124 <= 0.95, 3 * 516 / 3 = 516 >= 512 blocks, 2 * 5 * 22 <= 4608)
CASES = {"straddle": (3, 9, 33, 65, 260, 19, 19), "rows": (3, 65, 5, 516, 20, 22, 19)}


def pixel_weights(w, w_item, B, H, W, dtype):
    """-> [B][H][W] weights in `dtype`: w[b] broadcast, or gathered through the map with its bytes clamped to B - 1."""
    w = torch.as_tensor(np.asarray(w, dtype=np.float32)).to(dtype)
    if w_item is None:
        return w.view(B, 1, 1).expand(B, H, W)
    return w[torch.as_tensor(np.asarray(w_item)).long().clamp(max=B - 1)]


def weighted_ref(pred1, pred2, lab, w, w_item, lambda_seg, half, dtype, Cn=None):
    """pred1 (None: the one-output models) / pred2: [B][Q][h][w] logits; lab: [B][H][W] int64; w: [B]; w_item: [B][H][W] bytes or None.
    Cn: the number of classes a label may name (default Q).  -> dict(dpred1 | None, dpred2, l1 | None, l2, total, N)."""
    B, Q = pred2.shape[:2]
    H, W = lab.shape[1:]
    Cn = Q if Cn is None else Cn
    valid = (lab >= 0) & (lab < Cn) & (lab != 255)
    idx = torch.where(valid, lab, torch.zeros_like(lab))
    wp = pixel_weights(w, w_item, B, H, W, dtype) * valid.to(dtype)
    N = valid.sum().to(dtype)
    up = (lambda x: F.interpolate(x, size=(H, W), mode="bilinear")) if half else (lambda x: so.upsample(x, (H, W)))

    def loss(q):
        nll = -torch.log_softmax(up(q), 1).gather(1, idx[:, None])[:, 0]
        return (wp * nll).sum() / N
    q2 = pred2.to(dtype).clone().requires_grad_(True)
    l2 = loss(q2)
    q1, l1, total = None, None, l2
    if pred1 is not None:
        q1 = pred1.to(dtype).clone().requires_grad_(True)
        l1 = loss(q1)
        total = l2 + lambda_seg * l1
    total.backward()
    return {"dpred1": None if q1 is None else q1.grad, "dpred2": q2.grad, "l1": None if l1 is None else l1.detach(), "l2": l2.detach(),
            "total": total.detach(), "N": int(valid.sum())}


def inputs(case, cd, seed=0):
    """The inputs of test (e): -> (pred1, pred2, lab, w, w_item).  Logits randn * 3; labels of the synthetic batch with a band of 255s and two
    out-of-range values; general weights in (0, 1]; a blocky random item map that names every item, with one block of bytes >= B (clamped
    to B - 1)."""
    B, h, w_, H, W, Q, Cn = CASES[case]
    g = torch.Generator().manual_seed(100 + seed + H)
    p1 = torch.randn(B, Q, h, w_, generator=g) * 3
    p2 = torch.randn(B, Q, h, w_, generator=g) * 3
    _, lab = so.synthetic_batch(B, H, W, cd.numpy(), seed=17 + seed, block=8)
    lab[1, H // 2:H // 2 + 5] = 255
    lab[0, 0, 0], lab[B - 1, H - 1, W - 1] = Cn, 300
    wt = (torch.rand(B, generator=g) * 0.9 + 0.1).float().numpy()
    by, bx = (H + 12) // 13, (W + 6) // 7
    blocks = torch.randint(0, B, (B, by, bx), generator=g)
    blocks[0, 0, 0] = B + 3
    item = blocks.repeat_interleave(13, 1).repeat_interleave(7, 2)[:, :H, :W].to(torch.uint8).contiguous()
    assert all(bool((item[i] != i).any()) for i in range(B)) and set(item.unique().tolist()) >= set(range(B))
    return p1, p2, lab, wt, item


def shifted(w_item, B):
    """The map with every item moved on by one: what a kernel reads that applies the weights from the wrong item."""
    return ((w_item.long().clamp(max=B - 1) + 1) % B).to(torch.uint8)
