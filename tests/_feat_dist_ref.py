"""The contract of the ImageNet feature distance (include/simt_hip.h) restated in numpy / float64: the label windows, the mask,
N, the distances, the three scalars and the seed; the comparators the GPU tests hold the launches to; and the float64 oracle of a warm-up
step with the term, which adds it through autograd.  Nothing here imports the code under test."""
import numpy as np
import torch

from oracle import simt_oracle as so

DEFAULT_CLASSES = (6, 7, 11, 12, 13, 14, 15, 16, 17, 18)
EPS24 = 2.0 ** -24


def windows(N, n):
    """[(lo, hi)] of the n windows over N label rows (or columns): [(i*N)//n, ((i+1)*N)//n)."""
    assert 1 <= n <= N
    return [((i * N) // n, ((i + 1) * N) // n) for i in range(n)]


def mask_ref(label, h, w, classes, min_ratio):
    """label int64 [B, H, W] -> (mask uint8 [B*h*w], N).  A cell is kept iff some class c of `classes` has
    float32(count_c) >= float32(min_ratio) * float32(n), one float32 multiply."""
    label = np.asarray(label)
    B, H, W = label.shape
    r = np.float32(min_ratio)
    out = np.zeros((B, h, w), dtype=np.uint8)
    for b in range(B):
        for i, (r0, r1) in enumerate(windows(H, h)):
            for j, (c0, c1) in enumerate(windows(W, w)):
                win = label[b, r0:r1, c0:c1]
                bar = np.float32(r * np.float32(win.size))
                for c in classes:
                    if np.float32(int((win == c).sum())) >= bar:
                        out[b, i, j] = 1
    return out.reshape(-1), int(out.sum())


def dist_ref(fs, fi, mask, lam, gscale):
    """fs, fi: [M, C] arrays holding exactly the values the device buffers hold (any float dtype; NaN / Inf allowed in rows that are not
    kept) -> dict(d [M] float64, S, N, out [3] float64, seed [M, C] float64 -- unrounded --, lam_g)."""
    mask = np.asarray(mask).astype(bool)
    M, C = fs.shape
    N = int(mask.sum())
    lam_g = float(np.float32(float(lam) * float(gscale)))
    d = np.zeros(M, dtype=np.float64)
    seed = np.zeros((M, C), dtype=np.float64)
    for m in np.nonzero(mask)[0]:
        diff = np.asarray(fs[m], dtype=np.float64) - np.asarray(fi[m], dtype=np.float64)
        d[m] = np.sqrt((diff * diff).sum())
        if d[m] > 0:
            seed[m] = (lam_g / float(N)) / d[m] * diff
    S = float(d.sum())
    out = np.array([float(lam) * S / N, S / N, float(N)] if N else [0.0, 0.0, 0.0])
    return dict(d=d, S=S, N=N, out=out, seed=seed, lam_g=lam_g)


def half_ulp_bf16(v):
    """Half a bf16 unit in the last place of the float64 values v (8 significand bits; the smallest normal exponent below it)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 8)


def check_d(got, ref, mask, C):
    """The distances: a kept row within (C + 4) * 2^-24 relative -- the worst case of ANY-order float32 summation of C non-negative terms
    ((C - 1) * 2^-24 relative), the subtract and the square of every term (1.5 * 2^-24 on the sum after the root halves 3) and the root's
    own rounding, rounded up --, a row that is not kept exactly 0."""
    got, want, mask = np.asarray(got, dtype=np.float64), ref["d"], np.asarray(mask).astype(bool)
    assert got.shape == want.shape
    assert not np.isnan(got).any(), "NaN among the distances"
    assert (got[~mask] == 0).all(), "a row that is not kept has a distance"
    err = np.abs(got[mask] - want[mask])
    bar = (C + 4) * EPS24 * np.abs(want[mask])
    assert (err <= bar).all(), f"d: {int((err > bar).sum())} of {int(mask.sum())} kept rows beyond (C + 4) * 2^-24, worst {float((err / np.maximum(bar, 1e-300)).max()):.2f} x the bar"


def check_seed(got, ref, mask, C, bf16):
    """The seed, element by element: fp32 within (C + 8) * 2^-24 * |value| (the distance's (C + 4), the subtract, two divisions and the
    product, half a unit each), bf16 within that plus half a bf16 unit of the float64 value; a row that is not kept, and a kept row
    whose distance is 0, +0 in every column (the sign bit is checked)."""
    got, want, mask = np.asarray(got, dtype=np.float64), ref["seed"], np.asarray(mask).astype(bool)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any(), "NaN in the seed"
    zero_rows = ~mask | (ref["d"] == 0)
    z = got[zero_rows]
    assert (z == 0).all() and not np.signbit(z).any(), f"{int((z != 0).sum())} non-zero and {int(np.signbit(z).sum())} negative-zero elements in rows that must be +0"
    bar = (C + 8) * EPS24 * np.abs(want) + (half_ulp_bf16(want) if bf16 else 0.0)
    err = np.abs(got - want)
    bad = (err > bar) & ~zero_rows[:, None]
    assert not bad.any(), (f"seed: {int(bad.sum())} elements in {int(bad.any(axis=1).sum())} rows beyond the bar, worst "
                           f"{float((err[bad] / np.maximum(bar[bad], 1e-300)).max()):.2f} x")


def check_scalars(got, ref, M, C):
    """out[0..2]: N exactly; the two means within (C + 4 + ceil(M / 4)) * 2^-24 relative -- the distances' bar plus the float32 sums of at most
    ceil(M / 4) of them per workgroup (the partials are then summed in double) -- plus the final rounding to float32."""
    got = np.asarray(got, dtype=np.float64)
    assert got[2] == ref["out"][2], (got, ref["out"])
    for i in (0, 1):
        bar = (C + 5 + (M + 3) // 4) * EPS24 * abs(ref["out"][i])
        assert abs(got[i] - ref["out"][i]) <= bar, (i, got[i], ref["out"][i], bar)


def torch_mask(label, s, classes, min_ratio, num_classes=19):
    """DAFormer's downscale_label_ratio + class test, literally, for H = s*h, W = s*w: one_hot -> avg_pool2d -> max -> ratio -> class test."""
    lab = torch.as_tensor(label).clone()
    B, H, W = lab.shape
    ignore = (lab < 0) | (lab >= num_classes)
    lab[ignore] = num_classes
    oh = torch.nn.functional.one_hot(lab, num_classes + 1).permute(0, 3, 1, 2).double()
    share = torch.nn.functional.avg_pool2d(oh, kernel_size=s)          # exact: counts / s^2 in float64
    top, arg = share.max(dim=1)
    thing = torch.zeros(num_classes + 1, dtype=torch.bool)
    thing[list(classes)] = True
    count = (top * (s * s)).round().float()          # the share back as the pixel count it came from
    keep = (count >= float(np.float32(min_ratio) * np.float32(s * s))) & thing[arg]      # count >= ratio * n, both float32
    return keep.reshape(-1).numpy().astype(np.uint8)


class OracleFeatDistTrainer(so.OracleWarmupTrainer):
    """OracleWarmupTrainer whose labelled pass adds lambda * norm(f4 - f4_imagenet.detach(), dim=1)[mask].mean() through autograd:
    so.trunk(st, x, train) for both maps, the ImageNet one at train=False."""

    def __init__(self, st, hp, imnet_st, lam, classes=DEFAULT_CLASSES, min_ratio=0.75, layers=so.LAYERS, dtype=torch.float32):
        super().__init__(st, hp, layers=layers, dtype=dtype)
        self.imnet = {k: (v.to(dtype) if v.dtype != torch.long else v).clone() for k, v in imnet_st.items()}
        self.lam, self.classes, self.min_ratio = float(lam), tuple(classes), float(min_ratio)

    def step(self, image, label, it):
        hp = self.hp
        lr = so.lr_poly(hp.lr, it, hp.num_steps, hp.power)
        for v in self.st.values():
            if v.dtype != torch.long:
                v.grad = None
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        labels = list(label) if isinstance(label, (list, tuple)) else [label]
        assert len(images) == len(labels) == hp.iter_size
        for image, label in zip(images, labels):
            x = image.to(self.dtype)
            f = so.trunk(self.st, x, True, self.layers)
            x1, x2 = so._aspp(self.st, "layer5", f[3], 2), so._aspp(self.st, "layer6", f[4], 2)
            total, l1, l2 = so.warmup_losses(x1, x2, label, hp.lambda_seg, tuple(label.shape[1:]))
            with torch.no_grad():
                fi = so.trunk(self.imnet, x, False, self.layers)[4]
            B, _c, h, w = f[4].shape
            mask, N = mask_ref(label.numpy(), h, w, self.classes, self.min_ratio)
            keep = torch.from_numpy(mask.astype(bool)).view(B, h, w)
            dist = (f[4] - fi.detach()).norm(dim=1)[keep]
            fd = self.lam * dist.mean() if N else total * 0.0
            ((total + fd) / hp.iter_size).backward()
        with torch.no_grad():
            for g in self.groups:
                ps, gs, bs, ms = [], [], [], []
                for n, m in zip(g["names"], g["mult"]):
                    p = self.st[n]
                    if p.grad is None:
                        continue
                    if n not in self.bufs:
                        self.bufs[n] = torch.zeros_like(p)
                    ps.append(p); gs.append(p.grad); bs.append(self.bufs[n]); ms.append(m)
                so.sgd_step_(ps, gs, bs, ms, lr * g["lr_mult"], hp.weight_decay, hp.momentum, self.first)
            self.first = False
        return {"total": (total / hp.iter_size).detach(), "loss_seg1": l1.detach(), "loss_seg2": l2.detach(), "feat_dist": fd.detach(), "cells": N}
