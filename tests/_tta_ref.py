"""The float64 restatement of simt_tta_label (include/simt_hip.h) that tests/test_tta_cpu.py checks on the CPU and tests/test_gpu_tta.py
holds the kernel to, and the shared inputs of the GPU tests.

Term value: bilinear align_corners=True from the [h][w] map to (H, W) -- a flipped term reads every tap's column ix at w-1-ix, weights
unchanged; the two-resample family first forms the virtual [hi][wi] map (align_corners=False, half-pixel, clamped at 0) and applies the
same resample, mirror included, to it.  Combination: the sum in term order (mode 0) or that sum times 1/n (mode 1); label = first-index
arg-max.  Everything in float64 (numpy)."""
import numpy as np


def _axis_true(out, inp):
    """align_corners=True taps along one axis: (i0, i1, w0, w1), src = dst * (in-1)/(out-1)."""
    scale = (inp - 1) / (out - 1) if out > 1 else 0.0
    f = scale * np.arange(out, dtype=np.float64)
    i0 = np.minimum(f.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    w1 = f - i0
    return i0, i1, 1.0 - w1, w1


def _axis_half(out, inp):
    """align_corners=False taps: src = max((dst + 0.5) * in/out - 0.5, 0)."""
    f = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * (inp / out) - 0.5, 0.0)
    i0 = np.minimum(f.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    w1 = f - i0
    return i0, i1, 1.0 - w1, w1


def _gather(l, ty, tx):
    y0, y1, wy0, wy1 = ty
    x0, x1, wx0, wx1 = tx
    wy0, wy1 = wy0[None, :, None, None], wy1[None, :, None, None]
    wx0, wx1 = wx0[None, None, :, None], wx1[None, None, :, None]
    r0, r1 = l[:, y0], l[:, y1]
    return wy0 * (wx0 * r0[:, :, x0] + wx1 * r0[:, :, x1]) + wy1 * (wx0 * r1[:, :, x0] + wx1 * r1[:, :, x1])


def resample_true(l, H, W, flip=False):
    """l [B, h, w, C] -> [B, H, W, C], align_corners=True; flip: the taps' columns are read at w-1-ix."""
    l = np.asarray(l, np.float64)
    h, w = l.shape[1:3]
    x0, x1, wx0, wx1 = _axis_true(W, w)
    if flip:
        x0, x1 = w - 1 - x0, w - 1 - x1
    return _gather(l, _axis_true(H, h), (x0, x1, wx0, wx1))


def resample_half(l, H, W):
    """l [B, h, w, C] -> [B, H, W, C], align_corners=False (the in-model upsample of DeepLabv3)."""
    l = np.asarray(l, np.float64)
    return _gather(l, _axis_half(H, l.shape[1]), _axis_half(W, l.shape[2]))


def term_value(l, H, W, flip=False, hiwi=(0, 0)):
    """One term of simt_tta_label at every label pixel: [B, H, W, C] float64."""
    hi, wi = hiwi
    if hi > 0:
        return resample_true(resample_half(l, hi, wi), H, W, flip)
    return resample_true(l, H, W, flip)


def combine(terms, H, W, mode):
    """terms: [(l [B,h,w,C], flip, (hi, wi))] -> (s [B,H,W,C], arg [B,H,W], top [B,H,W], gap [B,H,W]): the combined map, its first-index
    arg-max, maximum and top-2 gap."""
    s = None
    for (l, flip, hiwi) in terms:
        v = term_value(l, H, W, flip, hiwi)
        s = v if s is None else s + v
    if mode == 1:
        s = s * (1.0 / len(terms))
    arg = np.argmax(s, axis=3)
    srt = np.sort(s, axis=3)
    return s, arg, srt[..., -1], srt[..., -1] - srt[..., -2]


# ---- shared inputs of the GPU tests ---------------------------------------------------------------------------------------------------
B, C, H, W = 2, 19, 17, 23                              # odd; W % 4 != 0: the quad tail and the row wrap of the packed label stores
SIZES = ((5, 7), (6, 9), (9, 12))
HIWI = ((11, 15), (13, 18), (19, 25))                   # the virtual maps of the two-resample family
FLIPS = (False, True, False, True, True)
SEED = 2


def make_logits(n, seed=SEED, flips=FLIPS):
    """n low-res logit maps [B, h, w, C] float32 of ONE scene: a coarse 3 x 4 field resampled to each term's size (mirrored for a term
    of the mirrored frame) plus per-term noise, so that the terms agree and the averaged confidence spreads over roughly 0.2 - 0.95
    (independent random terms average to ~0.16 and never cross a useful threshold)."""
    rng = np.random.default_rng(seed)
    coarse = rng.standard_normal((B, 3, 4, C)) * 2.5 * 1.6
    maps = []
    for i in range(n):
        h, w = SIZES[i % len(SIZES)]
        m = resample_true(coarse, h, w)
        if flips[i]:
            m = m[:, :, ::-1]
        maps.append(np.ascontiguousarray(m + 0.7 * rng.standard_normal(m.shape), dtype=np.float32))
    return maps


def softmax32(l):
    """float32 probabilities of float32 logits (formed in float64, rounded once): the kernel and the reference read the same values."""
    l = np.asarray(l, np.float64)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def pad_channels(m, ld, plant=1e4):
    """[B, h, w, C] -> [B, h, w, ld] float32 with channels C..ld-1 planted: a kernel that reads past C is caught."""
    o = np.full(m.shape[:3] + (ld,), plant, np.float32)
    o[..., :m.shape[3]] = m
    return o
