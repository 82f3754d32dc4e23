"""The yardstick of the scale-crop tests: Pillow itself plus numpy, restated from the issue's contract and independent of
simt_amd/data/scale_crop.py (sizes with fractions.Fraction, draws from a numpy generator in the documented order)."""
import math
from fractions import Fraction

import numpy as np

IMG_MEAN = (104.00698793, 116.66876762, 122.67891434)


def scaled(n, text):
    return math.floor(n * Fraction(text) + Fraction(1, 2))


def origin_range(scaled_n, crop_n):
    return min(0, scaled_n - crop_n), max(0, scaled_n - crop_n)


def origin(u, lo, hi):
    return min(hi, lo + math.floor(u * (hi - lo + 1)))


def draws(rng, B, choices, crop_wh, mirror_on):
    """One batch: the mirror draw as the loader always made it, then choice, x, y."""
    flags = (rng.integers(0, 2, B) == 0).tolist() if mirror_on else [False] * B
    pick = rng.integers(0, len(choices), B).tolist()
    ux, uy = rng.random(B), rng.random(B)
    w, h = crop_wh
    ox = [origin(float(ux[b]), *origin_range(scaled(w, choices[pick[b]]), w)) for b in range(B)]
    oy = [origin(float(uy[b]), *origin_range(scaled(h, choices[pick[b]]), h)) for b in range(B)]
    return flags, pick, ox, oy


class Resized:
    """Pillow's resize of whole frames, computed once per (frame, size) and shared by the tests of a module."""

    def __init__(self):
        self.memo = {}

    def get(self, key, rgb, lab, ws, hs):
        from PIL import Image
        k = (key, ws, hs)
        if k not in self.memo:
            S = np.asarray(Image.fromarray(rgb).resize((ws, hs), Image.BICUBIC))
            Ln = np.asarray(Image.fromarray(lab).resize((ws, hs), Image.NEAREST))
            S.setflags(write=False)
            Ln.setflags(write=False)
            self.memo[k] = (S, Ln)
        return self.memo[k]


def item(resized, key, rgb, lab, crop_wh, choice, ox, oy, mirror, mean=IMG_MEAN):
    """-> (x [3,h,w] f32, label [h,w] i64): Pillow resize of the whole frame, numpy window with pad 0 / 255, [:, :, ::-1] - mean in
    float32, the mirror rule (channel order swapped, only the label reversed along x)."""
    w, h = crop_wh
    ws, hs = scaled(w, choice), scaled(h, choice)
    S, Ln = resized.get(key, rgb, lab, ws, hs)
    img = np.zeros((h, w, 3), np.uint8)
    inside = np.zeros((h, w), bool)
    lb = np.full((h, w), 255, np.uint8)
    ya, yb = max(0, -oy), min(h, hs - oy)
    xa, xb = max(0, -ox), min(w, ws - ox)
    assert ya < yb and xa < xb
    img[ya:yb, xa:xb] = S[ya + oy:yb + oy, xa + ox:xb + ox]
    lb[ya:yb, xa:xb] = Ln[ya + oy:yb + oy, xa + ox:xb + ox]
    inside[ya:yb, xa:xb] = True
    f = img.astype(np.float32)
    if mirror:
        f = f[:, :, ::-1]
        lb = lb[:, ::-1]
    f = f[:, :, ::-1] - np.asarray(mean, np.float32)
    f[~inside] = 0.0
    return np.ascontiguousarray(f.transpose(2, 0, 1)), np.ascontiguousarray(lb).astype(np.int64)
