"""The yardstick of the rare-class sampling tests: a restatement of the sampler (class probabilities, draws) and of the device contract
(counts of a class inside a candidate window, the pick) from their written contracts, independent of simt_amd: Pillow's NEAREST resize of the
whole label plus a numpy window, as in _scale_crop_ref.py, and numpy generators in the documented order."""
import math
from fractions import Fraction

import numpy as np

import _scale_crop_ref as scref

TAG = 0x52435331          # the sampler's stream tag ("RCS1")
PARTS = 16


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------
def class_probs(counts, T, min_pixels):
    counts = np.asarray(counts, dtype=np.int64)
    C = counts.shape[1]
    total = int(counts.sum())
    f = [int(counts[:, c].sum()) / total for c in range(C)]
    ok = [bool((counts[:, c] >= min_pixels).any()) for c in range(C)]
    z = [(1.0 - f[c]) / T for c in range(C)]
    m = max(z[c] for c in range(C) if ok[c])
    e = [math.exp(z[c] - m) if ok[c] else 0.0 for c in range(C)]
    s = math.fsum(e)
    return np.array([v / s for v in e], dtype=np.float64)


def items_with_class(counts, min_pixels):
    counts = np.asarray(counts, dtype=np.int64)
    return [[i for i in range(counts.shape[0]) if counts[i, c] >= min_pixels] for c in range(counts.shape[1])]


def generator(seed, rank):
    return np.random.default_rng([seed, rank, TAG])


def draw_batch(rng, B, probs, lists):
    """Two draws per batch: random(B) for the classes, random(B) for the frames."""
    uc, ui = rng.random(B), rng.random(B)
    cdf = np.cumsum(probs)
    last = max(c for c in range(len(probs)) if probs[c] > 0)
    cls, idx = [], []
    for b in range(B):
        c = next((c for c in range(len(probs)) if cdf[c] > uc[b]), last)
        c = min(c, last)
        n = len(lists[c])
        cls.append(c)
        idx.append(lists[c][min(n - 1, math.floor(float(ui[b]) * n))])
    return cls, idx


def min_count(min_pixels, ratio_text):
    return math.floor(int(min_pixels) * Fraction(ratio_text))


# ---- the loader's window draws, K candidates per item ------------------------------------------------------------------------------------------
def cand_draws(rng, B, K, choices, crop_wh, mirror_on):
    """The mirror draw as ever, then integers(0, n, (B, K)), random((B, K)) for x, random((B, K)) for y."""
    flags = (rng.integers(0, 2, B) == 0).tolist() if mirror_on else [False] * B
    pick = rng.integers(0, len(choices), (B, K)).tolist()
    ux, uy = rng.random((B, K)), rng.random((B, K))
    w, h = crop_wh
    ox = [[scref.origin(float(ux[b, k]), *scref.origin_range(scref.scaled(w, choices[pick[b][k]]), w)) for k in range(K)] for b in range(B)]
    oy = [[scref.origin(float(uy[b, k]), *scref.origin_range(scref.scaled(h, choices[pick[b][k]]), h)) for k in range(K)] for b in range(B)]
    return flags, pick, ox, oy


# ---- the device contract -----------------------------------------------------------------------------------------------------------------------
def nearest(memo, key, lab, ws, hs):
    from PIL import Image
    k = (key, ws, hs)
    if k not in memo:
        memo[k] = np.asarray(Image.fromarray(lab).resize((ws, hs), Image.NEAREST))
    return memo[k]


def count(memo, key, lab, crop_wh, choice, ox, oy, c):
    """The pixels of class c in the w x h window at (ox, oy) of the NEAREST-resized label; 0 for c == 255 (nothing is counted)."""
    if c == 255:
        return 0
    w, h = crop_wh
    ws, hs = scref.scaled(w, choice), scref.scaled(h, choice)
    Ln = nearest(memo, key, lab, ws, hs)
    ya, yb = max(0, -oy), min(h, hs - oy)
    xa, xb = max(0, -ox), min(w, ws - ox)
    if ya >= yb or xa >= xb:
        return 0
    return int((Ln[ya + oy:yb + oy, xa + ox:xb + ox] == c).sum())


def pick(counts, bar, c):
    """k*: the smallest k with counts[k] > bar, K - 1 when there is none; 0 for class 255."""
    if c == 255:
        return 0
    return next((k for k, n in enumerate(counts) if n > bar), len(counts) - 1)


def windows(memo, keys, labs, crop_wh, choices, cand, cls, bar):
    """cand = (pick [B][K], ox [B][K], oy [B][K]) -> (counts [B][K], k* [B], win [B][4] = (choice index, ox, oy, count))."""
    pk, ox, oy = cand
    counts, ks, win = [], [], []
    for b in range(len(pk)):
        row = [count(memo, keys[b], labs[b], crop_wh, choices[pk[b][k]], ox[b][k], oy[b][k], cls[b]) for k in range(len(pk[b]))]
        k = pick(row, bar, cls[b])
        counts.append(row)
        ks.append(k)
        win.append([pk[b][k], ox[b][k], oy[b][k], row[k]])
    return counts, ks, win
