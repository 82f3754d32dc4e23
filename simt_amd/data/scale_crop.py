"""Random scale + crop (--scale-crop): the host side of csrc/scale_crop.hip -- sizes, draws, tables.  Pure Python / numpy.

For an item with decoded frame Hs x Ws and training crop (w, h): a scale s is drawn from the choices; the frame is resized ONCE, from the
original, to (ws, hs) = (floor(w*s + 1/2), floor(h*s + 1/2)) (BICUBIC; the label NEAREST); the network sees the w x h window of that at
origin (ox, oy), ox uniform over [min(0, ws-w), max(0, ws-w)] (oy likewise): a random crop of a larger frame, a random placement of a
smaller one (0.0 = the mean / label 255 around it).  The choices are DECIMAL TEXT and the sizes exact rational arithmetic on it:
1024 * 0.7 is 716.8 whatever binary float 0.7 happens to be.

Draws come from the loader's generator, per batch, in a fixed order and number (so a resumed loader can skip them without knowing them):
the mirror draw as ever (`integers(0, 2, B)`, only when mirroring is on), then `integers(0, n_choices, B)`, `random(B)` for x, `random(B)`
for y.  With rare-class crops (simt_amd/data/rare_class.py) the last three have shape (B, K): K candidate windows per item, one of which
the device picks.
"""
import math
from fractions import Fraction

import numpy as np

from . import resample as rs

MAX_CHOICES = 16          # include/simt_hip.h SIMT_SCALE_CROP_CHOICES
TILE_H, TILE_W = 16, 64   # SIMT_SCALE_CROP_TILE_H / _W
DEFAULT_CHOICES = ("0.5", "0.6", "0.7", "0.8", "0.9", "1.0", "1.1", "1.2", "1.3", "1.4", "1.5")


def parse_choices(texts):
    """--scale-crop's values -> tuple of decimal strings (no values: DEFAULT_CHOICES).  ValueError names what is wrong."""
    texts = [str(t) for t in texts]
    if not texts:
        return DEFAULT_CHOICES
    if len(texts) > MAX_CHOICES:
        raise ValueError(f"{len(texts)} scale choices, at most {MAX_CHOICES} are allowed")
    for t in texts:
        try:
            ok = Fraction(t) > 0 and "/" not in t
        except (ValueError, ZeroDivisionError):
            ok = False
        if not ok:
            raise ValueError(f"scale choice {t!r} is not a positive decimal number")
    return tuple(texts)


def scaled_size(n, choice):
    """floor(n * s + 1/2), s the decimal text `choice`, exactly."""
    return math.floor(n * Fraction(choice) + Fraction(1, 2))


def origin_range(scaled, crop):
    """-> (lo, hi), inclusive, of the window's origin along one axis: a crop of a larger frame (0 .. scaled - crop) or the placement of
    a smaller one (scaled - crop .. 0: a negative origin puts the frame inside the window)."""
    return min(0, scaled - crop), max(0, scaled - crop)


def origin(u, lo, hi):
    """u in [0, 1) -> uniform integer in [lo, hi]; the clamp keeps a u whose product rounds up to hi - lo + 1 inside."""
    return min(hi, lo + int(math.floor(u * (hi - lo + 1))))


def draw_batch(rng, batch_size, choices, crop_wh, mirror):
    """One batch's draws -> (mirror flags [B] bool, choice index [B], ox [B], oy [B]) as lists."""
    flags = (rng.integers(0, 2, batch_size) == 0).tolist() if mirror else [False] * batch_size
    pick = rng.integers(0, len(choices), batch_size).tolist()
    ux, uy = rng.random(batch_size), rng.random(batch_size)
    w, h = crop_wh
    ox = [origin(float(ux[b]), *origin_range(scaled_size(w, choices[pick[b]]), w)) for b in range(batch_size)]
    oy = [origin(float(uy[b]), *origin_range(scaled_size(h, choices[pick[b]]), h)) for b in range(batch_size)]
    return flags, pick, ox, oy


def draw_batch_candidates(rng, batch_size, n_cand, choices, crop_wh, mirror):
    """One batch's draws with K = n_cand candidate windows per item (rare-class crops, simt_amd/data/rare_class.py) -> (mirror flags [B],
    choice index [B][K], ox [B][K], oy [B][K]) as lists: the mirror draw as ever, then `integers(0, n_choices, (B, K))`, `random((B, K))`
    for x, `random((B, K))` for y."""
    flags = (rng.integers(0, 2, batch_size) == 0).tolist() if mirror else [False] * batch_size
    pick = rng.integers(0, len(choices), (batch_size, n_cand)).tolist()
    ux, uy = rng.random((batch_size, n_cand)), rng.random((batch_size, n_cand))
    w, h = crop_wh
    ox = [[origin(float(ux[b, k]), *origin_range(scaled_size(w, choices[pick[b][k]]), w)) for k in range(n_cand)] for b in range(batch_size)]
    oy = [[origin(float(uy[b, k]), *origin_range(scaled_size(h, choices[pick[b][k]]), h)) for k in range(n_cand)] for b in range(batch_size)]
    return flags, pick, ox, oy


def skip_scale_crop_draws(rng, batch_size, n_batches, n_choices, mirror, candidates=None):
    """Advance the loader's generator by the draws `n_batches` batches make with scale-crop on (skip_mirror_draws' sibling): the
    number of draws does not depend on their values.  candidates = K: the draws of draw_batch_candidates."""
    shape = batch_size if candidates is None else (batch_size, int(candidates))
    for _ in range(n_batches):
        if mirror:
            rng.integers(0, 2, batch_size)
        rng.integers(0, n_choices, shape)
        rng.random(shape)
        rng.random(shape)
    return rng


def tile_row_span(bounds_y, scaled_h, crop_h, tile_h=TILE_H):
    """The most source rows the vertical pass of one output tile reads, over every origin oy of origin_range and every tile: the tile
    of output rows y0 .. y1-1 shows rows a = max(0, y0 + oy) .. e-1, e = min(scaled_h, y1 + oy), of the scaled frame and reads source
    rows bounds[a].lo .. bounds[e-1].lo + n (bounds are monotone).  The kernel restates a and e; its LDS array is sized by this."""
    lo = bounds_y[:, 0].astype(np.int64)
    end = lo + bounds_y[:, 1].astype(np.int64)
    o_lo, o_hi = origin_range(scaled_h, crop_h)
    oy = np.arange(o_lo, o_hi + 1)[:, None]
    y0 = np.arange(0, crop_h, tile_h)[None, :]
    a = np.maximum(0, y0 + oy)
    e = np.minimum(scaled_h, np.minimum(y0 + tile_h, crop_h) + oy)
    shown = a < e
    span = end[np.where(shown, e - 1, 0)] - lo[np.where(shown, a, 0)]
    return int(np.where(shown, span, 0).max())


class Tables:
    """Everything the kernel needs for one (source geometry, crop, choices): one int32 buffer holding, per choice, bicubic bounds and
    coefficients for x and y (resample.bicubic_tables) and the NEAREST index tables, their offsets, and the worst tile row span."""

    def __init__(self, src_hw, crop_wh, choices):
        self.Hs, self.Ws = int(src_hw[0]), int(src_hw[1])
        self.w, self.h = int(crop_wh[0]), int(crop_wh[1])
        self.choices = parse_choices(choices)
        self.entries, parts, off = [], [], 0

        def put(a):
            nonlocal off
            a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
            parts.append(a)
            off += a.size
            return off - a.size

        self.max_rows = 0
        for c in self.choices:
            ws, hs = scaled_size(self.w, c), scaled_size(self.h, c)
            if ws < 1 or hs < 1:
                raise ValueError(f"scale choice {c} leaves nothing of a {self.w} x {self.h} crop")
            ksx, bx, cx = rs.bicubic_tables(self.Ws, ws)
            ksy, by, cy = rs.bicubic_tables(self.Hs, hs)
            self.entries.append({"ws": ws, "hs": hs, "ksx": ksx, "ksy": ksy, "bounds_x": put(bx), "coef_x": put(cx), "bounds_y": put(by),
                                 "coef_y": put(cy), "xtab": put(rs.nearest_table(self.Ws, ws)), "ytab": put(rs.nearest_table(self.Hs, hs))})
            self.max_rows = max(self.max_rows, tile_row_span(by, hs, self.h))
        self.data = np.concatenate(parts)

    def lds_bytes(self):
        """What simt_scale_crop_lds_bytes answers for these tables (restated for hosts without the library)."""
        return self.max_rows * 3 * TILE_W + 4 * (TILE_W * max(e["ksx"] for e in self.entries) + TILE_H * max(e["ksy"] for e in self.entries))
