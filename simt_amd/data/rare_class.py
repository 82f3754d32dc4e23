"""Rare-class sampling (--rare-class-sampling; Hoyer et al., DAFormer, CVPR'22, section 3.3): the host side -- statistics, the sampler's
probabilities and draws, the flag's validation.  Pure Python / numpy.  The device side is csrc/rare_crop.hip.

Which frame.  With f_c the share of class c among all counted pixels of the source set, a class is drawn with probability
softmax((1 - f) / T) over the classes that some frame holds with at least `min_pixels` pixels, then a frame uniformly among those frames.
Which window (only with scale-crop).  K candidate windows are drawn per item; the first that shows more than
min_count = floor(min_pixels * min_crop_ratio) pixels of the class is taken, the last one when none does (counted, picked and cropped on
the device: InputPrep.rare_crop_batch).

The statistics file is simt_amd.tools.compute_class_stats' JSON: per frame of the list, the pixel count of every class of the FULL-SIZE label.

Draws come from a generator OF THEIR OWN, `generator(seed, rank)`: per batch exactly `random(B)` for the classes, then `random(B)` for the
frames, so a resumed loader can skip them without knowing them.
"""
import json
import math
from fractions import Fraction

import numpy as np

MAX_CANDS = 16            # include/simt_hip.h SIMT_RARE_CROP_CANDS
STREAM_TAG = 0x52435331   # "RCS1": the third word of the generator's seed sequence


def generator(seed, rank):
    """The sampler's own generator of data-parallel rank `rank`."""
    return np.random.default_rng([int(seed), int(rank), STREAM_TAG])


def load_stats(path, dataset):
    """The statistics file -> counts int64 [items, n_classes], refused unless its names are exactly the dataset's list, in order."""
    with open(path) as f:
        doc = json.load(f)
    names = [it["name"] for it in doc["items"]]
    want = [f["name"] for f in dataset.files]
    for i, (a, b) in enumerate(zip(names, want)):
        if a != b:
            raise ValueError(f"{path}: item {i} is {a!r}, the dataset's list has {b!r} there (the statistics belong to another list)")
    if len(names) != len(want):
        raise ValueError(f"{path}: {len(names)} items, the dataset's list has {len(want)} (first difference at item {min(len(names), len(want))})")
    C = int(doc["n_classes"])
    counts = np.asarray([it["counts"] for it in doc["items"]], dtype=np.int64).reshape(len(names), -1)
    if counts.shape[1] != C or (counts < 0).any():
        raise ValueError(f"{path}: every item needs {C} non-negative counts")
    return counts


def class_probs(counts, T, min_pixels):
    """-> P float64 [C]: 0 for a class no item holds with >= min_pixels pixels, softmax((1 - f) / T) over the others."""
    counts = np.asarray(counts, dtype=np.int64)
    T = float(T)
    if not T > 0.0 or not math.isfinite(T):
        raise ValueError(f"rare-class sampling: the temperature {T!r} must be positive")
    total = counts.sum(dtype=np.int64)
    ok = (counts >= int(min_pixels)).any(axis=0)
    if total <= 0 or not ok.any():
        raise ValueError(f"rare-class sampling: no class has a frame with at least {min_pixels} pixels of it")
    f = counts.sum(axis=0).astype(np.float64) / np.float64(total)
    z = (1.0 - f) / T
    e = np.where(ok, np.exp(z - z[ok].max()), 0.0)
    return e / e.sum()


def items_with_class(counts, min_pixels):
    """-> per class, the ascending int64 array of the items that hold at least min_pixels pixels of it."""
    counts = np.asarray(counts, dtype=np.int64)
    return [np.flatnonzero(counts[:, c] >= min_pixels) for c in range(counts.shape[1])]


def draw_batch(rng, batch_size, cdf, lists):
    """One batch's draws -> (cls [B], index [B]) as lists.  cls[b]: the first class whose cumulative probability exceeds u_c[b], clamped
    to the last class that qualifies; index[b] = lists[cls][min(n - 1, floor(u_i[b] * n))]."""
    uc, ui = rng.random(batch_size), rng.random(batch_size)
    last = int(np.flatnonzero(np.diff(cdf, prepend=0.0) > 0.0)[-1])
    cls = np.minimum(np.searchsorted(cdf, uc, side="right"), last).tolist()
    index = []
    for b, c in enumerate(cls):
        n = len(lists[c])
        index.append(int(lists[c][min(n - 1, int(math.floor(float(ui[b]) * n)))]))
    return cls, index


def skip_draws(rng, batch_size, n_batches):
    """Advance the generator by the draws of `n_batches` batches: their number does not depend on their values."""
    for _ in range(n_batches):
        rng.random(batch_size)
        rng.random(batch_size)
    return rng


def _decimal(text, what):
    text = str(text)
    try:
        v = Fraction(text)
        ok = "/" not in text
    except (ValueError, ZeroDivisionError):
        ok = False
    if not ok:
        raise ValueError(f"{what} {text!r} is not a decimal number")
    return v


def parse(T, min_pixels, min_crop_ratio, K):
    """The flags' values -> (T float, min_pixels int, ratio decimal text, K int, min_count int).  min_count = floor(min_pixels * ratio),
    exactly (the ratio is DECIMAL TEXT: 3000 * 0.7 is 2100 whatever binary float 0.7 happens to be).  ValueError names what is wrong."""
    try:
        t = float(T)
    except (TypeError, ValueError):
        raise ValueError(f"--rare-class-sampling {T!r} is not a temperature") from None
    if not t > 0.0 or not math.isfinite(t):
        raise ValueError(f"--rare-class-sampling {T!r}: the temperature must be positive")
    mp = _decimal(min_pixels, "--rcs-min-pixels")
    if mp < 0 or mp.denominator != 1:
        raise ValueError(f"--rcs-min-pixels {min_pixels!r}: a number of pixels, 0 or more")
    r = _decimal(min_crop_ratio, "--rcs-min-crop-ratio")
    if not 0 <= r <= 1:
        raise ValueError(f"--rcs-min-crop-ratio {min_crop_ratio!r}: the ratio must lie in [0, 1]")
    try:
        k = int(K)
    except (TypeError, ValueError):
        raise ValueError(f"--rcs-crops {K!r} is not a number of crops") from None
    if not 1 <= k <= MAX_CANDS:
        raise ValueError(f"--rcs-crops {K!r}: 1 to {MAX_CANDS} candidate crops")
    return t, int(mp), str(min_crop_ratio), k, int(math.floor(mp * r))


class RareClass:
    """What GTA5DataSet(rare_class=...) carries: the statistics (counts [items, C]) and the validated settings, with everything the
    loader draws from -- the class probabilities, their cumulative sum and the frames of every class."""

    def __init__(self, stats, T=0.01, min_pixels=3000, min_crop_ratio="0.5", K=10):
        self.T, self.min_pixels, self.min_crop_ratio, self.K, self.min_count = parse(T, min_pixels, min_crop_ratio, K)
        self.counts = np.asarray(stats, dtype=np.int64)
        if self.counts.ndim != 2:
            raise ValueError("rare-class statistics: counts [items, classes] expected")
        self.probs = class_probs(self.counts, self.T, self.min_pixels)
        self.cdf = np.cumsum(self.probs)
        self.lists = items_with_class(self.counts, self.min_pixels)
