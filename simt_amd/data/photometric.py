"""Photometric augmentation (--colour-jitter, --gaussian-blur): the host side of csrc/photometric.hip -- the flags' validation, the draws
and the per-item parameters of the arithmetic contract (include/simt_hip.h).  Pure Python / numpy.

The strong augmentation of the self-training recipes built on ClassMix (DACS, DAFormer): colour jitter (brightness, contrast, saturation,
hue, in this fixed order) with probability 0.8, then a Gaussian blur with probability P, on the finished -- mixed -- batch.  Labels are not
touched.  The device works in float32 with every operation rounded on its own; what the host hands it is computed in float64 and rounded
once: fb, fc, omfc = 1 - fc, the saturation-and-hue matrix A and the six blur weights wk.

Draws come from a generator OF THEIR OWN, `generator(seed, rank)`: turning a flag on moves no mirror, scale-crop or class-mix draw.  Per
batch ONE `random((7, B))`, whatever the settings and the values (so a resumed loader can skip them without knowing them); its rows, in
order: jitter on, fb, fc, fs, theta, blur on, sigma.
"""
import math

import numpy as np

MAX_ITEMS = 32            # include/simt_hip.h SIMT_PHOTOMETRIC_MAX: items per launch (a larger batch is split)
RADIUS = 5                # the blur's: six weights wk[0..5]
STREAM_TAG = 0x50684D74   # "PhMt": the third word of the generator's seed sequence
JITTER_PROB = 0.8
SIGMA_MIN = 0.15          # sigma = SIGMA_MIN + u: uniform in [0.15, 1.15]
WEIGHT_FLOOR = 2.0 ** -24
DEFAULT_JITTER, DEFAULT_BLUR = "0.2", "0.5"       # --colour-jitter / --gaussian-blur without a value

WG = np.array([0.114, 0.587, 0.299])              # grey weights of the planes B, G, R
# RGB -> YIQ (NTSC); the I and Q rows sum to zero, so grey is the Y axis
_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
_FLIP = np.eye(3)[::-1]                            # RGB <-> BGR
# the quarter turn about the grey axis in YIQ space, in the plane order B, G, R: I -> Q, Q -> -I, Y -> 0
_QUARTER = _FLIP @ np.linalg.inv(_YIQ) @ np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) @ _YIQ @ _FLIP
_GREY = np.outer(np.ones(3), WG)                   # v -> grey(v) . (1, 1, 1)


def generator(seed, rank):
    """The photometric draws' own generator of data-parallel rank `rank`."""
    return np.random.default_rng([int(seed), int(rank), STREAM_TAG])


def _number(flag, value, what):
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{flag} {value!r} is not {what}") from None


def parse(colour_jitter=None, gaussian_blur=None):
    """The two flags' values (None: the flag is off) -> settings (S | None, P | None), or None when both are off.  ValueError names what
    is wrong."""
    S = P = None
    if colour_jitter is not None:
        S = _number("--colour-jitter", colour_jitter, "a strength")
        if not 0.0 < S <= 0.5:            # (a NaN fails both comparisons)
            raise ValueError(f"--colour-jitter {colour_jitter!r}: the strength must lie in (0, 0.5]")
    if gaussian_blur is not None:
        P = _number("--gaussian-blur", gaussian_blur, "a probability")
        if not 0.0 < P <= 1.0:
            raise ValueError(f"--gaussian-blur {gaussian_blur!r}: the probability must lie in (0, 1]")
    return None if S is None and P is None else (S, P)


def draw_batch(rng, batch_size, settings):
    """One batch's draws -> dict of [B] arrays: jit, blur (bool) and fb, fc, fs, theta (turns), sigma (float64)."""
    S, P = settings
    u = rng.random((7, batch_size))
    s = 0.0 if S is None else S
    return {"jit": (u[0] < JITTER_PROB) & (S is not None),
            "fb": (1.0 - s) + 2.0 * s * u[1], "fc": (1.0 - s) + 2.0 * s * u[2], "fs": (1.0 - s) + 2.0 * s * u[3],
            "theta": -s + 2.0 * s * u[4],
            "blur": (u[5] < (0.0 if P is None else P)),
            "sigma": SIGMA_MIN + u[6]}


def skip_draws(rng, batch_size, n_batches):
    """Advance the generator by the draws of `n_batches` batches: their number depends neither on their values nor on the settings."""
    for _ in range(n_batches):
        rng.random((7, batch_size))
    return rng


def hue_matrix(theta):
    """H(theta), float64 [3,3]: the rotation by `theta` turns about the grey axis in YIQ space, in the plane order B, G, R.  Written as
    grey + cos . (1 - grey) + sin . quarter turn, so that theta = 0 gives the identity exactly."""
    a = 2.0 * math.pi * float(theta)
    return _GREY + math.cos(a) * (np.eye(3) - _GREY) + math.sin(a) * _QUARTER


def colour_matrix(fs, theta):
    """A = H(theta) . (fs . I + (1 - fs) . 1 . wg^T) in float64, rounded once to float32 [3,3]."""
    fs = float(fs)
    return (hue_matrix(theta) @ (fs * np.eye(3) + (1.0 - fs) * _GREY)).astype(np.float32)


def blur_weights(sigma):
    """wk[0..5] float32: exp(-k^2 / 2 sigma^2) in float64, anything below 2^-24 set to exactly 0, normalised to wk0 + 2 sum wk[k] = 1,
    rounded once."""
    k = np.arange(RADIUS + 1, dtype=np.float64)
    e = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    e[e < WEIGHT_FLOOR] = 0.0
    return (e / (e[0] + 2.0 * e[1:].sum())).astype(np.float32)


def item_params(fb, fc, fs, theta, sigma):
    """One item's draws -> (fb, fc, omfc float32 scalars, A float32 [3,3], wk float32 [6]) exactly as the contract says: fb and fc rounded
    to float32, omfc = float32(1 - fc) of the ROUNDED fc."""
    fb, fc = np.float32(fb), np.float32(fc)
    return fb, fc, np.float32(1.0 - np.float64(fc)), colour_matrix(fs, theta), blur_weights(sigma)


def inv_pixels(h, w):
    """inv of the contract: float64(1 / (65536 . h . w))."""
    return 1.0 / (65536.0 * float(h) * float(w))
