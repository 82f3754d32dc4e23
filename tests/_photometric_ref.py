"""Colour jitter + Gaussian blur restated in numpy from the contract (include/simt_hip.h): float32 scalars and arrays, slicing,
`np.pad(mode="reflect")`, `np.rint`, integer sums.  numpy rounds every float32 multiply and add on its own, which is what the contract
asks of the device, so the comparison is bit for bit.  The yardstick of tests/test_photometric_cpu.py and tests/test_gpu_photometric.py; it
must not import simt_amd.data.photometric.

x [B,3,h,w] float32 is a finished batch, plane p = colour - mean[p]; per item: jit, blur (bool), fb, fc, omfc (float32), A (float32 [3,3]),
wk (float32 [6]).  `float64_item` is the same formulas carried out in float64 without the 16-bit quantisation of the grey mean: what the
restatement is held to in the CPU test."""
import math

import numpy as np

F = np.float32
TAG = 0x50684D74                      # the documented third word of the photometric generator's seed ("PhMt")
C255 = F(1.0 / 255.0)
WG = (F(0.114), F(0.587), F(0.299))   # planes B, G, R
RADIUS = 5


def generator(seed, rank):
    return np.random.default_rng([seed, rank, TAG])


def draws(rng, B, S, P):
    """The documented draws of one batch: ONE random((7, B)); rows: jitter on (p = 0.8), fb, fc, fs in [1-S, 1+S], theta in [-S, S] turns,
    blur on (p = P), sigma in [0.15, 1.15].  S / P None: that flag is off (its switch is never on; the draws are made all the same)."""
    u = rng.random((7, B))
    s = 0.0 if S is None else S
    lo = 1.0 - s
    return {"jit": (u[0] < 0.8) if S is not None else np.zeros(B, bool),
            "fb": lo + 2.0 * s * u[1], "fc": lo + 2.0 * s * u[2], "fs": lo + 2.0 * s * u[3], "theta": -s + 2.0 * s * u[4],
            "blur": (u[5] < P) if P is not None else np.zeros(B, bool),
            "sigma": 0.15 + u[6]}


# ---- the host's parameters (float64, rounded once) ---------------------------------------------------------------------------------
def hue(theta):
    """The rotation by theta turns about the grey axis in YIQ space, planes B, G, R: grey part + cos . chroma part + sin . quarter turn."""
    yiq = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
    flip = np.eye(3)[::-1]
    quarter = flip @ np.linalg.inv(yiq) @ np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) @ yiq @ flip
    grey = np.outer(np.ones(3), np.array([0.114, 0.587, 0.299]))
    a = 2.0 * math.pi * float(theta)
    return grey + math.cos(a) * (np.eye(3) - grey) + math.sin(a) * quarter


def params(fb, fc, fs, theta, sigma):
    """-> fb, fc, omfc (float32), A float32 [3,3], wk float32 [6]."""
    fb, fc, fs = F(fb), F(fc), float(fs)
    grey = np.outer(np.ones(3), np.array([0.114, 0.587, 0.299]))
    A = (hue(theta) @ (fs * np.eye(3) + (1.0 - fs) * grey)).astype(F)
    k = np.arange(RADIUS + 1, dtype=np.float64)
    e = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    e[e < 2.0 ** -24] = 0.0
    wk = (e / (e[0] + 2.0 * e[1:].sum())).astype(F)
    return fb, fc, F(1.0 - np.float64(fc)), A, wk


# ---- the device's arithmetic -----------------------------------------------------------------------------------------------------------
def clamp(v):
    return np.minimum(np.maximum(v, F(0)), F(1))


def normalise(x, mean):
    """x [3,h,w] float32 -> three planes in [0, 1]."""
    return [clamp((x[p] + F(mean[p])) * C255) for p in range(3)]


def grey_sum(v):
    """S of the contract for the planes v (after brightness): the integer sum of rint(65536 g)."""
    g = (WG[0] * v[0] + WG[1] * v[1]) + WG[2] * v[2]
    assert g.dtype == F
    q = np.rint(g * F(65536)).astype(np.uint64)
    return int(q.sum(dtype=np.uint64))


def grey_mean(S, h, w):
    return F(np.float64(S) * np.float64(1.0 / (65536.0 * h * w)))


def jitter(v, fb, fc, omfc, A):
    """-> (planes, S, m)."""
    h, w = v[0].shape
    v = [clamp(fb * v[p]) for p in range(3)]
    S = grey_sum(v)
    m = grey_mean(S, h, w)
    t = omfc * m
    v = [clamp(fc * v[p] + t) for p in range(3)]
    return [clamp((A[p, 0] * v[0] + A[p, 1] * v[1]) + A[p, 2] * v[2]) for p in range(3)], S, m


def blur_pass(v, wk, axis):
    n = v.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (RADIUS, RADIUS)
    p = np.pad(v, pad, mode="reflect")

    def at(k):                                   # the frame shifted by k along `axis`
        sl = [slice(None), slice(None)]
        sl[axis] = slice(RADIUS + k, RADIUS + k + n)
        return p[tuple(sl)]
    acc = wk[0] * at(0)
    for k in range(1, RADIUS + 1):
        acc = acc + wk[k] * (at(-k) + at(k))
    assert acc.dtype == F
    return acc


def blur(v, wk):
    return [clamp(blur_pass(blur_pass(v[p], wk, 1), wk, 0)) for p in range(3)]


def item(x, mean, jit, do_blur, fb, fc, omfc, A, wk):
    """One item x [3,h,w] float32 -> (x_out float32 [3,h,w], S | None, m | None)."""
    assert x.dtype == F
    if not jit and not do_blur:
        return x.copy(), None, None
    v = normalise(x, mean)
    S = m = None
    if jit:
        v, S, m = jitter(v, F(fb), F(fc), F(omfc), np.asarray(A, F))
    if do_blur:
        v = blur(v, np.asarray(wk, F))
    out = np.stack([v[p] * F(255) - F(mean[p]) for p in range(3)])
    assert out.dtype == F
    return out, S, m


def batch(x_bits, mean, d):
    """x_bits [B,3,h,w] int32 (the float32 words) and the draws `d` of `draws` -> the output's words, int32."""
    out = np.empty_like(x_bits)
    for i in range(x_bits.shape[0]):
        fb, fc, omfc, A, wk = params(d["fb"][i], d["fc"][i], d["fs"][i], d["theta"][i], d["sigma"][i])
        o, _S, _m = item(x_bits[i].view(F), mean, bool(d["jit"][i]), bool(d["blur"][i]), fb, fc, omfc, A, wk)
        out[i] = o.view(np.int32)
    return out


# ---- the same formulas in float64, the grey mean unquantised ---------------------------------------------------------------------------------
def float64_item(x, mean, jit, do_blur, fb, fc, omfc, A, wk):
    D = np.float64
    c = lambda t: np.minimum(np.maximum(t, 0.0), 1.0)
    v = [c((x[p].astype(D) + D(F(mean[p]))) * D(C255)) for p in range(3)]
    if jit:
        v = [c(D(fb) * v[p]) for p in range(3)]
        m = ((D(WG[0]) * v[0] + D(WG[1]) * v[1]) + D(WG[2]) * v[2]).mean()
        v = [c(D(fc) * v[p] + D(omfc) * m) for p in range(3)]
        A = np.asarray(A, D)
        v = [c((A[p, 0] * v[0] + A[p, 1] * v[1]) + A[p, 2] * v[2]) for p in range(3)]
    if do_blur:
        wk = np.asarray(wk, D)
        for p in range(3):
            t = v[p]
            for axis in (1, 0):
                n = t.shape[axis]
                pad = [(0, 0), (0, 0)]
                pad[axis] = (RADIUS, RADIUS)
                q = np.pad(t, pad, mode="reflect")
                t = sum(wk[abs(k)] * np.take(q, np.arange(RADIUS + k, RADIUS + k + n), axis=axis) for k in range(-RADIUS, RADIUS + 1))
            v[p] = c(t)
    return np.stack([v[p] * 255.0 - D(F(mean[p])) for p in range(3)])
