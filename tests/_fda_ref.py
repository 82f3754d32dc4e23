"""numpy restatement of the FDA contract (include/simt_hip.h; simt_fda_transfer in csrc/fda.hip).  Our own code, numpy only.

  fda_full   the PUBLISHED form (Yang & Soatto, CVPR'20) in float64: fft2, fftshift, replace the centre square of the amplitude, ifftshift,
             ifft2, real part.
  fda_band   the contract: only the (2b+1)^2 lowest frequencies are computed, from the two twiddle tables indexed by the integer
             (v y) mod w and (u x) mod h.  With dtype=np.float32 the tables are the contract's fp32 tables, every sum is a sequential fp32
             accumulation and every product is rounded on its own: the yardstick of the GPU tests' bar.  With dtype=np.float64 the tables
             keep their float64 values (fp32 tables alone are 1e-6 grey levels away from the full transform): the identity itself.
             `fault` plants one of the mistakes the comparator must reject.
  kappa      max over the band and the planes of |F_T| / |F_S| in float64: the conditioning of the inputs (the phase of a vanishing source
             coefficient says nothing about a kernel).
"""
import numpy as np

IMG_MEAN = (104.00698793, 116.66876762, 122.67891434)
FACTOR = 4.0              # the bar: max|gpu - fda_full| <= FACTOR * err32 + REL * max|out|
REL = 2.0 ** -22

# (B, h, w, beta, b, seed): the GPU test's geometries; the seeds are checked for kappa <= KAPPA_MAX in tests/test_fda_cpu.py
GEOMETRIES = [(1, 40, 56, 0.05, 2, 11),
              (2, 33, 47, 0.1, 3, 12),        # odd sizes, the scalar flavour, v y wraps
              (3, 64, 64, 0.01, 0, 13),       # DC only
              (2, 24, 40, 0.09, 2, 14),
              (1, 9, 516, 0.2, 1, 15),        # a row longer than 256 lanes x 1; 2b + 1 close to h
              (1, 130, 136, 0.49, 63, 110),    # the largest band: E and D at their biggest
              (32, 8, 12, 0.13, 1, 17)]       # B at its limit
KAPPA_MAX = 100.0
FAULTS = ("band_minus_1", "drop_coeff", "weight_1", "conj_synthesis", "no_mean")


def geo_id(g):
    return "B{}-{}x{}-b{}".format(g[0], g[1], g[2], g[4])


def inputs(B, h, w, seed, lo_s=0, hi_s=256, lo_t=0, hi_t=256, mean=IMG_MEAN):
    """-> (xs, xt) float32 [B, 3, h, w]: integer grey levels uniform in [lo, hi) minus the mean, as a loader hands them out."""
    g = np.random.default_rng(seed)
    m = np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)
    xs = g.integers(lo_s, hi_s, (B, 3, h, w)).astype(np.float32) - m
    xt = g.integers(lo_t, hi_t, (B, 3, h, w)).astype(np.float32) - m
    return xs, xt


def tables(h, w, dtype=np.float32):
    """(tw_h [h, 2], tw_w [w, 2]): (cos, sin)(2 pi k / n) in float64, rounded once to `dtype` -- float32 is the contract's pair of tables."""
    def table(n):
        a = 2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n)
        return np.stack([np.cos(a), np.sin(a)], axis=1).astype(dtype)
    return table(h), table(w)


def _mean64(mean):
    return np.asarray(mean, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)      # the descriptor carries the mean as fp32


def fda_full(xs, xt, mean, b):
    """The published form in float64 -> x_out [B, 3, h, w] float64 (colour - mean, not clipped)."""
    m = _mean64(mean)
    h, w = xs.shape[-2:]
    fs = np.fft.fftshift(np.fft.fft2(xs.astype(np.float64) + m, axes=(-2, -1)), axes=(-2, -1))
    ft = np.fft.fftshift(np.fft.fft2(xt.astype(np.float64) + m, axes=(-2, -1)), axes=(-2, -1))
    amp, pha = np.abs(fs), np.angle(fs)
    ch, cw = h // 2, w // 2
    amp[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = np.abs(ft)[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    out = np.fft.ifft2(np.fft.ifftshift(amp * np.exp(1j * pha), axes=(-2, -1)), axes=(-2, -1))
    return out.real - m


def kappa(xs, xt, mean, b):
    m = _mean64(mean)
    h, w = xs.shape[-2:]
    u = np.arange(-b, b + 1) % h
    v = np.arange(-b, b + 1) % w
    fs = np.fft.fft2(xs.astype(np.float64) + m, axes=(-2, -1))[..., u[:, None], v[None, :]]
    ft = np.fft.fft2(xt.astype(np.float64) + m, axes=(-2, -1))[..., u[:, None], v[None, :]]
    return float((np.abs(ft) / np.abs(fs)).max())


def _seq_sum(a, dtype):
    """The sum over the last axis, accumulated sequentially in `dtype`."""
    return np.cumsum(a, axis=-1, dtype=dtype)[..., -1]


def fda_band(xs, xt, mean, b, dtype=np.float64, fault=None):
    """The contract -> x_out [B, 3, h, w] of `dtype`.  fault: None or one of FAULTS."""
    assert fault is None or fault in FAULTS
    if fault == "band_minus_1":
        return fda_band(xs, xt, mean, b - 1, dtype)
    dt = np.dtype(dtype).type
    h, w = xs.shape[-2:]
    tw_h, tw_w = tables(h, w, dt)
    m = np.asarray(mean, dtype=np.float32).astype(dt).reshape(1, 3, 1, 1)
    if fault == "no_mean":
        m = m * dt(0)
    vv, uu = np.arange(b + 1), np.arange(-b, b + 1) % h
    iw = (vv[:, None] * np.arange(w)[None, :]) % w                       # [nv, w]: (v y) mod w
    ih = (uu[:, None].astype(np.int64) * np.arange(h)[None, :]) % h      # [nu, h]: (u x) mod h
    cw_, sw_ = tw_w[iw, 0].astype(dt), tw_w[iw, 1].astype(dt)
    ch_, sh_ = tw_h[ih, 0].astype(dt), tw_h[ih, 1].astype(dt)

    def coefficients(x):
        V = x.astype(dt) + m                                                                  # [B, 3, h, w]
        gr = _seq_sum(V[..., :, None, :] * cw_, dt)                                           # [B, 3, h, nv]: the row pass
        gi = _seq_sum(-(V[..., :, None, :] * sw_), dt)
        grt, git = np.swapaxes(gr, -1, -2)[..., None, :, :], np.swapaxes(gi, -1, -2)[..., None, :, :]      # [B, 3, 1, nv, h]
        c, s = ch_[:, None, :], sh_[:, None, :]                                               # [nu, 1, h]
        return _seq_sum(grt * c + git * s, dt), _seq_sum(git * c - grt * s, dt)               # [B, 3, nu, nv]: the column pass

    sr, si = coefficients(xs)
    tr, ti = coefficients(xt)
    a_s, a_t = np.sqrt(sr * sr + si * si), np.sqrt(tr * tr + ti * ti)
    nz = a_s > 0
    safe = np.where(nz, a_s, dt(1))
    pr, pi = np.where(nz, sr / safe, dt(1)), np.where(nz, si / safe, dt(0))
    dr, di = a_t * pr - sr, a_t * pi - si                                                     # D [B, 3, nu, nv]
    if fault == "drop_coeff":
        dr[..., 0, b], di[..., 0, b] = 0, 0                                                   # (u, v) = (-b, b)
    sgn = dt(-1) if fault == "conj_synthesis" else dt(1)
    # column synthesis: E[x][v] = sum_u D(u, v) e^{+2 pi i u x / h}
    drt, dit = np.moveaxis(dr, -2, -1)[..., None, :, :], np.moveaxis(di, -2, -1)[..., None, :, :]          # [B, 3, 1, nv, nu]
    c, s = ch_.T[:, None, :], sgn * sh_.T[:, None, :]                                         # [h, 1, nu]
    er, ei = _seq_sum(drt * c - dit * s, dt), _seq_sum(drt * s + dit * c, dt)                 # [B, 3, h, nv]
    wt = np.full(b + 1, 1 if fault == "weight_1" else 2, dtype=dt)
    wt[0] = 1
    c, s = cw_.T, sgn * sw_.T                                                                 # [w, nv]
    poly = _seq_sum(wt * (er[..., :, None, :] * c - ei[..., :, None, :] * s), dt)             # [B, 3, h, w]
    return xs.astype(dt) + dt(1.0 / (h * w)) * poly


def bar(err32, out):
    return FACTOR * err32 + REL * float(np.abs(out).max())
