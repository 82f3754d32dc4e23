"""FDA, Fourier low-band style transfer of the source batch (--fda): the host side of csrc/fda.hip -- the flag's validation, the band, the
twiddle tables and `FdaTransfer`, the stage between the two loaders and the trainer's step (include/simt_hip.h).

Fourier Domain Adaptation (Yang & Soatto, CVPR'20) replaces the low-frequency amplitude of each source image's spectrum with that of a target
image and keeps the source phase, so the source labels stay valid; the model trains on the result.  Only the (2b+1)^2 lowest frequencies
change, b = floor(min(h, w) * beta), so the device adds a band-limited trigonometric polynomial to the source batch: no FFT, no complex image.
There are no random draws: source item i takes the style of target item i of the same step.
"""
import math

import numpy as np

MAX_ITEMS = 32            # include/simt_hip.h SIMT_FDA_MAX_ITEMS
MAX_BAND = 64             # SIMT_FDA_MAX_BAND
DEFAULT_BETA = "0.01"     # --fda without a value: the paper's smallest beta


def band(h, w, beta):
    """b = floor(min(h, w) * beta): the half width of the swapped square of frequencies."""
    return int(math.floor(min(int(h), int(w)) * float(beta)))


def parse(beta, crop_wh):
    """--fda's value and the crop (w, h) -> (beta, b).  ValueError names what is wrong."""
    try:
        v = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"--fda {beta!r} is not a share of the spectrum") from None
    if not 0.0 < v < 1.0:                 # (a NaN fails both comparisons)
        raise ValueError(f"--fda {beta!r}: beta must lie in (0, 1)")
    w, h = int(crop_wh[0]), int(crop_wh[1])
    b = band(h, w, v)
    if 2 * b + 1 > min(h, w):
        raise ValueError(f"--fda {beta!r}: a band of {2 * b + 1} x {2 * b + 1} frequencies does not fit a crop of {w} x {h}")
    if b > MAX_BAND:
        raise ValueError(f"--fda {beta!r}: b = {b} at a crop of {w} x {h}, the launch holds b <= {MAX_BAND}: "
                         f"a beta below {(MAX_BAND + 1) / min(h, w):.4f} would fit")
    return v, b


def twiddle_tables(h, w):
    """-> (tw_h [h, 2], tw_w [w, 2]) float32: (cos, sin)(2 pi k / n), computed in float64 and rounded once.  The device indexes them by the
    integer (u x) mod h and (v y) mod w."""
    def table(n):
        a = 2.0 * np.pi * np.arange(int(n), dtype=np.float64) / float(n)
        return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    return table(h), table(w)


class FdaTransfer:
    """xs, xt [B, 3, h, w] on `device` -> x_out, the source batch with the target batch's low-band amplitudes: four launches
    (simt_fda_transfer) on the given or the current stream, nothing read back.  It owns the two tables, the workspace and a ring of `hold`
    output buffers -- the `iter_size` of a loop that keeps that many micro-batches alive per step, as GpuLoader(hold=): the tensor handed
    out stays whole until `hold` further calls.  A non-contiguous, mis-typed or misaligned input is staged once in a buffer of its own."""

    def __init__(self, B, h, w, beta, device, mean=None, hold=1):
        import torch
        from .. import ops
        from .pipeline import IMG_MEAN
        self.B, self.h, self.w = int(B), int(h), int(w)
        self.beta, self.b = parse(beta, (w, h))
        if not 1 <= self.B <= MAX_ITEMS:
            raise ValueError(f"a batch of {B} items: one launch takes 1 to {MAX_ITEMS}")
        self.mean = tuple(float(m) for m in (IMG_MEAN if mean is None else mean))
        self.device = torch.device(device)
        nbytes = ops.fda_workspace_bytes(self.B, self.h, self.w, self.b)
        if nbytes <= 0:
            raise ValueError(f"a batch of {B} x 3 x {h} x {w} with b = {self.b} is a geometry the launch refuses")
        tw_h, tw_w = twiddle_tables(self.h, self.w)
        self.tw_h, self.tw_w = torch.from_numpy(tw_h).to(self.device), torch.from_numpy(tw_w).to(self.device)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        shape = (self.B, 3, self.h, self.w)
        self.ring = [torch.empty(shape, dtype=torch.float32, device=self.device) for _ in range(max(1, int(hold)))]
        self._next = 0
        self._stage = [None, None]

    def _input(self, x, k):
        import torch
        if tuple(x.shape) != (self.B, 3, self.h, self.w):
            raise ValueError(f"image of shape {tuple(x.shape)}, expected {(self.B, 3, self.h, self.w)}")
        if x.device == self.device and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0:
            return x
        if self._stage[k] is None:
            self._stage[k] = torch.empty_like(self.ring[0])
        self._stage[k].copy_(x, non_blocking=True)
        return self._stage[k]

    def __call__(self, xs, xt, stream=None):
        import torch
        from .. import ops
        with torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream):
            xs, xt = self._input(xs, 0), self._input(xt, 1)
            out = self.ring[self._next]
            self._next = (self._next + 1) % len(self.ring)
            d = ops.make_fda_desc(xs, xt, out, self.tw_h, self.tw_w, self.work, B=self.B, h=self.h, w=self.w, b=self.b, mean=self.mean)
            ops.fda_transfer(d, torch.cuda.current_stream(self.device).cuda_stream)
        return out
