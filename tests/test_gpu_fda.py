"""simt_fda_transfer (csrc/fda.hip) and simt_amd.data.fda.FdaTransfer on the GPU against the PUBLISHED full-FFT form in float64
(tests/_fda_ref.py).  The bar is  max|gpu - fda_full| <= 4 * err32 + 2^-22 * max|out|,  err32 the error of the restatement's
sequential fp32 arithmetic on the same inputs -- never the kernel's own figure.  Measured gpu error / err32 per geometry: profiles/fda.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _fda_ref as fr
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.data.fda import FdaTransfer, twiddle_tables

pytestmark = pytest.mark.gpu
MEAN = fr.IMG_MEAN
DARK = (1, 40, 56, 0.05, 2, 21)       # a dark source beside a bright target: the only inputs that show a mean that was not added back


@functools.lru_cache(maxsize=None)
def _case(g, dark=False):
    """Computed once per geometry and shared: inputs, the published result, the fp32 restatement's error."""
    B, h, w, _beta, b, seed = g
    xs, xt = fr.inputs(B, h, w, seed, *((0, 100, 100, 256) if dark else ()))
    full = fr.fda_full(xs, xt, MEAN, b)
    err32 = float(np.abs(fr.fda_band(xs, xt, MEAN, b, np.float32) - full).max())
    for a in (xs, xt, full):
        a.setflags(write=False)
    return xs, xt, full, err32


def _gpu(dev, xs, xt, beta, hold=1):
    B, _c, h, w = xs.shape
    f = FdaTransfer(B, h, w, beta, dev, hold=hold)
    ds, dt = torch.from_numpy(np.array(xs)).to(dev), torch.from_numpy(np.array(xt)).to(dev)
    out = f(ds, dt)
    torch.cuda.synchronize()
    return f, ds, dt, out


@pytest.mark.parametrize("g", fr.GEOMETRIES + [DARK], ids=lambda g: fr.geo_id(g) + ("-dark" if g is DARK else ""))
def test_equals_the_published_form(dev, g):
    B, h, w, beta, b, _seed = g
    xs, xt, full, err32 = _case(g, g is DARK)
    if g is not DARK:
        assert fr.kappa(xs, xt, MEAN, b) <= fr.KAPPA_MAX
    f, ds, dt, out = _gpu(dev, xs, xt, beta)
    assert f.b == b
    got = out.cpu().numpy().astype(np.float64)
    err, bar = float(np.abs(got - full).max()), fr.bar(err32, full)
    print(f"fda {fr.geo_id(g)}{' dark' if g is DARK else ''}: gpu error {err:.3e}, err32 {err32:.3e}, ratio {err / err32:.3f}, bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, (err, err32, bar)
    assert np.array_equal(ds.cpu().numpy(), xs) and np.array_equal(dt.cpu().numpy(), xt), "an input was written"


@pytest.mark.parametrize("g", [fr.GEOMETRIES[0], fr.GEOMETRIES[1], fr.GEOMETRIES[4]], ids=fr.geo_id)
def test_target_equal_to_source_changes_nothing(dev, g):
    B, h, w, beta, b, _seed = g
    xs = _case(g)[0]
    err32 = float(np.abs(fr.fda_band(xs, xs, MEAN, b, np.float32) - xs).max())
    _f, _ds, _dt, out = _gpu(dev, xs, xs.copy(), beta)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - xs).max())
    assert err <= fr.bar(err32, xs), (err, err32)


def test_band_zero_moves_the_plane_means(dev):
    g = fr.GEOMETRIES[2]
    B, h, w, beta, b, _seed = g
    assert b == 0
    xs, xt, full, err32 = _case(g)
    _f, _ds, _dt, out = _gpu(dev, xs, xt, beta)
    shift = out.cpu().numpy().astype(np.float64) - xs
    want = (xt.astype(np.float64).mean(axis=(2, 3)) - xs.astype(np.float64).mean(axis=(2, 3)))[:, :, None, None]
    assert np.abs(shift - want).max() <= fr.bar(err32, full)


def test_zero_amplitude_plane_comes_back_bit_for_bit(dev):
    """S = T = 0 on a plane: every coefficient vanishes, p = 1, D = 0 and x_out == xs in every bit, no NaN anywhere."""
    xs, xt = fr.inputs(2, 24, 40, 5)
    m = np.asarray(MEAN, dtype=np.float32)
    xs[0, 1], xt[0, 1] = -m[1], -m[1]
    xs[1, 2], xt[1, 2] = -m[2], -m[2]
    _f, _ds, _dt, out = _gpu(dev, xs, xt, 0.09)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got[0, 1].view(np.uint32), xs[0, 1].view(np.uint32)) and np.array_equal(got[1, 2].view(np.uint32), xs[1, 2].view(np.uint32))
    assert not np.array_equal(got[0, 0], xs[0, 0])


def test_refusals_write_nothing(dev):
    B, h, w, b = 2, 24, 40, 2
    xs, xt = (torch.from_numpy(a).to(dev) for a in fr.inputs(B, h, w, 7))
    poison = torch.full((B * 3 * h * w + 8,), float("nan"), device=dev)
    x_out = poison[:B * 3 * h * w].view(B, 3, h, w)
    tw_h, tw_w = (torch.from_numpy(t).to(dev) for t in twiddle_tables(h, w))
    nbytes = ops.fda_workspace_bytes(B, h, w, b)
    assert nbytes == 8 * (3 * (3 * B * h) * (b + 1) + 3 * B * (2 * b + 1) * (b + 1))
    work = torch.full((nbytes // 4,), float("nan"), device=dev)
    lib = L.load()

    def call(**over):
        d = ops.make_fda_desc(xs, xt, x_out, tw_h, tw_w, work, B=B, h=h, w=w, b=b, mean=MEAN)
        for k, v in over.items():
            setattr(d, k, v)
        return lib.simt_fda_transfer(C.byref(d), ops.stream_ptr())

    cases = [dict(xs=None), dict(xt=None), dict(x_out=None), dict(tw_h=None), dict(tw_w=None), dict(work=None),
             dict(xs=xs.data_ptr() + 4), dict(xt=xt.data_ptr() + 8), dict(x_out=x_out.data_ptr() + 4), dict(work=work.data_ptr() + 8),
             dict(tw_h=tw_h.data_ptr() + 4), dict(tw_w=tw_w.data_ptr() + 4),
             dict(x_out=xs.data_ptr()), dict(x_out=xt.data_ptr()), dict(xs=x_out.data_ptr() + 16), dict(xt=x_out.data_ptr() + 4 * 3 * h * w),
             dict(B=0), dict(B=33), dict(b=-1), dict(b=12), dict(h=0), dict(w=0),
             dict(b=65, h=200, w=200), dict(h=65536, w=32768), dict(h=1 << 20, w=1 << 11)]
    for over in cases:
        assert call(**over) == 1, over                       # SIMT_ERR_INVALID
        assert lib.simt_last_error()
    assert lib.simt_fda_transfer(None, ops.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert torch.isnan(poison).all() and torch.isnan(work).all(), "a refused launch wrote"
    for geo in ((0, h, w, b), (33, h, w, b), (B, h, w, 12), (B, 200, 200, 65), (B, 65536, 32768, 0), (B, h, w, -1)):
        assert ops.fda_workspace_bytes(*geo) == 0
    assert call() == 0                                       # the same descriptor, untouched, launches
    torch.cuda.synchronize()
    assert not torch.isnan(x_out).any() and torch.isnan(poison[B * 3 * h * w:]).all()


def test_ring_and_staging(dev):
    """hold = 2: the buffer handed out stays whole through the next call; a mis-typed or non-contiguous input is staged and gives the
    same bits."""
    g = fr.GEOMETRIES[3]
    B, h, w, beta, b, _seed = g
    xs, xt, _full, _err32 = _case(g)
    f, ds, dt, first = _gpu(dev, xs, xt, beta, hold=2)
    kept = first.clone()
    second = f(dt, ds)
    torch.cuda.synchronize()
    assert second.data_ptr() != first.data_ptr() and torch.equal(first, kept) and not torch.equal(second, first)
    third = f(ds, dt)                                        # the ring comes round: the first buffer again, the same bits
    torch.cuda.synchronize()
    assert third.data_ptr() == first.data_ptr() and torch.equal(third, kept)
    wide = torch.zeros(B, 3, h, w + 3, device=dev)
    wide[..., :w] = ds
    staged = f(wide[..., :w], dt.double())                   # not contiguous | not fp32
    torch.cuda.synchronize()
    assert torch.equal(staged, kept)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    on_side = f(ds, dt, stream=side)
    side.synchronize()
    assert torch.equal(on_side, kept)
    with pytest.raises(ValueError, match="expected"):
        f(ds[:1], dt)
