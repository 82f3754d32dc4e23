"""Class-balanced online labels on the GPU (simt_online_label_cb / simt_class_thresholds in csrc/label_sweep.hip, simt_amd/online_labels.py,
DESIGN 7.17).  Every comparison is between two executions of the same arithmetic, or between integers, and therefore BITWISE.

  (a) the label kernel against the composition of existing launches: simt_pseudo_conf_u8 / simt_pseudo_conf2_u8 (hia = H, wia = W) with out +
      counts + hist in one call and the thresholds handed over from host memory; `out` widened to int64;
  (b) the threshold kernel against `balanced_update` (numpy): thr, t_out, the zeroed histogram;
  (c) a trainer with the keyword against a trainer WITHOUT online_labels, fed the labels the test makes from a separate eval-mode plan with the
      existing launches and `balanced_update` on the host;
  (d) the keyword off: the launches and the labels of online_labels alone.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_online_labels as O
import test_gpu_resume as R
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from simt_amd.ema_teacher import refresh_due
from simt_amd.online_labels import balanced_update
from test_gpu_online_labels import GARBAGE, GEOMETRIES, GUARD, SIZE, Composition, _input, _trainer, _views
from test_gpu_step_coherence import one_rank_group
from test_online_labels_cb_cpu import CRAFTED

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
BINS = L.CONF_BINS
# class 1 -- the winner of _input's tie band -- gets -1 (everything kept); the classes behind it 0.5, 0.968, 1.0, NaN, -1, ...
THR_VALUES = [float("nan"), -1.0, 0.5, 0.968, 1.0]
FGUARD = 16                      # floats on either side of the device thresholds


def _thr_vector(Cn):
    return np.array([THR_VALUES[c % 5] for c in range(Cn)], np.float32)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ---- (a) the label kernel ----------------------------------------------------------------------------------------------------------------------------
def _cb_desc(view, label, counts, hist, thr, family, B, h, w, ld, H, W, Cn):
    d = L.OnlineLabelCbDesc()
    d.fix, d.label, d.counts, d.hist, d.thr = view.data_ptr(), label.data_ptr(), counts.data_ptr(), hist.data_ptr(), thr.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family = B, h, w, ld, H, W, Cn, family
    return d


def _conf_yardstick(view, family, B, h, w, ld, H, W, Cn, thr_host, dev):
    """The existing launches: out + counts + hist in ONE call, thresholds from host memory."""
    out = torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
    hist = torch.zeros(Cn, BINS, dtype=torch.int64, device=dev)
    thr_host = np.ascontiguousarray(thr_host, dtype=np.float32)
    if family == 0:
        L.call("simt_pseudo_conf_u8", ops._p(view), h, w, ld, B, H, W, Cn, thr_host.ctypes.data, ops._p(out), ops._p(cnt), ops._p(hist),
               ops.stream_ptr())
    else:
        L.call("simt_pseudo_conf2_u8", ops._p(view), h, w, ld, H, W, B, H, W, Cn, thr_host.ctypes.data, ops._p(out), ops._p(cnt), ops._p(hist),
               ops.stream_ptr())
    torch.cuda.synchronize()
    return out, cnt, hist


_LABEL_HISTS = {}          # geometry -> the yardstick's histogram (host): inputs of the threshold-kernel tests


def _label_hist(dev, geo=GEOMETRIES[0]):
    if geo not in _LABEL_HISTS:
        family, B, h, w, H, W, Cn, ld = geo
        _buf, view = _input(family, B, h, w, Cn, ld, dev, seed=sum(geo))
        _LABEL_HISTS[geo] = _conf_yardstick(view, family, B, h, w, ld, H, W, Cn, _thr_vector(Cn), dev)[2].cpu().numpy()
    return _LABEL_HISTS[geo]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "fam{}-{}x{}x{}to{}x{}-C{}-ld{}".format(*g))
def test_label_kernel_equals_the_composition_of_existing_launches(dev, geo):
    family, B, h, w, H, W, Cn, ld = geo
    buf, view = _input(family, B, h, w, Cn, ld, dev, seed=sum(geo))
    before = buf.clone()
    P = B * H * W
    thr_host = _thr_vector(Cn)
    out, cnt, hist = _conf_yardstick(view, family, B, h, w, ld, H, W, Cn, thr_host, dev)
    _LABEL_HISTS.setdefault(geo, hist.cpu().numpy())
    lab = torch.full((2 * GUARD + P,), GARBAGE, dtype=torch.int64, device=dev)
    counts = torch.zeros(GUARD + Cn + 1 + GUARD, dtype=torch.int64, device=dev)
    hbuf = torch.zeros(GUARD + Cn * BINS + GUARD, dtype=torch.int64, device=dev)
    tbuf = torch.full((2 * FGUARD + Cn,), -3.0, device=dev)
    tbuf[FGUARD:FGUARD + Cn] = torch.from_numpy(thr_host)
    tbefore = tbuf.clone()
    d = _cb_desc(view, lab[GUARD:], counts[GUARD:], hbuf[GUARD:], tbuf[FGUARD:], family, B, h, w, ld, H, W, Cn)
    L.call("simt_online_label_cb", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    got = lab[GUARD:GUARD + P].view(B, H, W)
    got_counts, got_hist = counts[GUARD:GUARD + Cn + 1], hbuf[GUARD:GUARD + Cn * BINS].view(Cn, BINS)
    assert torch.equal(got, out.long()), f"{int((got != out.long()).sum())} of {P} labels differ"
    assert torch.equal(got_counts, cnt) and int(got_counts.sum()) == P, (got_counts.tolist(), cnt.tolist())
    assert torch.equal(got_hist, hist) and int(got_hist.sum()) == P
    assert bool((lab[:GUARD] == GARBAGE).all()) and bool((lab[GUARD + P:] == GARBAGE).all()), "guard words of the labels written"
    assert int(counts[:GUARD].abs().sum()) == 0 and int(counts[GUARD + Cn + 1:].abs().sum()) == 0, "guard words of the counts written"
    assert int(hbuf[:GUARD].abs().sum()) == 0 and int(hbuf[GUARD + Cn * BINS:].abs().sum()) == 0, "guard words of the histogram written"
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the input was written"
    assert torch.equal(tbuf.view(torch.int32), tbefore.view(torch.int32)), "the thresholds were written"
    L.call("simt_online_label_cb", C.byref(d), ops.stream_ptr())          # counts and hist accumulate across calls
    torch.cuda.synchronize()
    assert torch.equal(got_counts, 2 * cnt) and torch.equal(got_hist, 2 * hist) and torch.equal(got, out.long())
    # the inputs make the cases real
    per_class = hist.sum(1).cpu().numpy()
    kept = cnt[:Cn].cpu().numpy()
    assert (kept <= per_class).all() and int(cnt[Cn]) == P - int(kept.sum())
    nan_classes = [c for c in range(Cn) if thr_host[c] != thr_host[c]]
    assert all(kept[c] == 0 for c in nan_classes), "a NaN threshold keeps nothing"
    if h > 2:          # (h = w = 1: one low-res pixel, every label is its class's -- kept or not as that class's threshold says)
        assert bool((got != 255).any())
        assert any(0 < kept[c] < per_class[c] for c in range(Cn) if 0.0 < thr_host[c] < 1.0), "no class is kept in part"
        assert bool((got == 255).any()) and any(per_class[c] > 0 for c in nan_classes)
        assert int((got[0, :H // h] == 1).sum()) > 0, "the tie band never won: the case does not exercise first-index-wins"
        assert kept[1] == per_class[1] > 0                                    # thr[1] = -1


def test_label_kernel_refusals_write_nothing(dev):
    family, B, h, w, H, W, Cn, ld = GEOMETRIES[0]
    _buf, view = _input(family, B, h, w, Cn, ld, dev, seed=1)
    wide = torch.zeros(72, device=dev)
    P = B * H * W
    lab = torch.full((P + 1,), GARBAGE, dtype=torch.int64, device=dev)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    hist = torch.zeros(65 * BINS, dtype=torch.int64, device=dev)
    thr = torch.full((66,), 0.5, device=dev)
    good = dict(family=family, B=B, h=h, w=w, ld=ld, H=H, W=W, C=Cn)

    def desc(**kw):
        a = dict(good, **kw)
        d = _cb_desc(view, lab, counts, hist, thr, a["family"], a["B"], a["h"], a["w"], a["ld"], a["H"], a["W"], a["C"])
        for k in ("fix", "label", "counts", "hist", "thr"):
            if k in kw:
                setattr(d, k, kw[k])
        return d
    bad = [desc(fix=None), desc(label=None), desc(counts=None), desc(hist=None), desc(thr=None), desc(C=25),
           desc(fix=wide.data_ptr(), B=1, h=1, w=1, C=65, ld=72),                 # the LDS histogram's limit
           desc(family=2), desc(family=-1), desc(label=lab.data_ptr() + 4), desc(hist=hist.data_ptr() + 4), desc(thr=thr.data_ptr() + 2),
           desc(B=0), desc(H=0), desc(W=-1), desc(h=0), desc(w=0), desc(C=0),
           desc(family=1, B=1, h=32768, w=32768, ld=4, C=3)]                  # B*h*w*ld = 2^32: the 32-bit tap offsets of family 1
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_online_label_cb", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_online_label_cb", None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((lab == GARBAGE).all()) and int(counts.sum()) == 0 and int(hist.sum()) == 0
    L.call("simt_online_label_cb", C.byref(desc(thr=thr.data_ptr() + 4)), ops.stream_ptr())          # the descriptor itself is sound; 4-byte aligned thr
    torch.cuda.synchronize()
    assert int(counts.sum()) == P == int(hist.sum()) and bool((lab[:P] != GARBAGE).all()) and int(lab[P]) == GARBAGE


# ---- (b) the threshold kernel --------------------------------------------------------------------------------------------------------------------
def _thr_desc(hist, thr, t_out, Cn, P, T, M):
    d = L.ClassThresholdsDesc()
    d.hist, d.thr, d.t_out = hist.data_ptr(), thr.data_ptr(), (None if t_out is None else t_out.data_ptr())
    d.drop, d.C, d.cap, d.omd = 1.0 - P, Cn, T, 1.0 - M
    return d


def _check_thresholds(dev, hist_np, start, P, T, M, with_t_out=True):
    Cn = hist_np.shape[0]
    hbuf = torch.full((GUARD + Cn * BINS + GUARD,), 7, dtype=torch.int64, device=dev)
    hbuf[GUARD:GUARD + Cn * BINS] = torch.from_numpy(hist_np.reshape(-1)).to(dev)
    tbuf = torch.full((2 * FGUARD + Cn,), -3.0, device=dev)
    tbuf[FGUARD:FGUARD + Cn] = torch.from_numpy(start)
    obuf = torch.full((2 * FGUARD + Cn,), -5.0, device=dev)
    d = _thr_desc(hbuf[GUARD:], tbuf[FGUARD:], obuf[FGUARD:] if with_t_out else None, Cn, P, T, M)
    L.call("simt_class_thresholds", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    want_thr, want_t = balanced_update(start, hist_np, P, T, M)
    got_thr, got_t = tbuf[FGUARD:FGUARD + Cn].cpu(), obuf[FGUARD:FGUARD + Cn].cpu()
    what = f"C = {Cn}, P = {P}, T = {T}, M = {M}"
    assert torch.equal(_bits(got_thr), _bits(torch.from_numpy(want_thr))), (what, got_thr.tolist(), want_thr.tolist())
    if with_t_out:
        assert torch.equal(_bits(got_t), _bits(torch.from_numpy(want_t))), (what, got_t.tolist(), want_t.tolist())
    else:
        assert bool((obuf == -5.0).all())
    assert int(hbuf[GUARD:GUARD + Cn * BINS].abs().sum()) == 0, "the histogram was not zeroed"
    assert bool((hbuf[:GUARD] == 7).all()) and bool((hbuf[GUARD + Cn * BINS:] == 7).all()), "guard words of the histogram written"
    assert bool((tbuf[:FGUARD] == -3.0).all()) and bool((tbuf[FGUARD + Cn:] == -3.0).all()), "guard floats of the thresholds written"
    assert bool((obuf[:FGUARD] == -5.0).all()) and bool((obuf[FGUARD + Cn:] == -5.0).all()), "guard floats of t_out written"
    # the histogram is zero now: a second launch moves nothing
    L.call("simt_class_thresholds", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(tbuf[FGUARD:FGUARD + Cn].cpu()), _bits(torch.from_numpy(want_thr)))
    if with_t_out:
        assert bool((obuf[FGUARD:FGUARD + Cn] == 0).all())
    return want_thr


def _starts(Cn, T):
    """Start thresholds: T where the trainer starts, and values a few batches may have left."""
    s = np.full(Cn, T, np.float32)
    s[1::3] = np.float32(0.3)
    s[2::3] = np.float32(T) * np.float32(0.77)
    return s


SETTINGS = [(0.5, 0.9, 0.9), (0.625, 0.968, 0.0), (1.0, 0.5, 0.5), (0.01, 0.999, 0.99)]          # (P, T, M)


def test_threshold_kernel_C1_on_every_crafted_row(dev):
    for _name, row, P, _b in CRAFTED:
        for T, M in ((0.9, 0.9), (0.9, 0.0)):
            _check_thresholds(dev, row[None].copy(), np.array([T], np.float32), P, T, M)
    _check_thresholds(dev, CRAFTED[1][1][None].copy(), np.array([0.3], np.float32), 0.5, 0.9, 0.5, with_t_out=False)


@pytest.mark.parametrize("P,T,M", SETTINGS)
def test_threshold_kernel_C19_on_the_label_tests_histogram(dev, P, T, M):
    hist = _label_hist(dev).copy()
    assert hist.shape == (19, BINS) and (hist.sum(1) > 0).all()
    moved = _check_thresholds(dev, hist, _starts(19, T), P, T, M)
    assert (moved != _starts(19, T)).any()
    hist[3] = CRAFTED[10][1]          # counts above 2^32
    hist[5] = 0                       # a class without a pixel keeps its threshold
    assert hist[3].max() > 2 ** 32 and hist[5].sum() == 0
    moved = _check_thresholds(dev, hist, _starts(19, T), P, T, M)
    assert moved[5] == _starts(19, T)[5]


@pytest.mark.parametrize("P,T,M", SETTINGS[:2])
def test_threshold_kernel_C64(dev, P, T, M):
    rng = np.random.default_rng(64)
    rows = [c[1] for c in CRAFTED] + list(_label_hist(dev)) + list(_label_hist(dev, GEOMETRIES[4]))
    while len(rows) < 64:
        r = np.zeros(BINS, np.int64)
        idx = rng.integers(0, BINS, rng.integers(1, 40))
        r[idx] = rng.integers(1, 10000, idx.size)
        rows.append(r)
    hist = np.stack(rows[:64]).astype(np.int64)
    assert hist.shape == (64, BINS) and hist.max() > 2 ** 32 and (hist.sum(1) == 0).any()
    _check_thresholds(dev, hist, _starts(64, T), P, T, M)


def test_threshold_kernel_refusals_write_nothing(dev):
    Cn = 19
    hist_np = _label_hist(dev)
    hist = torch.from_numpy(hist_np.reshape(-1).copy()).to(dev)
    hist = torch.cat([hist, torch.zeros(46 * BINS + 1, dtype=torch.int64, device=dev)])
    thr = torch.full((66,), 0.9, device=dev)
    t_out = torch.full((66,), -5.0, device=dev)
    before = hist.clone()

    def desc(P=0.5, T=0.9, M=0.9, Cn=Cn, **kw):
        d = _thr_desc(hist, thr, t_out, Cn, P, T, M)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [desc(hist=None), desc(thr=None), desc(Cn=0), desc(Cn=-1), desc(Cn=65), desc(hist=hist.data_ptr() + 4), desc(thr=thr.data_ptr() + 2),
           desc(t_out=t_out.data_ptr() + 2), desc(drop=1.0), desc(drop=-0.1), desc(drop=float("nan")), desc(omd=0.0), desc(omd=1.5),
           desc(omd=float("nan")), desc(cap=float("nan"))]
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_class_thresholds", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_class_thresholds", None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(hist, before) and bool((thr == 0.9).all()) and bool((t_out == -5.0).all())
    L.call("simt_class_thresholds", C.byref(desc()), ops.stream_ptr())          # the descriptor itself is sound
    torch.cuda.synchronize()
    assert int(hist[:Cn * BINS].sum()) == 0 and bool((thr[:Cn] != 0.9).any()) and bool((thr[Cn:] == 0.9).all()) and bool((t_out[Cn:] == -5.0).all())


# ---- (c) trainers ----------------------------------------------------------------------------------------------------------------------------------
PORTION, MOMENTUM = 0.5, 0.5
PORT = 29591


class BalancedComposition(Composition):
    """The labels the EXISTING launches make of a separate eval-mode plan's output, with per-class thresholds kept on the HOST: label and count
    in one simt_pseudo_conf*_u8 call, read the histogram back, `balanced_update`."""

    def __init__(self, model, dev, dtype, tau, P, M):
        super().__init__(model, dev, dtype)
        self.tau, self.P, self.M = tau, P, M
        self.thr = np.full(19, tau, np.float32)
        self.hist = torch.zeros(19, BINS, dtype=torch.int64, device=dev)

    def label_balanced(self, image):
        B, H, W = SIZE
        self.forward(image)
        st = ops.stream_ptr()
        thr = np.ascontiguousarray(self.thr, dtype=np.float32)
        self.hist.zero_()
        if self.model == "v3":
            L.call("simt_pseudo_conf2_u8", ops._p(self.out), self.h, self.w, self.ld, H, W, B, H, W, 19, thr.ctypes.data, ops._p(self.u8),
                   ops._p(self.counts), ops._p(self.hist), st)
        else:
            ops.softmax_rows(self.out, self.ld, self.prob, self.ld, B * self.h * self.w, 19)
            L.call("simt_pseudo_conf_u8", ops._p(self.prob), self.h, self.w, self.ld, B, H, W, 19, thr.ctypes.data, ops._p(self.u8),
                   ops._p(self.counts), ops._p(self.hist), st)
        torch.cuda.synchronize()
        self.thr, _t = balanced_update(self.thr, self.hist.cpu().numpy(), self.P, self.tau, self.M)
        return self.u8.long()


def _losses(tr, what):
    l = tr.losses()
    assert l and all(v == v and abs(v) != float("inf") for k, v in l.items() if k != "label_thresholds"), f"{what}: losses {l}"
    return l


_RUNS = {}


def _run(model, dev, dtype, mode, every=None, steps=3, its=1, dp=False, scale=1.0):
    """One memoised run.  mode "online": the trainer with online_labels_balanced.  mode "composition": the trainer WITHOUT online_labels, fed
    BalancedComposition's labels (its plan refreshed from the trainer's EMA where refresh_due says so, when `every` is given)."""
    key = (model, dtype, mode, every, steps, its, dp, scale)
    if key in _RUNS:
        return _RUNS[key]
    data = _views(dev, steps, its)
    tau = Composition(model, dev, dtype).threshold(data[0][0][1], scale=scale)          # near the median confidence of step 0's weak view
    comp = BalancedComposition(model, dev, dtype, tau, PORTION, MOMENTUM)
    ema = {} if every is None else {"ema_decay": 0.9}
    res = dict(tau=tau, labels=[], scalars=[], shares=[], thr=[])
    with (one_rank_group(dev, PORT) if dp else contextlib.nullcontext()) as pg:
        if mode == "online":
            kw = dict(ema, online_labels=tau, online_labels_balanced=PORTION, online_labels_momentum=MOMENTUM)
            if every is not None:
                kw["online_labels_every"] = every
            tr = _trainer(model, dev, dtype, pg, its, **kw)
        else:
            tr = _trainer(model, dev, dtype, pg, its, **ema)
            assert not hasattr(tr, "fixed") and not hasattr(tr, "label_thr") and tr.online_labels is None
        for mb in data:
            strong = [m[0] for m in mb] if its > 1 else mb[0][0]
            weak = [m[1] for m in mb] if its > 1 else mb[0][1]
            if mode == "online":
                tr.step(strong, None, teacher_image=weak)
                torch.cuda.synchronize()
                res["labels"].append(tr.label.clone())                         # (iter_size > 1: the last micro-batch's)
                res["thr"].append(tr.label_thr.cpu().clone())
                assert int(tr.label_hist.abs().sum()) == 0, "the histogram is not zero between steps"
            else:
                labs = [comp.label_balanced(m[1]).clone() for m in mb]
                tr.step(strong, labs if its > 1 else labs[0])
                res["labels"].append(labs[-1])
                res["thr"].append(torch.from_numpy(comp.thr.copy()))
                res["shares"].append(float((torch.stack(labs) != 255).float().mean()))
                if every is not None and refresh_due(tr.ema_updates, every):
                    comp.follow(tr.ema_params)
            res["scalars"].append(R.scalars(tr))
        res["losses"] = _losses(tr, f"{model} {mode}")
        res["state"] = O._state(tr)
        del tr
    del comp
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


def _assert_same(got, comp, what):
    O._assert_same(got, comp, what)
    for i, (a, b) in enumerate(zip(got["thr"], comp["thr"])):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: the thresholds behind step {i + 1} differ: {a.tolist()} / {b.tolist()}"
    print(f"{what}: tau = {comp['tau']!r}, kept shares {comp['shares']}, thresholds {comp['thr'][-1].tolist()}")
    assert all(0.0 < s < 1.0 for s in comp["shares"]), comp["shares"]
    assert bool((comp["thr"][-1] != np.float32(comp["tau"])).any()), "the thresholds never moved"
    assert bool((comp["thr"][-1] <= np.float32(comp["tau"])).all())
    assert got["losses"]["label_thresholds"] == got["thr"][-1].tolist() and "label_thresholds" not in comp["losses"]
    assert abs(got["losses"]["labelled"] - sum(comp["shares"]) / len(comp["shares"])) < 1e-6


@pytest.mark.parametrize("model", O.MODELS)
def test_balanced_trainer_equals_the_composition(dev, model):
    """3 steps, bf16: the labels of every step, the loss scalars, every tensor of state_dict(), the momentum, the packed operands and the
    thresholds behind every step."""
    _assert_same(_run(model, dev, BF, "online"), _run(model, dev, BF, "composition"), f"{model} bf16")


def test_balanced_trainer_fp32(dev):
    _assert_same(_run("vgg", dev, F32, "online"), _run("vgg", dev, F32, "composition"), "vgg fp32")


def test_balanced_trainer_iter_size_2(dev):
    """Two micro-batches per step: the second is labelled with the thresholds the first one left."""
    _assert_same(_run("v2", dev, BF, "online", its=2), _run("v2", dev, BF, "composition", its=2), "v2 iter_size 2")


def test_balanced_trainer_with_a_moving_teacher(dev):
    sc = O.MOVING_SCALE["v2"]
    _assert_same(_run("v2", dev, BF, "online", every=1, scale=sc), _run("v2", dev, BF, "composition", every=1, scale=sc), "v2 moving teacher")


def test_balanced_trainer_one_rank_rccl_group(dev):
    got, single = _run("v3", dev, BF, "online", dp=True), _run("v3", dev, BF, "online")
    O._assert_same(got, single, "one-rank RCCL group")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got["thr"], single["thr"]))


def test_balanced_trainer_resumes(dev, tmp_path):
    """2 + save + a new trainer + load + 2 == 4, the thresholds and `labelled` included; the refusals of the train state."""
    model = "vgg"
    data = _views(dev, 4)
    tau = Composition(model, dev, BF).threshold(data[0][0][1])
    kw = dict(online_labels=tau, online_labels_balanced=PORTION, online_labels_momentum=MOMENTUM)

    def steps(tr, part, out):
        for mb in part:
            tr.step(mb[0][0], None, teacher_image=mb[0][1])
            out["scalars"].append(R.scalars(tr))
            l = tr.losses()
            out["read"].append((l["labelled"], l["label_thresholds"]))
            out["labels"].append(tr.label.clone())

    a = dict(scalars=[], read=[], labels=[])
    tr = _trainer(model, dev, **kw)
    steps(tr, data, a)
    a["state"] = O._state(tr)
    assert len({tuple(r[1]) for r in a["read"]}) == 4, "the thresholds did not move with every step"
    del tr
    b = dict(scalars=[], read=[], labels=[])
    tr = _trainer(model, dev, **kw)
    steps(tr, data[:2], b)
    ts = tr.training_state()
    assert ts["hyper"]["online_labels_balanced"] == PORTION and ts["hyper"]["online_labels_momentum"] == MOMENTUM
    assert set(ts["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported", "label_thresholds"}
    assert ts["accumulators"]["label_thresholds"].tolist() == b["read"][-1][1]
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = _trainer(model, dev, **kw)
    tr.load_training_state(ts)
    steps(tr, data[2:], b)
    b["state"] = O._state(tr)
    assert a["read"] == b["read"]
    O._assert_same(a, b, f"{model} resumed after step 2")
    one = _trainer(model, dev, online_labels=tau)
    with pytest.raises(ValueError, match=r"online_labels_balanced \(state: 0\.5, this trainer: None\)"):
        one.load_training_state(ts)
    with pytest.raises(ValueError, match=r"online_labels_balanced \(state: None, this trainer: 0\.5\)"):
        tr.load_training_state(one.training_state())
    with pytest.raises(ValueError, match=r"online_labels_momentum \(state: 0\.5, this trainer: 0\.9\)"):
        _trainer(model, dev, online_labels=tau, online_labels_balanced=PORTION).load_training_state(ts)
    for bad, named in [(dict(online_labels_balanced=0.5), "^online_labels_balanced needs online_labels"),
                       (dict(online_labels=tau, online_labels_momentum=0.5), "^online_labels_momentum needs online_labels_balanced"),
                       (dict(online_labels=tau, online_labels_balanced=0.0), "^online_labels_balanced 0.0"),
                       (dict(online_labels=tau, online_labels_balanced=0.5, online_labels_momentum=1.0), "^online_labels_momentum 1.0")]:
        with pytest.raises(ValueError, match=named):
            _trainer(model, dev, **bad)


def test_tool_trains_on_images_alone_with_balanced_thresholds_and_resumes(dev, tmp_path, capsys, monkeypatch):
    """trainV1_warmup --online-labels T --online-labels-balanced --online-labels-momentum 0.5 on 4 PNG images without label files: 3 + 3 == 6
    through --train-state, ` thr = lo..hi` in every loss line, one label launch and one threshold launch per step."""
    pytest.importorskip("PIL.Image")
    from simt_amd.tools import trainV1_warmup as tool
    root = tmp_path / "data"
    O._image_files(root)
    T = O._tool_threshold("DeepLabVGG", root, dev)
    assert 0.0 < T < 1.0
    common = ["--learning-rate", "2.5e-4", "--model", "DeepLabVGG", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
              "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2",
              "--data-dir-target", str(root), "--data-list-target", str(root / "images.lst"), "--online-labels", str(T)]
    flags = ["--online-labels-balanced", "--online-labels-momentum", "0.5"]
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run(tag, stop, *more):
        del calls[:]
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6, *flags)
    lines = R._loss_lines(out_a)
    assert len(lines) == 6 and not re.search(r"loss_seg\w* = nan", out_a), out_a
    thr = [re.search(r" labelled = ([0-9.]+) thr = ([0-9.]+)\.\.([0-9.]+)", ln).groups() for ln in lines]
    print(f"T = {T}, (labelled, lowest, highest threshold) per line: {thr}")
    assert all(0.0 <= float(lo) <= float(hi) <= round(T, 3) + 1e-9 for _s, lo, hi in thr)
    assert calls.count("simt_online_label_cb") == 6 == calls.count("simt_class_thresholds") and "simt_online_label" not in calls
    assert "; class-balanced: one threshold per class" in out_a and "(momentum 0.5)" in out_a
    out_b1, _ = run("b", 3, *flags, "--train-state", state)
    assert R._loss_lines(out_b1) == lines[:3]
    out_b2, snap_b = run("b", 6, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert R._loss_lines(out_b2) == lines[3:], (out_a, out_b2)
    R._same_snapshot(snap_a, snap_b)
    for other in ([], ["--online-labels-balanced", "0.25", "--online-labels-momentum", "0.5"], ["--online-labels-balanced"]):
        with pytest.raises(SystemExit, match="online_labels_balanced"):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state])
    capsys.readouterr()


# ---- (d) the keyword off ---------------------------------------------------------------------------------------------------------------------------
def test_online_labels_alone_is_what_it_was(dev, monkeypatch):
    """online_labels without online_labels_balanced: no threshold buffer, no histogram, the one simt_online_label launch per step, and its
    labels are the yardstick's of tests/test_gpu_online_labels.py (simt_pseudo_label_u8 at the one threshold)."""
    data = _views(dev, 2)
    comp = Composition("v2", dev, BF)
    tau = comp.threshold(data[0][0][1])
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    tr = _trainer("v2", dev, online_labels=tau)
    assert tr.online_labels_balanced is None and not hasattr(tr, "label_thr") and not hasattr(tr, "label_hist") and not hasattr(tr, "online_cb_desc")
    for mb in data:
        tr.step(mb[0][0], None, teacher_image=mb[0][1])
        torch.cuda.synchronize()
        assert torch.equal(tr.label, comp.label(mb[0][1], tau))
    assert calls.count("simt_online_label") == 2 and "simt_online_label_cb" not in calls and "simt_class_thresholds" not in calls
    l = tr.losses()
    assert "label_thresholds" not in l and 0.0 < l["labelled"] < 1.0
    ts = tr.training_state()
    assert set(ts["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported"} and not set(ts["hyper"]) & set(tsf.BALANCE_FIELDS)
    # the whole run of the parent's test, against its composition
    O._assert_same(O._run("v2", dev, BF, "online"), O._run("v2", dev, BF, "composition"), "v2 fixed teacher, one threshold")
