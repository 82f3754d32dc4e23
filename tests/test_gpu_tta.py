"""GPU tests of test-time augmentation: simt_tta_label (csrc/label_sweep.hip) -- up to 8 low-res maps, any of them of the mirrored frame,
combined into one label map -- and its plumbing through Evaluator, PseudoLabeller and the export.  The yardstick is the float64
restatement tests/_tta_ref.py (itself checked in tests/test_tta_cpu.py); the reference has no test-time augmentation.

Shared inputs (tests/_tta_ref.py): B = 2, C = 19, labels 17 x 23 (odd; W % 4 != 0: the quad tail and the row wrap of the packed label
stores), term maps 5 x 7, 6 x 9, 9 x 12 of ONE scene (a coarse field + per-term noise, so that averaged confidences spread over 0.15 - 0.99),
every test once at ld = 24 on 16-byte aligned maps (the float4 gathers) and once at ld = 19 (scalar), channels C..ld-1 planted with 1e4.
Every comparison with float64 first asserts on the reference alone that at most 1 of the 782 pixels lies inside the margin it grants."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import _tta_ref as R
from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu
B, C, H, W = R.B, R.C, R.H, R.W
P = B * H * W
BINS = L.CONF_BINS
LDS = [24, 19]


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    """kind "logits" / "prob": the five shared term maps [B, h, w, C] float32 (read only)."""
    maps = R.make_logits(5)
    return tuple(maps if kind == "logits" else [R.softmax32(m) for m in maps])


@functools.lru_cache(maxsize=None)
def _reference(kind, n, fam2, mode):
    """(arg, top, gap) of the float64 restatement over the first n shared terms (read only)."""
    terms = [(_inputs(kind)[i], R.FLIPS[i], R.HIWI[i % 3] if fam2 else (0, 0)) for i in range(n)]
    return R.combine(terms, H, W, mode)[1:]


def _dev_terms(dev, kind, n, ld, fam2=False, flips=R.FLIPS):
    """-> the `maps` of ops.tta_label for the first n shared terms at row pitch ld."""
    maps = []
    for i in range(n):
        t = torch.from_numpy(R.pad_channels(_inputs(kind)[i], ld)).to(dev)
        assert t.data_ptr() % 16 == 0
        hi, wi = R.HIWI[i % 3] if fam2 else (0, 0)
        maps.append((t, t.shape[1], t.shape[2], ld, hi, wi, flips[i]))
    return maps


class _Out:
    """Sentinel-filled outputs of one launch, 64 guard bytes / words behind the label maps."""

    def __init__(self, dev, pred=False, out=False, hist=False):
        self.pred = torch.full((P + 64,), -7, device=dev, dtype=torch.int32) if pred else None
        self.out = torch.full((P + 64,), 77, device=dev, dtype=torch.uint8) if out else None
        self.counts = torch.zeros(C + 1, device=dev, dtype=torch.int64) if out else None
        self.hist = torch.zeros(C, BINS, device=dev, dtype=torch.int64) if hist else None

    def kw(self):
        return dict(pred=self.pred, out=self.out, counts=self.counts, hist=self.hist)

    def fetch(self):
        torch.cuda.synchronize()
        r = {}
        if self.pred is not None:
            assert torch.all(self.pred[P:] == -7), "the kernel wrote past the end of pred"
            r["pred"] = self.pred[:P].view(B, H, W).cpu()
        if self.out is not None:
            assert torch.all(self.out[P:] == 77), "the kernel wrote past the end of the label map"
            r["out"] = self.out[:P].view(B, H, W).cpu()
            r["counts"] = self.counts.cpu()
        if self.hist is not None:
            r["hist"] = self.hist.cpu()
        return r


def _run(dev, maps, mode, *, threshold=0.0, thr=None, pred=False, out=False, hist=False):
    o = _Out(dev, pred, out, hist)
    ops.tta_label(maps, B=B, H=H, W=W, Cn=C, mode=mode, threshold=threshold, thr=thr, **o.kw())
    return o.fetch()


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: {int((a[k] != b[k]).sum())} entries differ"


# ---- 1. the mirror is exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_mirror_is_exact(dev, mode, n, ld):
    """A launch with flip flags equals, byte for byte, the launch without them on maps reversed along their columns."""
    flips = (True,) if n == 1 else (False, True, True, False)
    maps = _dev_terms(dev, "prob" if mode else "logits", n, ld, flips=flips)
    plain = [(torch.flip(t, [2]).contiguous() if f else t, h, w, l_, hi, wi, False) for (t, h, w, l_, hi, wi, f) in maps]
    assert any(f for *_r, f in maps) and not any(f for *_r, f in plain)
    if mode == 0:
        a, b = _run(dev, maps, 0, pred=True, out=True), _run(dev, plain, 0, pred=True, out=True)
        assert len(torch.unique(a["pred"])) >= 10
        _same(a, b)
        return
    thr = np.random.default_rng(5).uniform(0.3, 0.9, C).astype(np.float32)
    _same(_run(dev, maps, 1, thr=thr, out=True, hist=True), _run(dev, plain, 1, thr=thr, out=True, hist=True))
    a, b = _run(dev, maps, 1, threshold=0.5, out=True), _run(dev, plain, 1, threshold=0.5, out=True)
    assert 0 < int(a["counts"][C]) < P
    _same(a, b)
    # and a mirror that was dropped would show: the unflipped launch on the same maps gives other labels
    c = _run(dev, [(*m[:6], False) for m in maps], 1, threshold=0.5, out=True)
    assert not torch.equal(a["out"], c["out"])


# ---- 2. mode 0 against float64, both families ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("fam2", [False, True], ids=["one_resample", "two_resamples"])
def test_mode0_against_float64(dev, fam2, n, ld):
    arg, top, gap = _reference("logits", n, fam2, 0)
    exempt = gap < 1e-4 * (1 + np.abs(top))
    assert exempt.sum() <= 1 and len(np.unique(arg)) >= 10
    r = _run(dev, _dev_terms(dev, "logits", n, ld, fam2), 0, pred=True, out=True)
    got = r["pred"].numpy()
    diff = got != arg
    print(f"n={n} fam2={fam2} ld={ld}: {int(diff.sum())} labels differ, {int(exempt.sum())} pixels exempt")
    assert not np.any(diff & ~exempt) and diff.sum() <= 1
    assert torch.equal(r["out"], r["pred"].to(torch.uint8)) and int(r["pred"].min()) >= 0 and int(r["pred"].max()) < C
    assert np.array_equal(r["counts"].numpy(), np.bincount(r["out"].numpy().reshape(-1), minlength=C + 1)[:C + 1]) and r["counts"][C] == 0
    assert len(np.unique(got)) >= 10
    only_pred = _run(dev, _dev_terms(dev, "logits", n, ld, fam2), 0, pred=True)         # either output alone
    only_out = _run(dev, _dev_terms(dev, "logits", n, ld, fam2), 0, out=True)
    assert torch.equal(only_pred["pred"], r["pred"]) and torch.equal(only_out["out"], r["out"]) and torch.equal(only_out["counts"], r["counts"])


# ---- 3. against the existing launches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", LDS)
def test_two_terms_against_the_two_map_kernels(dev, ld):
    """Two unflipped terms: simt_upsample_sum_argmax / simt_pseudo_label_u8 mode 0 and simt_upsample2_sum_argmax label the same maps; no
    difference wherever the float64 top-2 gap is >= 1e-5 (the bar of test_upsample2_sum_argmax_vs_existing_launches)."""
    flips = (False, False)
    for fam2 in (False, True):
        maps = _dev_terms(dev, "logits", 2, ld, fam2, flips=flips)
        gap = R.combine([(_inputs("logits")[i], False, R.HIWI[i] if fam2 else (0, 0)) for i in range(2)], H, W, 0)[3]
        assert (gap < 1e-5).sum() <= 1
        r = _run(dev, maps, 0, pred=True, out=True)
        (la, ha, wa, _l, hia, wia, _f), (lb, hb, wb, _l2, hib, wib, _f2) = maps
        old = torch.full((B, H, W), -1, device=dev, dtype=torch.int32)
        if fam2:
            L.call("simt_upsample2_sum_argmax", ops._p(la), ha, wa, ld, hia, wia, ops._p(lb), hb, wb, ld, hib, wib, B, H, W, C, ops._p(old),
                   ops.stream_ptr())
        else:
            L.call("simt_upsample_sum_argmax", ops._p(la), ha, wa, ld, ops._p(lb), hb, wb, ld, B, H, W, C, ops._p(old), ops.stream_ptr())
            o8 = torch.zeros(B, H, W, device=dev, dtype=torch.uint8)
            cnt = torch.zeros(C + 1, device=dev, dtype=torch.int64)
            L.call("simt_pseudo_label_u8", ops._p(la), ha, wa, ld, ops._p(lb), hb, wb, ld, B, H, W, C, 0, 0.0, ops._p(o8), ops._p(cnt),
                   ops.stream_ptr())
            d8 = (o8.cpu() != r["out"]).numpy()
            assert not np.any(d8 & (gap >= 1e-5)), f"{int(d8.sum())} labels differ from simt_pseudo_label_u8"
        d = (old.cpu() != r["pred"]).numpy()
        print(f"fam2={fam2} ld={ld}: {int(d.sum())} labels differ from the two-map kernel")
        assert not np.any(d & (gap >= 1e-5))


@pytest.mark.parametrize("ld", LDS)
def test_one_term_mode1_equals_the_one_map_kernels(dev, ld):
    """One term, mode 1: 1.0f / 1 is exact and the arithmetic is that of simt_pseudo_label_u8 mode 1 / simt_pseudo_conf_u8 -- out, counts
    and hist are equal exactly."""
    maps = _dev_terms(dev, "prob", 1, ld, flips=(False,))
    (la, ha, wa, *_r), = maps
    thr = np.random.default_rng(6).uniform(0.3, 0.9, C).astype(np.float32)
    o8 = torch.zeros(B, H, W, device=dev, dtype=torch.uint8)
    cnt = torch.zeros(C + 1, device=dev, dtype=torch.int64)
    L.call("simt_pseudo_label_u8", ops._p(la), ha, wa, ld, None, 0, 0, 0, B, H, W, C, 1, 0.5, ops._p(o8), ops._p(cnt), ops.stream_ptr())
    r = _run(dev, maps, 1, threshold=0.5, out=True)
    assert 0 < int(cnt[C]) < P
    assert torch.equal(r["out"], o8.cpu()) and torch.equal(r["counts"], cnt.cpu())
    o8.zero_(), cnt.zero_()
    hist = torch.zeros(C, BINS, device=dev, dtype=torch.int64)
    L.call("simt_pseudo_conf_u8", ops._p(la), ha, wa, ld, B, H, W, C, thr.ctypes.data, ops._p(o8), ops._p(cnt), ops._p(hist), ops.stream_ptr())
    r = _run(dev, maps, 1, thr=thr, out=True, hist=True)
    assert torch.equal(r["out"], o8.cpu()) and torch.equal(r["counts"], cnt.cpu()) and torch.equal(r["hist"], hist.cpu())
    assert torch.equal(_run(dev, maps, 1, hist=True)["hist"], hist.cpu())                 # statistics only


# ---- 4. mode 1 against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("n", [2, 4])
def test_mode1_against_float64(dev, n, ld):
    arg, conf, gap = _reference("prob", n, False, 1)
    maps = _dev_terms(dev, "prob", n, ld)
    thr = np.random.default_rng(7).uniform(0.3, 0.9, C).astype(np.float32)
    for name, keep, edge in (("threshold 0.8", conf > 0.8, np.full_like(conf, 0.8)), ("per-class thr", conf >= thr[arg], thr[arg].astype(np.float64))):
        ref = np.where(keep, arg, 255)
        exempt = (np.abs(conf - edge) < 1e-5) | (gap < 1e-5)
        assert exempt.sum() <= 1 and 20 <= keep.sum() <= P - 20, "the reference must leave pixels on both sides, outside the margins"
        r = _run(dev, maps, 1, threshold=0.8, out=True) if name == "threshold 0.8" else _run(dev, maps, 1, thr=thr, out=True)
        got = r["out"].numpy()
        diff = got != ref
        print(f"n={n} ld={ld} {name}: {int(diff.sum())} labels differ, {int(exempt.sum())} exempt, {int(keep.sum())} of {P} kept")
        assert not np.any(diff & ~exempt) and diff.sum() <= 1
        assert np.array_equal(r["counts"].numpy(), np.bincount(got.reshape(-1), minlength=256)[list(range(C)) + [255]])


# ---- 5. histogram and labels agree exactly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", LDS)
def test_histogram_and_labels_agree(dev, ld):
    """k / 256 and conf * 256 are exact in fp32: a label launch with every thr[c] = k / 256 keeps, per class, exactly hist[c][k:].sum()."""
    maps = _dev_terms(dev, "prob", 4, ld)
    hist = _run(dev, maps, 1, hist=True)["hist"].numpy()
    assert hist.sum() == P and (hist.sum(1) > 0).sum() >= 10
    both = _run(dev, maps, 1, thr=np.full(C, 0.5, np.float32), out=True, hist=True)
    assert np.array_equal(both["hist"].numpy(), hist)
    edges = [0, 1, 255] + list(range(40, 250, 17))
    assert len(edges) == 16 and hist[:, :40].sum() > 0 and hist[:, 244:].sum() > 0          # the edges cut through occupied bins
    for k in edges:
        r = _run(dev, maps, 1, thr=np.full(C, k / 256.0, np.float32), out=True)
        cnt = r["counts"].numpy()
        assert np.array_equal(cnt[:C], hist[:, k:].sum(1)), f"edge {k}/256"
        assert cnt[C] == P - hist[:, k:].sum() and np.array_equal(cnt[:C], np.bincount(r["out"].numpy().reshape(-1), minlength=256)[:C])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    maps = _dev_terms(dev, "prob", 3, 24)
    maps2 = _dev_terms(dev, "prob", 2, 24, fam2=True)
    o = _Out(dev, pred=True, out=True, hist=True)
    thr = np.full(C, 0.5, np.float32)
    big_c = torch.zeros(65 * BINS, device=dev, dtype=torch.int64)
    wide = torch.zeros(B, 5, 7, 72, device=dev)
    base = dict(B=B, H=H, W=W, Cn=C)
    full = dict(out=o.out, counts=o.counts)
    cases = {
        "n = 0": ([], dict(base, mode=0, **full)),
        "n = 9": ([maps[0]] * 9, dict(base, mode=0, **full)),
        "mixed families": ([maps[0], maps2[1]], dict(base, mode=0, **full)),
        "mode 1, two resamples": (maps2, dict(base, mode=1, threshold=0.5, **full)),
        "pred in mode 1": (maps, dict(base, mode=1, threshold=0.5, pred=o.pred, **full)),
        "out without counts": (maps, dict(base, mode=0, out=o.out)),
        "nothing to write, mode 0": (maps, dict(base, mode=0)),
        "nothing to write, mode 1": (maps, dict(base, mode=1, thr=thr)),
        "C > ld": (maps, dict(B=B, H=H, W=W, Cn=25, mode=0, **full)),
        "hist with C > 64": ([(wide, 5, 7, 72, 0, 0, False)], dict(B=B, H=H, W=W, Cn=65, mode=1, hist=big_c)),
        "2^31 elements in a term": ([(maps[0][0], 40000, 40000, 24, 0, 0, False)], dict(base, mode=0, **full)),
        "mode 2": (maps, dict(base, mode=2, **full)),
    }
    for name, (m, kw) in cases.items():
        d = ops.make_tta_desc(m, **kw)
        rc = L.load().simt_tta_label(ctypes.byref(d), ops.stream_ptr())
        assert rc == 1, f"{name}: return code {rc}"                                # SIMT_ERR_INVALID
        assert L.load().simt_last_error(), name
        with pytest.raises(L.SimtHipError):
            L.call("simt_tta_label", ctypes.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.all(o.pred == -7) and torch.all(o.out == 77) and torch.all(o.counts == 0) and torch.all(o.hist == 0) and torch.all(big_c == 0)
    ops.tta_label(maps, **dict(base, mode=1, thr=thr, **full, hist=o.hist))                # and the same buffers are accepted
    assert int(o.fetch()["hist"].sum()) == P


# ---- 7. plumbing -------------------------------------------------------------------------------------------------------------------------
SCALES, LABEL_HW = ((64, 96), (80, 120)), (33, 47)
EV_MODEL = {"multi": "v2", "v3": "v3", "vgg": "vgg"}


def _frames(dev, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(1, 3, *SCALES[0], generator=g) * 50
    x2 = torch.nn.functional.interpolate(x1, size=SCALES[1], mode="bilinear", align_corners=True)
    return x1.to(dev), x2.to(dev)


def _forward_clone(ev, k, x):
    """One plain forward of the evaluator's plan k -> a copy of its low-res logits and their geometry (h, w, ld, hi, wi)."""
    plan = ev.plans[k]
    if ev.model == "v3":
        plan.x_in.copy_(x)
        ev._fwd[k].run()
        return plan.logits.clone(), (*plan.feat_hw, plan.ldq, *SCALES[k])
    o = plan.forward(x)["x2" if ev.model == "v2" else "x"]
    return o.clone(), (*o.shape[1:], 0, 0)


@pytest.mark.parametrize("arch", ["multi", "vgg", "v3"])
def test_evaluator_plumbing(dev, arch):
    from test_gpu_pseudo_labels_cb import _state
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    st, K, layers = _state(arch)
    Hl, Wl = LABEL_HW
    kw = dict(num_classes=C, open_classes=K, label_hw=LABEL_HW, scales=SCALES, device=dev, layers=layers)
    x = _frames(dev, 11)
    ev0 = Evaluator(st, model=EV_MODEL[arch], **kw)
    assert not ev0.tta and ev0.terms == [(64, 96, False), (80, 120, False)]
    # by hand: separate forwards of x and x.flip(3), their logits kept, one launch
    maps = []
    for k in range(2):
        for f in (False, True):
            lg, (h, w, ld, hi, wi) = _forward_clone(ev0, k, x[k].flip(3) if f else x[k])
            maps.append((lg, h, w, ld, hi, wi, f))
    hand = torch.full((1, Hl, Wl), -1, device=dev, dtype=torch.int32)
    ops.tta_label(maps, B=1, H=Hl, W=Wl, Cn=C, mode=0, pred=hand)
    ev = Evaluator(st, model=EV_MODEL[arch], flip=True, **kw)
    assert ev.tta and len(ev.terms) == 4
    got = ev.predict(*x)
    assert torch.equal(got, hand), f"{int((got != hand).sum())} labels differ from the launch by hand"
    assert len(torch.unique(hand)) >= 3
    # the default arguments still take the two-map kernel, launch for launch
    old = torch.full((1, Hl, Wl), -1, device=dev, dtype=torch.int32)
    (la, ga), (lb, gb) = (maps[0][0], maps[0][1:6]), (maps[2][0], maps[2][1:6])
    if arch == "v3":
        L.call("simt_upsample2_sum_argmax", ops._p(la), *ga, ops._p(lb), *gb, 1, Hl, Wl, C, ops._p(old), ops.stream_ptr())
    else:
        L.call("simt_upsample_sum_argmax", ops._p(la), *ga[:3], ops._p(lb), *gb[:3], 1, Hl, Wl, C, ops._p(old), ops.stream_ptr())
    assert torch.equal(ev0.predict(*x), old)
    # three scales without flip: the third used to be dropped silently
    if arch == "multi":
        s3 = SCALES + ((48, 72),)
        x3 = torch.nn.functional.interpolate(x[0], size=s3[2], mode="bilinear", align_corners=True)
        ev3 = Evaluator(st, model="v2", **dict(kw, scales=s3))
        lg3, (h, w, ld, hi, wi) = _forward_clone(ev3, 2, x3)
        ops.tta_label([maps[0], maps[2], (lg3, h, w, ld, hi, wi, False)], B=1, H=Hl, W=Wl, Cn=C, mode=0, pred=hand)
        assert torch.equal(ev3.predict(*x, x3), hand) and not torch.equal(hand, old)


@pytest.mark.parametrize("arch", ["multi", "vgg", "v3"])
def test_labeller_plumbing(dev, arch):
    from test_gpu_pseudo_labels_cb import _state
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    from simt_amd.tools.make_pseudo_labels import PseudoLabeller
    st, K, layers = _state(arch)
    Hl, Wl = LABEL_HW
    kw = dict(num_classes=C, open_classes=K, label_hw=LABEL_HW, scales=SCALES, device=dev, layers=layers)
    x = _frames(dev, 11)
    ev = Evaluator(st, model=EV_MODEL[arch], flip=True, **kw)
    got = ev.predict(*x)
    # arg-max mode gives the evaluator's labels
    lab = PseudoLabeller(st, arch=arch, tta=True, flip=True, **kw)
    out = lab.label(*x)
    assert torch.equal(out, got.to(torch.uint8))
    assert np.array_equal(lab.counts.cpu().numpy(), np.bincount(out.cpu().numpy().reshape(-1), minlength=C + 1)[:C + 1])
    if arch == "v3":                                            # no confidence rule over the two-resample family
        with pytest.raises(ValueError):
            PseudoLabeller(st, arch=arch, mode="class_balanced", tta=True, flip=True, **kw)
        return
    # class-balanced mode: the statistics and the labels agree exactly (the identity of test_histogram_and_labels_agree)
    cb = PseudoLabeller(st, arch=arch, mode="class_balanced", tta=True, flip=True, **kw)
    assert cb.terms == ev.terms and len(cb.plans) == 2
    cb.accumulate(*x)
    hist = cb.conf_hist.cpu().numpy()
    assert hist.sum() == Hl * Wl
    occupied = np.nonzero(hist.sum(0))[0]
    kmed = int(np.median(occupied))
    for kbin in sorted({0, int(occupied.min()), kmed, int(occupied.max()), 255}):
        cb.counts.zero_()
        cb.set_thresholds(np.full(C, kbin / 256.0, np.float32))
        o = cb.label(*x).cpu().numpy()
        cnt = cb.counts.cpu().numpy()
        assert np.array_equal(cnt[:C], hist[:, kbin:].sum(1)) and np.array_equal(cnt[:C], np.bincount(o.reshape(-1), minlength=256)[:C])
    # confidence mode: the plain threshold on the same averaged probabilities
    cf = PseudoLabeller(st, arch=arch, mode="confidence", threshold=kmed / 256.0, tta=True, flip=True, **kw)
    kept = int((cf.label(*x) != 255).sum())
    assert hist[:, kmed + 1:].sum() <= kept <= hist[:, kmed:].sum()      # conf > e: every pixel of the bins above e's, none below


def test_export_with_tta_flip(dev, tmp_path):
    """make_pseudo_labels --tta-flip --class-balanced over 3 small frames: the PNGs are label() of the same frames with the recorded
    thresholds, and the thresholds file records the term list."""
    from PIL import Image

    from test_gpu_pseudo_labels import _write_frames
    from simt_amd.data.pipeline import InputPrep
    from simt_amd.tools import make_pseudo_labels as mpl
    from simt_amd.tools.trainV2_simt import single_model_state
    root = str(tmp_path)
    names, _kit = _write_frames(root, 3, (96, 192), 3)
    st = single_model_state("DeepLabVGG", 19, seed=8)
    scales = ((48, 96), (64, 128))
    # the logits are linear in the classifier's weights and biases: scale them to a standard deviation of 3, so that the confidence
    # spreads and kept and ignored pixels both occur (tests/test_gpu_pseudo_labels_single.py)
    probe = mpl.PseudoLabeller(st, arch="vgg", scales=scales[:1], label_hw=(72, 144), device=dev)
    o = probe.plans[0].forward(torch.randn(1, 3, 48, 96, generator=torch.Generator().manual_seed(2)).to(dev) * 50)["x"][..., :C]
    f = 3.0 / float(o.std())
    st = {k: (v * f if k.startswith("classifier.") else v) for k, v in st.items()}
    del probe
    ckpt = os.path.join(root, "ckpt.pth")
    torch.save(st, ckpt)
    mpl.main(["--restore-from", ckpt, "--arch", "vgg", "--data-dir", root, "--data-list", os.path.join(root, "train.txt"),
              "--input-size", "96,48", "--input-size", "128,64", "--label-size", "144,72", "--num-workers", "2", "--tta-flip",
              "--class-balanced", "0.5", "--out-name", "pseudo_t", "--list-out", os.path.join(root, "pseudo_t.lst")])
    rec = json.load(open(os.path.join(root, "pseudo_t_thresholds.json")))
    assert rec["tta_terms"] == [{"h": 48, "w": 96, "flip": False}, {"h": 48, "w": 96, "flip": True},
                                {"h": 64, "w": 128, "flip": False}, {"h": 64, "w": 128, "flip": True}]
    lab = mpl.PseudoLabeller(st, arch="vgg", scales=scales, label_hw=(72, 144), mode="class_balanced", tta=True, flip=True, device=dev)
    lab.set_thresholds(np.array([e["threshold"] for e in rec["classes"]], np.float32))
    hist = np.array([e["hist"] for e in rec["classes"]], np.int64)
    assert hist.sum() == 3 * 72 * 144 and (hist > 0).sum() >= 10          # the confidences spread over many bins
    preps = None
    for name in names:
        rgb = np.asarray(Image.open(os.path.join(root, "train", name)).convert("RGB"))
        preps = preps or [InputPrep(1, rgb.shape[:2], (w, h), dev, with_label=False) for (h, w) in scales]
        xs = [torch.empty(1, 3, h, w, device=dev) for (h, w) in scales]
        for prep, x in zip(preps, xs):
            prep.run(torch.from_numpy(rgb[None].copy()).to(dev), x)
        png = np.asarray(Image.open(os.path.join(root, "pseudo_t", os.path.basename(name))))
        exp = lab.label(*xs)[0].cpu().numpy()
        assert png.dtype == np.uint8 and np.array_equal(png, exp), f"{name}: {int((png != exp).sum())} labels differ from label()"
    cnt = lab.counts.cpu().numpy()
    assert [e["kept"] for e in rec["classes"]] == [int(v) for v in cnt[:C]] and 0 < cnt[C] < cnt.sum()
