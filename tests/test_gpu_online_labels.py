"""Online labels on the GPU (simt_amd/online_labels.py, simt_online_label in csrc/label_sweep.hip).  Every comparison is between two
executions of the same arithmetic and therefore BITWISE.

  (a) the kernel against the export kernels it shares its device functions with: `label` == their uint8 output widened to int64, `counts`
      equal; garbage prefill, guard bands, the input untouched; every refusal;
  (b) a fixed teacher == the composition: a trainer WITHOUT the keyword, fed the labels the test makes from a separate eval-mode plan with
      simt_softmax_rows + simt_pseudo_label_u8 (DeepLabv3: simt_pseudo_label2_u8 at hia = H, wia = W);
  (c) a moving teacher == the composition whose plan the test refreshes from the other trainer's EMA where `refresh_due` says so;
  (d) iter_size = 2, teacher_image=None, a label passed with the keyword, the one-rank RCCL group;
  (e) resume: 3 + save + load + 3 == 6, `labelled` included, and the refusals of the train state;
  (f) the tool on image files WITHOUT label files.

The thresholds come from the composition: the median of the confidence a host restatement (torch) forms from the separate plan's output.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_resume as R
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from simt_amd.ema_teacher import refresh_due
from simt_amd.engine import LaunchList, TrunkPlan, multi_heads
from simt_amd.engine_v3 import v3_state_shapes
from simt_amd.step import Hyper, WarmupTrainer
from simt_amd.step_single import WarmupSingleTrainer
from test_gpu_single import VGG_SMALL, _vgg_state
from test_gpu_step_coherence import one_rank_group
from test_gpu_v3 import make_state

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF, F32 = torch.bfloat16, torch.float32
GARBAGE = 0x5EADBEEF5EADBEEF
GUARD = 64                      # int64 words on either side of the label map, floats on either side of the input


# ---- (a) the kernel --------------------------------------------------------------------------------------------------------------------------------
# (family, B, h, w, H, W, C, ld)
GEOMETRIES = [(0, 2, 9, 17, 65, 129, 19, 24),          # W % 4 != 0, a pixel count that is no multiple of the block
              (0, 3, 9, 9, 64, 64, 19, 24),
              (0, 1, 5, 5, 33, 33, 3, 8),
              (0, 1, 1, 1, 7, 5, 19, 24),              # the zero-scale case
              (1, 2, 9, 17, 65, 129, 19, 24),          # ld % 4 == 0 on a 16-byte-aligned base: the float4 path
              (1, 2, 8, 16, 64, 128, 19, 24),
              (1, 2, 9, 17, 65, 129, 19, 19),          # the scalar path
              (1, 2, 8, 16, 64, 128, 19, 19)]
THRESHOLDS = [-1.0, 0.5, 0.968, 1.0, float("nan")]


def _input(family, B, h, w, C, ld, dev, seed):
    """[GUARD | B*h*w*ld | GUARD] floats: softmaxed (family 0) or raw (family 1) randn * 3; in item 0 a band of low-res rows whose two largest
    channels are exactly equal (first index wins), one low-res pixel of NaNs; pad columns C..ld-1 = 1e30 (must be ignored)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g) * 3
    if h > 2:
        x[0, :2, :, 1] = x[0, :2].max(-1).values + 1.0
        x[0, :2, :, min(4, C - 1)] = x[0, :2, :, 1]                     # an exact two-way tie at the top, over two whole low-res rows
    if family == 0:
        x = torch.softmax(x, -1)
    if h > 2:
        x[-1, h - 1, w // 2, :] = float("nan")
    full = torch.full((B, h, w, ld), 1e30)
    full[..., :C] = x
    buf = torch.full((2 * GUARD + full.numel(),), -7.0)
    buf[GUARD:GUARD + full.numel()] = full.reshape(-1)
    buf = buf.to(dev)
    view = buf[GUARD:GUARD + full.numel()]
    assert view.data_ptr() % 16 == 0
    return buf, view


def _desc(view, label, counts, family, B, h, w, ld, H, W, C, thr):
    d = L.OnlineLabelDesc()
    d.fix, d.label, d.counts = view.data_ptr(), label.data_ptr(), counts.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, ld, H, W, C, family, thr
    return d


def _yardstick(view, family, B, h, w, ld, H, W, C, thr, dev):
    out = torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    if family == 0:
        L.call("simt_pseudo_label_u8", ops._p(view), h, w, ld, None, 0, 0, 0, B, H, W, C, 1, thr, ops._p(out), ops._p(cnt), ops.stream_ptr())
    else:
        L.call("simt_pseudo_label2_u8", ops._p(view), h, w, ld, H, W, None, 0, 0, 0, 0, 0, B, H, W, C, 1, thr, ops._p(out), ops._p(cnt),
               ops.stream_ptr())
    return out, cnt


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "fam{}-{}x{}x{}to{}x{}-C{}-ld{}".format(*g))
def test_kernel_equals_the_export_kernels_bit_for_bit(dev, geo):
    family, B, h, w, H, W, Cn, ld = geo
    buf, view = _input(family, B, h, w, Cn, ld, dev, seed=sum(geo))
    before = buf.clone()
    P = B * H * W
    seen_kept, seen_ignored, ties = False, False, 0
    for thr in THRESHOLDS:
        lab = torch.full((2 * GUARD + P,), GARBAGE, dtype=torch.int64, device=dev)
        counts = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
        d = _desc(view, lab[GUARD:], counts, family, B, h, w, ld, H, W, Cn, thr)
        L.call("simt_online_label", C.byref(d), ops.stream_ptr())
        out, cnt = _yardstick(view, family, B, h, w, ld, H, W, Cn, thr, dev)
        torch.cuda.synchronize()
        got = lab[GUARD:GUARD + P].view(B, H, W)
        assert torch.equal(got, out.long()), f"threshold {thr}: {int((got != out.long()).sum())} of {P} labels differ"
        assert torch.equal(counts, cnt) and int(counts.sum()) == P, (thr, counts.tolist(), cnt.tolist())
        assert bool((lab[:GUARD] == GARBAGE).all()) and bool((lab[GUARD + P:] == GARBAGE).all()), "guard words written"
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the input was written"
        if thr != thr:
            assert bool((got == 255).all()), "a NaN threshold keeps nothing"
        if thr == -1.0:
            seen_ignored = seen_ignored or bool((got == 255).any())          # only the NaN pixels' neighbourhood
            ties = int((got[0, :H // h] == 1).sum())                            # rows resampled from the two tied low-res rows alone
            L.call("simt_online_label", C.byref(d), ops.stream_ptr())          # counts accumulate across calls
            torch.cuda.synchronize()
            assert torch.equal(counts, 2 * cnt)
        seen_kept = seen_kept or bool((got != 255).any())
    assert seen_kept
    if h > 2:
        assert seen_ignored, "the NaN pixel gave no 255 at threshold -1"
        assert ties > 0, "the tie band never won: the case does not exercise first-index-wins"


def test_kernel_refusals_write_nothing(dev):
    family, B, h, w, H, W, Cn, ld = GEOMETRIES[0]
    buf, view = _input(family, B, h, w, Cn, ld, dev, seed=1)
    P = B * H * W
    lab = torch.full((P + 1,), GARBAGE, dtype=torch.int64, device=dev)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    good = dict(family=family, B=B, h=h, w=w, ld=ld, H=H, W=W, C=Cn, thr=0.5)

    def desc(**kw):
        a = dict(good, **kw)
        d = _desc(view, lab, counts, a["family"], a["B"], a["h"], a["w"], a["ld"], a["H"], a["W"], a["C"], a["thr"])
        for k in ("fix", "label", "counts"):
            if k in kw:
                setattr(d, k, kw[k])
        return d
    bad = [desc(fix=None), desc(label=None), desc(counts=None), desc(C=25), desc(C=256, ld=256), desc(family=2), desc(family=-1),
           desc(label=lab.data_ptr() + 4), desc(B=0), desc(H=0), desc(w=0), desc(C=0),
           desc(family=1, B=1, h=32768, w=32768, ld=4, C=3)]                  # B*h*w*ld = 2^32: the 32-bit tap offsets of family 1
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_online_label", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_online_label", None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((lab == GARBAGE).all()) and int(counts.sum()) == 0
    L.call("simt_online_label", C.byref(desc()), ops.stream_ptr())          # the descriptor itself is sound
    torch.cuda.synchronize()
    assert int(counts.sum()) == P and bool((lab[:P] != GARBAGE).all()) and int(lab[P]) == GARBAGE


# ---- trainers ----------------------------------------------------------------------------------------------------------------------------------------
SIZE = (2, 65, 129)
SMALL = R.SMALL
MODELS = ["v2", "v3", "vgg"]
PORT = 29587


def _start(model, seed=0):
    """(state, arch) of the reduced models the trainer tests use (tests/test_gpu_resume.py)."""
    if model == "v2":
        return so.recipe_state(so.state_shapes(19, 0, False, layers=SMALL), seed=31 + seed, head_scale=8.0), {"layers": SMALL}
    if model == "v3":
        # the classifier of tests/test_gpu_v3.make_state scaled DOWN: as it is, 94 % of the pixels have a confidence of exactly 1.0f on the
        # synthetic images (98.6 % with the x 4 of test_gpu_single._v3_state), so no threshold below 1 would keep less than 0.9 of them
        layers, width, ac = (1, 2, 2), 64, 64
        st = make_state(v3_state_shapes(19, 0, False, layers, width, ac), 3 + 10 * seed)
        st["conv.weight"] = st["conv.weight"] * 0.02
        return st, {"layers": layers, "width": width, "assp_ch": ac}
    lay = [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in VGG_SMALL]
    return _vgg_state(19, lay, 5 + 10 * seed), {"vgg_layers": lay}


def _trainer(model, dev, dtype=BF, pg=None, iter_size=1, seed=0, **kw):
    st, arch = _start(model, seed)
    hkw = dict(R.HP, iter_size=iter_size)
    if model == "vgg":
        hkw["lr"] = R.VGG_LR
    hp = Hyper(open_classes=0, **hkw)
    if model == "v2":
        return WarmupTrainer(st, hp, *SIZE, dtype=dtype, device=dev, layers=SMALL, process_group=pg, **kw)
    return WarmupSingleTrainer(model, st, hp, *SIZE, dtype=dtype, device=dev, arch=arch, process_group=pg, **kw)


class Composition:
    """A separate eval-mode plan over a copy of the start state, and the labels the EXISTING launches make of its output."""

    def __init__(self, model, dev, dtype, seed=0, start=None):
        st, arch = _start(model, seed) if start is None else start
        B, H, W = SIZE
        self.model, self.dev = model, dev
        self.params = {k: v.detach().to(dev, torch.long if v.dtype == torch.long else F32).clone() for k, v in st.items()}
        if model == "v2":
            self.plan = TrunkPlan(self.params, B, H, W, multi_heads(19, 0, False), dtype=dtype, train=False, **arch)
            self.fwd, self.out, self.ld = self.plan.fwd_list, self.plan.out["x2"], self.plan.ldp["x2"]
            self.h, self.w = self.plan.heads[1].h, self.plan.heads[1].w
        elif model == "v3":
            from simt_amd.engine_v3 import V3Plan
            self.plan = V3Plan(self.params, B, H, W, 19, 0, False, dtype=dtype, train=False, **arch)
            self.fwd = LaunchList()
            self.fwd.items = self.plan.fwd_list.items[:-1]
            self.out, self.ld = self.plan.logits, self.plan.ldq
            self.h, self.w = self.plan.feat_hw
        else:
            from simt_amd.engine_vgg import VggPlan
            self.plan = VggPlan(self.params, B, H, W, 19, dtype=dtype, train=False, **arch)
            self.fwd, self.out, self.ld = self.plan.fwd_list, self.plan.out["x"], self.plan.ldp["x"]
            self.h, self.w = self.plan.heads[0].h, self.plan.heads[0].w
        self.prob = torch.zeros(B * self.h * self.w, self.ld, device=dev)
        self.u8 = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(20, dtype=torch.int64, device=dev)

    def forward(self, image):
        self.plan.x_in.copy_(image)
        self.fwd.run()

    def confidence(self, image):
        """Host restatement (torch) of the posterior's maximum: what the thresholds of these tests are chosen from."""
        B, H, W = SIZE
        self.forward(image)
        torch.cuda.synchronize()
        lo = self.out.view(B, self.h, self.w, self.ld)[..., :19].permute(0, 3, 1, 2).float().cpu()
        if self.model == "v3":
            post = torch.softmax(F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False), 1)
        else:
            post = F.interpolate(torch.softmax(lo, 1), size=(H, W), mode="bilinear", align_corners=True)
        return post.max(1).values.numpy()

    def threshold(self, image, q=0.5, scale=1.0):
        tau = float(np.float32(np.quantile(self.confidence(image), q))) * scale
        return min(tau, float(np.nextafter(np.float32(1), np.float32(0))))          # the keyword takes [0, 1)

    def label(self, image, tau):
        B, H, W = SIZE
        self.forward(image)
        st = ops.stream_ptr()
        if self.model == "v3":
            L.call("simt_pseudo_label2_u8", ops._p(self.out), self.h, self.w, self.ld, H, W, None, 0, 0, 0, 0, 0, B, H, W, 19, 1, tau,
                   ops._p(self.u8), ops._p(self.counts), st)
        else:
            ops.softmax_rows(self.out, self.ld, self.prob, self.ld, B * self.h * self.w, 19)
            L.call("simt_pseudo_label_u8", ops._p(self.prob), self.h, self.w, self.ld, None, 0, 0, 0, B, H, W, 19, 1, tau, ops._p(self.u8),
                   ops._p(self.counts), st)
        return self.u8.long()

    def follow(self, ema_params):
        torch.cuda.synchronize()
        for k, v in self.params.items():
            if v.is_floating_point():
                v.copy_(ema_params[k])
        self.plan.repack()
        torch.cuda.synchronize()


def _views(dev, n, its=1):
    """n steps of (strong image, weak image): the weak view is the synthetic image, the strong one a deterministic distortion of it."""
    B, H, W = SIZE
    out = []
    for i in range(n):
        mb = []
        for j in range(its):
            weak, _lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=700 + 10 * i + j, block=8)
            g = torch.Generator().manual_seed(9000 + 10 * i + j)
            strong = (weak * 0.8 + torch.randn(weak.shape, generator=g) * 12).contiguous()
            mb.append((strong.to(dev), weak.to(dev)))
        out.append(mb)
    return out


def _state(tr):
    out = R.full_state(tr)
    if getattr(tr, "ema", None) is not None:
        out.update({f"ema {k}": v.cpu() for k, v in tr.ema.shadow.items()})
    return out


_RUNS = {}
# The thresholds of the MOVING-teacher runs, as a share of the start model's median confidence.  These states are untrained: the running
# variance of DeepLabv3's stem BatchNorm goes from about 1 to about 500 in one step on the synthetic images, so the refreshed teacher's
# confidence lies in 0.18 .. 0.42 where the start model's lies in 0.58 .. 0.999 (measured on MI355X).  At the median it would label nothing,
# and a step without a labelled pixel has a NaN loss -- cross-entropy over zero pixels, as nn.CrossEntropyLoss -- which no bitwise comparison
# survives.  A quarter of the median keeps about three quarters of the refreshed teacher's pixels.
MOVING_SCALE = {"v2": 1.0, "v3": 0.25, "vgg": 1.0}


def _run(model, dev, dtype, mode, every=None, steps=3, its=1, dp=False, pass_weak=True, scale=1.0):
    """One memoised run.  mode "online": the trainer with online_labels (and online_labels_every = `every`, ema 0.9); nothing synchronises the
    teacher by hand.  mode "composition": the trainer WITHOUT the keyword (with the EMA when `every` is given), fed the labels of a
    Composition that the test refreshes where refresh_due says so.  -> dict(tau, labels, scalars, state, shares, refreshes)."""
    key = (model, dtype, mode, every, steps, its, dp, pass_weak, scale)
    if key in _RUNS:
        return _RUNS[key]
    data = _views(dev, steps, its)
    comp = Composition(model, dev, dtype)
    tau = comp.threshold(data[0][0][1], scale=scale)                           # the median confidence on step 0's weak view (x scale)
    ema = {} if every is None else {"ema_decay": 0.9}
    res = dict(tau=tau, labels=[], scalars=[], shares=[], refreshes=0)
    with (one_rank_group(dev, PORT) if dp else contextlib.nullcontext()) as pg:
        if mode == "online":
            kw = dict(ema, online_labels=tau)
            if every is not None:
                kw["online_labels_every"] = every
            tr = _trainer(model, dev, dtype, pg, its, **kw)
            assert tr.frozen_sha256 == tsf.state_sha256(comp.params)
        else:
            tr = _trainer(model, dev, dtype, pg, its, **ema)
            assert not hasattr(tr, "fixed") and not hasattr(tr, "label_counts") and tr.teacher is None
        for mb in data:
            strong = [m[0] for m in mb] if its > 1 else mb[0][0]
            weak = [m[1] for m in mb] if its > 1 else mb[0][1]
            if mode == "online":
                tr.step(strong, None, teacher_image=weak) if pass_weak else tr.step(strong)
                torch.cuda.synchronize()
                res["labels"].append(tr.label.clone())                         # (iter_size > 1: the last micro-batch's)
            else:
                labs = [comp.label(m[1], tau).clone() for m in mb]
                tr.step(strong, labs if its > 1 else labs[0])
                res["labels"].append(labs[-1])
                res["shares"].append(float((torch.stack(labs) != 255).float().mean()))
                if every is not None and refresh_due(tr.ema_updates, every):
                    comp.follow(tr.ema_params)
                    res["refreshes"] += 1
            res["scalars"].append(R.scalars(tr))
        res["losses"] = R.finite_losses(tr, f"{model} {mode}")
        res["state"] = _state(tr)
        if mode == "online" and every is not None:
            res["refreshes"] = tr.teacher_refreshes
            res["teacher_keys"] = list(tr.teacher_state_dict()) == list(tr.fixed_params) and tr.teacher_params is tr.fixed_params
        del tr
    del comp
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


def _assert_same(a, b, what, steps=None):
    n = len(a["scalars"]) if steps is None else steps
    for i in range(n):
        assert torch.equal(a["labels"][i], b["labels"][i]), \
            f"{what}: {int((a['labels'][i] != b['labels'][i]).sum())} labels of step {i + 1} differ"
        assert torch.equal(a["scalars"][i], b["scalars"][i]), f"{what}: the scalars of step {i + 1} differ"
    if steps is None:
        sa, sb = a["state"], b["state"]
        assert sa.keys() == sb.keys()
        diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
        assert not diff, f"{what}: {len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", MODELS)
def test_fixed_teacher_equals_the_composition(dev, model, dtype):
    """(b) 3 steps, a weak view that differs from the strong one: the labels of every step, the loss scalars, every tensor of state_dict(),
    the momentum and the packed operands.  tau: the median of the composition's confidence on step 0; the kept share of every step must lie
    in (0.1, 0.9), so a kernel that keeps everything or nothing cannot pass."""
    comp = _run(model, dev, dtype, "composition")
    print(f"{model}: tau = {comp['tau']!r}, kept shares {comp['shares']}")
    assert 0.0 <= comp["tau"] < 1.0 and all(0.1 < s < 0.9 for s in comp["shares"]), comp["shares"]
    got = _run(model, dev, dtype, "online")
    assert got["tau"] == comp["tau"]
    _assert_same(got, comp, f"{model} fixed teacher")
    # losses() read once, after 3 steps: the share of all three steps' pixels
    assert abs(got["losses"]["labelled"] - sum(comp["shares"]) / 3) < 1e-6 and "labelled" not in comp["losses"]


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("model", MODELS)
def test_moving_teacher_equals_the_composition_refreshed_by_hand(dev, model, every):
    """(c) ema_decay = 0.9, 4 steps: bit for bit the composition whose plan receives the other trainer's ema_params + repack() behind the
    updates refresh_due names; the refresh count; until the first refresh the run is the fixed-teacher run."""
    sc = MOVING_SCALE[model]
    comp = _run(model, dev, BF, "composition", every=every, steps=4, scale=sc)
    got = _run(model, dev, BF, "online", every=every, steps=4, scale=sc)
    print(f"{model}: tau = {comp['tau']!r}, kept shares {comp['shares']}")
    assert got["refreshes"] == comp["refreshes"] == 4 // every and got["teacher_keys"]
    _assert_same(got, comp, f"{model} moving teacher, every {every}")
    fixed = _run(model, dev, BF, "online", steps=4, scale=sc)
    _assert_same(got, fixed, f"{model} until the first refresh", steps=every)
    if model != "vgg":      # (the BatchNorm statistics move at once; the reduced VGG has none and its bf16 weights barely move in 4 steps)
        assert any(not torch.equal(got["labels"][i], fixed["labels"][i]) for i in range(every, 4)), "the refresh never changed a label"


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_iter_size_2(dev, model):
    comp = _run(model, dev, BF, "composition", its=2)
    _assert_same(_run(model, dev, BF, "online", its=2), comp, f"{model} iter_size 2")


def test_no_teacher_image_means_the_students_image(dev):
    """teacher_image=None == passing the student's image; a label passed with the keyword raises, and so does a teacher_image without it."""
    data = _views(dev, 2)
    comp = Composition("v2", dev, BF)
    tau = comp.threshold(data[0][0][0])
    a, b = _trainer("v2", dev, online_labels=tau), _trainer("v2", dev, online_labels=tau)
    for mb in data:
        a.step(mb[0][0])
        b.step(mb[0][0], None, teacher_image=mb[0][0])
        torch.cuda.synchronize()
        assert torch.equal(a.label, b.label) and torch.equal(R.scalars(a), R.scalars(b))
        assert torch.equal(a.label, comp.label(mb[0][0], tau))
    assert 0.0 < a.losses()["labelled"] < 1.0
    with pytest.raises(ValueError, match="labels come from the teacher"):
        a.step(data[0][0][0], torch.zeros(SIZE, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match=r"teacher_image of shape"):
        a.step(data[0][0][0], None, teacher_image=data[0][0][0][:1])
    plain = _trainer("v2", dev)
    with pytest.raises(ValueError, match="online_labels"):
        plain.step(data[0][0][0], torch.zeros(SIZE, dtype=torch.int64, device=dev), teacher_image=data[0][0][0])
    with pytest.raises(ValueError, match="needs a label"):
        plain.step(data[0][0][0])
    with pytest.raises(RuntimeError, match="does not move"):
        a.teacher_refreshes
    for kw, named in [(dict(online_labels=1.0), "online_labels 1.0"), (dict(online_labels=-0.1), "online_labels -0.1"),
                      (dict(online_labels=float("nan")), "online_labels nan"),
                      (dict(online_labels=0.5, online_labels_every=2), "online_labels_every needs ema_decay"),
                      (dict(online_labels_every=2, ema_decay=0.9), "online_labels_every needs online_labels"),
                      (dict(online_labels=0.5, online_labels_every=0, ema_decay=0.9), "online_labels_every 0")]:
        with pytest.raises(ValueError, match=named):
            _trainer("v2", dev, **kw)


def test_one_rank_rccl_group_equals_the_single_gpu_trainer(dev):
    _assert_same(_run("v2", dev, BF, "online", every=2, steps=4, dp=True), _run("v2", dev, BF, "online", every=2, steps=4), "one-rank RCCL group")


# ---- (e) resume ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_resume_between_two_refreshes(dev, tmp_path, model):
    """N = 2: 3 steps (one refresh behind step 2), save, a fresh trainer, load, 3 more == 6 steps; `labelled` of every read-out included."""
    data = _views(dev, 6)
    tau = Composition(model, dev, BF).threshold(data[0][0][1], scale=MOVING_SCALE[model])
    kw = dict(online_labels=tau, online_labels_every=2, ema_decay=0.9)

    def steps(tr, part, out):
        for mb in part:
            tr.step(mb[0][0], None, teacher_image=mb[0][1])
            out["scalars"].append(R.scalars(tr))
            out["labelled"].append(tr.losses()["labelled"])
            out["labels"].append(tr.label.clone())

    a = dict(scalars=[], labelled=[], labels=[])
    tr = _trainer(model, dev, **kw)
    steps(tr, data, a)
    a["state"], a["teacher"], refreshes = _state(tr), {k: v.cpu() for k, v in tr.fixed_params.items()}, tr.teacher_refreshes
    print(f"{model}: tau = {tau!r}, labelled {a['labelled']}")
    # (a teacher may be confident everywhere: 1.0 is a legitimate share; none may label nothing, MOVING_SCALE)
    assert refreshes == 3 and all(0.0 < s <= 1.0 for s in a["labelled"]) and len(set(a["labelled"])) > 1, a["labelled"]
    del tr
    b = dict(scalars=[], labelled=[], labels=[])
    tr = _trainer(model, dev, **kw)
    steps(tr, data[:3], b)
    ts = tr.training_state()
    assert ts["hyper"]["online_labels"] == tau and ts["hyper"]["online_labels_every"] == 2 and ts["teacher"]["refreshes"] == 1
    assert set(ts["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported"} and "frozen_sha256" in ts
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = _trainer(model, dev, **kw)
    tr.load_training_state(ts)
    assert tr.teacher_refreshes == 1 and tr.it_done == 3
    steps(tr, data[3:], b)
    b["state"] = _state(tr)
    assert tr.teacher_refreshes == 3 and b["labelled"] == a["labelled"]
    _assert_same(a, b, f"{model} resumed after step 3")
    assert all(torch.equal(v.cpu(), a["teacher"][k]) for k, v in tr.fixed_params.items()), "the teacher after the resumed run differs"
    if model != "v2":
        return
    # the refusals: the keyword added or dropped, tau or N differing, another start model
    plain = _trainer(model, dev, ema_decay=0.9)
    with pytest.raises(ValueError, match=r"online_labels \(state: [0-9.e-]+, this trainer: None\)"):
        plain.load_training_state(ts)
    with pytest.raises(ValueError, match=r"online_labels \(state: None, this trainer: [0-9.e-]+\)"):
        tr.load_training_state(plain.training_state())
    for other, named in [(dict(kw, online_labels=tau / 2), r"online_labels \(state"), (dict(kw, online_labels_every=1), r"online_labels_every \(state: 2, this trainer: 1\)"),
                         (dict(online_labels=tau, ema_decay=0.9), r"online_labels_every \(state: 2, this trainer: None\)")]:
        with pytest.raises(ValueError, match=named):
            _trainer(model, dev, **other).load_training_state(ts)
    with pytest.raises(ValueError, match="frozen_sha256 differs"):
        _trainer(model, dev, seed=1, **kw).load_training_state(ts)
    # a trainer without the keyword writes the state it always wrote
    pts = plain.training_state()
    assert set(pts["accumulators"]) == {"hout", "bad_labels"} and "frozen_sha256" not in pts and "teacher" not in pts
    assert not any(k.startswith("online") for k in pts["hyper"])


# ---- (f) the tool --------------------------------------------------------------------------------------------------------------------------------------
def _image_files(root):
    """4 PNG images, a ONE-column list, and no label file anywhere."""
    from PIL import Image
    rng = np.random.default_rng(0)
    (root / "train_img").mkdir(parents=True)
    lines = []
    for i in range(4):
        blocks = rng.integers(0, 256, (6, 12, 3), dtype=np.uint8)
        img = np.kron(blocks, np.ones((16, 16, 1), np.uint8)).astype(np.int16) + rng.integers(-20, 21, (96, 192, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(root / "train_img" / f"t{i}.png")
        lines.append(f"train_img/t{i}.png")
    (root / "images.lst").write_text("\n".join(lines) + "\n")
    assert not [f for f in os.listdir(root) if "lab" in f]


def _tool_threshold(tool_model, root, dev):
    """T of the tool test: the 1 % quantile of the confidence of the tool's START model (its constructor init at the tool's default seed, as
    main() builds it with --from-scratch) over the four images as the loader hands them out WITHOUT augmentation -- the teacher's view at
    step 0 -- formed by a separate eval-mode plan and the host restatement (Composition.confidence), never by the code under test.  The first
    line's share is then about 0.99.  Not the median: DeepLabv3's constructor init is confident (median 0.9999994) and the teacher refreshed
    from a one-step-old student is not (MOVING_SCALE above); at the median it labels nothing from step 2 on and the losses are NaN, at the
    1 % quantile (0.547) the shares measured on MI355X are 0.988, 0.727, 0.598, 0.558, 0.532, 0.507."""
    from simt_amd import model_spec as ms
    from simt_amd.data.pipeline import IMG_MEAN, GpuLoader
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    from simt_amd.tools.trainV2_simt import single_model_state
    B, H, W = SIZE
    model = {"DeepLab": "v2", "DeepLabv3": "v3", "DeepLabVGG": "vgg"}[tool_model]
    if model == "v2":
        start = ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), {}
    else:
        start = single_model_state(tool_model, 19, (3, 4, 6), seed=1234), ({"layers": (3, 4, 6)} if model == "v3" else {})
    comp = Composition(model, dev, BF, start=start)
    ds = cityscapesPseudo(str(root), str(root / "images.lst"), crop_size=(W, H), scale=False, mirror=False, mean=IMG_MEAN, labels=False)
    conf = [comp.confidence(img) for (img, lab, _s, _n) in GpuLoader(ds, B, shuffle=False, num_workers=1, device=dev, epochs=1) if lab is None]
    assert len(conf) == 2
    tau = min(float(np.float32(np.quantile(np.concatenate(conf), 0.01))), 0.9999)
    del comp
    torch.cuda.empty_cache()
    return tau


@pytest.mark.parametrize("tool_model", ["DeepLab", "DeepLabv3", "DeepLabVGG"])
def test_tool_trains_on_images_alone_and_resumes(dev, tmp_path, capsys, monkeypatch, tool_model):
    """trainV1_warmup --online-labels T --ema 0.9 --online-labels-every 1 --colour-jitter --mask-patches --mask-patch-size 16 on 4 PNG images
    with no label file on disk, a one-column list, B = 2, 129,65: 3 + 3 == 6 through --train-state in the loss lines and in every tensor
    of the final and the EMA snapshot; `labelled` of the first line lies in (0, 1); the flag-off run launches no simt_online_label and builds
    no second plan; a resume with the flag changed is refused."""
    pytest.importorskip("PIL.Image")
    from simt_amd import step_single
    from simt_amd.tools import trainV1_warmup as tool
    from test_gpu_patch_mask import _tool_files
    root = tmp_path / "data"
    _image_files(root)
    T = _tool_threshold(tool_model, root, dev)
    assert 0.0 < T < 1.0
    common = ["--learning-rate", "2.5e-4", "--model", tool_model, "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
              "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2",
              "--data-dir-target", str(root)]
    flags = ["--data-list-target", str(root / "images.lst"), "--online-labels", str(T), "--ema", "0.9", "--online-labels-every", "1",
             "--colour-jitter", "--mask-patches", "--mask-patch-size", "16"]
    calls, built = [], []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    for mod, name in ((tool, "WarmupTrainer"), (step_single, "WarmupSingleTrainer")):
        cls = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _cls=cls, **k: (built.append(_cls(*a, **k)), built[-1])[1])

    def run(tag, stop, *more):
        del calls[:], built[:]
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6, *flags)
    lines = R._loss_lines(out_a)
    assert len(lines) == 6 and not re.search(r"loss_seg\w* = nan", out_a), out_a
    shares = [float(re.search(r" labelled = ([0-9.]+)", ln).group(1)) for ln in lines]
    print(f"{tool_model}: T = {T}, labelled {shares}")
    assert 0.0 < shares[0] < 1.0, shares
    assert calls.count("simt_online_label") == 6 and len(built) == 1 and built[0].teacher_refreshes == 6
    assert re.search(r"online labels: a teacher that follows the weight EMA \(decay 0\.9\), refreshed every 1 update\(s\) labels every batch, "
                     r"kept where its confidence is > [0-9.]+; the teacher sees the batch before --colour-jitter, --mask-patches", out_a), out_a
    out_b1, _ = run("b", 3, *flags, "--train-state", state)
    assert R._loss_lines(out_b1) == lines[:3]
    out_b2, snap_b = run("b", 6, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert R._loss_lines(out_b2) == lines[3:], (out_a, out_b2)
    R._same_snapshot(snap_a, snap_b)
    R._same_snapshot(snap_a[:-4] + "_ema.pth", snap_b[:-4] + "_ema.pth")
    for other in (flags[:2] + ["--ema", "0.9", "--colour-jitter", "--mask-patches", "--mask-patch-size", "16"],
                  flags[:3] + [str(T / 2)] + flags[4:], flags[:7] + ["2"] + flags[8:]):
        with pytest.raises(SystemExit, match="online_labels"):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state])
    capsys.readouterr()
    # a fixed teacher on the same files: no refresh, one start-up line that says so
    out_f, _ = run("f", 1, *flags[:4], "--colour-jitter")
    assert "online labels: a fixed teacher (the start weights) labels every batch" in out_f and built[0].teacher is None
    # the flag-off run: the tool as it was -- label files, a two-column list, no second plan, no label launch
    _tool_files(tmp_path / "pairs")
    off = [a if a != str(root) else str(tmp_path / "pairs") for a in common] + ["--data-list-target", str(tmp_path / "pairs" / "pseudo.lst")]
    del calls[:], built[:]
    tool.main(off + ["--snapshot-dir", str(tmp_path / "o"), "--num-steps-stop", "2"])
    out_o = capsys.readouterr().out
    assert "simt_online_label" not in calls and "online labels" not in out_o and "labelled" not in out_o and len(R._loss_lines(out_o)) == 2
    assert len(built) == 1 and not hasattr(built[0], "fixed") and not hasattr(built[0], "label_counts") and built[0].online_labels is None
