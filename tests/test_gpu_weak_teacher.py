"""The weak-view teacher on the device: simt_class_mix_items, simt_head_loss_views / simt_head_grad_views, the trainers'
`teacher_view`, the loader's two views and trainV2_simt --weak-teacher.

The yardsticks: tests/_weak_teacher_ref.py (the item map on tests/_class_mix_ref.py; the losses of oracle/simt_oracle.py with the frozen posterior
gathered by the map) and the one-view launches themselves -- a NULL map must be them word for word, a constant map per item must be them on
the frozen operand gathered by items.  Selections and gathers are compared BITWISE; the losses and gradients under a mixed map go to float64
through the bars of tests/_head_bar.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as cmref
import _head_bar as hb
import _weak_teacher_ref as wt
from _launch_oracle import SENTINEL
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import IMG_MEAN, GpuLoader
from simt_amd.engine import TrunkPlan, multi_heads
from simt_amd.engine_v3 import v3_state_shapes
from simt_amd.step import Hyper, SimTTrainer
from simt_amd.step_single import SimTSingleTrainer
from test_gpu_class_mix import (CHOICES, CROP, HS, N_CLASSES, WS, _assert_same_batches, _common, _images, _labels, _loss_lines, _same_snapshot,
                                _tool_files, _write_files)
from test_gpu_head_ntm import HEAD_GEOMS, close, nhwc_pad
from test_gpu_resume import HP, SMALL, VGG_LR, full_state, scalars
from test_gpu_single import VGG_SMALL, _v3_state, _vgg_state

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF, F32 = torch.bfloat16, torch.float32
GUARD, PATTERN = 64, 0x5A


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 1. the mix kernel --------------------------------------------------------------------------------------------------------------------------
# (B, h, w, classes): h*w % 4 in {0, 1, 3}; fewer pixels than one quad; just over one workgroup of quads (256 * 4 pixels); B = 2 and 5; 32 classes
MIX_SHAPES = [(2, 40, 64, 19), (5, 37, 41, 19), (2, 9, 7, 19), (5, 1, 3, 19), (2, 1, 1028, 19), (5, 3, 343, 19), (2, 8, 8, 32)]


def _mix_desc(x, lab, x_out, lab_out, part, B, h, w, Cn, apply, rank):
    d = L.ClassMixDesc()
    d.x, d.lab, d.x_out, d.lab_out, d.part = x.data_ptr(), lab.data_ptr(), x_out.data_ptr(), lab_out.data_ptr(), part.data_ptr()
    d.B, d.h, d.w, d.n_classes = B, h, w, Cn
    for i in range(B):
        d.partner[i], d.apply[i] = (i + 1) % B, 1 if apply[i] else 0
        C.memmove(d.rank[i], np.ascontiguousarray(rank[i], dtype=np.uint8).ctypes.data, Cn)
    return d


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_items_equals_the_mix_and_the_item_map_bit_for_bit(dev, shape):
    B, h, w, Cn = shape
    assert (h * w) % 4 in (0, 1, 3)
    n_x, n_l, n_i = B * 3 * h * w, B * h * w, B * h * w
    rng = np.random.default_rng([7, B, h, w, Cn])
    partner = [(i + 1) % B for i in range(B)]
    both = 0
    for kind in ("blocky", "special_a"):                                  # special_a: item 0 has no valid label (nothing to paste from it), item 1 one class
        lab, xb = _labels(kind, B, h, w, Cn), _images(B, h, w)
        rank = rng.permuted(np.tile(np.arange(Cn, dtype=np.uint8), (B, 1)), axis=1)
        for apply in (np.ones(B, bool), np.arange(B) % 2 == 0):            # the second: items with apply = 0
            x_d, lab_d = torch.from_numpy(xb).to(dev).view(F32), torch.from_numpy(lab).to(dev)
            part = torch.zeros(B * L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)
            x0, l0 = torch.empty(B, 3, h, w, device=dev), torch.empty(B, h, w, dtype=torch.int64, device=dev)
            x1, l1 = torch.empty_like(x0), torch.empty_like(l0)
            pad = (-n_i) % 4
            buf = torch.full((GUARD + n_i + pad + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
            item = buf[GUARD:GUARD + n_i].view(B, h, w)
            assert item.data_ptr() % 4 == 0
            L.call("simt_label_presence", lab_d.data_ptr(), B, h * w, Cn, part.data_ptr(), _stream(dev))
            L.call("simt_class_mix", C.byref(_mix_desc(x_d, lab_d, x0, l0, part, B, h, w, Cn, apply, rank)), _stream(dev))
            L.call("simt_class_mix_items", C.byref(_mix_desc(x_d, lab_d, x1, l1, part, B, h, w, Cn, apply, rank)), item.data_ptr(), _stream(dev))
            torch.cuda.synchronize()
            assert torch.equal(x0.view(torch.int32), x1.view(torch.int32)), f"{kind}: image words differ from simt_class_mix"
            assert torch.equal(l0, l1), f"{kind}: labels differ from simt_class_mix"
            want = wt.item_map(lab, partner, apply, rank, Cn)
            got = item.cpu().numpy()
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{kind}: {len(bad)} item bytes differ, first at {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
            g = buf.cpu().numpy()
            assert (g[:GUARD] == PATTERN).all() and (g[GUARD + n_i:] == PATTERN).all(), f"{kind}: a guard byte around item_out was written"
            for i in range(B):
                if not apply[i]:
                    assert (got[i] == i).all()
            both += int(any(len(np.unique(got[i])) == 2 for i in range(B)))
            if kind == "special_a" and apply.all():
                assert (got[B - 1] == B - 1).all()                          # its partner, item 0, has no valid label
    assert both > 0 or h * w < 4, "no item of any case holds both values: the case shows nothing"


def test_mix_items_refuses_a_null_or_misaligned_map_and_writes_nothing(dev):
    B, h, w, Cn = 2, 8, 8, 19
    x, lab = torch.zeros(B, 3, h, w, device=dev), torch.zeros(B, h, w, dtype=torch.int64, device=dev)
    x_out, lab_out = torch.full((B, 3, h, w), 7.0, device=dev), torch.full((B, h, w), 7, dtype=torch.int64, device=dev)
    part = torch.zeros(B * L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)
    item = torch.full((B * h * w + 8,), 7, dtype=torch.uint8, device=dev)
    apply, rank = np.ones(B, bool), np.tile(np.arange(Cn, dtype=np.uint8), (B, 1))
    d = _mix_desc(x, lab, x_out, lab_out, part, B, h, w, Cn, apply, rank)
    L.call("simt_label_presence", lab.data_ptr(), B, h * w, Cn, part.data_ptr(), _stream(dev))
    assert item.data_ptr() % 4 == 0
    for ptr in (None, item.data_ptr() + 1, item.data_ptr() + 2):
        with pytest.raises(L.SimtHipError):
            L.call("simt_class_mix_items", C.byref(d), ptr, _stream(dev))
    torch.cuda.synchronize()
    assert (x_out == 7.0).all() and (lab_out == 7).all() and (item == 7).all()
    L.call("simt_class_mix_items", C.byref(d), item.data_ptr() + 4, _stream(dev))          # the descriptor itself is sound
    torch.cuda.synchronize()
    assert (x_out == 0).all() and (lab_out == 0).all() and (item[:4] == 7).all() and (item[4 + B * h * w:] == 7).all()
    assert (item[4:4 + B * h * w].view(B, h, w)[0] == 1).all() and (item[4:4 + B * h * w].view(B, h, w)[1] == 0).all()      # one class everywhere: all pasted


# ---- 2. the head --------------------------------------------------------------------------------------------------------------------------------
VIEW_GEOMS = {"up8_two_chunks": HEAD_GEOMS["up8_two_chunks"], "b3": (3, 5, 9, 33, 65)}
assert VIEW_GEOMS["up8_two_chunks"] == (2, 13, 37, 97, 289)
# (single, fix_logits, up_half_pixel): DeepLab-v2, a two-head model that upsamples inside, DeepLab-VGG16, DeepLabv3
FORMS = {"two_head": (False, 0, 0), "two_head_logits_half": (False, 1, 1), "single_vgg": (True, 0, 0), "single_v3": (True, 1, 1)}
D = dict(hb.DEFAULT_D)


PEAK_SEED = 3


def _head_inputs(geom, K, peaked=False):
    """(pred1, pred2, fixed2, label, [ntm1, ntm2]) as tests/_head_bar.head_inputs draws them.  peaked: the frozen logits of item i are N(0, 1)
    (a generator of their own, PEAK_SEED) plus 8 on class i: the posterior maximum is ~0.99 on class i at a typical pixel.  Its MINIMUM over
    the ~1 000 low-res pixels is what the condition of test_head_views_against_float64 needs above th_high = 0.8: a pixel whose own-class
    draw falls below -3.2 misses it, which half of all seeds contain at the larger geometry (seeds 0-7: minima 0.70 .. 0.83); at PEAK_SEED the
    minimum is 0.83 / 0.86 there and 0.86 / 0.89 at the smaller one (probabilities / logits interpolated).  The test asserts this from the
    float64 restatement before it looks at the kernel."""
    p1, p2, f2, lab, ntm = hb.head_inputs(VIEW_GEOMS[geom], K, CD)
    if peaked:
        f2 = torch.randn(*f2.shape, generator=torch.Generator().manual_seed(PEAK_SEED))
        for i in range(f2.shape[0]):
            f2[i, i] += 8
    return p1, p2, f2, lab, ntm


def _blocky_map(B, H, W, seed=3):
    """8 x 8 blocks, values in {i, (i + 1) % B}, both in every item."""
    rng = np.random.default_rng([seed, B, H, W])
    sel = np.kron(rng.integers(0, 2, (B, -(-H // 8), -(-W // 8))), np.ones((1, 8, 8), np.int64))[:, :H, :W].astype(bool)
    sel[:, 0, 0], sel[:, -1, -1] = False, True
    own = np.arange(B)[:, None, None]
    m = np.where(sel, (own + 1) % B, own).astype(np.uint8)
    assert all(set(np.unique(m[i])) == {i, (i + 1) % B} for i in range(B))
    return m, sel


class _Head:
    """The head / NTM launches of the SimT trainers on explicit low-res logits, in the form the trainers ask for (dpred*_t in bf16 with a
    pitch) plus the fp32 gradients; every output is pre-filled, so that a launch that wrote nothing shows."""

    def __init__(self, dev, inp, K, form, maps):
        self.dev, self.K, self.maps = dev, K, maps
        self.single, self.fix_logits, self.half = FORMS[form]
        p1, p2, f2, lab, ntm = inp
        Cn = 19
        Q = self.Q = Cn + K
        B, _, h, w = p2.shape
        H, W = lab.shape[1:]
        self.shape = (B, h, w, H, W)
        st = ops.stream_ptr()
        self.ldp = ldp = max(32, ops.round_up(Q, 8))
        self.p1, self.p2 = nhwc_pad(p1, ldp).to(dev), nhwc_pad(p2, ldp).to(dev)
        fl = nhwc_pad(f2, 32).to(dev)
        self.fixp = fl
        if not self.fix_logits:
            self.fixp = torch.zeros_like(fl)
            ops.softmax_rows(fl, 32, self.fixp, 32, B * h * w, Cn)
        self.lab = lab.to(dev)
        self.cd = CD.float().to(dev)
        slots = (1,) if self.single else (0, 1)
        self.ntm = [n.clone().to(dev) for n in ntm]
        self.ngrad = [torch.zeros(Q, Cn, device=dev) for _ in range(2)]
        self.wraw = [so.w_init(Cn, K).to(dev) for _ in range(2)]
        wm, wv = [torch.zeros(Q, Q, device=dev) for _ in range(2)], [torch.zeros(Q, Q, device=dev) for _ in range(2)]
        self.T = [torch.zeros(Q, Cn, device=dev) for _ in range(2)]
        ni = L.NtmInnerDesc()
        for k in slots:
            ni.ntm[k], ni.w[k], ni.ntm_grad[k] = self.ntm[k].data_ptr(), self.wraw[k].data_ptr(), self.ngrad[k].data_ptr()
            ni.w_m[k], ni.w_v[k], ni.T_out[k] = wm[k].data_ptr(), wv[k].data_ptr(), self.T[k].data_ptr()
        ni.class_dist, ni.Q, ni.C, ni.steps, ni.step0, ni.single = self.cd.data_ptr(), Q, Cn, 10, 0, int(self.single)
        ni.lr, ni.beta1, ni.beta2, ni.eps = float(D["lr_T"]), 0.9, 0.999, 1e-8
        L.call("simt_ntm_inner_loop", C.byref(ni), st)
        torch.cuda.synchronize()
        self.leak = [g.clone() for g in self.ngrad]
        lib = L.load()
        self.nblk, self.pf, self.nk, self.nh = lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Cn), lib.simt_head_keys_count(), lib.simt_head_hout_floats(Q, Cn)
        self.QP = ops.round_up(Q, 8)

    def run(self, item="plain", fixp=None, mode=0, expect_refusal=False):
        """item: "plain" -> simt_head_loss / simt_head_grad; None -> the _views symbols with a NULL map; a uint8 [B,H,W] array -> with it.
        fixp: another frozen operand ([B*h*w, 32]) than the instance's."""
        dev, Q, Cn, QP, ldp = self.dev, self.Q, 19, self.QP, self.ldp
        B, h, w, H, W = self.shape
        st = ops.stream_ptr()
        fixp = self.fixp if fixp is None else fixp
        part = torch.zeros(self.nblk, self.pf, device=dev)
        keys = torch.zeros(self.nk, device=dev, dtype=torch.int64)
        hout, lout = torch.full((self.nh,), 7.0, device=dev), torch.zeros(16, device=dev)
        g1 = torch.zeros(2, B, H, w, QP, device=dev)
        dp = [torch.full((B * h * w, ldp), 7.0, device=dev) for _ in range(2)]
        dt = [torch.full((B * h * w, ldp), SENTINEL, dtype=BF, device=dev) for _ in range(2)]
        for k in range(2):
            self.ngrad[k].copy_(self.leak[k])
        hd = L.HeadDesc()
        hd.pred1, hd.pred2 = (None if self.single else self.p1.data_ptr()), self.p2.data_ptr()
        hd.fixp, hd.label = fixp.data_ptr(), self.lab.data_ptr()
        hd.T1, hd.T2 = (None if self.single else self.T[0].data_ptr()), self.T[1].data_ptr()
        hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
        hd.dpred1_f32, hd.dpred2_f32 = (None if self.single else dp[0].data_ptr()), dp[1].data_ptr()
        hd.dpred1_t, hd.dpred2_t = (None if self.single else dt[0].data_ptr()), dt[1].data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Cn, Q
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = ldp, 32, QP, ldp, ldp, ops.dt_code(BF)
        hd.th_high, hd.th_low = float(D["th"][0]), float(D["th"][1])
        hd.lambda_seg, hd.lambda_place, hd.gscale = (0.0 if self.single else float(D["lambda_seg"])), float(D["lambda_place"]), 1.0
        hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = mode, int(self.single), self.half, self.fix_logits
        conf = lws = None
        if self.maps:
            conf, lws = (torch.full((B, H, W), 77, dtype=torch.uint8, device=dev) for _ in range(2))
            hd.conf_out, hd.label_ws = conf.data_ptr(), lws.data_ptr()
        item_d = None
        if isinstance(item, np.ndarray):
            assert item.dtype == np.uint8 and item.shape == (B, H, W)
            item_d = torch.from_numpy(item).to(dev)
        loss = (lambda: L.call("simt_head_loss", C.byref(hd), st)) if isinstance(item, str) else \
            (lambda: L.call("simt_head_loss_views", C.byref(hd), None if item_d is None else item_d.data_ptr(), st))
        grad = (lambda: L.call("simt_head_grad", C.byref(hd), st)) if isinstance(item, str) else \
            (lambda: L.call("simt_head_grad_views", C.byref(hd), None if item_d is None else item_d.data_ptr(), st))
        if expect_refusal:
            for fn in (loss, grad):
                with pytest.raises(L.SimtHipError):
                    fn()
        else:
            loss()
            npd = L.NtmPostDesc()
            for k in ((1,) if self.single else (0, 1)):
                npd.ntm[k], npd.w[k], npd.ntm_grad[k] = self.ntm[k].data_ptr(), self.wraw[k].data_ptr(), self.ngrad[k].data_ptr()
            npd.class_dist, npd.hout, npd.lout, npd.Q, npd.C = self.cd.data_ptr(), hout.data_ptr(), lout.data_ptr(), Q, Cn
            npd.lambda_seg = 0.0 if self.single else float(D["lambda_seg"])
            npd.lambda_convex, npd.lambda_volume, npd.lambda_anchor = (float(v) for v in D["lam"])
            npd.gscale, npd.single = 1.0, int(self.single)
            L.call("simt_ntm_post", C.byref(npd), st)
            grad()
        torch.cuda.synchronize()
        out = {"hout": hout.cpu().view(torch.int32), "lout": lout.cpu().view(torch.int32), "dp2": dp[1].cpu().view(torch.int32),
               "dt2": dt[1].cpu().view(torch.int16), "ntm_grad2": self.ngrad[1].cpu().view(torch.int32)}
        if not self.single:
            out.update({"dp1": dp[0].cpu().view(torch.int32), "dt1": dt[0].cpu().view(torch.int16), "ntm_grad1": self.ngrad[0].cpu().view(torch.int32)})
        if self.maps:
            out.update({"conf": conf.cpu(), "lws": lws.cpu()})
        return out

    def back(self, raw_bits, dtype=F32):
        B, h, w, _H, _W = self.shape
        g = raw_bits.view(dtype)
        return g[:, :self.Q].reshape(B, h, w, self.Q).permute(0, 3, 1, 2)

    def gathered(self, items):
        B, h, w, _H, _W = self.shape
        return self.fixp.view(B, h * w, 32)[torch.as_tensor(items, device=self.dev)].reshape(B * h * w, 32).contiguous()


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        diff = int((a[k] != b[k]).sum())
        assert diff == 0, f"{what}: {diff} of {a[k].numel()} words of {k} differ (first at {(a[k] != b[k]).nonzero()[0].tolist()})"


# every (geometry, K, form) with and without the byte maps, and the two VIEWS builds K = 3 and 15 do not reach: K = 6 (Q = 25, the second
# compile-time-count build) and K = 4 (Q = 23, the run-time-count build of the narrow width)
BITWISE = [(g, K, f, m) for g in VIEW_GEOMS for K in (3, 15) for f in FORMS for m in (True, False)] + \
    [("b3", 6, "two_head", True), ("b3", 6, "single_v3", False), ("b3", 4, "two_head_logits_half", True), ("b3", 4, "single_vgg", False)]


@pytest.mark.parametrize("geom,K,form,maps", BITWISE, ids=lambda v: {True: "byte_maps", False: "no_byte_maps"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_head_views_bitwise(dev, geom, K, form, maps):
    """(a) a NULL map is the one-view launch; (b) a constant map per item is the one-view launch on the frozen operand gathered by items, the
    anchor rows of hout included; (c) under a blocky map conf_out is, per pixel, the select between the one-view conf_out on the frozen
    operand itself and on the rolled one; (d) a byte >= B reads item B - 1."""
    hd = _Head(dev, _head_inputs(geom, K), K, form, maps)
    B, h, w, H, W = hd.shape
    plain = hd.run("plain")
    assert not (plain["hout"].view(F32)[:14] == 7.0).any() and not (plain["dp2"].view(F32)[:, :hd.Q] == 7.0).all()
    _same(plain, hd.run(None), "(a) NULL map")
    roll = [(i + 1) % B for i in range(B)]
    const = [roll, [B - 1] * B] + ([[2, 0, 0]] if B == 3 else [])
    rolled = None
    for s in const:
        item = np.array(s, dtype=np.uint8)[:, None, None] * np.ones((B, H, W), np.uint8)
        want = hd.run("plain", fixp=hd.gathered(s))
        _same(want, hd.run(item), f"(b) constant map {s}")
        if s == roll:
            rolled = want
            moved = [k for k in want if (want[k] != plain[k]).any()]
            assert "hout" in moved and "dp2" in moved, f"the rolled frozen operand changes nothing ({moved}): the case shows nothing"
    m, sel = _blocky_map(B, H, W)
    mixed = hd.run(m)
    if maps:
        want = torch.where(torch.from_numpy(sel), rolled["conf"], plain["conf"])
        assert torch.equal(mixed["conf"], want), f"(c) {int((mixed['conf'] != want).sum())} confidence labels are not the select"
        assert (rolled["conf"] != plain["conf"])[torch.from_numpy(sel)].any() and torch.equal(mixed["lws"], plain["lws"])
    assert (mixed["hout"] != plain["hout"]).any() and (mixed["hout"] != rolled["hout"]).any()
    high = m.copy()
    high[m == B - 1] = 200
    high[0, 0, 0] = B if m[0, 0, 0] == B - 1 else high[0, 0, 0]
    high[(m == B - 1) & (np.arange(W)[None, None, :] % 2 == 0)] = 255
    assert (high >= B).any() and np.array_equal(np.minimum(high, B - 1), m)
    _same(mixed, hd.run(high), "(d) bytes >= B against the map clamped on the host")


def test_head_views_refuse_the_warmup_mode_with_a_map(dev):
    hd = _Head(dev, _head_inputs("b3", 3), 3, "two_head", True)
    B, h, w, H, W = hd.shape
    m, _ = _blocky_map(B, H, W)
    r = hd.run(m, mode=1, expect_refusal=True)
    assert (r["hout"].view(F32) == 7.0).all() and (r["dp2"].view(F32) == 7.0).all() and (r["dp1"].view(F32) == 7.0).all()
    assert (r["dt2"].view(BF) == SENTINEL).all() and (r["conf"] == 77).all() and (r["lws"] == 77).all()
    ok = hd.run(None, mode=1)                                              # mode 1 through the _views symbols without a map: the warm-up launch
    _same(ok, hd.run("plain", mode=1), "mode 1, NULL map")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("K", [3, 15])
@pytest.mark.parametrize("geom", list(VIEW_GEOMS))
def test_head_views_against_float64(dev, geom, K, form):
    """Scalars and gradients under a blocky map against view_losses in float64, by the bars of tests/_head_bar.py (the fp32 oracle is the
    yardstick they measure from).  The frozen logits of item i are N(0, 1) plus 8 on class i, so every posterior maximum is ~0.99 > th_high
    (bilinear interpolation of probabilities, or of logits that all peak on one class, keeps it there): a pixel whose map byte names the
    partner must carry the PARTNER's class in conf_out -- all of them, or the map was ignored."""
    inp = _head_inputs(geom, K, peaked=True)
    p1, p2, f2, lab, ntm = inp
    hd = _Head(dev, inp, K, form, True)
    single, fix_logits, half = FORMS[form]
    B, h, w, H, W = hd.shape
    m, sel = _blocky_map(B, H, W)
    assert all(set(np.unique(m[i])) == {i, (i + 1) % B} for i in range(B))
    up = (lambda x: torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear")) if half else (lambda x: so.upsample(x, (H, W)))
    post = torch.softmax(up(f2.double()), 1) if fix_logits else up(torch.softmax(f2.double(), 1))
    pmax, parg = post.max(1)
    assert pmax.min().item() > float(D["th"][0]) + 0.02 and bool((parg == torch.arange(B)[:, None, None]).all()), "the inputs miss the condition"
    r = hd.run(m)
    conf = r["conf"].long()
    partner_class = torch.from_numpy((np.arange(B)[:, None, None] + 1) % B * np.ones((B, H, W), np.int64))
    share = (conf == partner_class)[torch.from_numpy(sel)].double().mean().item()
    print(f"[weak-teacher] {geom} K={K} {form}: share of partner-mapped pixels that carry the partner's class {share:.6f}")
    assert share == 1.0
    own = torch.from_numpy(np.arange(B)[:, None, None] * np.ones((B, H, W), np.int64))
    assert bool((conf == own)[torch.from_numpy(~sel)].all())
    tag = f"views {geom} K={K} {form}"
    if single:
        r64, r32 = hb.ref_pair(("views1", geom, K, form), lambda dt: wt.single_view_ref(p2, f2, lab, ntm[1], K, CD, dt, m, half=bool(half), fix_logits=bool(fix_logits)))
        names = [(0, "total"), (2, "loss_p"), (4, "loss_y"), (5, "place"), (6, "convex"), (7, "volume"), (8, "anchor")]
        grads = [("dpred2", hd.back(r["dp2"]), hd.back(r["dt2"], BF)), ("ntm_grad2", r["ntm_grad2"].view(F32), None)]
    else:
        r64, r32 = hb.ref_pair(("views2", geom, K, form), lambda dt: wt.two_head_view_ref(p1, p2, f2, lab, ntm, dict(D, K=K), CD, dt, m, half=bool(half),
                                                                                         fix_logits=bool(fix_logits)))
        names = [(0, "total"), (1, "loss_p1"), (2, "loss_p2"), (3, "loss_y1"), (4, "loss_y2"), (5, "place"), (6, "convex"), (7, "volume"), (8, "anchor")]
        grads = [("dpred1", hd.back(r["dp1"]), hd.back(r["dt1"], BF)), ("dpred2", hd.back(r["dp2"]), hd.back(r["dt2"], BF)),
                 ("ntm_grad1", r["ntm_grad1"].view(F32), None), ("ntm_grad2", r["ntm_grad2"].view(F32), None)]
    assert torch.equal(conf, r32["out"]["conf"].long().view_as(conf)), "conf_out differs from the fp32 restatement's"
    lo = r["lout"].view(F32)
    for idx, key in names:
        print(f"[weak-teacher] {tag} {key}: gpu {float(lo[idx]):.7g} f64 {float(r64['out'][key]):.7g} f32 {float(r32['out'][key]):.7g}")
    # The anchor pixel of a channel is the FIRST arg-max over all pixels.  Where the upsample clamps (the half-pixel form repeats the last
    # low-res row over three image rows) the maximum is a plateau of values that differ by rounding only, and the float64 restatement, the fp32
    # one and the kernel may each name another pixel of it -- harmless with one view (the frozen posterior has the same plateau), but under a
    # map whose block edge crosses the plateau the pixels read different items.  So the kernel's anchor pixels are first held to be
    # arg-maxes of the float64 upsampled logits up to fp32 rounding (1e-5 (1 + |max|): four fp32 operations on |v| < 20) and its anchor rows
    # to be the float64 posterior, gathered by the map, at THOSE pixels; where they are not the restatements' own pixels, both restatements
    # are evaluated again with the anchor term AT the kernel's pixels (anchor_at), so that every scalar and every gradient is held in every case.
    idx_keys = ["anchor_idx"] if single else ["anchor_idx1", "anchor_idx2"]
    QM, Q, QC = 40, hd.Q, hd.Q * 19
    base = 16 + 2 * QC + 2 * QM
    gathered = wt.gather_views(torch.zeros(B, H, W, dtype=torch.long), post.permute(0, 2, 3, 1).reshape(-1, 19), m)[1]
    kernel_idx = []
    for hdx, k, pred in zip(((1,) if single else (0, 1)), idx_keys, ((p2,) if single else (p1, p2))):
        ai = r["hout"][base + hdx * QM: base + hdx * QM + Q].long()
        flat = up(pred.double()).permute(0, 2, 3, 1).reshape(-1, Q)
        mx, at = flat.max(0).values, flat[ai, torch.arange(Q)]
        assert bool((mx - at <= 1e-5 * (1 + mx.abs())).all()), f"{tag}: an anchor pixel of head {hdx + 1} is no arg-max of its channel"
        rows = r["hout"].view(F32)[16 + hdx * QC: 16 + (hdx + 1) * QC].view(Q, 19)
        close(rows, gathered[ai], 1e-5, f"{tag}: anchor rows of head {hdx + 1} against the gathered posterior at the kernel's anchor pixels")
        kernel_idx.append(ai)
    same_anchors = all(torch.equal(ai, r64["out"][k]) and torch.equal(ai, r32["out"][k]) for ai, k in zip(kernel_idx, idx_keys))
    print(f"[weak-teacher] {tag}: kernel, fp32 and float64 restatement name {'the same' if same_anchors else 'DIFFERENT'} anchor pixels")
    assert same_anchors or half, f"{tag}: the align-corners upsample has no plateau, yet the anchor pixels differ"
    if not same_anchors:
        if single:
            r64, r32 = hb.ref_pair(("views1@kernel", geom, K, form), lambda dt: wt.single_view_ref(p2, f2, lab, ntm[1], K, CD, dt, m, half=bool(half),
                                                                                                  fix_logits=bool(fix_logits), anchor_idx=kernel_idx[0]))
        else:
            r64, r32 = hb.ref_pair(("views2@kernel", geom, K, form), lambda dt: wt.two_head_view_ref(p1, p2, f2, lab, ntm, dict(D, K=K), CD, dt, m,
                                                                                                    half=bool(half), fix_logits=bool(fix_logits),
                                                                                                    anchor_idx=tuple(kernel_idx)))
        for idx, key in names:
            print(f"[weak-teacher] {tag} at the kernel's anchors {key}: gpu {float(lo[idx]):.7g} f64 {float(r64['out'][key]):.7g} f32 {float(r32['out'][key]):.7g}")
    for idx, key in names:
        close(lo[idx], r64["out"][key], 1e-4, f"{tag} {key}")
    for k, g32, g16 in grads:
        hb.report(tag, k, hb.grad_bar(g32, r64[k], r32[k], f"{tag} {k}"))
        if g16 is not None:
            hb.report(tag, k + " bf16", hb.bf16_bar(g16, r64[k], r32[k], f"{tag} {k} bf16", got_f32=g32))


# ---- 3. the trainers ----------------------------------------------------------------------------------------------------------------------------
RK = 3


def _simt(dev, tv, dtype=BF, iter_size=1):
    st = so.recipe_state(so.state_shapes(19, RK, True, layers=SMALL), seed=31, head_scale=8.0)
    fst = so.recipe_state(so.state_shapes(19, 0, False, layers=SMALL), seed=32, head_scale=8.0)
    kw = {"teacher_view": True} if tv else {}
    return SimTTrainer(st, fst, so.ntm_init(19, RK, 911), so.ntm_init(19, RK, 912), Hyper(open_classes=RK, **dict(HP, iter_size=iter_size)), CD.numpy(),
                       2, 97, 97, dtype=dtype, device=dev, layers=SMALL, **kw)


def _single(dev, model, tv, dtype=BF):
    kw = {"teacher_view": True} if tv else {}
    if model == "v3":
        Kx, layers, width, ac = 6, (1, 2, 2), 64, 64
        st = _v3_state(v3_state_shapes(19, Kx, True, layers, width, ac), 3)
        fst = _v3_state(v3_state_shapes(19, 0, False, layers, width, ac), 4)
        arch, hkw = {"layers": layers, "width": width, "assp_ch": ac}, dict(HP)
    else:
        Kx = 3
        lay = [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in VGG_SMALL]
        st, fst = _vgg_state(19 + Kx, lay, 5), _vgg_state(19, lay, 6)
        arch, hkw = {"vgg_layers": lay}, dict(HP, lr=VGG_LR)
    return SimTSingleTrainer(model, st, fst, so.ntm_init(19, Kx, 9), Hyper(open_classes=Kx, **hkw), CD.numpy(), 2, 96, 128, dtype=dtype, device=dev,
                             arch=arch, **kw)


def _batch(dev, B, H, W, seed):
    img, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=seed, block=8)
    return img.to(dev), lab.to(dev)


INERT = {"SimTTrainer": ("simt", {}), "SimTTrainer-late_sgd": ("simt", {"late": True}), "SimTTrainer-iter_size2": ("simt", {"iter_size": 2}),
         "SimTSingleTrainer-v3": ("v3", {}), "SimTSingleTrainer-vgg": ("vgg", {})}


@pytest.mark.parametrize("case", list(INERT))
def test_teacher_view_fed_the_same_image_is_the_trainer_without_it(dev, monkeypatch, case):
    """teacher_view=True, teacher_image = image, no map: three steps equal the keyword-less trainer bit for bit -- the scalars of every step and
    everything a resume must reproduce.  (The frozen plan's own one-set stem launch is the second set of the shared launch, bit for bit: per
    set the same patch, the same MFMA sequence into accumulators of its own -- csrc/stem7.hip.)"""
    kind, kw = INERT[case]
    monkeypatch.setenv("SIMT_EARLY_SGD", "0" if kw.get("late") else "1")
    its = kw.get("iter_size", 1)
    size = (2, 97, 97) if kind == "simt" else (2, 96, 128)
    data = [[_batch(dev, *size, 700 + 10 * i + j) for j in range(its)] for i in range(3)]
    runs = []
    for tv in (False, True):
        tr = _simt(dev, tv, iter_size=its) if kind == "simt" else _single(dev, kind, tv)
        assert tr.teacher_view == tv and (tr.fix_item is not None) == tv
        if kind == "simt":
            assert tr._early_sgd == (not kw.get("late") and its == 1)
            assert tr.plan.stem_desc.nsets == (1 if tv else 2) and (tr.fixed.x_in.data_ptr() != tr.plan.x_in.data_ptr()) == tv
            assert (tr.fixed.fwd_list.items[0].tag == "simt_stem7_fwd") == tv
        louts = []
        for mb in data:
            img, lab = ([m[0] for m in mb], [m[1] for m in mb]) if its > 1 else mb[0]
            if tv:
                tr.step(img, lab, teacher_image=[t.clone() for t in img] if its > 1 else img.clone())
            else:
                tr.step(img, lab)
            louts.append(scalars(tr))
        l = tr.losses()
        assert all(v == v for v in l.values()), l
        runs.append((louts, full_state(tr)))
        del tr
        torch.cuda.empty_cache()
    (la, sa), (lb, sb) = runs
    for i in range(3):
        assert torch.equal(la[i], lb[i]), f"{case}: the scalars of step {i + 1} differ: {la[i].view(F32).tolist()} vs {lb[i].view(F32).tolist()}"
    assert sa.keys() == sb.keys()
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{case}: {len(diff)} of {len(sa)} tensors differ after step 3: {diff[:8]}"


@pytest.mark.parametrize("kind", ["simt", "v3"])
def test_the_frozen_model_saw_the_weak_view(dev, kind):
    size = (2, 97, 97) if kind == "simt" else (2, 96, 128)
    (img, lab), (weak, _l) = _batch(dev, *size, 700), _batch(dev, *size, 900)
    tr = _simt(dev, True) if kind == "simt" else _single(dev, kind, True)
    tr.step(img, lab, teacher_image=weak)
    torch.cuda.synchronize()
    if kind == "simt":
        got = tr.fixed.out["x2"].clone()
        alone = TrunkPlan(tr.fixed_params, *size, multi_heads(19, 0, False), dtype=BF, train=False, layers=SMALL)
        run = lambda x: alone.forward(x)["x2"].clone()
    else:
        from simt_amd.engine_v3 import V3Plan
        got = tr.fixed.logits.clone()
        alone = V3Plan(tr.fixed_params, *size, 19, 0, False, dtype=BF, train=False, layers=(1, 2, 2), width=64, assp_ch=64)

        def run(x):
            alone.forward(x)
            return alone.logits.clone()
    on_weak, on_strong = run(weak), run(img)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), on_weak.view(torch.int32)), "the frozen plan's output is not the stand-alone plan's on teacher_image"
    assert not torch.equal(got, on_strong)


def test_trainer_scalars_under_a_map_match_view_losses_fp32(dev):
    """One fp32 step with an unrelated weak view and a blocky map: the scalars against view_losses on the trainer's own low-res outputs, within
    1e-4 (1 + |ref|) (tests/test_gpu_iteration.py's bar for iteration 0) -- and not within it of the losses without the map."""
    B, H, W = 2, 97, 97
    (img, lab), (weak, _l) = _batch(dev, B, H, W, 700), _batch(dev, B, H, W, 900)
    m, _sel = _blocky_map(B, H, W)
    tr = _simt(dev, True, dtype=F32)
    tr.step(img, lab, teacher_image=weak, fix_item=torch.from_numpy(m).to(dev))
    got = tr.lout.cpu().double().numpy()[:9]
    Q = 19 + RK
    nchw = lambda t, n: t.detach().float().cpu()[..., :n].permute(0, 3, 1, 2).contiguous()
    p1, p2, f2 = nchw(tr.plan.out["x1"], Q), nchw(tr.plan.out["x2"], Q), nchw(tr.fixed.out["x2"], 19)
    T = [t.cpu() for t in tr.T]
    Wm = [so.sig_w_forward(x.cpu()) for x in tr.wraw]
    ohp = so.Hyper(open_classes=RK, **HP)
    keys = ["total", "loss_p1", "loss_p2", "loss_y1", "loss_y2", "place", "convex", "volume", "anchor"]
    refs = {}
    for name, item in (("map", m), ("no map", None)):
        out = wt.view_losses(p1, p2, f2, lab.cpu(), T[0], T[1], Wm[0], Wm[1], ohp, (H, W), item=item)
        refs[name] = np.array([float(out[k]) for k in keys])
    print("[weak-teacher] trainer scalars", got, "view_losses", refs["map"], "without the map", refs["no map"])
    assert np.all(np.abs(got - refs["map"]) <= 1e-4 * (1 + np.abs(refs["map"]))), (got, refs["map"])
    assert np.any(np.abs(got - refs["no map"]) > 1e-4 * (1 + np.abs(refs["no map"]))), "the map changes no scalar: the case shows nothing"


def test_step_refuses_views_that_do_not_fit_the_trainer(dev):
    B, H, W = 2, 97, 97
    img, lab = _batch(dev, B, H, W, 700)
    off, on = _simt(dev, False), _simt(dev, True)
    with pytest.raises(ValueError, match="teacher_view=True"):
        off.step(img, lab, teacher_image=img)
    with pytest.raises(ValueError, match="teacher_view=True"):
        off.step(img, lab, fix_item=torch.zeros(B, H, W, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="needs teacher_image"):
        on.step(img, lab)
    for bad in (torch.zeros(B, H, W + 1, dtype=torch.uint8, device=dev), torch.zeros(B, 1, H, W, dtype=torch.uint8, device=dev),
                torch.zeros(B, H, W, dtype=torch.int64, device=dev)):
        with pytest.raises(ValueError, match="fix_item"):
            on.step(img, lab, teacher_image=img, fix_item=bad)
    with pytest.raises(ValueError, match="teacher_image of shape"):
        on.step(img, lab, teacher_image=img[:, :, :-1])
    assert off.it_done == 0 and on.it_done == 0
    one = _single(dev, "vgg", True)
    with pytest.raises(ValueError, match="needs teacher_image"):
        one.step(*_batch(dev, 2, 96, 128, 700))
    assert one.it_done == 0


# ---- 4. the loader ------------------------------------------------------------------------------------------------------------------------------
def _ds(root, lst, mix, photo, tv, choices=None):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    return cityscapesPseudo(root, lst, crop_size=CROP, mean=IMG_MEAN, mirror=True, scale_crop=choices, class_mix=mix, photometric=photo, teacher_view=tv)


def _collect(loader):
    out = []
    for batch in loader:
        out.append(tuple(t.clone() if torch.is_tensor(t) else t for t in batch))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("choices", [None, CHOICES], ids=["plain", "scale-crop"])
def test_loader_hands_out_both_views_and_the_item_map(dev, tmp_path, choices):
    """8 items, B = 2, shuffle + mirror, 2 epochs, class-mix and photometric on: the weak image is the flag-off loader's batch, the strong image
    and the labels are the 3-tuple loader's, the item map is item_map of the same draws -- bit for bit, cached and uncached."""
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2)
    mix, photo = (N_CLASSES, 0.7), (0.2, 0.5)
    off = _collect(GpuLoader(_ds(root, lst, None, None, False, choices), 2, **kw))
    strong = _collect(GpuLoader(_ds(root, lst, mix, photo, False, choices), 2, **kw))
    assert len(off) == len(strong) == 8 and all(len(b) == 4 for b in off + strong)
    rng = cmref.generator(3, 0)
    maps = []
    for x, lab, _s, names in off:
        apply, rank = cmref.draws(rng, len(names), N_CLASSES, mix[1])
        maps.append(wt.item_map(lab.cpu().numpy(), [1, 0], apply, rank, N_CLASSES))
    assert any(len(np.unique(m[i])) == 2 for m in maps for i in range(2))
    cache = DatasetCache((WS, HS) if choices is not None else CROP, slab_slots=3, device=dev)
    for what, cch in (("uncached", None), ("cached", cache)):
        got = _collect(GpuLoader(_ds(root, lst, mix, photo, True, choices), 2, cache=cch, **kw))
        assert len(got) == 8 and all(len(b) == 6 for b in got)
        _assert_same_batches(strong, [b[:4] for b in got])
        _assert_same_batches(off, [(b[4], o[1], b[2], b[3]) for b, o in zip(got, off)])
        for k, (b, m) in enumerate(zip(got, maps)):
            assert b[5].dtype == torch.uint8 and np.array_equal(b[5].cpu().numpy(), m), f"{what} batch {k}: the item map differs"
            assert not torch.equal(b[0], b[4])
    # photometric alone: two views, no map; class-mix alone: a map
    got = _collect(GpuLoader(_ds(root, lst, None, photo, True, choices), 2, **kw))
    _assert_same_batches(off, [(b[4], b[1], b[2], b[3]) for b in got])
    assert all(b[5] is None for b in got) and any(not torch.equal(b[0], b[4]) for b in got)
    got = _collect(GpuLoader(_ds(root, lst, mix, None, True, choices), 2, **kw))
    assert all(np.array_equal(b[5].cpu().numpy(), m) for b, m in zip(got, maps))
    with pytest.raises(ValueError, match="--class-mix"):
        GpuLoader(_ds(root, lst, None, None, True, choices), 2, **kw)


# ---- 5. the tool --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["DeepLab", "DeepLabv3", "DeepLabVGG"])
def test_tool_weak_teacher_runs_differs_and_resumes(dev, tmp_path, capsys, model):
    """trainV2_simt --class-mix --colour-jitter --weak-teacher on 4 PNG pairs, B = 2, at 129 x 65: 4 steps whose loss lines differ from the run
    without the flag; 2 steps + resume + 2 steps equal them (loss lines, every tensor of the final snapshot); a resume with the flag dropped is
    refused."""
    pytest.importorskip("PIL.Image")
    from simt_amd.tools import trainV2_simt as tool
    _tool_files(tmp_path / "data")
    # A frozen model with an opinion: at the constructor init the posterior is flat in either view (DeepLab, DeepLabv3: every pixel below
    # th_low; the full VGG16's activations shrink layer by layer until its classifier sees nothing and both networks print ln 22 on every
    # line), and a flat teacher labels both views alike.  So both models restore a checkpoint: trained-like weights for DeepLab, a scaled-up
    # classifier for DeepLabv3, and for VGG16 the variance-preserving draw tests/test_gpu_single.py uses for its reduced VGG, with a
    # classifier scaled so that its logits have a standard deviation near 10 (four of five pixels above th_high, on ten classes).
    ckpt = str(tmp_path / "frozen.pth")
    if model == "DeepLab":
        from simt_amd import model_spec as ms
        torch.save(ms.trained_like_init(ms.state_shapes(19, 0, False), seed=7), ckpt)
    elif model == "DeepLabVGG":
        g = torch.Generator().manual_seed(6)
        sd = {}
        for k, v in tool.single_model_state(model, 19).items():
            if k.endswith("bias"):
                sd[k] = torch.randn(v.shape, generator=g) * 0.05
            else:
                sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * 9)) ** 0.5 * (0.2 if k.startswith("classifier") else 1.0)
        torch.save(sd, ckpt)
    else:
        sd = tool.single_model_state(model, 19)
        for k, v in sd.items():
            if k.startswith(tool.RESTORE_LAST[model]) and v.is_floating_point():
                v.mul_(20.0)
        torch.save(sd, ckpt)
    common = ["--model", model, "--open-classes", "3", "--learning-rate", "6e-4" if model != "DeepLabVGG" else "2.5e-5", "--learning-rate-T", "6e-3",
              "--class-mix", "--colour-jitter"] + [ckpt if a == "" else a for a in _common(tmp_path)]
    assert ckpt in common

    def run(tag, stop, *flags):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(flags))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_4.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 4, "--weak-teacher")
    assert len(_loss_lines(out_a)) == 4 and "weak-view teacher: the frozen model sees the batch before --class-mix, --colour-jitter" in out_a
    out_o, _ = run("o", 4)
    assert len(_loss_lines(out_o)) == 4 and "weak-view teacher" not in out_o
    assert _loss_lines(out_a) != _loss_lines(out_o), (out_a, out_o)
    out_b1, _ = run("b", 2, "--weak-teacher", "--train-state", state)
    assert _loss_lines(out_b1) == _loss_lines(out_a)[:2]
    out_b2, snap_b = run("b", 4, "--weak-teacher", "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_b2), out_b2
    assert _loss_lines(out_b2) == _loss_lines(out_a)[2:], (out_a, out_b2)
    _same_snapshot(snap_a, snap_b)
    with pytest.raises(SystemExit, match="weak_teacher"):          # the flag dropped
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
