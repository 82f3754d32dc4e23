"""Evaluation and checkpoints of the one-output models (DeepLabv3, DeepLab-VGG16):

  * simt_upsample2_sum_argmax -- DeepLabv3's in-model upsample (align_corners=False, model/deeplabv3.py:137) followed by the
    evaluation's align_corners=True resample to the label size (evaluate_cityscapes.py:108-133), summed over two scales, arg-maxed --
    against float64 CPU torch, and against the composition of the existing launches (simt_upsample_nchw + simt_upsample_sum_argmax);
  * Evaluator(model="v3" | "vgg") against the oracle forwards + the CPU resample composition (small depth; DeepLabv3 R-50 at the
    reference geometry);
  * SimTSingleTrainer.state_dict(): loads strict into the nn.Modules, num_batches_tracked, and Evaluator.load of it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import model_spec as ms
from simt_amd import ops
from simt_amd.tools.evaluate_cityscapes import Evaluator, fast_hist, per_class_iu

pytestmark = pytest.mark.gpu


def _logits(B, h, w, ld, C, seed):
    """NHWC logits [B*h*w, ld]: smooth-ish random fields in the first C channels, large values planted in channels >= C."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, h, w, ld), 1e3)
    x[..., :C] = torch.randn(B, h, w, C, generator=g) * 2.0
    return x.reshape(B * h * w, ld)


def _ref64(maps, C, HW):
    """maps: [(logits [B*h*w, ld], h, w, (hi, wi))].  float64: align_corners=False to (hi, wi), align_corners=True to HW, summed.
    -> (arg-max [B,H,W], top-2 gap [B,H,W]), one image at a time."""
    B = maps[0][0].shape[0] // (maps[0][1] * maps[0][2])
    preds, gaps = [], []
    for b in range(B):
        tot = None
        for (lg, h, w, hiwi) in maps:
            x = lg.reshape(B, h, w, -1)[b:b + 1, :, :, :C].permute(0, 3, 1, 2).double()
            v = F.interpolate(F.interpolate(x, size=hiwi, mode="bilinear", align_corners=False), size=HW, mode="bilinear", align_corners=True)
            tot = v if tot is None else tot + v
        t2 = tot.topk(2, dim=1)
        preds.append(t2.indices[:, 0])
        gaps.append(t2.values[:, 0] - t2.values[:, 1])
        del tot
    return torch.cat(preds).numpy(), torch.cat(gaps).numpy()


def _run_up2(dev, maps, C, B, HW):
    pred = torch.full((B, *HW), -1, device=dev, dtype=torch.int32)
    d = [(lg.to(dev), h, w, hiwi) for (lg, h, w, hiwi) in maps]
    (la, ha, wa, (hia, wia)) = d[0]
    if len(d) > 1:
        (lb, hb, wb, (hib, wib)) = d[1]
    else:
        lb, hb, wb, hib, wib = None, 0, 0, 0, 0
    L.call("simt_upsample2_sum_argmax", ops._p(la), ha, wa, la.shape[1], hia, wia, ops._p(lb), hb, wb, lb.shape[1] if lb is not None else 0,
           hib, wib, B, HW[0], HW[1], C, ops._p(pred), ops.stream_ptr())
    torch.cuda.synchronize()
    return pred.cpu().numpy()


CASES = {
    # name: (B, C, [(h, w, ld, (hi, wi))], (H, W))
    "small": (2, 19, [(5, 7, 24, (17, 23)), (6, 9, 32, (21, 29))], (33, 45)),
    "small_ld_odd": (2, 19, [(5, 7, 21, (17, 23)), (6, 9, 19, (21, 29))], (33, 45)),     # ld % 4 != 0: the scalar-gather instantiation
    "single_scale": (2, 19, [(6, 9, 32, (21, 29))], (40, 51)),
    "hi_eq_H": (2, 19, [(8, 12, 32, (40, 56)), (10, 14, 32, (40, 56))], (40, 56)),
    "production": (2, 19, [(32, 64, 32, (512, 1024)), (40, 80, 32, (640, 1280))], (1024, 2048)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_upsample2_sum_argmax_vs_float64(dev, case):
    B, C, geo, HW = CASES[case]
    maps = [(_logits(B, h, w, ld, C, 100 + i), h, w, hiwi) for i, (h, w, ld, hiwi) in enumerate(geo)]
    got = _run_up2(dev, maps, C, B, HW)
    if case == "production":
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    ref, gap = _ref64(maps, C, HW)
    diff = got != ref
    P = diff.size
    print(f"{case}: {int(diff.sum())} of {P} labels differ, {int((gap < 1e-4).sum())} pixels with a top-2 gap < 1e-4")
    assert got.min() >= 0 and got.max() < C                       # planted channels >= C never win
    assert not np.any(diff & (gap >= 1e-4)), f"{int((diff & (gap >= 1e-4)).sum())} labels differ outside the 1e-4 margin"
    assert diff.sum() <= max(1, int(1e-5 * P))
    assert len(np.unique(ref)) >= 10                                # a non-degenerate label map


@pytest.mark.parametrize("case", ["small", "production"])
def test_upsample2_sum_argmax_vs_existing_launches(dev, case):
    """The same labels as writing the in-model upsample out (simt_upsample_nchw, align_corners=False), repacking it NHWC and running
    simt_upsample_sum_argmax on it -- except where the top-2 gap is below 1e-5 (FMA contraction differs between the two)."""
    B, C, geo, HW = CASES[case]
    maps = [(_logits(B, h, w, ld, C, 200 + i), h, w, hiwi) for i, (h, w, ld, hiwi) in enumerate(geo)]
    got = _run_up2(dev, maps, C, B, HW)
    nhwc = []
    for (lg, h, w, (hi, wi)) in maps:
        src = lg.to(dev)
        full = torch.empty(B, C, hi, wi, device=dev)
        L.call("simt_upsample_nchw", ops._p(src), B, h, w, src.shape[1], C, hi, wi, 0, ops._p(full), ops.stream_ptr())
        nhwc.append((full.permute(0, 2, 3, 1).contiguous(), hi, wi))
    pred = torch.full((B, *HW), -1, device=dev, dtype=torch.int32)
    (a, ha, wa), (b, hb, wb) = nhwc
    L.call("simt_upsample_sum_argmax", ops._p(a), ha, wa, C, ops._p(b), hb, wb, C, B, HW[0], HW[1], C, ops._p(pred), ops.stream_ptr())
    with torch.no_grad():
        tot = sum(F.interpolate(t.permute(0, 3, 1, 2), size=HW, mode="bilinear", align_corners=True) for (t, _h, _w) in nhwc)
        t2 = tot.topk(2, dim=1)
        gap = (t2.values[:, 0] - t2.values[:, 1]).cpu().numpy()
    old = pred.cpu().numpy()
    diff = got != old
    print(f"{case}: {int(diff.sum())} of {diff.size} labels differ from the two-launch composition")
    assert not np.any(diff & (gap >= 1e-5))


# ---------------------------------------------------------------------------------------------------------------- Evaluator
def _score(out, got, margin_rel=1e-4):
    """out: the oracle's summed logits [B,C,H,W]; got: device labels.  Labels equal wherever the oracle's top-2 gap >= margin_rel *
    max|out| (the fp32 conv parity error, tests/test_gpu_eval.py); fewer than 0.5 % of the pixels exempt."""
    t2 = out.topk(2, dim=1)
    pred = t2.indices[:, 0].numpy()
    gap = (t2.values[:, 0] - t2.values[:, 1]).numpy()
    margin = margin_rel * float(out.abs().max())
    diff = got != pred
    print(f"{int(diff.sum())} of {diff.size} labels differ; {int((gap < margin).sum())} pixels with a top-2 gap below {margin:.2e}; "
          f"{len(np.unique(pred))} distinct labels")
    assert len(np.unique(pred)) >= 3, "degenerate label map"
    assert not np.any(diff & (gap >= margin)), f"{int((diff & (gap >= margin)).sum())} labels differ outside the rounding margin"
    assert (gap < margin).mean() < 5e-3
    return pred


def _check_hist(ev, gt, got):
    h = fast_hist(gt.numpy().flatten(), got.flatten().astype(np.int64), 19)
    assert np.array_equal(ev.hist.cpu().numpy().reshape(19, 19), h)
    miou, _ = ev.result()
    assert miou == round(float(np.nanmean(per_class_iu(h))) * 100, 2)


def _v3_small_state(K, layers, seed):
    from test_gpu_v3 import make_state
    from simt_amd.engine_v3 import v3_state_shapes
    st = make_state(v3_state_shapes(19, K, True, layers), seed)
    st["conv.weight"] = st["conv.weight"] * 4.0
    return st


def test_evaluator_v3_small_depth_vs_oracle(dev):
    K, layers = 3, (1, 1, 1)
    st = _v3_small_state(K, layers, 41)
    g = torch.Generator().manual_seed(5)
    B, (H, W) = 1, (64, 96)
    s1, s2 = (48, 64), (56, 80)
    img1 = torch.randn(B, 3, *s1, generator=g) * 50
    img2 = F.interpolate(img1, size=s2, mode="bilinear", align_corners=True)
    gt = torch.randint(0, 19, (B, H, W), generator=g)
    ev = Evaluator(st, num_classes=19, open_classes=K, batch=B, label_hw=(H, W), scales=(s1, s2), dtype=torch.float32, device=dev,
                   layers=layers, model="v3")
    ev.add(img1, img2, gt)
    got = ev.pred.cpu().numpy()
    with torch.no_grad():
        o1 = so.v3_forward(st, img1, layers, openset=True, train=False)
        o2 = so.v3_forward(st, img2, layers, openset=True, train=False)
        out = (F.interpolate(o1[:, :19], size=(H, W), mode="bilinear", align_corners=True) +
               F.interpolate(o2[:, :19], size=(H, W), mode="bilinear", align_corners=True))
    _score(out, got)
    _check_hist(ev, gt, got)


def test_evaluator_vgg_small_depth_vs_oracle(dev):
    from test_gpu_single import VGG_SMALL, _vgg_state
    K = 3
    st = _vgg_state(19 + K, VGG_SMALL, 8)
    g = torch.Generator().manual_seed(6)
    B, (H, W) = 1, (64, 96)
    s1, s2 = (48, 64), (64, 96)
    img1 = torch.randn(B, 3, *s1, generator=g) * 50
    img2 = F.interpolate(img1, size=s2, mode="bilinear", align_corners=True)
    gt = torch.randint(0, 19, (B, H, W), generator=g)
    ev = Evaluator(st, num_classes=19, open_classes=K, batch=B, label_hw=(H, W), scales=(s1, s2), dtype=torch.float32, device=dev,
                   layers=VGG_SMALL, model="vgg")
    ev.add(img1, img2, gt)
    got = ev.pred.cpu().numpy()
    with torch.no_grad():
        o1, o2 = so.vgg_forward(st, img1, VGG_SMALL), so.vgg_forward(st, img2, VGG_SMALL)
        out = (F.interpolate(o1[:, :19], size=(H, W), mode="bilinear", align_corners=True) +
               F.interpolate(o2[:, :19], size=(H, W), mode="bilinear", align_corners=True))
    _score(out, got)
    _check_hist(ev, gt, got)


def test_evaluator_v3_r50_fp32_at_reference_geometry(dev):
    """One DeepLabv3 (R-50, model/deeplabv3.py as written) frame at 1024 x 512 and 1280 x 640 -> in-model upsample to the input size ->
    align_corners=True to 1024 x 2048, summed, arg-maxed; the default Evaluator (fp32) against the oracle forward x 2 + the CPU resamples.
    BatchNorm running statistics calibrated by train-mode forwards of the HIP trunk (uncalibrated eval-mode statistics collapse the features)."""
    from simt_amd.engine_v3 import V3Plan, v3_state_shapes
    K = 6
    cd = ms.load_class_dist("bapa")
    st = ms.kaiming_init(v3_state_shapes(19, K, True), seed=1234)
    st["conv.weight"] = st["conv.weight"] * 4.0
    p = {k: v.clone().to(dev) for k, v in st.items()}
    cal = V3Plan(p, 1, 384, 768, 19, K, True, dtype=torch.float32, train=True)
    img_c, _ = ms.synthetic_batch(1, 384, 768, cd, seed=99, device=dev)
    cal.x_in.copy_(img_c)
    for _ in range(40):
        cal.fwd_list.run()
    torch.cuda.synchronize()
    for k in st:
        if k.endswith("running_mean") or k.endswith("running_var"):
            st[k] = p[k].detach().cpu().clone()
    del cal, p
    torch.cuda.empty_cache()
    H, W = 1024, 2048
    s1, s2 = (512, 1024), (640, 1280)
    g = torch.Generator().manual_seed(77)
    base = torch.randn(1, 3, 32, 64, generator=g) * 60
    full = F.interpolate(base, size=(H, W), mode="nearest") + torch.randn(1, 3, H, W, generator=g) * 12
    img1 = F.interpolate(full, size=s1, mode="bilinear", align_corners=False).contiguous()
    img2 = F.interpolate(full, size=s2, mode="bilinear", align_corners=False).contiguous()
    gt = torch.randint(0, 19, (1, H, W), generator=g)
    gt[torch.rand(1, H, W, generator=g) < 0.1] = 255
    ev = Evaluator(st, num_classes=19, open_classes=K, device=dev, model="v3")
    assert ev.dtype == torch.float32 and (ev.H, ev.W) == (H, W)
    ev.add(img1, img2, gt)
    got = ev.pred.cpu().numpy()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    with torch.no_grad():
        o1 = so.v3_forward(st, img1, openset=True, train=False)
        o2 = so.v3_forward(st, img2, openset=True, train=False)
        out = (F.interpolate(o1[:, :19], size=(H, W), mode="bilinear", align_corners=True) +
               F.interpolate(o2[:, :19], size=(H, W), mode="bilinear", align_corners=True))
    del o1, o2
    _score(out, got)
    _check_hist(ev, gt, got)


# ---------------------------------------------------------------------------------------------------------------- state_dict
@pytest.mark.parametrize("model", ["v3", "vgg"])
def test_single_trainer_state_dict_round_trip(dev, model):
    from simt_amd.step import Hyper
    from simt_amd.step_single import SimTSingleTrainer
    from simt_amd.tools.trainV2_simt import single_model_states
    C, K, B, H, W = 19, 3, 1, 96, 128
    name = {"v3": "DeepLabv3", "vgg": "DeepLabVGG"}[model]
    st, fst = single_model_states(name, C, K, seed=11)
    st0 = {k: v.clone() for k, v in st.items()}
    cd = ms.load_class_dist("bapa")
    tr = SimTSingleTrainer(model, st, fst, ms.ntm_init(C, K, 2), Hyper(open_classes=K, lr=2.5e-3, lr_T=6e-3), cd, B, H, W,
                           dtype=torch.float32, device=dev)
    for it in range(2):
        img, lab = ms.synthetic_batch(B, H, W, cd, seed=30 + it, device=dev)
        tr.step(img, lab, it)
    tr.losses()
    sd = tr.state_dict()
    assert set(sd) == set(st0)
    assert all(v.device.type == "cpu" for v in sd.values())
    assert all(v.dtype == (torch.long if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    if model == "v3":
        from simt_amd.model.deeplabv3 import DeepLabv3
        m = DeepLabv3(C, K, openset=True)
        dead = {n for n, mod in m.named_modules() if mod in m._dead_bns()}
        nbt = {k[:-len(".num_batches_tracked")]: int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")}
        assert nbt and all(v == (0 if n in dead else 2) for n, v in nbt.items()), nbt
        assert nbt["resnet.resnet_50.bn1"] == 2 and nbt["assp.bnf"] == 2 and nbt["resnet.resnet_50.layer4.0.bn1"] == 0
        untouched = [k for k in sd if ".layer4." in k or ".fc." in k]
        trained = ["conv.weight", "conv_1.bias", "assp.convf.weight", "resnet.resnet_50.layer3.0.conv1.weight"]
        assert not torch.equal(sd["resnet.resnet_50.layer3.0.bn1.running_mean"], st0["resnet.resnet_50.layer3.0.bn1.running_mean"])
    else:
        from simt_amd.model.deeplab_vgg import DeeplabVGG
        m = DeeplabVGG(C + K)
        untouched = [k for k in sd if k.startswith(("classifier.conv2d_list.2.", "classifier.conv2d_list.3."))]
        trained = ["features.0.weight", "features.31.bias", "classifier.conv2d_list.0.weight", "classifier.conv2d_list.1.bias"]
    assert untouched and all(torch.equal(sd[k], st0[k]) for k in untouched)
    assert all(not torch.equal(sd[k], st0[k]) for k in trained)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
    print(m.load_state_dict(sd, strict=True))
    # the checkpoint evaluates like the live weights: Evaluator.load(state_dict) == an Evaluator built from trainer.params
    g = torch.Generator().manual_seed(3)
    s1, s2, HW = (96, 128), (112, 160), (96, 128)
    img1 = torch.randn(1, 3, *s1, generator=g) * 50
    img2 = F.interpolate(img1, size=s2, mode="bilinear", align_corners=True)
    kw = dict(num_classes=C, open_classes=K, batch=1, label_hw=HW, scales=(s1, s2), device=dev, model=model)
    live = Evaluator(tr.params, **kw).predict(img1, img2).cpu().clone()
    ev = Evaluator(st0, **kw)
    ev.predict(img1, img2)
    ev.load(sd)
    after = ev.predict(img1, img2).cpu()
    assert torch.equal(after, live)
