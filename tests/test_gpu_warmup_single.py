"""Warm-up stage over the ONE-OUTPUT models (DeepLabv3, DeepLab-VGG16): the fused head kernel in its one-head warm-up flavour
(simt_head_desc single = 1, mode = 1), `simt_amd.step_single.WarmupSingleTrainer` against the CPU reference of
tests/_warmup_single_oracle.py, data parallelism over a one-rank RCCL group, and `trainV1_warmup --model DeepLabv3 | DeepLabVGG` on real
files up to the SimT stage's restore of its final checkpoint.

Bars: those of the SimT-stage tests of the same models (tests/test_gpu_single.py) and of the DeepLab-v2 warm-up's accumulation test
(tests/test_gpu_iteration.py::test_warmup_gradient_accumulation_iter_size2)."""
import ctypes as C
import glob
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import _head_bar as hb
from _launch_oracle import SENTINEL
from _warmup_single_oracle import OracleWarmupSingleTrainer
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.engine_v3 import v3_geometry, v3_state_shapes
from simt_amd.step import Hyper
from simt_amd.step_single import WarmupSingleTrainer
from test_gpu_single import VGG_SMALL, _v3_state, _vgg_state, close

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
CN = 19


def _v3_feat_hw(H, W):
    """DeepLabv3's low-res map (V3Plan.feat_hw): stem + max-pool, then the stride-2 3x3 convs of layer2 and layer3."""
    (_h0, _w0), (h, w) = v3_geometry(H, W)
    for _ in range(2):
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    return h, w


def _run_head(dev, pred, lab, half, single=True, *, pred1=None, lambda_seg=0.0, f32=True, grad_dtype=None, ld_t=0, gscale=1.0, ldp=None,
              byte_maps=False, full=False):
    """One-head warm-up flavour (single = 1, mode = 1) of simt_head_loss + simt_head_grad on low-res logits pred [B, Q, h, w] (fp32, device)
    and labels lab [B, H, W] (int64, device): -> (hout, d/dpred [B, Q, h, w], g1).  single=False: the DeepLab-v2 warm-up mode with both heads
    fed the same logits, or the auxiliary head fed pred1 (weighted lambda_seg).

    One launch can ask for everything the warm-up trainers ask for (simt_amd/step.py WarmupTrainer, step_single.py WarmupSingleTrainer:
    dpred*_f32 = NULL, dpred*_t in the plan's dtype with the plan's pitch, gscale = 1 / iter_size): f32=False drops the fp32 outputs;
    grad_dtype adds dpred*_t with pitch ld_t, pre-filled with SENTINEL; byte_maps gives conf_out + label_ws (these trainers leave them NULL);
    full=True returns a dict instead (hout, dpred1, dpred2, dt1, dt2 raw, dp1_raw, dp2_raw, conf, g1)."""
    B, Q, h, w = pred.shape
    H, W = lab.shape[1:]
    lib = L.load()
    ldp = ops.round_up(Q, 8) if ldp is None else ldp
    p_d = torch.zeros(B * h * w, ldp, device=dev)
    p_d[:, :Q] = pred.permute(0, 2, 3, 1).reshape(-1, Q)
    p1_d = p_d
    if pred1 is not None:
        assert not single
        p1_d = torch.zeros(B * h * w, ldp, device=dev)
        p1_d[:, :Q] = pred1.permute(0, 2, 3, 1).reshape(-1, Q)
    part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Q), device=dev)
    keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
    hout = torch.zeros(lib.simt_head_hout_floats(Q, Q), device=dev)
    QP = ops.round_up(Q, 8)
    g1 = torch.full((2, B, H, w, QP), 7.0, device=dev)           # sentinel: the one-head flavour never writes the head-1 half
    dp = torch.full((B * h * w, ldp), 5.0, device=dev)
    dp1 = torch.zeros(B * h * w, ldp, device=dev)
    hd = L.HeadDesc()
    hd.pred1 = None if single else p1_d.data_ptr()
    hd.pred2, hd.fixp, hd.label, hd.T1, hd.T2 = p_d.data_ptr(), None, lab.data_ptr(), None, None
    hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
    hd.dpred1_f32, hd.dpred2_f32, hd.dpred1_t, hd.dpred2_t = (None if single else dp1.data_ptr()), dp.data_ptr(), None, None
    if not f32:
        hd.dpred1_f32, hd.dpred2_f32 = None, None
    hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Q, Q
    hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = ldp, ldp, QP, ldp, 0, L.SIMT_F32
    dt = [None, None]
    if grad_dtype is not None:
        assert ld_t >= QP
        dt = [torch.full((B * h * w, ld_t), SENTINEL, dtype=grad_dtype, device=dev) for _ in range(2)]
        hd.dpred1_t, hd.dpred2_t = (None if single else dt[0].data_ptr()), dt[1].data_ptr()
        hd.ld_t, hd.grad_dtype = ld_t, ops.dt_code(grad_dtype)
    hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, lambda_seg, 0.0, gscale
    hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1, int(single), int(half), 0
    conf = lws = None
    if byte_maps:
        conf, lws = (torch.full((B, H, W), 77, dtype=torch.uint8, device=dev) for _ in range(2))
        hd.conf_out, hd.label_ws = conf.data_ptr(), lws.data_ptr()
    st = ops.stream_ptr()
    L.call("simt_head_loss", C.byref(hd), st)
    L.call("simt_head_grad", C.byref(hd), st)
    torch.cuda.synchronize()
    if full:
        back = lambda g: g.cpu()[:, :Q].reshape(B, h, w, Q).permute(0, 3, 1, 2)
        return dict(hout=hout.cpu(), dpred1=back(dp1), dpred2=back(dp), dp1_raw=dp1.cpu(), dp2_raw=dp.cpu(), back=back, g1=g1,
                    dt1=None if (dt[0] is None or single) else dt[0].cpu(), dt2=None if dt[1] is None else dt[1].cpu(),
                    conf=None if conf is None else conf.cpu().long())
    return hout.cpu(), dp[:, :Q].reshape(B, h, w, Q).permute(0, 3, 1, 2).cpu(), dp[:, Q:].cpu(), g1


def _upsample64(x, size, half):
    return F.interpolate(x, size=size, mode="bilinear") if half else so.upsample(x, size)


SHAPES = {"v3": (2, 11, 19, 88, 152), "vgg": (2, 11, 19, 81, 145),
          "v3prod": (4,) + _v3_feat_hw(512, 1024) + (512, 1024), "vggprod": (8, 64, 64, 512, 512)}


@pytest.mark.parametrize("case", ["v3", "vgg", "v3prod", "vggprod"])
def test_one_head_warmup_kernel_vs_float64(dev, case):
    """single = 1, mode = 1: nn.CrossEntropyLoss(ignore_index=255) of the upsampled logits (half-pixel taps for DeepLabv3's in-model
    F.interpolate, align_corners=True for VGG's interp_target) and its gradient w.r.t. the low-res logits, against float64 autograd:
    loss 1e-4 relative, d/dlogits 1e-5.  Two out-of-range labels are skipped and counted (hout[15]); hout[14] is the loss; the pad
    columns of the gradient are zero and the head-1 rows of the workspace are never written."""
    half = case.startswith("v3")
    B, h, w, H, W = SHAPES[case]
    g = torch.Generator().manual_seed(len(case) + H)
    pred = torch.randn(B, CN, h, w, generator=g) * 3
    _, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=13, block=8)
    lab[0, 0, 0], lab[B - 1, H - 1, W - 1] = 19, 300                      # neither a class nor the ignore value
    ref_lab = lab.clone()
    ref_lab[(ref_lab >= CN) & (ref_lab != 255)] = 255
    hout, got, pad, g1 = _run_head(dev, pred.to(dev), lab.to(dev), half)
    q = pred.double().to(dev).requires_grad_(True)
    loss = F.cross_entropy(_upsample64(q, (H, W), half), ref_lab.to(dev), ignore_index=255)
    loss.backward()
    ref = float(loss.detach())
    assert abs(float(hout[1]) - ref) <= 1e-4 * abs(ref), (float(hout[1]), ref)
    assert float(hout[14]) == float(hout[1])
    assert int(hout[6]) == int((ref_lab != 255).sum()) and int(hout[15]) == 2
    close(got, q.grad.cpu(), 1e-5, "d/dlogits")
    assert torch.all(pad == 0)
    assert torch.all(g1[0] == 7.0), "the one-head flavour wrote head-1 gradient rows"
    # ... and every element on its own scale (tests/_head_bar.py): the float64 reference above, the same in fp32 on the CPU for the threshold
    r32 = hb.cached(("warm1", case), lambda: hb.warmup_ref(None, pred, lab, 0.0, half, torch.float32))
    hb.report(case, "d/dlogits", hb.grad_bar(got, q.grad.cpu(), r32["dpred2"], f"{case} d/dlogits"))


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("model", ["v3", "vgg"])
def test_one_head_warmup_production_form(dev, model, gscale):
    """The one-head warm-up launch (single = 1, mode = 1) as WarmupSingleTrainer asks for it at the benchmarked sizes (DeepLabv3: B = 4,
    512 x 1024; DeepLab-VGG16: B = 8, 512 x 512): bf16 dpred2_t with the plan's pitch, the plan's logits pitch, gscale = 1 / iter_size -- and
    dpred2_f32 from the SAME launch, so that the bf16 store is held bit for bit against the fp32 one.  The bars of tests/_head_bar.py
    against float64 autograd of the cross entropy; pad columns; the fp32 output at gscale = 0.5 bit for bit half the one at gscale = 1
    (gscale enters once, in the factor gscale / N_valid of head_pass2: a power of two is exact); hout[14] = the unscaled loss."""
    from test_gpu_single import PROD, single_plan_geometry
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 8)))
    B, H, W, _K = PROD[model]
    h, w, ldp, ld_t = single_plan_geometry(dev, model, warmup=True)
    half = model == "v3"
    assert (B, h, w, H, W) == SHAPES[model + "prod"]
    pred = torch.randn(B, CN, h, w, generator=torch.Generator().manual_seed(31)) * 3
    _, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=13)
    r64, r32 = hb.ref_pair(("warm prod refs", model), lambda dt: hb.warmup_ref(None, pred, lab, 0.0, half, dt))
    run = lambda gs: _run_head(dev, pred.to(dev), lab.to(dev), half, grad_dtype=torch.bfloat16, ld_t=ld_t, gscale=gs, ldp=ldp, full=True)
    base = hb.cached(("gpu warm", model, 1.0), lambda: run(1.0))
    r = base if gscale == 1.0 else run(gscale)
    tag = f"{model} warm-up {B}x{H}x{W}"
    hb.trainer_form(tag, "dpred", r["dp2_raw"], r["dt2"], r["back"], CN, ops.round_up(CN, 8), r64["dpred2"], r32["dpred2"], gscale)
    tot = float(r64["total"])
    assert abs(float(r["hout"][14]) - tot) <= 1e-4 * abs(tot) and float(r["hout"][14]) == float(r["hout"][1])
    assert torch.all(r["g1"][0] == 7.0), "the one-head flavour wrote head-1 gradient rows"
    if gscale == 0.5:
        QP = ops.round_up(CN, 8)                                   # (the columns the kernel writes: the driver pre-fills the fp32 buffer)
        hb.half_is_bitwise(tag, "dpred", r["dp2_raw"][:, :QP], base["dp2_raw"][:, :QP])


@pytest.mark.parametrize("half", [True, False])
def test_one_head_warmup_kernel_all_ignored_like_two_head_mode(dev, half):
    """A batch whose labels are all 255: the loss over zero pixels is NaN and the gradient zero, as in the DeepLab-v2 warm-up mode today."""
    B, h, w, H, W = SHAPES["v3" if half else "vgg"]
    pred = torch.randn(B, CN, h, w, generator=torch.Generator().manual_seed(3)).to(dev)
    lab = torch.full((B, H, W), 255, dtype=torch.int64, device=dev)
    one, two = _run_head(dev, pred, lab, half), _run_head(dev, pred, lab, half, single=False)
    for hout, d, _pad, _g1 in (one, two):
        assert math.isnan(float(hout[1])) and math.isnan(float(hout[14])) and float(hout[6]) == 0 and float(hout[15]) == 0
        assert torch.all(d == 0)


def test_vgg_warmup_three_iterations_fp32(dev):
    B, H, W = 2, 96, 128
    st = _vgg_state(CN, VGG_SMALL, 5)
    kw = dict(open_classes=0, lr=2.5e-4)
    tr = WarmupSingleTrainer("vgg", st, Hyper(**kw), B, H, W, dtype=torch.float32, device=dev, arch={"vgg_layers": VGG_SMALL})
    assert len(tr.sgd_names) == 2 * 15 + 4                             # every conv weight + bias, the two live classifier branches
    orc = OracleWarmupSingleTrainer("vgg", st, so.Hyper(**kw), {"layers": VGG_SMALL})
    names = ["features.0.weight", "features.14.bias", "features.29.weight", "classifier.conv2d_list.0.weight", "classifier.conv2d_list.1.bias"]
    for it in range(3):
        img, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=40 + it, block=8)
        tr.step(img.to(dev), lab.to(dev), it)
        out = orc.step(img, lab, it)
        l = tr.losses()
        assert set(l) == {"total", "loss_seg"}
        for k in ("total", "loss_seg"):
            close(l[k], out[k].detach(), 2e-4, f"it {it} {k}")
        for n in names:
            close(tr.params[n].cpu(), orc.st[n].detach(), 1e-5, f"it {it} {n}")


def test_v3_warmup_iterations_fp32(dev):
    B, H, W = 2, 96, 128
    layers, width, ac = (1, 2, 2), 32, 32
    st = _v3_state(v3_state_shapes(CN, 0, False, layers, width, ac), 3)
    kw = dict(open_classes=0, lr=2.5e-4)
    arch = {"layers": layers, "width": width, "assp_ch": ac}
    tr = WarmupSingleTrainer("v3", st, Hyper(**kw), B, H, W, dtype=torch.float32, device=dev, arch=arch)
    g0, g1 = tr.optim_groups()
    assert g0 and all(n.startswith("resnet.resnet_50.layer3.") for n in g0)
    assert "conv.weight" in g1 and "assp.bnf.bias" in g1 and not any(n.startswith("conv_1.") for n in g1)
    o32 = OracleWarmupSingleTrainer("v3", st, so.Hyper(**kw), {"layers": layers})
    o64 = OracleWarmupSingleTrainer("v3", st, so.Hyper(**kw), {"layers": layers}, dtype=torch.float64)
    names = ["resnet.resnet_50.layer3.0.conv1.weight", "resnet.resnet_50.layer3.1.bn2.weight", "assp.conv3.weight", "assp.bnf.bias",
             "conv.weight", "conv.bias"]
    keys = ["total", "loss_seg"]
    for it in range(2):
        img, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=60 + it, block=8)
        tr.step(img.to(dev), lab.to(dev), it)
        a, b = o32.step(img, lab, it), o64.step(img, lab, it)
        l = tr.losses()
        got = np.array([l[k] for k in keys])
        r32, r64 = np.array([float(a[k]) for k in keys]), np.array([float(b[k]) for k in keys])
        print(f"it {it}: gpu {got} f32 {r32} f64 {r64}")
        bound = 5 * np.abs(r32 - r64) + (2e-4 if it == 0 else 2e-2) * (1 + np.abs(r64))
        assert np.all(np.abs(got - r64) <= bound), f"it {it}"
        if it == 0:
            for n in names:
                p64 = o64.st[n].detach()
                e_ref = (o32.st[n].detach().double() - p64).abs().max().item()
                e_gpu = (tr.params[n].cpu().double() - p64).abs().max().item()
                assert e_gpu <= 5 * e_ref + 1e-6, f"{n}: gpu-vs-f64 {e_gpu:.2e}, fp32-oracle-vs-f64 {e_ref:.2e}"
    sd = tr.state_dict()
    assert set(sd) == set(st)
    assert int(sd["resnet.resnet_50.bn1.num_batches_tracked"]) == int(st["resnet.resnet_50.bn1.num_batches_tracked"]) + 2


def _small(model, width=32):
    if model == "v3":
        layers, ac = (1, 2, 2), width
        st = _v3_state(v3_state_shapes(CN, 0, False, layers, width, ac), 3)
        return st, {"layers": layers, "width": width, "assp_ch": ac}, {"layers": layers}
    lay = VGG_SMALL if width == 32 else [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in VGG_SMALL]
    return _vgg_state(CN, lay, 5), {"vgg_layers": lay}, {"layers": lay}


@pytest.mark.parametrize("model", ["v3", "vgg"])
def test_warmup_single_gradient_accumulation_iter_size2(dev, model):
    """--iter-size 2: two micro-batches, loss / 2, summed gradients, one SGD step, against the float64 oracle: loss 1e-4; parameters within
    3x the distance of the same oracle run in fp32 from float64 (+5e-6)."""
    B, H, W = 2, 97, 97
    st, arch, oarch = _small(model)
    kw = dict(open_classes=0, lr=2.5e-4, iter_size=2)
    tr = WarmupSingleTrainer(model, st, Hyper(**kw), B, H, W, dtype=torch.float32, device=dev, arch=arch)
    truth = OracleWarmupSingleTrainer(model, st, so.Hyper(**kw), oarch, dtype=torch.float64)
    ref32 = OracleWarmupSingleTrainer(model, st, so.Hyper(**kw), oarch)
    mb = [so.synthetic_batch(B, H, W, CD.numpy(), seed=500 + j, block=8) for j in range(2)]
    tr.step([m[0].to(dev) for m in mb], [m[1].to(dev) for m in mb], 0)
    o64 = truth.step([m[0] for m in mb], [m[1] for m in mb], 0)
    ref32.step([m[0] for m in mb], [m[1] for m in mb], 0)
    l = tr.losses()
    assert abs(l["total"] - float(o64["total"])) < 1e-4 * abs(float(o64["total"])), (l, o64)
    names = (["resnet.resnet_50.conv1.weight", "resnet.resnet_50.layer1.0.conv2.weight", "resnet.resnet_50.layer3.1.conv3.weight",
              "assp.convf.weight", "conv.weight", "conv.bias"] if model == "v3" else
             ["features.0.weight", "features.14.bias", "features.29.weight", "classifier.conv2d_list.0.weight", "classifier.conv2d_list.1.bias"])
    for k in names:
        v, p64 = tr.params[k].detach().cpu().double(), truth.st[k].detach()
        e_ref = (ref32.st[k].detach().double() - p64).abs().max().item()
        assert (v - p64).abs().max().item() < 3 * e_ref + 5e-6, (k, e_ref)
    with pytest.raises(ValueError, match="micro-batch"):
        tr.step(mb[0][0].to(dev), mb[0][1].to(dev), 1)


@pytest.mark.parametrize("model", ["v3", "vgg"])
def test_warmup_single_bf16_sanity(dev, model):
    B, H, W = 2, 96, 128
    st, arch, oarch = _small(model, width=64)
    kw = dict(open_classes=0, lr=2.5e-4)
    tr = WarmupSingleTrainer(model, st, Hyper(**kw), B, H, W, dtype=torch.bfloat16, device=dev, arch=arch)
    orc = OracleWarmupSingleTrainer(model, st, so.Hyper(**kw), oarch, dtype=torch.float64)
    img, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=77, block=8)
    tr.step(img.to(dev), lab.to(dev), 0)
    out = orc.step(img, lab, 0)
    l = tr.losses()
    got, ref = np.array([l["total"], l["loss_seg"]]), np.array([float(out["total"]), float(out["loss_seg"])])
    print(model, "bf16", got, "f64", ref)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= 0.1 * (1 + np.abs(ref)))
    for n in tr.sgd_names:
        assert torch.isfinite(tr.params[n]).all()


def test_warmup_single_counts_bad_labels(dev):
    st, arch, _ = _small("vgg")
    tr = WarmupSingleTrainer("vgg", st, Hyper(open_classes=0), 2, 64, 64, dtype=torch.float32, device=dev, arch=arch)
    img, lab = so.synthetic_batch(2, 64, 64, CD.numpy(), seed=9, block=8)
    lab[1, 5, 7] = 40
    tr.step(img.to(dev), lab.to(dev), 0)
    with pytest.raises(ValueError, match="1 label value"):
        tr.losses()
    lab[1, 5, 7] = 3
    tr.step(img.to(dev), lab.to(dev), 1)
    assert np.isfinite(tr.losses()["loss_seg"])


def _rccl_worker(model, port, q):
    """ONE rank, backend "nccl" (= RCCL), SIMT_DP_FORCE=1: the bucket reducer's collectives run; a mean over one rank is the identity, so the
    trajectory must be bit-identical to the plain trainer's."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SIMT_CU_BUDGET"] = "240"      # a data-parallel plan's default CU budget, given to both plans: the same tile lists in both
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        dev = torch.device("cuda:0")
        st, arch, _ = _small(model, width=64)
        hp = Hyper(open_classes=0, lr=6e-4)
        os.environ["SIMT_DP_FORCE"] = "1"
        dp = WarmupSingleTrainer(model, st, hp, 2, 96, 128, dtype=torch.bfloat16, device=dev, arch=arch, process_group=dist.group.WORLD)
        assert dp.reducer is not None and not dp.reducer.single and dp.plan.data_parallel
        solo = WarmupSingleTrainer(model, st, hp, 2, 96, 128, dtype=torch.bfloat16, device=dev, arch=arch)
        ok = True
        for it in range(3):
            img, lab = so.synthetic_batch(2, 96, 128, CD.numpy(), seed=100 + it, block=8)
            dp.step(img.to(dev), lab.to(dev), it)
            solo.step(img.to(dev), lab.to(dev), it)
            sel = [1, 6, 14, 15]             # loss, valid pixels, total, bad labels (the SimT-only slots hold NaN: 0 / 0)
            ok = ok and torch.equal(dp.hout[sel], solo.hout[sel])
        torch.cuda.synchronize()
        same = all(torch.equal(dp.params[k], solo.params[k]) for k in dp.params) and all(torch.equal(dp.mom[k], solo.mom[k]) for k in dp.mom)
        dp.losses()
        q.put((bool(ok), bool(same), dp.reducer.world))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("model", ["v3", "vgg"])
def test_warmup_single_rccl_group_same_trajectory(dev, model):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    p = ctx.Process(target=_rccl_worker, args=(model, port, q))
    p.start()
    try:
        ok, same, world = q.get(timeout=600)
    finally:
        p.join(120)
    assert p.exitcode == 0, p.exitcode
    assert ok and same and world == 1, "RCCL world-1 data-parallel warm-up diverges from the single-GPU trainer"


@pytest.mark.parametrize("model", ["DeepLabv3", "DeepLabVGG"])
def test_warmup_tool_single_model_real_files_and_simt_handoff(dev, tmp_path, capsys, model):
    """trainV1_warmup --model DeepLabv3 | DeepLabVGG on real files: evaluations at iterations 2 and 4, the best-mIoU rotation with the
    warm-up's file names, the final GTA5_6.pth loading strict=True into the module; then trainV2_simt --model <same> restores it: the
    frozen model every tensor, the trainable one every tensor but conv_1 (DeepLabv3) / the features (VGG: the wider classifier keeps its
    init)."""
    Image = pytest.importorskip("PIL.Image")
    import re

    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as simt
    from test_gpu_tools import _make_dataset
    _make_dataset(tmp_path, Image)
    snap = str(tmp_path / "snap")
    val = ["--data-dir-val", str(tmp_path), "--data-list-val", str(tmp_path / "kit" / "val.txt"), "--gt-dir-val", str(tmp_path / "gt"),
           "--devkit-dir", str(tmp_path / "kit")]
    argv = ["--model", model, "--data-dir-target", str(tmp_path), "--data-list-target", str(tmp_path / "pseudo.lst"),
            "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--num-steps-stop", "6", "--save-pred-every", "2",
            "--print-every", "1", "--learning-rate", "2.5e-4", "--from-scratch", "--restore-from", "", "--snapshot-dir", snap,
            "--num-workers", "2", "--random-mirror"]
    tool.main(argv + val)
    out = capsys.readouterr().out
    assert out.count("Begin evaluation") == 2 and out.count("===> mIoU:") == 2
    assert "iter =        5/" in out and "loss_seg = " in out and "save model" in out
    final = os.path.join(snap, "GTA5_6.pth")
    sd = torch.load(final)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
    if model == "DeepLabv3":
        from simt_amd.model.deeplabv3 import DeepLabv3
        m = DeepLabv3(CN)
        assert int(sd["resnet.resnet_50.bn1.num_batches_tracked"]) == 6 and int(sd["resnet.resnet_50.layer4.0.bn1.num_batches_tracked"]) == 0
    else:
        from simt_amd.model.deeplab_vgg import DeeplabVGG
        m = DeeplabVGG(CN)
    m.load_state_dict(sd, strict=True)
    best = glob.glob(os.path.join(snap, "GTA5_BAPA_warmup_iter*_mIoU*.pth"))
    assert len(best) == 1
    # no validation set: one rolling periodic snapshot
    snap2 = str(tmp_path / "snap2")
    i = argv.index("--snapshot-dir")
    tool.main(argv[:i] + ["--snapshot-dir", snap2] + argv[i + 2:])
    assert sorted(os.listdir(snap2)) == ["GTA5_6.pth", "GTA5_BAPA_warmup_iter4.pth"]
    capsys.readouterr()
    # the SimT stage starts from the warm-up's file
    simt.main(["--model", model, "--synthetic", "--restore-from", final, "--input-size-target", "129,65", "--batch-size", "2",
               "--num-steps-stop", "1", "--open-classes", "3", "--snapshot-dir", str(tmp_path / "simt")])
    out = capsys.readouterr().out
    n1, n2 = map(int, re.search(r"restored (\d+)/(\d+) tensors", out).groups())
    trainable, frozen = simt.single_model_states(model, CN, 3)
    assert n2 == len(frozen) == len(sd)
    if model == "DeepLabv3":
        assert n1 == len(trainable) - 2 and not any(k.startswith("conv_1.") for k in sd)
    else:
        assert n1 == len([k for k in trainable if k.startswith("features.")])
