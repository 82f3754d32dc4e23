"""GPU parity of the pseudo-label export for DeepLabv3 and DeepLab-VGG16 (make_pseudo_labels --arch v3 | vgg; csrc/label_sweep.hip
simt_pseudo_label2_u8): arg-max mode bitwise against simt_upsample2_sum_argmax (the evaluator's kernel), confidence mode against the
oracle's confidence_labels of the model's input-size output, PseudoLabeller against Evaluator.predict and the fp32 oracle forwards,
the command line end to end (PNGs, list, prior, the SimT trainer reading the prior), and one DeepLabv3 R-50 run at full size."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from test_gpu_pseudo_labels import _write_frames

pytestmark = pytest.mark.gpu


def _logits(B, h, w, ld, C, seed, scale=3.0):
    """NHWC logits [B*h*w, ld] on the CPU: random in the first C channels, 1e3 planted in channels >= C (never read)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, h, w, ld), 1e3)
    x[..., :C] = torch.randn(B, h, w, C, generator=g) * scale
    return x.reshape(B * h * w, ld)


def _scale_args(maps, dev):
    d = [(lg.to(dev), h, w, hiwi) for (lg, h, w, hiwi) in maps]
    (la, ha, wa, (hia, wia)) = d[0]
    args = [ops._p(la), ha, wa, la.shape[1], hia, wia]
    if len(d) > 1:
        (lb, hb, wb, (hib, wib)) = d[1]
        args += [ops._p(lb), hb, wb, lb.shape[1], hib, wib]
    else:
        args += [None, 0, 0, 0, 0, 0]
    return d, args


GEOS = {
    # name: (B, H, W, [(h, w, (hi, wi))])
    "reference": (1, 1024, 2048, [(64, 128, (512, 1024)), (80, 160, (640, 1280))]),
    "odd": (2, 1001, 1537, [(33, 47, (257, 371)), (41, 59, (321, 463))]),
}


@pytest.mark.parametrize("geo", list(GEOS))
@pytest.mark.parametrize("ld", [22, 24])
def test_argmax_mode_equals_upsample2_sum_argmax(dev, geo, ld):
    B, H, W, scales = GEOS[geo]
    C = 19
    P = B * H * W
    maps = [(_logits(B, h, w, ld, C, 10 * i + ld + H), h, w, hiwi) for i, (h, w, hiwi) in enumerate(scales)]
    for n in (2, 1):
        d, args = _scale_args(maps[:n], dev)
        assert all(t.data_ptr() % 16 == 0 for (t, *_r) in d)                     # ld 24: the float4 gathers, ld 22: scalar
        pred = torch.full((B, H, W), -1, device=dev, dtype=torch.int32)
        L.call("simt_upsample2_sum_argmax", *args, B, H, W, C, ops._p(pred), ops.stream_ptr())
        buf = torch.full((P + 64,), 77, device=dev, dtype=torch.uint8)         # 64 guard bytes behind the map
        counts = torch.zeros(C + 1, device=dev, dtype=torch.int64)
        for _ in range(2):                                                      # counts accumulate across calls
            L.call("simt_pseudo_label2_u8", *args, B, H, W, C, 0, 0.0, ops._p(buf), ops._p(counts), ops.stream_ptr())
        out = buf[:P].view(B, H, W).cpu()
        ref = pred.cpu()
        assert int(ref.min()) >= 0 and int(ref.max()) < C and len(torch.unique(ref)) >= 10
        assert torch.equal(out, ref.to(torch.uint8)), f"{n} scale(s): {int((out != ref.to(torch.uint8)).sum())} labels differ"
        assert torch.all(buf[P:].cpu() == 77), "the kernel wrote past the end of the label map"
        exp = np.bincount(out.numpy().reshape(-1), minlength=C + 1)[:C + 1]
        assert exp[C] == 0
        assert np.array_equal(counts.cpu().numpy(), 2 * exp)


def _check_confidence(got, prob, th, counts, C, margin=1e-5, max_exempt=1e-3):
    """got: device labels [B,H,W] (numpy); prob: the oracle's probabilities [B,C,H,W].  Labels equal the oracle's confidence labels outside
    the margin (top probability within `margin` of the threshold, or a top-2 gap below it; at most `max_exempt` of the pixels exempt)."""
    m, a = prob.max(1)
    ref = torch.where(m > th, a, torch.full_like(a, 255)).numpy()
    top2 = prob.topk(2, dim=1).values.numpy()
    assert 0.05 < (ref != 255).mean() < 0.95, "both sides of the threshold must occur"
    exempt = (np.abs(top2[:, 0] - th) < margin) | (top2[:, 0] - top2[:, 1] < margin)
    diff = got != ref
    print(f"{int(diff.sum())} labels differ; {int(exempt.sum())} of {exempt.size} pixels exempt; {100 * (ref != 255).mean():.1f} % confident")
    assert exempt.mean() <= max_exempt
    assert not np.any(diff & ~exempt), f"{int((diff & ~exempt).sum())} labels differ outside the margin"
    c = counts.cpu().numpy()
    assert c[C] == int((got == 255).sum()) and c.sum() == got.size
    assert np.array_equal(c[:C], np.bincount(got[got != 255], minlength=C))


@pytest.mark.parametrize("ld", [22, 24])
def test_confidence_mode_matches_oracle(dev, ld):
    C, B, h, w, (hi, wi), (H, W) = 19, 2, 37, 53, (150, 211), (301, 423)
    lg = _logits(B, h, w, ld, C, 11, scale=2.5)
    x = lg.view(B, h, w, ld)
    x[..., 3] += torch.linspace(-2, 12, w).view(1, 1, w)                   # confident on one side, uncertain on the other
    logits = x[..., :C].permute(0, 3, 1, 2).contiguous()
    up = F.interpolate(logits, size=(hi, wi), mode="bilinear", align_corners=False)
    hp = types.SimpleNamespace(th_high=0.8, th_low=-1.0, num_classes=C)
    _, prob_flat = so.confidence_labels(up, (H, W), hp)
    prob = prob_flat.view(B, H, W, C).permute(0, 3, 1, 2)
    d, args = _scale_args([(lg, h, w, (hi, wi))], dev)
    out = torch.zeros(B, H, W, device=dev, dtype=torch.uint8)
    counts = torch.zeros(C + 1, device=dev, dtype=torch.int64)
    L.call("simt_pseudo_label2_u8", *args, B, H, W, C, 1, 0.8, ops._p(out), ops._p(counts), ops.stream_ptr())
    _check_confidence(out.cpu().numpy(), prob, 0.8, counts, C)
    with pytest.raises(L.SimtHipError):                                       # confidence mode takes one scale
        L.call("simt_pseudo_label2_u8", *args[:6], *args[:6], B, H, W, C, 1, 0.8, ops._p(out), ops._p(counts), ops.stream_ptr())


# ------------------------------------------------------------------------------------------------------------ PseudoLabeller
def _v3_state(K, seed):
    from test_gpu_single import _v3_state as scaled
    from simt_amd.engine_v3 import v3_state_shapes
    return scaled(v3_state_shapes(19, K, K > 0, (1, 1, 1)), seed)


def _images(s1, s2, seed):
    g = torch.Generator().manual_seed(seed)
    img1 = torch.randn(1, 3, *s1, generator=g) * 50
    return img1, F.interpolate(img1, size=s2, mode="bilinear", align_corners=True)


def _threshold(prob):
    """A threshold at the median of the oracle's top probability (rounded): confident and unconfident pixels both occur."""
    return float(np.round(np.quantile(prob.max(1)[0].numpy(), 0.5), 2))


@pytest.mark.parametrize("arch", ["v3", "vgg"])
@pytest.mark.parametrize("K", [0, 6])
def test_labeller_matches_evaluator_and_oracle(dev, arch, K):
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    from simt_amd.tools.make_pseudo_labels import PseudoLabeller
    from test_gpu_single import VGG_SMALL, _vgg_state
    C, HW = 19, (64, 96)
    s1, s2 = (48, 64), (56, 80)
    if arch == "v3":
        st, layers = _v3_state(K, 41 + K), (1, 1, 1)
    else:
        st, layers = _vgg_state(C + K, VGG_SMALL, 8 + K), VGG_SMALL
    img1, img2 = _images(s1, s2, 5 + K)
    with torch.no_grad():
        if arch == "v3":
            o = so.v3_forward(st, img1, layers, openset=K > 0, train=False)
        else:
            o = so.vgg_forward(st, img1, layers)
    # the logits are linear in the classifier's weights and biases: scale them to a standard deviation of 3, so that the softmax is
    # neither saturated nor flat and confident and unconfident pixels both occur
    f = 3.0 / float(o[:, :C].std())
    head = ("conv.", "conv_1.") if arch == "v3" else ("classifier.",)
    st = {k: (v * f if k.startswith(head) else v) for k, v in st.items()}
    o = o * f
    kw = dict(num_classes=C, open_classes=K, label_hw=HW, scales=(s1, s2), device=dev, layers=layers)
    lab = PseudoLabeller(st, arch=arch, **kw)
    got = lab.label(img1, img2)[0].cpu().numpy()
    ref = Evaluator(st, model=arch, **kw).predict(img1, img2)[0].cpu().numpy()
    assert len(np.unique(ref)) >= 3
    assert np.array_equal(got, ref.astype(np.uint8)), f"{int((got != ref).sum())} labels differ from Evaluator.predict"
    assert np.array_equal(lab.counts.cpu().numpy(), np.bincount(got.reshape(-1), minlength=C + 1)[:C + 1])
    # confidence mode (first scale) against the fp32 oracle forward + confidence_labels
    hp = types.SimpleNamespace(th_high=0.8, th_low=-1.0, num_classes=C)
    _, prob_flat = so.confidence_labels(o[:, :C], HW, hp)
    prob = prob_flat.view(1, *HW, C).permute(0, 3, 1, 2)
    th = _threshold(prob)
    lab = PseudoLabeller(st, arch=arch, mode="confidence", threshold=th, **kw)
    got = lab.label(img1)[0].cpu().numpy()
    # the forwards differ from the oracle's by the fp32 conv parity error (tests/test_gpu_eval_single.py: 1e-4 of the logits' range)
    _check_confidence(got[None], prob, th, lab.counts, C, margin=1e-4, max_exempt=5e-3)


# ------------------------------------------------------------------------------------------------------------ command line
def _check_export(dev, root, names, kit, st, arch, K, layers, scales, label_hw, out_name, counts_npy):
    from PIL import Image

    from simt_amd.data.pipeline import InputPrep
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    from simt_amd.tools import compute_ClassDistribution as ccd
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    ev = Evaluator(st, num_classes=19, open_classes=K, label_hw=label_hw, scales=scales, device=dev, layers=layers, model=arch)
    hist = np.zeros(20, np.int64)
    preps = {}
    for name in names:
        rgb = np.asarray(Image.open(os.path.join(root, "train", name)).convert("RGB"))
        key = rgb.shape[:2]
        if key not in preps:
            preps[key] = [InputPrep(1, key, (w, h), dev, with_label=False) for (h, w) in scales]
        xs = [torch.empty(1, 3, h, w, device=dev) for (h, w) in scales]
        for prep, x in zip(preps[key], xs):
            prep.run(torch.from_numpy(rgb[None].copy()).to(dev), x)
        ref = ev.predict(*xs)[0].cpu().numpy()
        png = np.asarray(Image.open(os.path.join(root, out_name, os.path.basename(name))))
        assert png.dtype == np.uint8 and png.shape == tuple(label_hw)
        assert np.array_equal(png, ref.astype(np.uint8)), f"{name}: {int((png != ref).sum())} labels differ from Evaluator.predict"
        hist += np.bincount(png.reshape(-1), minlength=20)[:20]
    lst = os.path.join(root, out_name + ".lst")
    assert open(lst).read().splitlines() == [f"train/{n}\t{out_name}/{os.path.basename(n)}" for n in names]
    ds = cityscapesPseudo(root, lst)
    for i in range(len(ds)):
        _, lab, _ = ds.decode(i)
        assert lab.shape == tuple(label_hw)
    ref_npy = os.path.join(root, out_name + "_ref.npy")
    ccd.main(["--pred-dir", os.path.join(root, out_name), "--devkit-dir", kit, "--out", ref_npy, "--device", str(dev)])
    mine = np.load(counts_npy)
    assert mine.dtype == np.float64 and np.array_equal(mine, np.load(ref_npy))
    assert np.array_equal(mine, hist[:19] / (hist[:19].sum() + 10e-10))


@pytest.mark.parametrize("arch", ["v3", "vgg"])
def test_command_line_end_to_end(dev, tmp_path, arch):
    from simt_amd.tools import make_pseudo_labels as mpl
    from simt_amd.tools import trainV2_simt
    from simt_amd.tools.trainV2_simt import single_model_state, single_model_states
    root = str(tmp_path)
    names, kit = _write_frames(root, 3, (96, 192), 3)
    if arch == "v3":          # a warm-up checkpoint of DeepLabv3 at a small depth
        K, layers, model = 0, (1, 1, 1), "DeepLabv3"
        st = single_model_state(model, 19, layers, seed=7)
        extra = ["--v3-layers", "1", "1", "1"]
    else:                     # a SimT checkpoint of DeeplabVGG(19 + 3), full VGG16 width
        K, layers, model = 3, None, "DeepLabVGG"
        st, _ = single_model_states(model, 19, K, seed=8)
        extra = ["--open-classes", "3"]
    ckpt = os.path.join(root, "ckpt.pth")
    torch.save(st, ckpt)
    scales, label_hw = ((48, 96), (64, 128)), (72, 144)
    npy = os.path.join(root, f"ClassDist_pseudo_{arch}.npy")
    mpl.main(["--restore-from", ckpt, "--arch", arch, *extra, "--data-dir", root, "--data-list", os.path.join(root, "train.txt"),
              "--input-size", "96,48", "--input-size", "128,64", "--label-size", "144,72", "--out-name", f"pseudo_{arch}",
              "--list-out", os.path.join(root, f"pseudo_{arch}.lst"), "--num-workers", "2"])
    _check_export(dev, root, names, kit, st, arch, K, layers, scales, label_hw, f"pseudo_{arch}", npy)
    trainV2_simt.main(["--model", model, "--synthetic", "--class-dist", npy, "--num-steps-stop", "2", "--num-steps", "10",
                       "--input-size-target", "128,64", "--snapshot-dir", os.path.join(root, "snap"), "--print-every", "1",
                       "--open-classes", "3", *(["--v3-layers", "1", "1", "1"] if arch == "v3" else [])])
    assert os.path.exists(os.path.join(root, "snap", "GTA5_2.pth"))


def test_v3_r50_full_size(dev, tmp_path):
    """--arch v3 at model/deeplabv3.py's R-50 depth, fp32, the default scales 1024 x 512 + 1280 x 640, labels 2048 x 1024, two frames."""
    from simt_amd.tools import make_pseudo_labels as mpl
    from simt_amd.tools.trainV2_simt import single_model_state
    root = str(tmp_path)
    names, kit = _write_frames(root, 2, (1024, 2048), 4)
    st = single_model_state("DeepLabv3", 19, seed=9)
    ckpt = os.path.join(root, "v3.pth")
    torch.save(st, ckpt)
    mpl.main(["--restore-from", ckpt, "--arch", "v3", "--data-dir", root, "--data-list", os.path.join(root, "train.txt"),
              "--out-name", "pseudo_r50", "--list-out", os.path.join(root, "pseudo_r50.lst"), "--num-workers", "2"])
    _check_export(dev, root, names, kit, st, "v3", 0, None, ((512, 1024), (640, 1280)), (1024, 2048), "pseudo_r50",
                  os.path.join(root, "ClassDist_pseudo_r50.npy"))
