"""GPU parity of the pseudo-label export (simt_amd.tools.make_pseudo_labels, csrc/label_sweep.hip simt_pseudo_label_u8):
arg-max mode bitwise against simt_upsample_sum_argmax (the evaluation kernel, which tests/test_gpu_eval.py pins to the reference),
confidence mode against the oracle's confidence_labels (trainV2_simt.py:353-359), the exported files against Evaluator.predict,
cityscapesPseudo and compute_ClassDistribution, the single-head model against the fp32 oracle, and the command line at full depth."""
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu


def _nhwc(t, ld, dev):
    o = torch.zeros(t.shape[0], t.shape[2], t.shape[3], ld)
    o[..., :t.shape[1]] = t.permute(0, 2, 3, 1)
    return o.to(dev)


@pytest.mark.parametrize("B,H,W", [(1, 1024, 2048), (2, 1001, 1537)])
def test_argmax_mode_equals_upsample_sum_argmax(dev, B, H, W):
    g = torch.Generator().manual_seed(H + W)
    C, ld = 19, 22
    la = _nhwc(torch.randn(B, C, 65, 129, generator=g) * 3, ld, dev)
    lb = _nhwc(torch.randn(B, C, 81, 161, generator=g) * 3, ld, dev)
    P = B * H * W
    for two in (True, False):
        pred = torch.full((B, H, W), -1, device=dev, dtype=torch.int32)
        L.call("simt_upsample_sum_argmax", ops._p(la), 65, 129, ld, ops._p(lb) if two else None, 81 if two else 0, 161 if two else 0,
               ld if two else 0, B, H, W, C, ops._p(pred), ops.stream_ptr())
        buf = torch.full((P + 64,), 77, device=dev, dtype=torch.uint8)            # 64 guard bytes behind the map
        counts = torch.zeros(C + 1, device=dev, dtype=torch.int64)
        for _ in range(2):                                                       # counts accumulate across calls
            L.call("simt_pseudo_label_u8", ops._p(la), 65, 129, ld, ops._p(lb) if two else None, 81 if two else 0,
                   161 if two else 0, ld if two else 0, B, H, W, C, 0, 0.0, ops._p(buf), ops._p(counts), ops.stream_ptr())
        out = buf[:P].view(B, H, W).cpu()
        ref = pred.cpu()
        assert int(ref.min()) >= 0 and int(ref.max()) < C
        assert torch.equal(out, ref.to(torch.uint8)), f"{int((out != ref.to(torch.uint8)).sum())} labels differ"
        assert torch.all(buf[P:].cpu() == 77), "the kernel wrote past the end of the label map"
        exp = np.bincount(out.numpy().reshape(-1), minlength=C + 1)[:C + 1]
        exp[C] = 0
        assert np.array_equal(counts.cpu().numpy(), 2 * exp)


def test_confidence_mode_matches_oracle(dev):
    g = torch.Generator().manual_seed(11)
    C, ld, h, H = 19, 22, 97, 769
    logits = torch.randn(1, C, h, h, generator=g) * 2.5
    logits[:, 3] += torch.linspace(-2, 12, h).view(1, h, 1)                    # confident on one side, uncertain on the other
    hp = types.SimpleNamespace(th_high=0.8, th_low=-1.0, num_classes=C)
    conf, prob_flat = so.confidence_labels(logits, (H, H), hp)
    ref = conf[0].numpy()
    top2 = np.sort(prob_flat.numpy(), axis=1)[:, -2:].reshape(H, H, 2)
    assert 0.05 < (ref != 255).mean() < 0.95, "both sides of the threshold must occur"
    src = _nhwc(logits, ld, dev)
    prob = torch.zeros_like(src)
    ops.softmax_rows(src, ld, prob, ld, h * h, C)
    out = torch.zeros(1, H, H, device=dev, dtype=torch.uint8)
    counts = torch.zeros(C + 1, device=dev, dtype=torch.int64)
    L.call("simt_pseudo_label_u8", ops._p(prob), h, h, ld, None, 0, 0, 0, 1, H, H, C, 1, 0.8, ops._p(out), ops._p(counts),
           ops.stream_ptr())
    got = out[0].cpu().numpy()
    exempt = (np.abs(top2[..., 1] - 0.8) < 1e-5) | (top2[..., 1] - top2[..., 0] < 1e-5)
    diff = got != ref
    print(f"{int(diff.sum())} labels differ; {int(exempt.sum())} of {exempt.size} pixels exempt")
    assert exempt.mean() <= 1e-3
    assert not np.any(diff & ~exempt), f"{int((diff & ~exempt).sum())} labels differ outside the margin"
    c = counts.cpu().numpy()
    assert c[C] == int((got == 255).sum()) and c.sum() == got.size
    assert np.array_equal(c[:C], np.bincount(got[got != 255], minlength=C))
    with pytest.raises(L.SimtHipError):                                       # confidence mode takes one scale
        L.call("simt_pseudo_label_u8", ops._p(prob), h, h, ld, ops._p(prob), h, h, ld, 1, H, H, C, 1, 0.8, ops._p(out),
               ops._p(counts), ops.stream_ptr())


def _write_frames(root, n, hw, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i in range(n):
        name = f"city/city_{i:06d}_000019_leftImg8bit.png"
        os.makedirs(os.path.join(root, "train", "city"), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (*hw, 3), dtype=np.uint8)).save(os.path.join(root, "train", name))
        names.append(name)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    kit = os.path.join(root, "kit")
    os.makedirs(kit, exist_ok=True)
    with open(os.path.join(kit, "train.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    pal = [[(37 * c) % 256, (91 * c) % 256, (53 * c) % 256] for c in range(19)] + [[0, 0, 0]]
    json.dump({"classes": 19, "palette": pal}, open(os.path.join(kit, "info.json"), "w"))
    return names, kit


def test_export_multi_head_end_to_end(dev, tmp_path):
    from PIL import Image

    from simt_amd.data.pipeline import InputPrep
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    from simt_amd.tools import compute_ClassDistribution as ccd
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    from simt_amd.tools.make_pseudo_labels import export
    layers, K = (1, 1, 2, 1), 3
    st = so.recipe_state(so.state_shapes(19, K, True, layers=layers), seed=31, head_scale=8.0)
    root = str(tmp_path)
    names, kit = _write_frames(root, 3, (96, 192), 1)
    scales, label_hw = ((48, 96), (64, 128)), (72, 144)
    lst = os.path.join(root, "pseudo_t.lst")
    counts = export(st, root, os.path.join(root, "train.txt"), "pseudo_t", lst, workers=2, num_classes=19, open_classes=K,
                    scales=scales, label_hw=label_hw, device=dev, layers=layers)
    ev = Evaluator(st, num_classes=19, open_classes=K, label_hw=label_hw, scales=scales, device=dev, layers=layers)
    preps = [InputPrep(1, (96, 192), (w, h), dev, with_label=False) for (h, w) in scales]
    hist = np.zeros(20, np.int64)
    for name in names:
        rgb = np.asarray(Image.open(os.path.join(root, "train", name)).convert("RGB"))
        xs = [torch.empty(1, 3, h, w, device=dev) for (h, w) in scales]
        for prep, x in zip(preps, xs):
            prep.run(torch.from_numpy(rgb[None].copy()).to(dev), x)
        ref = ev.predict(*xs)[0].cpu().numpy()
        png = np.asarray(Image.open(os.path.join(root, "pseudo_t", os.path.basename(name))))
        assert png.dtype == np.uint8 and png.shape == label_hw
        assert np.array_equal(png, ref.astype(np.uint8)), f"{name}: {int((png != ref).sum())} labels differ from Evaluator.predict"
        hist += np.bincount(png.reshape(-1), minlength=20)[:20]
    assert np.array_equal(counts[:19], hist[:19]) and counts[19] == 0
    assert not [f for f in os.listdir(os.path.join(root, "pseudo_t")) if f.endswith(".tmp")]
    lines = open(lst).read().splitlines()
    assert lines == [f"train/{n}\tpseudo_t/{os.path.basename(n)}" for n in names]
    ds = cityscapesPseudo(root, lst)
    for i in range(len(ds)):
        rgb, lab, _ = ds.decode(i)
        assert rgb.shape == (96, 192, 3) and lab.shape == label_hw
    cd = ccd.compute_CD("", os.path.join(root, "pseudo_t"), kit, device=dev, workers=2)
    assert np.array_equal(cd, counts[:19].astype(np.float64))
    ref_npy = os.path.join(root, "ref.npy")
    ccd.main(["--pred-dir", os.path.join(root, "pseudo_t"), "--devkit-dir", kit, "--out", ref_npy, "--device", str(dev)])
    mine = np.load(os.path.join(root, "ClassDist_pseudo_t.npy"))
    assert mine.dtype == np.float64 and np.array_equal(mine, np.load(ref_npy))


def test_single_head_matches_oracle(dev):
    from simt_amd.tools.make_pseudo_labels import PseudoLabeller
    layers = (1, 1, 2, 1)
    st = so.recipe_state(so.state_shapes(19, single_head=True, layers=layers), seed=7, head_scale=8.0)
    g = torch.Generator().manual_seed(4)
    img = torch.randn(1, 3, 41, 61, generator=g) * 50
    H, W = 64, 96
    lab = PseudoLabeller(st, arch="single", scales=((41, 61),), label_hw=(H, W), device=dev, layers=layers)
    got = lab.label(img)[0].cpu().numpy()
    y, _ = so.deeplab_single_forward(st, img, False, layers=layers)
    out = so.upsample(y, (H, W))[0].numpy()
    ref = out.argmax(0)
    top2 = np.sort(out, axis=0)[-2:]
    gap = top2[1] - top2[0]
    margin = 1e-4 * np.abs(out).max()
    diff = got != ref
    print(f"{int(diff.sum())} of {diff.size} labels differ; {int((gap < margin).sum())} pixels with a top-2 gap below {margin:.2e}")
    assert not np.any(diff & (gap >= margin))
    assert (gap < margin).mean() < 5e-3
    assert np.array_equal(lab.counts.cpu().numpy(), np.bincount(got.reshape(-1), minlength=20)[:20])


def test_command_line_full_depth_confidence_and_training_prior(dev, tmp_path):
    from PIL import Image

    from simt_amd import model_spec as ms
    from simt_amd.tools import make_pseudo_labels as mpl
    from simt_amd.tools import trainV2_simt
    root = str(tmp_path)
    names, kit = _write_frames(root, 2, (130, 258), 2)
    st = ms.reference_init(ms.state_shapes(19, 0, False), seed=3)
    # a random-init head is unconfident everywhere: scale layer6 (weights and bias: logits are linear in them) so the logits of
    # the fp32 oracle have a standard deviation of ~8 -> confident and unconfident pixels both occur
    with torch.no_grad():
        _, y = so.deeplab_multi_forward(st, torch.randn(1, 3, 65, 129, generator=torch.Generator().manual_seed(0)) * 50, False, False)
    s = 8.0 / max(float(y.std()), 1e-12)
    for k in list(st):
        if k.startswith("layer6."):
            st[k] = st[k] * s
    ckpt = os.path.join(root, "src.pth")
    torch.save(st, ckpt)
    lst, npy = os.path.join(root, "p.lst"), os.path.join(root, "cd.npy")
    mpl.main(["--restore-from", ckpt, "--data-dir", root, "--data-list", os.path.join(root, "train.txt"), "--input-size", "129,65",
              "--label-size", "258,130", "--threshold", "0.8", "--save-color", "--devkit-dir", kit, "--out-name", "pseudo_c",
              "--list-out", lst, "--class-dist-out", npy, "--num-workers", "2"])
    for n in names:
        base = os.path.join(root, "pseudo_c", os.path.basename(n)[:-4])
        lab = Image.open(base + ".png")
        col = Image.open(base + "_color.png")
        assert lab.mode == "L" and lab.size == (258, 130) and col.mode == "P"
        assert np.array_equal(np.array(col), np.array(lab))
    labs = np.concatenate([np.array(Image.open(os.path.join(root, "pseudo_c", os.path.basename(n)))).reshape(-1) for n in names])
    assert 0 < (labs == 255).mean() < 1
    cd = np.load(npy)
    assert cd.shape == (19,) and abs(cd.sum() - 1) < 1e-6
    assert len(open(lst).read().splitlines()) == 2
    trainV2_simt.main(["--synthetic", "--class-dist", npy, "--num-steps-stop", "2", "--num-steps", "10", "--input-size-target", "129,65",
                       "--snapshot-dir", os.path.join(root, "snap"), "--print-every", "1", "--open-classes", "3"])
    assert os.path.exists(os.path.join(root, "snap", "GTA5_2.pth"))
