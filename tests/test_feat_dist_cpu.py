"""The ImageNet feature distance without a GPU: the restatement of tests/_feat_dist_ref.py against literal torch forms, the
comparators the GPU tests use against planted errors, the keyword checks, the checkpoint mapping and the tool's flags."""
import numpy as np
import pytest
import torch

import _feat_dist_ref as fr
from simt_amd import feat_dist as fd
from simt_amd import model_spec as ms
from simt_amd import pretrained


def _blocky_labels(B, H, W, block, seed, values=tuple(range(19)) + (255, 255, 40, -1)):
    g = np.random.default_rng(seed)
    by, bx = -(-H // block), -(-W // block)
    cells = np.asarray(values, dtype=np.int64)[g.integers(0, len(values), (B, by, bx))]
    lab = cells.repeat(block, 1).repeat(block, 2)[:, :H, :W].copy()
    noise = g.random((B, H, W)) < 0.08
    lab[noise] = np.asarray(values, dtype=np.int64)[g.integers(0, len(values), int(noise.sum()))]
    return lab


@pytest.mark.parametrize("N,n", [(768, 97), (65, 9), (129, 17), (97, 5), (9, 9), (17, 1), (64, 8)])
def test_windows_partition_the_label(N, n):
    win = fr.windows(N, n)
    owner = np.zeros(N, dtype=np.int64)
    for lo, hi in win:
        assert hi > lo
        owner[lo:hi] += 1
    assert (owner == 1).all() and win[0][0] == 0 and win[-1][1] == N
    if (N, n) == (768, 97):
        assert {hi - lo for lo, hi in win} == {7, 8}


@pytest.mark.parametrize("s,h,w,ratio", [(8, 5, 7, 0.75), (7, 6, 4, 0.75), (3, 9, 5, 1.0), (4, 4, 4, 0.51), (1, 6, 5, 0.75)])
def test_mask_equals_downscale_label_ratio(s, h, w, ratio):
    lab = _blocky_labels(2, s * h, s * w, max(s, 2) + 1, seed=s * 10 + h)
    got, N = fr.mask_ref(lab, h, w, fr.DEFAULT_CLASSES, ratio)
    want = fr.torch_mask(lab, s, fr.DEFAULT_CLASSES, ratio)
    assert (got == want).all() and N == int(want.sum())
    assert 0 < N < got.size, "the case shows nothing"


def test_mask_at_and_under_the_ratio():
    lab = np.full((1, 8, 16), 255, dtype=np.int64)
    lab[0, :, :8] = np.array([13] * 48 + [0] * 16).reshape(8, 8)          # 48 of 64: exactly 0.75
    lab[0, :, 8:] = np.array([13] * 47 + [0] * 17).reshape(8, 8)          # one pixel under
    got, N = fr.mask_ref(lab, 1, 2, (13,), 0.75)
    assert got.tolist() == [1, 0] and N == 1
    assert fr.mask_ref(lab, 1, 2, (0,), 0.75)[1] == 0 and fr.mask_ref(lab, 1, 2, (13,), 1.0)[1] == 0


def _case(M=40, C=64, seed=0, lam=0.005, gscale=0.5):
    g = np.random.default_rng(seed)
    fs = g.standard_normal((M, C)).astype(np.float32)
    fi = (fs + 0.5 * g.standard_normal((M, C))).astype(np.float32)
    mask = (g.random(M) < 0.5).astype(np.uint8)
    mask[:4] = [1, 0, 1, 1]
    fs[3] = fi[3]          # a kept row at distance 0
    return fs, fi, mask, fr.dist_ref(fs, fi, mask, lam, gscale)


def test_seed_equals_autograd_in_float64():
    fs, fi, mask, ref = _case()
    x = torch.tensor(fs, dtype=torch.float64, requires_grad=True)
    keep = torch.from_numpy(mask.astype(bool))
    rows = keep.clone()
    rows[3] = False          # (the norm has no gradient at 0: autograd gives NaN there, the contract +0)
    loss = ref["lam_g"] * (x - torch.tensor(fi, dtype=torch.float64)).norm(dim=1)[rows].sum() / ref["N"]
    loss.backward()
    assert np.abs(x.grad.numpy() - ref["seed"]).max() <= 1e-12 * max(1.0, np.abs(ref["seed"]).max())
    assert (ref["seed"][3] == 0).all() and ref["d"][3] == 0 and (ref["seed"][mask == 0] == 0).all()
    mean = (torch.tensor(fs, dtype=torch.float64) - torch.tensor(fi, dtype=torch.float64)).norm(dim=1)[keep].mean().item()
    assert abs(ref["out"][1] - mean) <= 1e-12 * mean and abs(ref["out"][0] - 0.005 * mean) <= 1e-12 * mean and ref["out"][2] == ref["N"]
    empty = fr.dist_ref(fs, fi, np.zeros_like(mask), 0.005, 1.0)
    assert empty["out"].tolist() == [0.0, 0.0, 0.0] and not empty["seed"].any()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_the_comparators_reject_planted_errors(bf16):
    C = 128
    fs, fi, mask, ref = _case(M=48, C=C, seed=3)
    t = torch.tensor(ref["seed"], dtype=torch.float32)
    good = (t.bfloat16() if bf16 else t).double().numpy()
    fr.check_seed(good, ref, mask, C, bf16)
    fr.check_d(ref["d"].astype(np.float32), ref, mask, C)
    fr.check_scalars(ref["out"].astype(np.float32), ref, 48, C)
    kept = [m for m in np.nonzero(mask)[0] if ref["d"][m] > 0]
    planted = {"a 1 % scale error": good * 1.01, "rows shifted by one cell": np.roll(good, 1, axis=0)}
    dropped = good.copy()
    dropped[kept[1], 64:128] = 0
    planted["a dropped 64-channel group"] = dropped
    zero = good.copy()
    zero[kept[2]] = 0
    planted["a kept row left at zero"] = zero
    neg = good.copy()
    neg[1] = -0.0
    planted["-0 in a row that is not kept"] = neg
    for what, bad in planted.items():
        with pytest.raises(AssertionError):
            fr.check_seed(bad, ref, mask, C, bf16)
            pytest.fail(f"the comparator accepted {what}")
    with pytest.raises(AssertionError):
        fr.check_d((ref["d"] * 1.001).astype(np.float32), ref, mask, C)
    with pytest.raises(AssertionError):
        fr.check_scalars((ref["out"] * [1.001, 1, 1]).astype(np.float32), ref, 48, C)
    with pytest.raises(AssertionError):
        fr.check_scalars((ref["out"] + [0, 0, 1]).astype(np.float32), ref, 48, C)


# ---- keywords ------------------------------------------------------------------------------------------------------------------------------------
def test_check_feat_dist():
    st = {"conv1.weight": torch.zeros(1)}
    assert fd.check_feat_dist(None, None, None, None, None, False, 19) == (None, None, None)
    assert fd.check_feat_dist(0.005, st, None, None, None, False, 19) == (0.005, fd.DEFAULT_CLASSES, fd.DEFAULT_MIN_RATIO)
    assert fd.check_feat_dist(0, st, [12, 11], 1.0, 0.9, True, 19) == (0.0, (11, 12), 1.0)
    assert fd.DEFAULT_CLASSES == fr.DEFAULT_CLASSES and fd.DEFAULT_LAMBDA == 0.005 and fd.DEFAULT_MIN_RATIO == 0.75
    assert fd.class_word(fd.DEFAULT_CLASSES) == sum(1 << c for c in fr.DEFAULT_CLASSES) and fd.class_word((0, 63)) == 1 | 1 << 63
    for kw in ("feat_dist_state", "feat_dist_classes", "feat_dist_min_ratio"):
        args = dict(feat_dist_state=None, feat_dist_classes=None, feat_dist_min_ratio=None)
        args[kw] = st if kw == "feat_dist_state" else [11] if kw == "feat_dist_classes" else 0.75
        with pytest.raises(ValueError, match=f"^{kw} needs feat_dist"):
            fd.check_feat_dist(None, args["feat_dist_state"], args["feat_dist_classes"], args["feat_dist_min_ratio"], None, False, 19)
    for bad in (-1.0, float("nan"), float("inf"), True, "x"):
        with pytest.raises(ValueError, match="^feat_dist "):
            fd.check_feat_dist(bad, st, None, None, None, False, 19)
    with pytest.raises(ValueError, match="^feat_dist with online_labels needs online_source"):
        fd.check_feat_dist(0.005, st, None, None, 0.9, False, 19)
    with pytest.raises(ValueError, match="^feat_dist_state is required"):
        fd.check_feat_dist(0.005, None, None, None, None, False, 19)
    with pytest.raises(ValueError, match="^feat_dist_classes is required with num_classes = 16"):
        fd.check_feat_dist(0.005, st, None, None, None, False, 16)
    for bad in ([19], [-1], [3, 3], [], [1.5], "ab"):
        with pytest.raises(ValueError, match="^feat_dist_classes "):
            fd.check_feat_dist(0.005, st, bad, None, None, False, 19)
    assert fd.check_feat_dist(0.005, st, [63], None, None, False, 80)[1] == (63,)
    with pytest.raises(ValueError, match="^feat_dist_classes "):
        fd.check_feat_dist(0.005, st, [64], None, None, False, 80)
    for bad in (0.5, 0.0, 1.0001, float("nan"), True, "r"):
        with pytest.raises(ValueError, match="^feat_dist_min_ratio "):
            fd.check_feat_dist(0.005, st, None, bad, None, False, 19)


def test_train_state_fields():
    from simt_amd import train_state as ts
    a = {"feat_dist": 0.005, "feat_dist_classes": [6, 7], "feat_dist_min_ratio": 0.75, "feat_dist_sha256": "ab"}
    assert ts.value_mismatches(a, dict(a, feat_dist_classes=(6, 7)), fields=ts.FEAT_DIST_FIELDS) == []
    assert ts.value_mismatches(a, {}, fields=ts.FEAT_DIST_FIELDS) == list(ts.FEAT_DIST_FIELDS)
    assert ts.value_mismatches(a, dict(a, feat_dist_sha256="cd"), fields=ts.FEAT_DIST_FIELDS) == ["feat_dist_sha256"]
    assert ts.value_mismatches(a, dict(a, feat_dist=0.01), fields=ts.FEAT_DIST_FIELDS) == ["feat_dist"]


# ---- the checkpoint mapping ----------------------------------------------------------------------------------------------------------------------
LAYERS = (1, 1, 1, 1)


def _shapes():
    return ms.state_shapes(19, 0, False, layers=LAYERS)


def _file(shapes):
    return {k: torch.zeros(s, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32) for k, s in shapes.items()}


def test_imagenet_trunk_mapping():
    shapes = _shapes()
    trunk_keys = {k for k in shapes if not k.startswith(("layer5.", "layer6."))}
    assert trunk_keys and len(trunk_keys) < len(shapes)
    # a file in DeeplabMulti's keys: the head keys are dropped
    layout, got = pretrained.imagenet_trunk(_file(shapes), shapes)
    assert layout == "DeeplabMulti" and set(got) == trunk_keys
    # a torchvision file: no heads, fc.* dropped
    tv = {k: v for k, v in _file(shapes).items() if k in trunk_keys}
    tv["fc.weight"], tv["fc.bias"] = torch.zeros(1000, 2048), torch.zeros(1000)
    layout, got = pretrained.imagenet_trunk(tv, shapes)
    assert layout == "torchvision ResNet" and set(got) == trunk_keys and not any(k.startswith("fc.") for k in got)
    # a file without num_batches_tracked is taken
    old = {k: v for k, v in tv.items() if not k.endswith("num_batches_tracked")}
    assert set(pretrained.imagenet_trunk(old, shapes)[1]) == {k for k in trunk_keys if not k.endswith("num_batches_tracked")}
    # a missing and a mis-shaped trunk key are named
    gone = dict(tv)
    del gone["layer3.0.conv2.weight"]
    with pytest.raises(ValueError, match=r"trunk key 'layer3\.0\.conv2\.weight' is missing"):
        pretrained.imagenet_trunk(gone, shapes)
    bent = dict(tv)
    bent["layer4.0.bn3.running_var"] = torch.zeros(7)
    with pytest.raises(ValueError, match=r"trunk key 'layer4\.0\.bn3\.running_var' has shape \(7,\)"):
        pretrained.imagenet_trunk(bent, shapes)


# ---- the tool's flags ----------------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from simt_amd.tools import trainV1_warmup as tool
    return tool.get_arguments(list(argv))


def test_cli_flags():
    a = _parse()
    assert a.feat_dist is None and a.feat_dist_from is None and a.feat_dist_classes is None and a.feat_dist_min_ratio is None
    a = _parse("--feat-dist", "--feat-dist-from", "w.pth")
    assert a.feat_dist == 0.005 and a.feat_dist_from == "w.pth"
    a = _parse("--feat-dist", "0.01", "--feat-dist-from", "w.pth", "--feat-dist-classes", "11", "12", "--feat-dist-min-ratio", "0.9")
    assert (a.feat_dist, a.feat_dist_classes, a.feat_dist_min_ratio) == (0.01, [11, 12], 0.9)
    a = _parse("--feat-dist", "--feat-dist-from", "w.pth", "--online-labels", "--online-source")
    assert a.feat_dist == 0.005 and a.online_source
    from simt_amd.tools import trainV1_warmup as tool
    assert tool.feat_dist_kwargs(_parse(), {}) == {} and tool.feat_dist_text(_parse(), {}) == ""
    assert tool.feat_dist_text(a, {"feat_dist": 0.01234, "feat_dist_cells": 17}) == " fd = 0.0123 (17)"


@pytest.mark.parametrize("argv,msg", [
    (["--feat-dist"], "--feat-dist needs --feat-dist-from"),
    (["--feat-dist", "--feat-dist-from", "w", "--online-labels"], "needs --online-source"),
    (["--feat-dist", "--feat-dist-from", "w", "--model", "DeepLabv3"], "--model DeepLab only"),
    (["--feat-dist", "--feat-dist-from", "w", "--model", "DeepLabVGG"], "--model DeepLab only"),
    (["--feat-dist-from", "w"], "--feat-dist-from needs --feat-dist"),
    (["--feat-dist-classes", "3"], "--feat-dist-classes needs --feat-dist"),
    (["--feat-dist-min-ratio", "0.8"], "--feat-dist-min-ratio needs --feat-dist"),
    (["--feat-dist", "-1", "--feat-dist-from", "w"], "LAMBDA >= 0"),
    (["--feat-dist", "--feat-dist-from", "w", "--feat-dist-min-ratio", "0.5"], "0.5 < R <= 1"),
    (["--feat-dist", "--feat-dist-from", "w", "--feat-dist-classes", "19"], "feat_dist_classes"),
    (["--feat-dist", "--feat-dist-from", "w", "--num-classes", "16"], "feat_dist_classes is required"),
])
def test_cli_refusals(capsys, argv, msg):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_single_trainer_refuses_the_keyword():
    """Refused in front of everything that needs a GPU."""
    from simt_amd.step import Hyper
    from simt_amd.step_single import WarmupSingleTrainer
    with pytest.raises(ValueError, match="^feat_dist: the ImageNet feature distance is built for DeepLab-v2"):
        WarmupSingleTrainer("v3", {}, Hyper(open_classes=0), 2, 65, 65, feat_dist=0.005)
    with pytest.raises(ValueError, match="^feat_dist_state: "):
        WarmupSingleTrainer("vgg", {}, Hyper(open_classes=0), 2, 65, 65, feat_dist_state={})
