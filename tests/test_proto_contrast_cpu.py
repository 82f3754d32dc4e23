"""The prototype contrastive term without a GPU: the restatement of tests/_proto_contrast_ref.py against torch autograd, its float32
form against its float64 form, the cell labels against 7.22's mask, the comparator of the GPU tests against planted mistakes, the keyword
refusals of simt_amd/proto_contrast.py and the tool's flags."""
import math

import numpy as np
import pytest
import torch

import _feat_dist_ref as fr
import _proto_contrast_ref as pr
from simt_amd import proto_contrast as PC

SMALL = ["f32_9_8_2", "f32_162_64_64", "bf16_363_128_19", "f32_33_64_19", "f32_40_24_19"]


@pytest.mark.parametrize("name", SMALL + ["f32_243_1024_19"])
def test_restatement_equals_autograd(name):
    k = pr.case(name)
    r = pr.refs(k)
    seen, valid, N = r["seen"], r["valid"], r["N"]
    assert N > 0 and seen.sum() >= 2
    f = torch.tensor(k["F"], dtype=torch.float64, requires_grad=True)
    eta = torch.tensor(np.nan_to_num(k["eta"]), dtype=torch.float64)[torch.from_numpy(seen)]
    rows = torch.from_numpy(np.nonzero(valid)[0])
    y = torch.from_numpy(np.searchsorted(np.nonzero(seen)[0], k["lab"][valid].astype(np.int64)))
    F_ = torch.nn.functional
    logits = F_.normalize(f[rows], dim=1, eps=0.0) @ F_.normalize(eta, dim=1, eps=0.0).T / k["temp"]
    lam_g = float(np.float32(k["lam"] * k["gscale"]))
    per = F_.cross_entropy(logits, y, reduction="none")
    (lam_g * per.sum() / N).backward()
    g = f.grad.numpy()
    assert np.abs(r["d"][valid] - per.detach().numpy()).max() <= 1e-12 * np.abs(per.detach().numpy()).max()
    assert np.abs(r["seed"] - g).max() <= 1e-12 * np.abs(g).max() and not r["seed"][~valid].any() and not r["d"][~valid].any()
    S = float(per.detach().sum())
    assert np.allclose(r["out"], [k["lam"] * S / N, S / N, N], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", SMALL)
def test_float32_restatement_stays_within_its_derived_bound(name):
    """The float32 form rounds every operation: the dot products and norms carry at most D * 2^-24 relative each (sequential sums of D terms), the
    logits inherit 3 D * 2^-24 * |s| + a few units, exp / log / the softmax a few more: (3 D + 16) * 2^-24 * max(|s|, 1) absolute on the loss, and the
    seed -- a sum of C products of such terms -- (3 D + C + 16) * 2^-24 * max(|s|, 1) relative to its largest element."""
    k = pr.case(name)
    r64, r32 = pr.refs(k), pr.refs(k, dt=np.float32)
    assert r32["d"].dtype == np.float32 and r32["seed"].dtype == np.float32 and r32["N"] == r64["N"]
    smax = max(1.0, 1.0 / k["temp"])
    eps = 2.0 ** -24
    assert np.abs(r32["d"] - r64["d"]).max() <= (3 * k["D"] + 16) * eps * smax
    assert np.abs(r32["seed"] - r64["seed"]).max() <= (3 * k["D"] + k["C"] + 16) * eps * smax * np.abs(r64["seed"]).max()
    assert np.abs(r32["out"][:2] - r64["out"][:2]).max() <= (3 * k["D"] + 16 + k["M"]) * eps * smax * max(1.0, abs(r64["out"][1]))
    assert np.abs(r32["d"] - r64["d"]).max() > 0, "the float32 restatement is the float64 one"


def test_too_few_seen_classes_and_empty_selections_are_zero():
    k = dict(pr.case("f32_33_64_19"))
    one = np.zeros_like(k["n"])
    one[3] = 4
    for kw in (dict(n=np.zeros_like(k["n"])), dict(n=one), dict(lab=np.full_like(k["lab"], 255))):
        r = pr.refs(dict(k, **kw))
        assert r["N"] == 0 and not r["d"].any() and not r["seed"].any() and not r["out"].any()


@pytest.mark.parametrize("geo", [(1, 7, 5, 7, 5), (2, 65, 129, 9, 17), (1, 33, 33, 5, 5), (3, 16, 16, 1, 1)], ids=str)
@pytest.mark.parametrize("ratio", [0.75, 1.0, 0.51])
def test_cell_labels_restricted_to_a_class_set_are_the_mask_of_feat_dist(geo, ratio):
    B, H, W, h, w = geo
    g = np.random.default_rng(H + w)
    values = np.array([0, 0, 6, 6, 13, 18, 1, 255, 19, 64, -1], dtype=np.int64)
    lab = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        for (r0, r1) in fr.windows(H, h):
            for (c0, c1) in fr.windows(W, w):
                lab[b, r0:r1, c0:c1] = values[g.integers(0, len(values))]
    noise = g.random((B, H, W)) < 0.2
    lab[noise] = values[g.integers(0, len(values), int(noise.sum()))]
    for Cn, classes in ((19, fr.DEFAULT_CLASSES), (19, (0, 6)), (64, (0, 13, 63)), (2, (0,))):
        cells, count = pr.cell_labels_ref(lab, h, w, Cn, ratio)
        mask, N = fr.mask_ref(lab, h, w, classes, ratio)
        assert np.array_equal(((cells < Cn) & np.isin(cells, classes)).astype(np.uint8), mask)
        assert count == int((cells < Cn).sum()) and ((cells < Cn) | (cells == 255)).all()
        n = np.zeros(Cn, dtype=np.int32)
        n[list(classes)] = 2
        assert pr.cell_labels_ref(lab, h, w, Cn, ratio, n)[1] == N


@pytest.mark.parametrize("name", ["f32_162_64_64", "bf16_363_128_19"])
def test_comparator_passes_the_restatement_and_rejects_planted_mistakes(name):
    k = pr.case(name)
    r64, r32 = pr.refs(k), pr.refs(k, dt=np.float32)
    pr.check_contrast(pr.as_got(r32, k), k, r64=r64, r32=r32)
    for m in pr.MISTAKES:
        wrong = pr.refs(k, mistake=m, dt=np.float32)
        with pytest.raises(AssertionError):
            pr.check_contrast(pr.as_got(wrong, k), k, r64=r64, r32=r32)
    wrong = pr.as_got(r32, k)
    wrong["out"] = wrong["out"].copy()
    wrong["out"][2] += 1
    with pytest.raises(AssertionError, match="N:"):
        pr.check_contrast(wrong, k, r64=r64, r32=r32)


def test_keyword_refusals():
    ok = dict(proto_contrast=0.1, proto_contrast_temp=None, proto_contrast_min_ratio=None, proto_denoise=1.0, feat_dist=None, num_classes=19)

    def check(**kw):
        return PC.check_proto_contrast(**dict(ok, **kw))
    assert check() == (0.1, PC.DEFAULT_TEMP, 0.75) and check(proto_contrast=0) == (0.0, 0.1, 0.75)
    assert check(proto_contrast_temp=0.07, proto_contrast_min_ratio=1.0) == (0.1, 0.07, 1.0)
    assert check(proto_contrast=None, proto_denoise=None) == (None, None, None)
    for kw, named in [(dict(proto_contrast=-0.1), "proto_contrast -0.1"), (dict(proto_contrast=math.nan), "proto_contrast nan"),
                      (dict(proto_contrast=math.inf), "proto_contrast inf"), (dict(proto_contrast=True), "proto_contrast True"),
                      (dict(proto_contrast="x"), "proto_contrast 'x'"), (dict(proto_denoise=None), "proto_contrast needs proto_denoise"),
                      (dict(feat_dist=0.005), "proto_contrast with feat_dist"), (dict(num_classes=65), "proto_contrast with num_classes = 65"),
                      (dict(proto_contrast_temp=0.0), "proto_contrast_temp 0.0"), (dict(proto_contrast_temp=math.nan), "proto_contrast_temp nan"),
                      (dict(proto_contrast_temp=math.inf), "proto_contrast_temp inf"), (dict(proto_contrast_temp=False), "proto_contrast_temp False"),
                      (dict(proto_contrast_min_ratio=0.5), "proto_contrast_min_ratio 0.5"), (dict(proto_contrast_min_ratio=1.01), "proto_contrast_min_ratio 1.01"),
                      (dict(proto_contrast_min_ratio=math.nan), "proto_contrast_min_ratio nan"), (dict(proto_contrast_min_ratio="r"), "proto_contrast_min_ratio 'r'"),
                      (dict(proto_contrast=None, proto_contrast_temp=0.1), "proto_contrast_temp needs proto_contrast"),
                      (dict(proto_contrast=None, proto_contrast_min_ratio=0.8), "proto_contrast_min_ratio needs proto_contrast")]:
        with pytest.raises(ValueError) as e:
            check(**kw)
        assert str(e.value).startswith(named), (kw, str(e.value))


def _parse(argv, capsys=None):
    from simt_amd.tools import trainV1_warmup as tool
    return tool.get_arguments(argv)


def test_tool_flags(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    base = ["--online-labels", "0.3", "--proto-denoise"]
    a = _parse(base)
    assert a.proto_contrast is None and tool.proto_contrast_kwargs(a) == {} and tool.proto_contrast_text(a, {}) == ""
    a = _parse(base + ["--proto-contrast"])
    assert tool.proto_contrast_kwargs(a) == dict(proto_contrast=0.1, proto_contrast_temp=0.1, proto_contrast_min_ratio=0.75)
    a = _parse(base + ["--proto-contrast", "0.5", "--proto-contrast-temp", "0.07", "--proto-contrast-min-ratio", "0.9"])
    assert tool.proto_contrast_kwargs(a) == dict(proto_contrast=0.5, proto_contrast_temp=0.07, proto_contrast_min_ratio=0.9)
    assert tool.proto_contrast_text(a, {"proto_contrast": 0.25, "proto_contrast_cells": 7}) == " pc = 0.2500 (7)"
    for argv, named in [(["--proto-contrast"], "--proto-contrast needs --proto-denoise"),
                        (base + ["--proto-contrast-temp", "0.1"], "--proto-contrast-temp needs --proto-contrast"),
                        (base + ["--proto-contrast-min-ratio", "0.8"], "--proto-contrast-min-ratio needs --proto-contrast"),
                        (base + ["--proto-contrast", "-1"], "--proto-contrast -1"),
                        (base + ["--proto-contrast", "--proto-contrast-temp", "0"], "--proto-contrast-temp 0"),
                        (base + ["--proto-contrast", "--proto-contrast-min-ratio", "0.5"], "--proto-contrast-min-ratio 0.5"),
                        (base + ["--proto-contrast", "--model", "DeepLabv3"], "--proto-contrast"),
                        (base + ["--proto-contrast", "--model", "DeepLabVGG"], "--proto-contrast")]:
        with pytest.raises(SystemExit) as e:
            _parse(argv)
        assert e.value.code == 2
        assert named in capsys.readouterr().err, (argv, named)
