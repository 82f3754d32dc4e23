"""The uncertainty rectification without a GPU: the restatement of tests/_uncertain_ref.py against the analytic gradient of
include/simt_hip.h and closed forms, the comparator of the GPU tests against six planted mistakes, the references' own exclusion sets, and the
host side -- keyword checks, flag parsing, the trainers' refusals, train-state fields."""
import numpy as np
import pytest
import torch

import _head_bar as hb
import _uncertain_ref as ur
from oracle import simt_oracle as so

CD = so.load_class_dist()
F64 = torch.float64
LAMBDA_SEG = 0.1
_IN, _REFS = {}, {}


def _inputs(case):
    if case not in _IN:
        _IN[case] = ur.inputs(case, CD)
    return _IN[case]


def _args(case, setting):
    """"kl": w = 0, lambda_kl = 1;  "ce": the general weights through the map, lambda_kl = 0;  "sum": those weights, lambda_kl = 1;  "null": no table."""
    B = ur.CASES[case][0]
    _p1, _p2, _lab, wt, item = _inputs(case)
    return {"kl": (np.zeros(B, np.float32), None, 1.0), "ce": (wt, item, 0.0), "sum": (wt, item, 1.0), "null": (None, None, 1.0)}[setting]


def _ref(c, setting, dtype, mutant=None):
    key = (c, setting, dtype, mutant)
    if key not in _REFS:
        case, half = c
        Cn = ur.CASES[case][6]
        p1, p2, lab, _wt, _item = _inputs(case)
        w, m, lam = _args(case, setting)
        _REFS[key] = ur.uncertain_ref(p1, p2, lab, w, m, LAMBDA_SEG, half, dtype, Cn, lam, mutant=mutant)
    return _REFS[key]


SETTINGS = ["kl", "ce", "sum", "null"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("c", ur.HEADS, ids=ur.HID)
def test_autograd_equals_the_analytic_gradient(c, setting):
    case, half = c
    Cn = ur.CASES[case][6]
    p1, p2, lab, _wt, _item = _inputs(case)
    w, m, lam = _args(case, setting)
    r = _ref(c, setting, F64)
    want = ur.analytic_grad(p1, p2, lab, w, m, LAMBDA_SEG, half, Cn, lam)
    for k, g in (("dpred1", want[0]), ("dpred2", want[1])):
        scale = float(g.abs().max())
        assert scale > 0 and float((r[k] - g).abs().max()) <= 1e-12 * scale, (c, setting, k, float((r[k] - g).abs().max()), scale)


def test_identical_heads_give_the_plain_cross_entropy():
    """D = 0 exactly, every weight 1, K = 0: R_k is tests/_head_bar.py's warm-up loss, and so is the gradient (c_k's two terms cancel in the sum
    over the heads only where lambda_seg = 1; here each is checked through the total)."""
    case, half = "straddle", False
    Cn = ur.CASES[case][6]
    _p1, p2, lab, _wt, _item = _inputs(case)
    r = ur.uncertain_ref(p2.clone(), p2, lab, None, None, LAMBDA_SEG, half, F64, Cn, 1.0)
    base = hb.warmup_ref(p2.clone(), p2, lab, LAMBDA_SEG, half, F64)
    assert float(r["k1"]) == 0.0 and float(r["k2"]) == 0.0 and float(r["m1"]) == 1.0 and float(r["m2"]) == 1.0
    assert abs(float(r["r1"]) - float(base["l1"])) <= 1e-12 and abs(float(r["r2"]) - float(base["l2"])) <= 1e-12
    assert abs(float(r["total"]) - float(base["total"])) <= 1e-12


def test_the_saturated_block_underflows_the_weight():
    """The inputs do what the GPU tests' `finite` property needs: somewhere D is far above 104 (exp(-D) = 0 in fp32) and every word stays finite."""
    c = ("straddle", False)
    case, half = c
    B, h, w_, H, W, Q, Cn = ur.CASES[case]
    p1, p2, _lab, _wt, _item = _inputs(case)
    ls1, ls2 = (torch.log_softmax(so.upsample(p.double(), (H, W)), 1) for p in (p1, p2))
    D2 = (ls1.exp() * (ls1 - ls2)).sum(1)
    assert float(D2.max()) > 200.0 and float(D2.min()) > -1e-12
    r32 = _ref(c, "sum", torch.float32)
    assert all(bool(torch.isfinite(r32[k]).all()) for k in ("dpred1", "dpred2", "total"))


# ---- the comparator and the references' own noise --------------------------------------------------------------------------------------------------
def _as_launch(r):
    hout, grads = ur.as_launch(r)
    return hout.float(), {k: v.float() for k, v in grads.items()}


@pytest.mark.parametrize("c", ur.HEADS, ids=ur.HID)
def test_comparator_rejects_the_planted_mistakes(c):
    r64, r32 = _ref(c, "sum", F64), _ref(c, "sum", torch.float32)
    ur.compare(f"{ur.HID(c)} fp32 restatement", *_as_launch(r32), r64, r32)          # the comparator accepts a correct fp32 evaluation
    for m in ur.MUTANTS:
        bad = _ref(c, "sum", torch.float32, mutant=m)
        with pytest.raises(AssertionError):
            ur.compare(f"{ur.HID(c)} {m}", *_as_launch(bad), r64, r32)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("c", ur.HEADS, ids=ur.HID)
def test_references_leave_no_element_in_the_exclusion_set(c, setting):
    """tests/_head_bar.py excuses the elements where the fp32 and the float64 reference disagree (discrete decisions of the SimT loss).  This
    loss has no discrete decision: the set must be EMPTY, so the cap of 0.1 % is a condition here and no budget."""
    r64, r32 = _ref(c, setting, F64), _ref(c, setting, torch.float32)
    for k in ("dpred1", "dpred2"):
        m = hb.measure(r64[k], r32[k])
        print(f"{ur.HID(c)} {setting} {k}: tau {m['tau']:.3e}, q99.9 {m['q']:.3e}, excluded {int(m['excl'].sum())} of {m['excl'].numel()}")
        assert int(m["excl"].sum()) == 0, (c, setting, k, int(m["excl"].sum()))
        assert bool(torch.isfinite(r32[k]).all()) and bool(torch.isfinite(r64[k]).all())
    for k in ("r1", "r2", "k1", "k2", "m1", "m2", "total"):
        assert abs(float(r32[k]) - float(r64[k])) <= 1e-5 * (1 + abs(float(r64[k]))), (c, setting, k)


# ---- the host side ---------------------------------------------------------------------------------------------------------------------------------------
def test_check_uncertainty():
    from simt_amd.online_labels import check_uncertainty
    assert check_uncertainty(None, None) is None and check_uncertainty(None, 0.005) is None
    assert check_uncertainty(1, None) == 1.0 and check_uncertainty(0, None) == 0.0 and check_uncertainty(np.float32(0.5), None) == 0.5
    for args, named in [((-0.1, None), "uncertainty_rectify -0.1"), ((float("nan"), None), "uncertainty_rectify nan"),
                        ((float("inf"), None), "uncertainty_rectify inf"), ((True, None), "uncertainty_rectify True"),
                        (("much", None), "uncertainty_rectify 'much'"), ((1.0, 0.005), "uncertainty_rectify beside entropy_min")]:
        with pytest.raises(ValueError, match=named):
            check_uncertainty(*args)


def test_flag_defaults_lines_and_refusals(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools.trainV2_simt import RUN_DEFAULTS, run_identity
    off = tool.get_arguments(["--synthetic"])
    assert off.uncertainty_rectify is None and tool.uncertainty_kwargs(off) == {}
    assert "uncertainty_rectify" not in run_identity(off, CD.numpy()) and RUN_DEFAULTS["uncertainty_rectify"] is False
    assert run_identity(tool.get_arguments(["--synthetic", "--uncertainty-rectify", "0"]), CD.numpy())["uncertainty_rectify"] == [0.0]
    assert run_identity(tool.get_arguments(["--synthetic", "--online-labels", "0.9", "--uncertainty-rectify"]), CD.numpy())["uncertainty_rectify"] == [1.0]
    tool.uncertainty_line(off)
    assert capsys.readouterr().out == ""
    bare = tool.get_arguments(["--synthetic", "--uncertainty-rectify"])
    assert tool.uncertainty_kwargs(bare) == {"uncertainty_rectify": 1.0}
    full = tool.get_arguments(["--synthetic", "--online-labels", "0.9", "--online-source", "--uncertainty-rectify", "0.25"])
    assert tool.uncertainty_kwargs(full) == {"uncertainty_rectify": 0.25}
    assert tool.uncertainty_kwargs(tool.get_arguments(["--synthetic", "--uncertainty-rectify", "0"])) == {"uncertainty_rectify": 0.0}
    tool.uncertainty_line(full)
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and "0.25 * mean KL" in line and "the target pass" in line and "no class weights" in line
    assert "division by the labelled pixels" in line and "--lambda-seg" in line
    tool.uncertainty_line(bare)
    assert "every pass" in capsys.readouterr().out
    assert tool.uncertainty_text({"uncertainty2": 0.25, "rectify2": 0.5}) == " unc = 0.250 x0.500" and tool.uncertainty_text({"loss_seg1": 1.0}) == ""
    base = ["--synthetic", "--online-labels", "0.9"]
    for bad, named in [(["--synthetic", "--uncertainty-rectify", "-1"], "--uncertainty-rectify -1.0"),
                       (["--synthetic", "--uncertainty-rectify", "nan"], "--uncertainty-rectify nan"),
                       (["--synthetic", "--uncertainty-rectify", "inf"], "--uncertainty-rectify inf"),
                       (["--synthetic", "--model", "DeepLabv3", "--uncertainty-rectify"], "--uncertainty-rectify needs --model DeepLab"),
                       (["--synthetic", "--model", "DeepLabVGG", "--uncertainty-rectify"], "--uncertainty-rectify needs --model DeepLab"),
                       (base + ["--entropy-min", "--uncertainty-rectify"], "--uncertainty-rectify beside --entropy-min")]:
        with pytest.raises(SystemExit) as e:
            tool.get_arguments(bad)
        assert e.value.code == 2 and named in capsys.readouterr().err, (bad, named)


def test_trainers_refuse_what_is_not_built():
    """WarmupSingleTrainer: one head (refused before anything is built); WarmupTrainer: beside entropy_min (check_uncertainty, the first thing
    its constructor does with the keyword)."""
    from simt_amd.step_single import WarmupSingleTrainer
    for model in ("v3", "vgg"):
        with pytest.raises(ValueError, match="uncertainty_rectify: .*one head"):
            WarmupSingleTrainer(model, {}, None, 2, 65, 65, uncertainty_rectify=1.0)
    import inspect
    from simt_amd.step import WarmupTrainer
    assert inspect.signature(WarmupTrainer.__init__).parameters["uncertainty_rectify"].default is None
    assert inspect.signature(WarmupSingleTrainer.__init__).parameters["uncertainty_rectify"].default is None


def test_train_state_fields():
    from simt_amd import train_state as tsf
    F = tsf.UNCERTAINTY_FIELDS
    assert F == ("uncertainty_rectify",)
    on = {"uncertainty_rectify": 1.0}
    assert tsf.value_mismatches({}, {}, fields=F) == [] and tsf.value_mismatches(on, dict(on), fields=F) == []
    assert tsf.value_mismatches({}, on, fields=F) == list(F)          # added
    assert tsf.value_mismatches(on, {}, fields=F) == list(F)          # dropped
    assert tsf.value_mismatches(on, {"uncertainty_rectify": 0.5}, fields=F) == list(F)
    assert tsf.value_mismatches({"uncertainty_rectify": 0.0}, {}, fields=F) == list(F)          # lambda_kl = 0 is ON: the rectified cross-entropy

    class _Plan:
        layers = (3, 4, 23, 3)

    class _T(tsf.TrainStateMixin):          # the hyper dict of a trainer with the keyword, and without it
        def __init__(self, lam):
            self.hp, self.B, self.H, self.W, self.dtype, self.plan = so.Hyper(), 2, 65, 65, torch.float32, _Plan()
            self.uncertainty_rectify = lam
    assert _T(0.5)._hyper_state()["uncertainty_rectify"] == 0.5 and _T(0.0)._hyper_state()["uncertainty_rectify"] == 0.0
    assert "uncertainty_rectify" not in _T(None)._hyper_state()


def test_bindings_declare_the_entry_points():
    from simt_amd import _lib as L
    for name in ("simt_head_loss_uncertain", "simt_head_grad_uncertain"):
        res, args = L.SIGNATURES[name]
        assert len(args) == 6 and args[4]._type_ is L.HeadUncertainty
    assert [f for f, _t in L.HeadUncertainty._fields_] == ["lambda_kl"] and L.C.sizeof(L.HeadUncertainty) == 4
    header = open(L.os.path.join(L.os.path.dirname(L.os.path.dirname(L.os.path.abspath(L.__file__))), "include", "simt_hip.h")).read()
    assert "typedef struct { float lambda_kl; } simt_head_uncertainty;" in header
