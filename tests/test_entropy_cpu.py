"""The entropy term of the target pass without a GPU: the restatement of tests/_entropy_ref.py against closed forms and the
analytic gradient of include/simt_hip.h, the comparator of the GPU tests against five planted mistakes, the references' own exclusion sets,
and the host side -- keyword checks, flag parsing, run identity, train-state fields.

The `oracle` package holds no entropy function; the plain entropy is the reference's EntropyLoss formula, -(softmax * log_softmax).sum(1), as
tests/test_gpu_modules.py restates it, on oracle/simt_oracle.upsample's pixels."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _entropy_ref as er
import _head_bar as hb
from oracle import simt_oracle as so

CD = so.load_class_dist()
F64 = torch.float64
LAMBDA_SEG = 0.1
_IN, _REFS = {}, {}


def _inputs(case):
    if case not in _IN:
        _IN[case] = er.inputs(case, CD)
    return _IN[case]


def _ref(case, setting, dtype, mutant=None, half=False):
    """setting "pure": w = 0, lambda_ent = 1; ("pure", eta);  "sum": the general weights through the map, lambda_ent = 0.005, eta = 2."""
    key = (case, setting, dtype, mutant, half)
    if key not in _REFS:
        B, h, w_, H, W, Q, Cn = er.CASES[case]
        p1, p2, lab, wt, item = _inputs(case)
        if setting == "sum":
            args = (wt, item, LAMBDA_SEG, half, dtype, Cn, 0.005, 2.0)
        else:
            args = (np.zeros(B, np.float32), None, LAMBDA_SEG, half, dtype, Cn, 1.0, setting[1])
        _REFS[key] = er.entropy_ref(p1, p2, lab, *args, mutant=mutant)
    return _REFS[key]


SETTINGS = [("pure", 2.0), ("pure", 0.5), "sum"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [2.0, 0.5, 1.0])
def test_uniform_logits_give_the_closed_form(eta):
    B, Q, h, w, H, W = 2, 7, 3, 4, 9, 11
    p = torch.full((B, Q, h, w), 0.7, dtype=F64)
    lab = torch.zeros(B, H, W, dtype=torch.int64)
    r = er.entropy_ref(p, p, lab, None, None, LAMBDA_SEG, False, F64, Q, 1.0, eta)
    want = (1.0 + 1e-8) ** eta
    assert abs(float(r["ent2"]) - want) <= 1e-12 and abs(float(r["ent1"]) - want) <= 1e-12
    assert abs(float(r["total"]) - (math.log(Q) * (1 + LAMBDA_SEG) + want * (1 + LAMBDA_SEG))) <= 1e-12      # CE of uniform logits is ln Q
    # e = 1 is the maximum of the entropy: the term's gradient is zero up to float64 rounding -- H - u_j is a few 2^-52 per pixel, the chain
    # factor at most 2 eta (1 + eps)^eta / ln Q < 4 and every low-res element gathers H W / (h w) < 9 pixels' worth of weight out of B H W = 198
    only = er.entropy_ref(p, p, lab, np.zeros(B, np.float32), None, LAMBDA_SEG, False, F64, Q, 1.0, eta)
    assert float(only["dpred2"].abs().max()) <= 4 * 9 / 198 * 8 * 2.0 ** -52 and float(only["l2"]) == 0.0


@pytest.mark.parametrize("case", list(er.CASES))
def test_eta_half_is_the_plain_entropy_up_to_sqrt_eps(case):
    """sqrt(e^2 + eps) - e <= sqrt(eps) = 1e-4 at every pixel, so the mean is within 1e-4 ABSOLUTE of mean(H) / ln Q -- and above it."""
    B, h, w_, H, W, Q, Cn = er.CASES[case]
    p1, p2, lab, _wt, _item = _inputs(case)
    r = _ref(case, ("pure", 0.5), F64)
    for p, k in ((p2, "ent2"), (p1, "ent1")):
        up = so.upsample(p.double(), (H, W))
        plain = float((-(F.softmax(up, 1) * F.log_softmax(up, 1)).sum(1)).mean()) / math.log(Q)
        assert 0.0 <= float(r[k]) - plain <= 1e-4, (case, k, float(r[k]), plain)
    # the planted blocks do what they are there for: a saturated region (e * e far below eps) and a uniform one (e = 1)
    up = so.upsample(p2.double(), (H, W))
    e = (-(F.softmax(up, 1) * F.log_softmax(up, 1)).sum(1)) / math.log(Q)
    assert float((e[0] * e[0] < 1e-10).double().mean()) > 0.0 and bool((e[1] > 1 - 1e-12).any())


@pytest.mark.parametrize("half", [False, True], ids=["align", "half"])
@pytest.mark.parametrize("eta", [2.0, 0.5])
@pytest.mark.parametrize("case", list(er.CASES))
def test_autograd_equals_the_analytic_gradient(case, eta, half):
    B, h, w_, H, W, Q, Cn = er.CASES[case]
    p1, p2, lab, _wt, _item = _inputs(case)
    r = _ref(case, ("pure", eta), F64, half=half)
    for p, k, lam in ((p2, "dpred2", 1.0), (p1, "dpred1", LAMBDA_SEG)):
        want = er.analytic_grad(p, (H, W), half, lam, eta)
        scale = float(want.abs().max())
        assert scale > 0 and float((r[k] - want).abs().max()) <= 1e-12 * scale, (case, k, float((r[k] - want).abs().max()), scale)


# ---- the comparator and the references' own noise --------------------------------------------------------------------------------------------------
def _as_launch(r):
    """A restatement's result in the form the comparator takes from a launch: (hout[:16], {name: gradient})."""
    hout = torch.zeros(16)
    hout[0], hout[1], hout[2], hout[3], hout[14], hout[6] = float(r["l1"]), float(r["l2"]), float(r["ent1"]), float(r["ent2"]), float(r["total"]), r["N"]
    return hout, {"dpred1": r["dpred1"].float(), "dpred2": r["dpred2"].float()}


@pytest.mark.parametrize("setting", SETTINGS, ids=str)
@pytest.mark.parametrize("case", list(er.CASES))
def test_comparator_rejects_the_planted_mistakes(case, setting):
    r64, r32 = _ref(case, setting, F64), _ref(case, setting, torch.float32)
    er.compare(f"{case} fp32 restatement", *_as_launch(r32), r64, r32, False)          # the comparator accepts a correct fp32 evaluation
    for m in er.MUTANTS:
        bad = _ref(case, setting, torch.float32, mutant=m)
        with pytest.raises(AssertionError):
            er.compare(f"{case} {m}", *_as_launch(bad), r64, r32, False)


@pytest.mark.parametrize("half", [False, True], ids=["align", "half"])
@pytest.mark.parametrize("setting", SETTINGS, ids=str)
@pytest.mark.parametrize("case", list(er.CASES))
def test_references_leave_no_element_in_the_exclusion_set(case, setting, half):
    """tests/_head_bar.py excuses the elements where the fp32 and the float64 reference disagree (discrete decisions of the SimT loss).  The
    term has no discrete decision: the set must be EMPTY at the three cases, so the cap of 0.1 % is a condition here and no budget."""
    r64, r32 = _ref(case, setting, F64, half=half), _ref(case, setting, torch.float32, half=half)
    for k in ("dpred1", "dpred2"):
        m = hb.measure(r64[k], r32[k])
        print(f"{case} {setting} {k}: tau {m['tau']:.3e}, q99.9 {m['q']:.3e}, excluded {int(m['excl'].sum())} of {m['excl'].numel()}")
        assert int(m["excl"].sum()) == 0, (case, setting, k, int(m["excl"].sum()))
        assert bool(torch.isfinite(r32[k]).all()) and bool(torch.isfinite(r64[k]).all())


# ---- the host side ---------------------------------------------------------------------------------------------------------------------------------------
def test_check_entropy():
    from simt_amd.online_labels import DEFAULT_ENTROPY_ETA, DEFAULT_ENTROPY_LAMBDA, check_entropy
    assert (DEFAULT_ENTROPY_LAMBDA, DEFAULT_ENTROPY_ETA) == (0.005, 2.0)
    assert check_entropy(None, None, None, None) == (None, 2.0, 0) and check_entropy(None, 2.0, 0, 0.9) == (None, 2.0, 0)
    assert check_entropy(0.005, 2.0, 0, 0.0) == (0.005, 2.0, 0) and check_entropy(1, 0.5, np.int64(7), 0.9) == (1.0, 0.5, 7)
    for args, named in [((0.005, 2.0, 0, None), "entropy_min needs online_labels"), ((0, 2.0, 0, 0.9), "entropy_min 0"),
                        ((-0.1, 2.0, 0, 0.9), "entropy_min -0.1"), ((float("nan"), 2.0, 0, 0.9), "entropy_min nan"),
                        ((float("inf"), 2.0, 0, 0.9), "entropy_min inf"), ((True, 2.0, 0, 0.9), "entropy_min True"),
                        (("much", 2.0, 0, 0.9), "entropy_min 'much'"), ((0.005, 0.0, 0, 0.9), "entropy_eta 0.0"),
                        ((0.005, -2.0, 0, 0.9), "entropy_eta -2.0"), ((0.005, float("nan"), 0, 0.9), "entropy_eta nan"),
                        ((0.005, float("inf"), 0, 0.9), "entropy_eta inf"), ((0.005, True, 0, 0.9), "entropy_eta True"),
                        ((0.005, 2.0, -1, 0.9), "entropy_after -1"), ((0.005, 2.0, 1.5, 0.9), "entropy_after 1.5"),
                        ((0.005, 2.0, True, 0.9), "entropy_after True"), ((None, 0.5, 0, 0.9), "entropy_eta needs entropy_min"),
                        ((None, 2.0, 3, 0.9), "entropy_after needs entropy_min")]:
        with pytest.raises(ValueError, match=named):
            check_entropy(*args)


def test_flags_defaults_refusals_and_run_identity(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools.trainV2_simt import RUN_DEFAULTS, run_identity
    base = ["--synthetic", "--online-labels", "0.9"]
    off = tool.get_arguments(base)
    assert (off.entropy_min, off.entropy_eta, off.entropy_after) == (None, 2.0, 0) and tool.entropy_kwargs(off) == {}
    ident = run_identity(off, CD.numpy())
    assert "entropy_min" not in ident and RUN_DEFAULTS["entropy_min"] is False
    assert ident == run_identity(tool.get_arguments(base), CD.numpy())
    tool.entropy_line(off)
    assert capsys.readouterr().out == ""
    bare = tool.get_arguments(base + ["--entropy-min"])
    assert tool.entropy_kwargs(bare) == {"entropy_min": 0.005, "entropy_eta": 2.0, "entropy_after": 0}
    assert run_identity(bare, CD.numpy())["entropy_min"] == [0.005, 2.0, 0]
    full = tool.get_arguments(base + ["--model", "DeepLabVGG", "--entropy-min", "0.01", "--entropy-eta", "0.5", "--entropy-after", "7"])
    assert tool.entropy_kwargs(full) == {"entropy_min": 0.01, "entropy_eta": 0.5, "entropy_after": 7}
    assert run_identity(full, CD.numpy())["entropy_min"] == [0.01, 0.5, 7]
    tool.entropy_line(full)
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and "lambda 0.01" in line and "^0.5" in line and "from iteration 7 on" in line and "EVERY pixel" in line
    assert tool.entropy_text({"entropy2": 0.25}) == " ent = 0.250" and tool.entropy_text({"loss_seg": 1.0}) == ""
    for bad, named in [(["--synthetic", "--entropy-min"], "--entropy-min needs --online-labels"),
                       (base + ["--entropy-min", "0"], "--entropy-min 0.0"), (base + ["--entropy-min", "nan"], "--entropy-min nan"),
                       (base + ["--entropy-min", "-1"], "--entropy-min -1.0"), (base + ["--entropy-min", "--entropy-eta", "0"], "--entropy-eta 0.0"),
                       (base + ["--entropy-min", "--entropy-eta", "inf"], "--entropy-eta inf"),
                       (base + ["--entropy-min", "--entropy-after", "-1"], "--entropy-after -1"),
                       (base + ["--entropy-eta", "0.5"], "--entropy-eta needs --entropy-min"),
                       (base + ["--entropy-after", "3"], "--entropy-after needs --entropy-min")]:
        with pytest.raises(SystemExit) as e:
            tool.get_arguments(bad)
        assert e.value.code == 2 and named in capsys.readouterr().err, (bad, named)


def test_train_state_fields():
    from simt_amd import train_state as tsf
    assert tsf.ENTROPY_FIELDS == ("entropy_min", "entropy_eta", "entropy_after")
    on = {"entropy_min": 0.005, "entropy_eta": 2.0, "entropy_after": 4}
    assert tsf.value_mismatches({}, {}, fields=tsf.ENTROPY_FIELDS) == [] and tsf.value_mismatches(on, dict(on), fields=tsf.ENTROPY_FIELDS) == []
    assert tsf.value_mismatches({}, on, fields=tsf.ENTROPY_FIELDS) == list(tsf.ENTROPY_FIELDS)          # added
    assert tsf.value_mismatches(on, {}, fields=tsf.ENTROPY_FIELDS) == list(tsf.ENTROPY_FIELDS)          # dropped
    assert tsf.value_mismatches(on, dict(on, entropy_after=5), fields=tsf.ENTROPY_FIELDS) == ["entropy_after"]
    assert tsf.value_mismatches(on, dict(on, entropy_min=0.01), fields=tsf.ENTROPY_FIELDS) == ["entropy_min"]


def test_bindings_declare_the_entry_points():
    from simt_amd import _lib as L
    for name in ("simt_head_loss_entropy", "simt_head_grad_entropy"):
        res, args = L.SIGNATURES[name]
        assert len(args) == 6 and args[4]._type_ is L.HeadEntropy
    assert [f for f, _t in L.HeadEntropy._fields_] == ["lambda_ent", "eta"] and L.C.sizeof(L.HeadEntropy) == 8
    header = open(L.os.path.join(L.os.path.dirname(L.os.path.dirname(L.os.path.abspath(L.__file__))), "include", "simt_hip.h")).read()
    assert "typedef struct { float lambda_ent, eta; } simt_head_entropy;" in header
