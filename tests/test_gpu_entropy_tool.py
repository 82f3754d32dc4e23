"""trainV1_warmup --entropy-min on the GPU, on synthetic data, for all three models: the ` ent = ` field appears exactly from
iteration --entropy-after on; with the switch beyond --num-steps-stop the loss lines and the final snapshot are the flag-off run's, byte for
byte; with the term on the final weights differ; 2 + 2 == 4 through --train-state; a resume with the flag changed or dropped is refused."""
import os
import re

import pytest
import torch

import test_gpu_resume as R
from test_gpu_fda_tool import _differ

pytestmark = pytest.mark.gpu
MODELS = ["DeepLab", "DeepLabv3", "DeepLabVGG"]
H, W, B = 65, 129, 2          # the smallest sizes of the --online-source tool tests
# A from-scratch DeepLabVGG predicts almost uniformly (tests/test_gpu_fda_tool.py): the entropy is at its maximum there and the term's gradient is
# first order in the logits' spread, far below a bf16 ulp of the cross-entropy's at FDA's 0.005.  The runs that must MOVE the weights take a
# lambda at which they do for all three models.
LAM = "20"


def _common(model):
    return ["--learning-rate", "2.5e-4", "--model", model, "--input-size-target", f"{W},{H}", "--batch-size", str(B), "--num-steps", "50",
            "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--synthetic", "--online-labels", "0.05",
            "--online-labels-weighted", "--online-source", "--online-mix"]


@pytest.mark.parametrize("model", MODELS)
def test_tool_switches_the_term_on_and_resumes(dev, tmp_path, capsys, model):
    from simt_amd.tools import trainV1_warmup as tool
    common = _common(model)

    def run(tag, stop, *more):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, f"GTA5_{stop}.pth")

    out_o, snap_o = run("o", 4)                                                        # flag off
    off = R._loss_lines(out_o)
    assert len(off) == 4 and "entropy term" not in out_o and not any(" ent = " in ln for ln in off), out_o
    out_b, snap_b = run("b", 4, "--entropy-min", LAM, "--entropy-after", "9")        # the switch beyond the run
    assert out_b.count("entropy term: lambda 20.0 * mean of (e^2 + 1e-8)^2.0") == 1 and "from iteration 9 on" in out_b
    assert R._loss_lines(out_b) == off, (out_b, out_o)
    assert open(snap_b, "rb").read() == open(snap_o, "rb").read(), "the final snapshot differs from the flag-off run's"
    out_a, snap_a = run("a", 4, "--entropy-min", LAM, "--entropy-after", "2")        # on from iteration 2
    on = R._loss_lines(out_a)
    assert len(on) == 4 and not re.search(r"= (nan|inf)", out_a), out_a
    assert [" ent = " in ln for ln in on] == [False, False, True, True], out_a
    assert on[:2] == off[:2], (out_a, out_o)
    ents = [float(re.search(r" ent = (\d\.\d{3})\b", ln).group(1)) for ln in on[2:]]
    assert all(0.0 < e <= 1.001 for e in ents), out_a          # (a from-scratch DeepLabVGG predicts uniformly: e = 1, the penalty's maximum)
    assert _differ(snap_a, snap_o), "the term changed no weight"
    out_d, _ = run("d", 3, "--entropy-min")                                            # the bare flag: FDA's 0.005, every iteration
    assert "entropy term: lambda 0.005 * mean of (e^2 + 1e-8)^2.0" in out_d and "from every iteration" in out_d
    assert all(" ent = " in ln for ln in R._loss_lines(out_d))
    # 2 + 2 == 4 through --train-state, the switch at the resume
    state = str(tmp_path / "run.state")
    flags = ["--entropy-min", LAM, "--entropy-after", "2"]
    out_r1, _ = run("r", 2, *flags, "--train-state", state)
    assert R._loss_lines(out_r1) == on[:2]
    out_r2, snap_r = run("r", 4, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_r2), out_r2
    assert R._loss_lines(out_r2) == on[2:], (out_a, out_r2)
    R._same_snapshot(snap_a, snap_r)
    for other, named in ((["--entropy-min", "10", "--entropy-after", "2"], r"differs in: entropy_min \(state: \[20\.0, 2\.0, 2\], this run: \[10\.0, 2\.0, 2\]\)"),
                         ([], r"differs in: entropy_min \(state: \[20\.0, 2\.0, 2\], this run: False\)")):
        with pytest.raises(SystemExit, match=named):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "r"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
    torch.cuda.synchronize()
