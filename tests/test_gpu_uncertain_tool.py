"""trainV1_warmup --uncertainty-rectify on the GPU, on synthetic data: every loss line carries ` unc = `; the lines and the final
weights equal a hand-driven WarmupTrainer with the keyword; the final weights differ from the flag-off run's; 2 + 2 == 4 through --train-state;
a resume with the flag changed or dropped is refused."""
import os
import re

import pytest
import torch

import test_gpu_resume as R
from test_gpu_fda_tool import _differ

pytestmark = pytest.mark.gpu
H, W, B = 65, 129, 2          # the sizes of the entropy tool test


def _common():
    return ["--learning-rate", "2.5e-4", "--model", "DeepLab", "--input-size-target", f"{W},{H}", "--batch-size", str(B), "--num-steps", "50",
            "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--synthetic"]


def test_tool_rectifies_and_resumes(dev, tmp_path, capsys, monkeypatch):
    from simt_amd.tools import trainV1_warmup as tool
    common = _common()

    def run(tag, stop, *more):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, f"GTA5_{stop}.pth")

    out_o, snap_o = run("o", 4)                                                        # flag off
    off = R._loss_lines(out_o)
    assert len(off) == 4 and "uncertainty rectification" not in out_o and not any(" unc = " in ln for ln in off), out_o
    # the flag on; the trainer the tool builds is kept, with every step's arguments, and driven again by hand below
    built = []
    real = tool.WarmupTrainer

    class Kept(real):
        def __init__(self, *a, **kw):
            built.append((a, kw, []))
            super().__init__(*a, **kw)

        def step(self, *a, **kw):
            built[-1][2].append(([x.clone() if torch.is_tensor(x) else x for x in a], dict(kw)))
            return super().step(*a, **kw)
    monkeypatch.setattr(tool, "WarmupTrainer", Kept)
    out_a, snap_a = run("a", 4, "--uncertainty-rectify")
    monkeypatch.undo()
    on = R._loss_lines(out_a)
    assert out_a.count("uncertainty rectification: cross-entropy * exp(-KL between the two heads) + 1.0 * mean KL on every pass") == 1, out_a
    assert len(on) == 4 and not re.search(r"= (nan|inf)", out_a) and all(" unc = " in ln for ln in on), out_a
    vals = [re.search(r" unc = (\d+\.\d{3}) x(\d\.\d{3})\b", ln).groups() for ln in on]
    assert all(float(k) > 0.0 and 0.0 < float(m) <= 1.0 for k, m in vals), out_a
    assert _differ(snap_a, snap_o), "the flag changed no weight"
    (a, kw, steps), = built
    assert kw["uncertainty_rectify"] == 1.0 and len(steps) == 4
    tr = real(*a, **kw)
    for i, (sa, skw) in enumerate(steps):
        tr.step(*sa, **skw)
        l = tr.losses()
        text = "loss_seg1 = {loss_seg1:.3f} loss_seg2 = {loss_seg2:.3f}".format(**l) + tool.uncertainty_text(l)
        assert text in on[i], (text, on[i])
    saved = torch.load(snap_a, map_location="cpu")
    for k, v in tr.state_dict().items():
        assert torch.equal(saved[k], v), f"{k}: the tool's final weights differ from the hand-driven trainer's"
    # 2 + 2 == 4 through --train-state
    state = str(tmp_path / "run.state")
    out_r1, _ = run("r", 2, "--uncertainty-rectify", "--train-state", state)
    assert R._loss_lines(out_r1) == on[:2]
    out_r2, snap_r = run("r", 4, "--uncertainty-rectify", "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_r2), out_r2
    assert R._loss_lines(out_r2) == on[2:], (out_a, out_r2)
    R._same_snapshot(snap_a, snap_r)
    for other, named in ((["--uncertainty-rectify", "0.5"], r"differs in: uncertainty_rectify \(state: \[1\.0\], this run: \[0\.5\]\)"),
                         ([], r"differs in: uncertainty_rectify \(state: \[1\.0\], this run: False\)")):
        with pytest.raises(SystemExit, match=named):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "r"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
    torch.cuda.synchronize()
