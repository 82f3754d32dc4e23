"""trainV1_warmup --fda on the GPU: the flag's loop stage is FdaTransfer on each source micro-batch and nothing else, for all three
models, with --iter-size 2 and through --train-state."""
import os
import re

import pytest
import torch

import test_gpu_resume as R

pytestmark = pytest.mark.gpu
MODELS = ["DeepLab", "DeepLabv3", "DeepLabVGG"]
H, W, B = 65, 129, 2          # the smallest sizes of the --online-source tool tests


def _common(model):
    return ["--learning-rate", "2.5e-4", "--model", model, "--input-size-target", f"{W},{H}", "--batch-size", str(B), "--num-steps", "50",
            "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--synthetic", "--online-labels", "0",
            "--online-source"]


def _differ(a, b):
    """Two final snapshots of the same keys of which at least one tensor differs."""
    sa, sb = torch.load(a), torch.load(b)
    assert set(sa) == set(sb) and len(sa) > 0
    return any(not torch.equal(sa[k], sb[k]) for k in sa)


def _by_hand(tool, monkeypatch, dev, beta, hold):
    """The loop of a run WITHOUT the flag, its source images transformed by an FdaTransfer of the test's own in front of step_args."""
    from simt_amd.data.fda import FdaTransfer
    fda = FdaTransfer(B, H, W, beta, dev, hold=hold)
    real = tool.step_args

    def step_args(args, mb, sb=None):
        assert args.fda is None and sb is not None
        return real(args, mb, [(fda(s[0], m[0] if m[2] is None else m[2]), s[1]) for m, s in zip(mb, sb)])
    monkeypatch.setattr(tool, "step_args", step_args)


@pytest.mark.parametrize("model", MODELS)
def test_tool_trains_on_the_restyled_source_batch(dev, tmp_path, capsys, monkeypatch, model):
    """--synthetic --online-labels 0 --online-source --fda, three steps: finite loss lines, a run that differs from the flag-off run's, and
    loss lines and weights equal, bit for bit, to those of a run without the flag whose source images went through FdaTransfer by hand; the
    same with --iter-size 2 and a band b = 13; 2 + 2 == 4 steps through --train-state; a resume with beta changed or the flag dropped is
    refused with the field named.
    "Differs" is read off the trained weights, not off the loss lines: at 129 x 65 the bare flag is b = 0, which moves each plane of white
    noise by under one grey level, and a from-scratch DeepLabVGG prints ln 19 to three decimals whatever it is shown (measured: the three loss
    lines of flag on and flag off are the same text there, while DeepLab's and DeepLabv3's differ)."""
    from simt_amd.tools import trainV1_warmup as tool
    common = _common(model)

    def run(tag, stop, *more):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, f"GTA5_{stop}.pth")

    out_a, snap_a = run("a", 3, "--fda")
    lines = R._loss_lines(out_a)
    assert len(lines) == 3 and not re.search(r"= (nan|inf)", out_a) and all(" src = " in ln for ln in lines), out_a
    assert out_a.count("FDA: beta = 0.01, b = 0: the amplitudes of the 1 x 1 lowest frequencies") == 1
    out_o, snap_o = run("o", 3)
    assert "FDA" not in out_o and len(R._loss_lines(out_o)) == 3 and _differ(snap_a, snap_o), (out_o, out_a)
    out_w, snap_w = run("w", 2, "--fda", "0.2", "--iter-size", "2")
    assert "b = 13" in out_w and len(R._loss_lines(out_w)) == 2 and not re.search(r"= (nan|inf)", out_w)
    state = str(tmp_path / "run.state")
    out_c, snap_c = run("c", 4, "--fda", "0.2")
    whole = R._loss_lines(out_c)
    assert len(whole) == 4 and not re.search(r"= (nan|inf)", out_c)
    out_d1, _ = run("d", 2, "--fda", "0.2", "--train-state", state)
    assert R._loss_lines(out_d1) == whole[:2]
    out_d2, snap_d = run("d", 4, "--fda", "0.2", "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_d2), out_d2
    assert R._loss_lines(out_d2) == whole[2:], (out_c, out_d2)
    R._same_snapshot(snap_c, snap_d)
    for other in (["--fda", "0.1"], []):                      # beta changed | the flag dropped
        with pytest.raises(SystemExit, match=r"differs in: fda \(state: 0\.2, this run: "):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "d"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
    # by hand: the flag's runs again, the transform done by the test
    with monkeypatch.context() as mp:
        _by_hand(tool, mp, dev, "0.01", 1)
        out_h, snap_h = run("h", 3)
    assert "FDA" not in out_h and R._loss_lines(out_h) == lines, (out_h, out_a)
    R._same_snapshot(snap_a, snap_h)
    with monkeypatch.context() as mp:
        _by_hand(tool, mp, dev, "0.2", 2)
        out_hw, snap_hw = run("hw", 2, "--iter-size", "2")
    assert R._loss_lines(out_hw) == R._loss_lines(out_w), (out_hw, out_w)
    R._same_snapshot(snap_w, snap_hw)
    with monkeypatch.context() as mp:                         # and the by-hand comparison can fail: another beta is another run
        _by_hand(tool, mp, dev, "0.1", 2)
        _out, snap_x = run("x", 2, "--iter-size", "2")
    assert _differ(snap_w, snap_x)
    torch.cuda.synchronize()
