"""trainV1_warmup --proto-denoise on the GPU, on synthetic data, for all three models: the ` proto = ` field of the loss line; the
flag-off loss lines and snapshot bytes are those of a run that never heard of the flag (two flag-off runs agree, and the flag's first
iteration -- no class seen -- prints the flag-off line); the flag moves the weights; 2 + 2 == 4 through --train-state; a resume with the flag
changed or dropped is refused.

DeepLab and DeepLabv3 start from scratch.  The from-scratch DeepLab-VGG16 predicts ONE class at every pixel of the synthetic batches (measured:
` proto = 1/19 moved 0.0000` at every iteration), and with one prototype every class takes the same distance: the rule is the identity there,
whatever the code does.  Its runs therefore start from a checkpoint the test makes -- the tool's own one-step snapshot with the classifier's
weights times 100 and noise on its biases -- on which the teacher finds three classes (measured: ` proto = 3/19 moved 0.0312` from iteration 1)."""
import os
import re

import pytest
import torch

import test_gpu_resume as R
from test_gpu_fda_tool import _differ

pytestmark = pytest.mark.gpu
MODELS = ["DeepLab", "DeepLabv3", "DeepLabVGG"]
H, W, B = 65, 129, 2
PROTO = re.compile(r" proto = (\d+)/19 moved (\d\.\d{4})")


def _common(model, restore=None):
    return ["--learning-rate", "2.5e-4", "--model", model, "--input-size-target", f"{W},{H}", "--batch-size", str(B), "--num-steps", "50",
            "--save-pred-every", "100", "--print-every", "1", "--synthetic", "--online-labels", "0.05"] + \
        (["--from-scratch", "--restore-from", ""] if restore is None else ["--restore-from", restore])


def _confident_vgg(tool, tmp_path, capsys):
    """A DeepLab-VGG16 start whose teacher finds more than one class: the tool's one-step snapshot, classifier weights x 100, biases + noise."""
    snap = str(tmp_path / "start")
    tool.main(_common("DeepLabVGG") + ["--snapshot-dir", snap, "--num-steps-stop", "1"])
    capsys.readouterr()
    sd = torch.load(os.path.join(snap, "GTA5_1.pth"), map_location="cpu")
    g = torch.Generator().manual_seed(3)
    for k in [k for k in sd if k.startswith("classifier")]:
        sd[k] = sd[k] * 100.0 + (torch.randn(sd[k].shape, generator=g) * 0.5 if k.endswith("bias") else 0.0)
    path = str(tmp_path / "start.pth")
    torch.save(sd, path)
    return path


@pytest.mark.parametrize("model", MODELS)
def test_tool_prints_the_field_moves_the_weights_and_resumes(dev, tmp_path, capsys, model):
    from simt_amd.tools import trainV1_warmup as tool
    common = _common(model, _confident_vgg(tool, tmp_path, capsys) if model == "DeepLabVGG" else None)

    def run(tag, stop, *more):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, f"GTA5_{stop}.pth")

    out_o, snap_o = run("o", 4)                                                        # flag off
    off = R._loss_lines(out_o)
    assert len(off) == 4 and "prototype weights" not in out_o and not any(" proto = " in ln for ln in off), out_o
    out_p, snap_p = run("p", 4)                                                        # flag off again: the same lines, the same bytes
    assert R._loss_lines(out_p) == off and open(snap_p, "rb").read() == open(snap_o, "rb").read()
    flags = ["--proto-denoise", "0.5", "--proto-momentum", "0.9"]
    out_a, snap_a = run("a", 4, *flags)
    assert out_a.count("prototype weights: the teacher's posterior times softmax(-(d - d_min) / 0.5)") == 1 and "momentum 0.9)" in out_a
    on = R._loss_lines(out_a)
    assert len(on) == 4 and not re.search(r"= (nan|inf)", out_a) and all(PROTO.search(ln) for ln in on), out_a
    seen = [int(PROTO.search(ln).group(1)) for ln in on]
    moved = [float(PROTO.search(ln).group(2)) for ln in on]
    assert PROTO.sub("", on[0]) == off[0] and moved[0] == 0.0 and 0 < seen[0] <= 19 and seen == sorted(seen) and max(moved[1:]) > 0.0, out_a
    assert _differ(snap_a, snap_o), "the flag changed no weight"
    out_d, _ = run("d", 2, "--proto-denoise")                                          # the bare flag: ProDA's temperature and momentum
    assert "softmax(-(d - d_min) / 1.0)" in out_d and "momentum 0.9999)" in out_d and all(PROTO.search(ln) for ln in R._loss_lines(out_d))
    # 2 + 2 == 4 through --train-state
    state = str(tmp_path / "run.state")
    out_r1, _ = run("r", 2, *flags, "--train-state", state)
    assert R._loss_lines(out_r1) == on[:2]
    out_r2, snap_r = run("r", 4, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_r2), out_r2
    assert R._loss_lines(out_r2) == on[2:], (out_a, out_r2)
    R._same_snapshot(snap_a, snap_r)
    for other, named in ((["--proto-denoise", "1.0", "--proto-momentum", "0.9"], r"differs in: proto_denoise \(state: \[0\.5, 0\.9\], this run: \[1\.0, 0\.9\]\)"),
                         ([], r"differs in: proto_denoise \(state: \[0\.5, 0\.9\], this run: False\)")):
        with pytest.raises(SystemExit, match=named):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "r"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
    torch.cuda.synchronize()
