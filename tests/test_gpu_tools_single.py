"""trainV2_simt --model DeepLabv3 | DeepLabVGG on real files (the small tree of tests/test_gpu_tools.py): the SimT loop over
SimTSingleTrainer, the periodic evaluate_simt of that model, the best-mIoU snapshot and the final GTA5_<stop>.pth with the module's keys;
then `python -m simt_amd.tools.test` scores the best snapshot and prints the mIoU in its file name."""
import glob
import os
import re

import pytest
import torch

from test_gpu_tools import _make_dataset

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", ["DeepLabv3", "DeepLabVGG"])
def test_train_tool_single_model_eval_snapshots_and_test_tool(dev, tmp_path, capsys, model):
    Image = pytest.importorskip("PIL.Image")
    from simt_amd.tools import test as ttool
    from simt_amd.tools import trainV2_simt as tool
    _make_dataset(tmp_path, Image)
    snap = str(tmp_path / "snap")
    val = ["--data-dir-val", str(tmp_path), "--data-list-val", str(tmp_path / "kit" / "val.txt"), "--gt-dir-val", str(tmp_path / "gt"),
           "--devkit-dir", str(tmp_path / "kit")]
    argv = ["--model", model, "--data-dir-target", str(tmp_path), "--data-list-target", str(tmp_path / "pseudo.lst"),
            "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--num-steps-stop", "5", "--save-pred-every", "2",
            "--print-every", "1", "--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3", "--from-scratch",
            "--restore-from", "", "--snapshot-dir", snap, "--num-workers", "2", "--random-mirror"] + val
    tool.main(argv)
    out = capsys.readouterr().out
    assert out.count("Begin evaluation") == 1 and out.count("===> mIoU:") == 1
    assert "iter =        4/" in out and "Place_loss" in out and "save model" in out
    final = os.path.join(snap, "GTA5_5.pth")
    sd = torch.load(final)
    st, _ = tool.single_model_states(model, 19, 3)
    assert set(sd) == set(st)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
    if model == "DeepLabv3":
        assert int(sd["resnet.resnet_50.bn1.num_batches_tracked"]) == 5 and int(sd["resnet.resnet_50.layer4.0.bn1.num_batches_tracked"]) == 0
    best = glob.glob(os.path.join(snap, "GTA5_iter*_mIoU*.pth"))
    assert len(best) == 1 and "GTA5_iter2_mIoU" in best[0]
    miou_name = re.search(r"_mIoU([0-9.]+)\.pth$", best[0]).group(1)
    got = ttool.main(["--model", model, "--open-classes", "3", "--restore-from", best[0], "--num-workers", "2"] + val)
    out = capsys.readouterr().out
    print(out)
    assert "restore_from: " in out and "Finish Evaluation: " in out
    printed = re.findall(r"===> mIoU: ([0-9.]+)", out)
    assert printed == [miou_name] and str(got) == miou_name


def test_train_tool_refuses_iter_size_for_single_models(dev, tmp_path):
    from simt_amd.tools import trainV2_simt as tool
    with pytest.raises(SystemExit, match="--iter-size 2"):
        tool.main(["--model", "DeepLabv3", "--iter-size", "2", "--synthetic", "--snapshot-dir", str(tmp_path)])
