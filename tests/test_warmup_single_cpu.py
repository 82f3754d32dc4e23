"""CPU checks of `trainV1_warmup --model DeepLabv3 | DeepLabVGG` (no GPU): --model validation, --v3-layers, and the torchvision ImageNet
layouts its --restore-from accepts (simt_amd/pretrained.py): a ResNet file lands under `resnet.resnet_50.`, a vgg16 file's conv5_x
(features 24 / 26 / 28) on DeeplabVGG's 23 / 25 / 27 -- on synthetic checkpoints built from the modules' own state shapes."""
import pytest
import torch

from simt_amd import pretrained
from simt_amd.tools import trainV1_warmup as tool
from simt_amd.tools.trainV2_simt import single_model_state

TV_VGG16_CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
                  (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]


def _tv_vgg16(seed=0):
    """torchvision vgg16's state-dict layout: 13 convs in `features` (pool4 at index 23), a Linear classifier (small stand-ins here)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for (i, cin, cout) in TV_VGG16_CONVS:
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g)
        sd[f"features.{i}.bias"] = torch.randn(cout, generator=g)
    for i in (0, 3, 6):
        sd[f"classifier.{i}.weight"], sd[f"classifier.{i}.bias"] = torch.randn(8, 16, generator=g), torch.randn(8, generator=g)
    return sd


def _tv_resnet(state, seed=0):
    """torchvision ResNet layout of a DeepLabv3 state: its `resnet.resnet_50.` keys without the prefix, fresh values."""
    g = torch.Generator().manual_seed(seed)
    return {k[len(pretrained.RESNET_PREFIX):]: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone())
            for k, v in state.items() if k.startswith(pretrained.RESNET_PREFIX)}


def test_model_flag_is_validated(tmp_path):
    with pytest.raises(SystemExit, match="--model"):
        tool.main(["--model", "DeepLabV3", "--synthetic", "--snapshot-dir", str(tmp_path)])
    for m in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        tool.check_model(tool.get_arguments(["--model", m, "--iter-size", "2"]))      # --iter-size works for every model here


def test_v3_layers_flag():
    assert tool.get_arguments([]).v3_layers == [3, 4, 6]
    assert tool.get_arguments(["--model", "DeepLabv3", "--v3-layers", "3", "4", "23"]).v3_layers == [3, 4, 23]
    with pytest.raises(SystemExit):
        tool.get_arguments(["--v3-layers", "3", "4"])


@pytest.mark.parametrize("layers", [(3, 4, 6), (3, 4, 23)])
def test_torchvision_resnet_maps_onto_deeplabv3(tmp_path, capsys, layers):
    state = single_model_state("DeepLabv3", 19, layers)
    ck = _tv_resnet(state, seed=1)
    assert "conv1.weight" in ck and f"layer3.{layers[2] - 1}.conv3.weight" in ck and "fc.weight" in ck
    path = str(tmp_path / "resnet.pth")
    torch.save(ck, path)
    n, layout = tool.restore_single(state, path, "v3", required=True)
    assert layout == "torchvision ResNet" and n == len(ck)
    assert torch.equal(state["resnet.resnet_50.layer1.0.conv2.weight"], ck["layer1.0.conv2.weight"])
    assert torch.equal(state[f"resnet.resnet_50.layer3.{layers[2] - 1}.bn3.running_var"], ck[f"layer3.{layers[2] - 1}.bn3.running_var"])
    # the module's own layout (a warm-up checkpoint) is taken as it is
    path2 = str(tmp_path / "own.pth")
    torch.save(state, path2)
    fresh = single_model_state("DeepLabv3", 19, layers, seed=5)
    assert tool.restore_single(fresh, path2, "v3", required=True) == (len(state), "DeepLabv3")


def test_torchvision_vgg16_conv5_lands_on_23_25_27(tmp_path):
    state = single_model_state("DeepLabVGG", 19)
    init = {k: v.clone() for k, v in state.items()}
    ck = _tv_vgg16(seed=2)
    mapped = pretrained.vgg16_to_deeplab_vgg(ck)
    assert sorted(mapped) == sorted(f"features.{i}.{p}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 23, 25, 27) for p in ("weight", "bias"))
    path = str(tmp_path / "vgg16.pth")
    torch.save(ck, path)
    n, layout = tool.restore_single(state, path, "vgg", required=True)
    assert layout == "torchvision vgg16" and n == 26
    for src, dst in ((0, 0), (21, 21), (24, 23), (26, 25), (28, 27)):
        assert torch.equal(state[f"features.{dst}.weight"], ck[f"features.{src}.weight"]), (src, dst)
        assert torch.equal(state[f"features.{dst}.bias"], ck[f"features.{src}.bias"]), (src, dst)
    for k in ("features.29.weight", "features.31.bias", "classifier.conv2d_list.0.weight", "classifier.conv2d_list.3.bias"):
        assert torch.equal(state[k], init[k]), f"{k}: fc6 / fc7 / the classifier keep their init"


def test_checkpoint_that_matches_nothing_is_an_error(tmp_path):
    path = str(tmp_path / "other.pth")
    torch.save({"encoder.weight": torch.zeros(3, 3)}, path)
    for model, name in (("v3", "DeepLabv3"), ("vgg", "DeepLabVGG")):
        state = single_model_state(name, 19)
        with pytest.raises(RuntimeError, match="no tensor matched"):
            tool.restore_single(state, path, model, required=True)
    assert pretrained.checkpoint_layout({"encoder.weight": torch.zeros(1)}, "vgg")[0] == "unrecognised"
    # a ResNet file given to the VGG warm-up matches nothing either
    path2 = str(tmp_path / "resnet.pth")
    torch.save(_tv_resnet(single_model_state("DeepLabv3", 19)), path2)
    with pytest.raises(RuntimeError, match="no tensor matched"):
        tool.restore_single(single_model_state("DeepLabVGG", 19), path2, "vgg", required=True)
    with pytest.raises(FileNotFoundError):
        tool.restore_single(single_model_state("DeepLabVGG", 19), str(tmp_path / "missing.pth"), "vgg", required=True)
