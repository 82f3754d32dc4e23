"""Host side of the pseudo-label export for DeepLabv3 and DeepLab-VGG16 (make_pseudo_labels --arch v3 | vgg): the binding of
simt_pseudo_label2_u8 against its header declaration, the new arguments, and the restore checks that run before any GPU work."""
import os
import re

import pytest
import torch

from simt_amd import pretrained
from simt_amd.tools import make_pseudo_labels as mpl
from simt_amd.tools.trainV2_simt import single_model_state, single_model_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(decl):
    return [" ".join(p.split()) for p in decl.split(",")]


def test_pseudo_label2_binding_matches_header():
    from simt_amd import _lib as L
    assert L.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
    m = re.search(r"int\s+simt_pseudo_label2_u8\s*\(([^)]*)\)\s*;", hdr)
    assert m, "simt_pseudo_label2_u8 is not declared in include/simt_hip.h"
    params = _params(m.group(1))
    kinds = []
    for p in params:
        if "*" in p or p.startswith("simt_stream_t"):
            kinds.append("ptr")
        elif p.split()[0] == "float":
            kinds.append("float")
        else:
            assert p.split()[0] == "int", p
            kinds.append("int")
    res, args = L.SIGNATURES["simt_pseudo_label2_u8"]
    assert res is L.C.c_int
    got = ["ptr" if a is L.C.c_void_p else "int" if a is L.C.c_int else "float" if a is L.C.c_float else repr(a) for a in args]
    assert got == kinds
    assert len(kinds) == 21
    # the arguments of simt_upsample2_sum_argmax, then the mode / threshold / out / counts tail of simt_pseudo_label_u8
    names = [p.split()[-1].lstrip("*") for p in params]
    up2 = [p.split()[-1].lstrip("*") for p in _params(re.search(r"int\s+simt_upsample2_sum_argmax\s*\(([^)]*)\)\s*;", hdr).group(1))]
    pl = [p.split()[-1].lstrip("*") for p in _params(re.search(r"int\s+simt_pseudo_label_u8\s*\(([^)]*)\)\s*;", hdr).group(1))]
    assert names[:16] == up2[:16] and names[16:] == pl[12:]


def test_arguments():
    a = mpl.get_arguments(["--restore-from", "m.pth", "--arch", "v3", "--v3-layers", "3", "4", "23"])
    assert a.arch == "v3" and a.v3_layers == [3, 4, 23]
    a = mpl.get_arguments(["--restore-from", "m.pth", "--arch", "vgg", "--open-classes", "6"])
    assert a.arch == "vgg" and a.open_classes == 6
    a = mpl.get_arguments(["--restore-from", "m.pth"])
    assert a.arch == "multi" and a.v3_layers == [3, 4, 6] and a.open_classes == 0
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--model", "DeepLabv3"])
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--arch", "single", "--open-classes", "3"])
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--arch", "v2"])


def _main(ckpt, *extra):
    mpl.main(["--restore-from", str(ckpt), "--data-dir", "unused", *extra])


def test_v3_trunk_only_checkpoint_is_refused(tmp_path):
    st = single_model_state("DeepLabv3", 19, (1, 1, 1), seed=3)
    trunk = {k: v for k, v in st.items() if not k.startswith("conv.")}
    torch.save(trunk, tmp_path / "trunk.pth")
    with pytest.raises(SystemExit, match="--open-classes") as e:
        _main(tmp_path / "trunk.pth", "--arch", "v3", "--v3-layers", "1", "1", "1")
    assert "--v3-layers 1 1 1" in str(e.value)


def test_torchvision_files_are_refused(tmp_path):
    st = single_model_state("DeepLabv3", 19, (1, 1, 1), seed=3)
    g = torch.Generator().manual_seed(0)
    tv = {k[len(pretrained.RESNET_PREFIX):]: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone())
          for k, v in st.items() if k.startswith(pretrained.RESNET_PREFIX)}
    torch.save(tv, tmp_path / "resnet.pth")
    assert pretrained.checkpoint_layout(tv, "v3")[0] == "torchvision ResNet"
    with pytest.raises(SystemExit, match="torchvision ResNet.*--open-classes"):
        _main(tmp_path / "resnet.pth", "--arch", "v3", "--v3-layers", "1", "1", "1")
    vgg = single_model_state("DeepLabVGG", 19, seed=4)
    conv = {f"features.{i}": f"features.{j}" for i, j in ((0, 0), (2, 2), (5, 5), (7, 7), (10, 10), (12, 12), (14, 14), (17, 17),
                                                           (19, 19), (21, 21), (23, 24), (25, 26), (27, 28))}
    tvv = {}
    for ours, theirs in conv.items():
        tvv[theirs + ".weight"], tvv[theirs + ".bias"] = vgg[ours + ".weight"].clone(), vgg[ours + ".bias"].clone()
    torch.save(tvv, tmp_path / "vgg16.pth")
    assert pretrained.checkpoint_layout(tvv, "vgg")[0] == "torchvision vgg16"
    with pytest.raises(SystemExit, match="torchvision vgg16.*--open-classes"):
        _main(tmp_path / "vgg16.pth", "--arch", "vgg")


def test_vgg_checkpoint_with_other_open_classes_is_refused(tmp_path):
    st, _ = single_model_states("DeepLabVGG", 19, 3, seed=5)          # a SimT checkpoint, DeeplabVGG(19 + 3)
    torch.save(st, tmp_path / "simt.pth")
    with pytest.raises(SystemExit, match="--open-classes 0"):
        _main(tmp_path / "simt.pth", "--arch", "vgg")
    state, n, layout = mpl.restore_single_model("vgg", str(tmp_path / "simt.pth"), 19, 3, (3, 4, 6))
    assert layout == "DeeplabVGG" and n == len(st)
    assert all(torch.equal(state[k], v) for k, v in st.items())


def test_v3_checkpoint_restores_with_its_keys(tmp_path):
    st, _ = single_model_states("DeepLabv3", 19, 6, (1, 1, 1), seed=6)
    torch.save(st, tmp_path / "v3.pth")
    state, n, layout = mpl.restore_single_model("v3", str(tmp_path / "v3.pth"), 19, 6, (1, 1, 1))
    assert layout == "DeepLabv3" and n == len(st)
    assert all(torch.equal(state[k], v) for k, v in st.items())
    with pytest.raises(FileNotFoundError):
        _main(tmp_path / "missing.pth", "--arch", "v3")
