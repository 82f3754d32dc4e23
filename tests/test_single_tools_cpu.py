"""Host side of training / scoring the one-output models (no GPU): `python -m simt_amd.tools.test` flag parsing (every flag of the
reference's tools/test.py, written out), trainV2_simt --model validation, the --not-restore-last filter per model, and the binding of
simt_upsample2_sum_argmax against include/simt_hip.h."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/test.py of the reference: (flag, kind), in its order
REFERENCE_TEST_FLAGS = [
    ("--model", "str"), ("--target", "str"), ("--batch-size", "int"), ("--iter-size", "int"), ("--num-workers", "int"),
    ("--data-dir", "str"), ("--data-list", "str"), ("--ignore-label", "int"), ("--input-size", "str"), ("--data-dir-target", "str"),
    ("--data-list-target", "str"), ("--input-size-target", "str"), ("--is-training", "store_true"), ("--learning-rate", "float"),
    ("--learning-rate-T", "float"), ("--lambda-seg", "float"), ("--Threshold-high", "float"), ("--Threshold-low", "float"),
    ("--lambda-Place", "float"), ("--lambda-Convex", "float"), ("--lambda-Volume", "float"), ("--lambda-Anchor", "float"),
    ("--momentum", "float"), ("--not-restore-last", "store_true"), ("--num-classes", "int"), ("--open-classes", "int"),
    ("--num-steps", "int"), ("--num-steps-stop", "int"), ("--power", "float"), ("--random-mirror", "store_true"),
    ("--random-scale", "store_true"), ("--random-seed", "int"), ("--restore-from", "str"), ("--save-pred-every", "int"),
    ("--snapshot-dir", "str"), ("--weight-decay", "float"), ("--gpu", "int"), ("--set", "str"), ("--log-dir", "str"),
]
VALUE = {"int": ("3", 3), "float": ("0.25", 0.25), "str": ("x,y", "x,y")}


def test_test_tool_accepts_every_reference_flag_and_its_own():
    from simt_amd.tools import test as tool
    argv = []
    for name, kind in REFERENCE_TEST_FLAGS:
        argv += [name] if kind == "store_true" else [name, VALUE[kind][0]]
    argv += ["--data-dir-val", "v", "--data-list-val", "v.txt", "--gt-dir-val", "g", "--devkit-dir", "k", "--eval-dtype", "bf16",
             "--v3-layers", "3", "4", "23"]
    ns = vars(tool.get_arguments(argv))
    for name, kind in REFERENCE_TEST_FLAGS:
        assert ns[name[2:].replace("-", "_")] == (True if kind == "store_true" else VALUE[kind][1]), name
    assert (ns["data_dir_val"], ns["data_list_val"], ns["gt_dir_val"], ns["devkit_dir"]) == ("v", "v.txt", "g", "k")
    assert ns["eval_dtype"] == "bf16" and ns["v3_layers"] == [3, 4, 23]
    d = tool.get_arguments([])
    assert d.model == "DeepLab" and d.eval_dtype == "f32" and d.v3_layers == [3, 4, 6] and d.set == "val"


def test_train_tool_v3_layers_flag():
    from simt_amd.tools import trainV2_simt as tool
    assert tool.get_arguments([]).v3_layers == [3, 4, 6] and tool.get_arguments([]).model == "DeepLab"
    assert tool.get_arguments(["--model", "DeepLabv3", "--v3-layers", "3", "4", "23"]).v3_layers == [3, 4, 23]
    with pytest.raises(SystemExit):
        tool.get_arguments(["--v3-layers", "3", "4"])


def test_model_validation(tmp_path):
    from simt_amd.tools import test as ttool
    from simt_amd.tools import trainV2_simt as tool
    for m in ("DeepLabV3", "deeplab", "VGG", ""):
        with pytest.raises(SystemExit, match="--model"):
            tool.main(["--model", m, "--synthetic"])
        with pytest.raises(SystemExit, match="--model"):
            ttool.main(["--model", m, "--restore-from", "x.pth"])
    for m in ("DeepLabv3", "DeepLabVGG"):              # SimTSingleTrainer asserts iter_size == 1: refused before anything starts
        with pytest.raises(SystemExit, match="--iter-size 2"):
            tool.main(["--model", m, "--iter-size", "2", "--synthetic"])
    with pytest.raises(SystemExit, match="--data-dir-val"):
        ttool.main(["--model", "DeepLabVGG", "--restore-from", "x.pth", "--data-dir-val", str(tmp_path / "missing")])
    with pytest.raises(SystemExit, match="--restore-from"):
        ttool.main(["--model", "DeepLabVGG", "--restore-from", str(tmp_path / "missing.pth"), "--data-dir-val", str(tmp_path)])


def _ckpt(tmp_path, state, name="c.pth"):
    ck = {k: (v + 1.0 if v.is_floating_point() else v + 1) for k, v in state.items()}
    path = str(tmp_path / name)
    torch.save(ck, path)
    return path, ck


@pytest.mark.parametrize("model,last", [("DeepLab", ("layer5", "layer6")), ("DeepLabv3", ("conv.", "conv_1.")),
                                        ("DeepLabVGG", ("classifier.",))])
def test_restore_not_restore_last_per_model(tmp_path, model, last):
    from simt_amd import model_spec as ms
    from simt_amd.tools import test as ttool
    from simt_amd.tools import trainV2_simt as tool
    if model == "DeepLab":
        state = ms.reference_init(ms.state_shapes(19, 3, True, layers=(1, 1, 1, 1)), seed=1)
    else:
        state, _ = tool.single_model_states(model, 19, 3)
    assert tool.RESTORE_LAST[model] == last
    path, ck = _ckpt(tmp_path, state)
    n_all = tool.restore(dict(state), path, required=True, last=tool.RESTORE_LAST[model])
    assert n_all == len(state)
    fresh = dict(state)
    n = tool.restore(fresh, path, not_restore_last=True, required=True, last=tool.RESTORE_LAST[model])
    skipped = [k for k in state if k.startswith(last)]
    assert skipped and n == len(state) - len(skipped)
    for k in state:
        assert torch.equal(fresh[k], state[k] if k in skipped else ck[k]), k
    # a shape mismatch is filtered, a file with no matching tensor is an error (restore(required=True)), as tools/test.py uses it
    k0 = next(k for k in state if k.endswith("weight") and state[k].dim() == 4)
    torch.save({k0: torch.zeros(1, 1, 1, 1), "nothing.here": torch.zeros(2)}, str(tmp_path / "bad.pth"))
    with pytest.raises(RuntimeError, match="no tensor matched"):
        tool.restore(dict(state), str(tmp_path / "bad.pth"), required=True)
    args = ttool.get_arguments(["--model", model, "--open-classes", "3", "--restore-from", path])
    if model == "DeepLab":
        return                                       # full-depth DeepLab-v2 state: covered by the restore() calls above
    st, n_t = ttool.model_state(args)
    assert n_t == len(st) and set(st) == set(state)
    assert all(torch.equal(st[k], ck[k]) for k in st)


def test_single_model_states_load_into_modules():
    from simt_amd.model.deeplab_vgg import DeeplabVGG
    from simt_amd.model.deeplabv3 import DeepLabv3
    from simt_amd.tools import trainV2_simt as tool
    st, fst = tool.single_model_states("DeepLabv3", 19, 6)
    DeepLabv3(19, 6, openset=True).load_state_dict(st, strict=True)
    DeepLabv3(19).load_state_dict(fst, strict=True)
    assert st["conv_1.weight"].shape == (6, 256, 1, 1) and "conv_1.weight" not in fst
    deep, _ = tool.single_model_states("DeepLabv3", 19, 6, (3, 4, 23))
    assert sum(1 for k in deep if ".layer3." in k and k.endswith("conv2.weight")) == 23 and set(st) <= set(deep)
    vt, vf = tool.single_model_states("DeepLabVGG", 19, 3)
    DeeplabVGG(22).load_state_dict(vt, strict=True)
    DeeplabVGG(19).load_state_dict(vf, strict=True)


def test_upsample2_binding_matches_header():
    from simt_amd import _lib as L
    assert L.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
    m = re.search(r"int\s+simt_upsample2_sum_argmax\s*\(([^)]*)\)\s*;", hdr)
    assert m, "simt_upsample2_sum_argmax is not declared in include/simt_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    kinds = []
    for p in params:
        if "*" in p or p.startswith("simt_stream_t"):
            kinds.append("ptr")
        else:
            assert p.split()[0] == "int", p
            kinds.append("int")
    res, args = L.SIGNATURES["simt_upsample2_sum_argmax"]
    assert res is L.C.c_int
    got = ["ptr" if a is L.C.c_void_p else "int" if a is L.C.c_int else repr(a) for a in args]
    assert got == kinds
    assert len(kinds) == 18
    # the arguments of simt_upsample_sum_argmax, plus (hi, wi) after each scale's ld
    m0 = re.search(r"int\s+simt_upsample_sum_argmax\s*\(([^)]*)\)\s*;", hdr)
    names0 = [p.split()[-1].lstrip("*") for p in m0.group(1).split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert [n for n in names if n not in ("hia", "wia", "hib", "wib")] == names0
    assert names.index("hia") == names.index("lda") + 1 and names.index("hib") == names.index("ldb") + 1
