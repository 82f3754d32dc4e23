"""The weak-view teacher without a GPU: the --weak-teacher flag and its run identity, the three new symbols against the
header, the item map's properties, the two-view restatement of the losses against the oracle, the loader's refusal and the train-state
refusal on fake trainers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as cm
import _weak_teacher_ref as wt
from oracle import simt_oracle as so
from simt_amd import _lib
from simt_amd import train_state as tsf
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD = so.load_class_dist()


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------------
def test_flag_needs_an_augmentation_and_real_data(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    assert get_arguments([]).weak_teacher is False and get_arguments(["--class-mix"]).weak_teacher is False
    for aug in (["--class-mix"], ["--class-mix", "0.5"], ["--colour-jitter"], ["--gaussian-blur", "0.3"], ["--class-mix", "--colour-jitter", "--gaussian-blur"]):
        for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
            assert get_arguments(["--model", model, "--batch-size", "2", "--weak-teacher"] + aug).weak_teacher is True
    for argv in (["--weak-teacher"], ["--weak-teacher", "--scale-crop"], ["--weak-teacher", "--synthetic"],
                 ["--weak-teacher", "--class-mix", "--synthetic"], ["--weak-teacher", "--colour-jitter", "--gaussian-blur", "--synthetic"]):
        with pytest.raises(SystemExit) as e:
            get_arguments(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2, argv
        assert "--weak-teacher needs --class-mix, --colour-jitter or --gaussian-blur" in err, (argv, err)


def test_the_warmup_tool_has_no_such_flag(capsys):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(["--class-mix", "--weak-teacher"])
    assert e.value.code == 2 and "--weak-teacher" in capsys.readouterr().err


def test_run_identity_carries_the_flag_only_when_it_is_on():
    from simt_amd.tools import trainV2_simt as tool
    cd = CD.numpy()
    on = tool.run_identity(tool.get_arguments(["--batch-size", "2", "--class-mix", "--weak-teacher"]), cd)
    off = tool.run_identity(tool.get_arguments(["--batch-size", "2", "--class-mix"]), cd)
    assert on["weak_teacher"] is True and "weak_teacher" not in off
    assert {k: v for k, v in on.items() if k != "weak_teacher"} == off
    assert tool.RUN_DEFAULTS["weak_teacher"] is False


def test_train_state_file_refuses_the_flag_added_or_dropped(tmp_path, no_device_sync):
    """TrainStateFile.resume compares run identities with RUN_DEFAULTS filled in: a state written without the key is a run without the flag."""
    from simt_amd.tools import trainV2_simt as tool
    cd = CD.numpy()
    base = ["--batch-size", "2", "--class-mix", "--train-state", str(tmp_path / "s.state")]
    tr = _advanced(_Fake())

    class Keeper:
        def state(self):
            return {}

        def load_state(self, s):
            pass
    for first, second in ((["--weak-teacher"], []), ([], ["--weak-teacher"])):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        tool.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(tr, Keeper())
        assert tool.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(seed=1), Keeper()) == 3
        with pytest.raises(SystemExit, match="weak_teacher"):
            tool.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(seed=1), Keeper())


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_match_the_header_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
    assert re.search(r"int simt_class_mix_items\(const simt_class_mix_desc\* d, uint8_t\* item_out, simt_stream_t stream\);", header)
    assert re.search(r"int simt_head_loss_views\(const simt_head_desc\* d, const uint8_t\* fix_item, simt_stream_t stream\);", header)
    assert re.search(r"int simt_head_grad_views\(const simt_head_desc\* d, const uint8_t\* fix_item, simt_stream_t stream\);", header)
    assert re.search(r"#define SIMT_ABI_VERSION 2\b", header) and _lib.ABI_VERSION == 2
    assert _lib.SIGNATURES["simt_class_mix_items"] == (C.c_int, [C.POINTER(_lib.ClassMixDesc), C.c_void_p, C.c_void_p])
    for name in ("simt_head_loss_views", "simt_head_grad_views"):
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(_lib.HeadDesc), C.c_void_p, C.c_void_p])
    # the one-view entry points keep their prototypes
    assert _lib.SIGNATURES["simt_class_mix"] == (C.c_int, [C.POINTER(_lib.ClassMixDesc), C.c_void_p])
    assert _lib.SIGNATURES["simt_head_loss"] == _lib.SIGNATURES["simt_head_grad"] == (C.c_int, [C.POINTER(_lib.HeadDesc), C.c_void_p])


# ---- the item map -------------------------------------------------------------------------------------------------------------------------------
def _labels(B, h, w, Cn, seed):
    rng = np.random.default_rng([seed, B, h, w])
    blocks = rng.integers(0, Cn, (B, -(-h // 8), -(-w // 8))).astype(np.int64)
    blocks[rng.random(blocks.shape) < 0.15] = 255
    lab = np.kron(blocks, np.ones((1, 8, 8), np.int64))[:, :h, :w].copy()
    lab[rng.random(lab.shape) < 0.03] = 255
    lab[0, 1, 2] = Cn + 1
    return lab


@pytest.mark.parametrize("B,h,w,Cn", [(2, 24, 40, 19), (5, 17, 23, 19), (3, 16, 16, 32)])
def test_item_map_properties(B, h, w, Cn):
    lab = _labels(B, h, w, Cn, 3)
    rng = np.random.default_rng(4)
    rank = rng.permuted(np.tile(np.arange(Cn, dtype=np.uint8), (B, 1)), axis=1)
    partner = [(i + 1) % B for i in range(B)]
    on, off = np.ones(B, bool), np.zeros(B, bool)
    m = wt.item_map(lab, partner, on, rank, Cn)
    assert m.dtype == np.uint8 and m.shape == lab.shape
    paste = cm.paste_masks(lab, on, rank, Cn)
    for i in range(B):
        assert set(np.unique(m[i])) <= {i, partner[i]}                         # every value is the item or its partner
        assert np.array_equal(m[i] == partner[i], paste[i])                     # ... the partner exactly where the mix pastes
        invalid = (lab[partner[i]] < 0) | (lab[partner[i]] >= Cn)
        assert invalid.any() and (m[i][invalid] == i).all()                     # an ignore label is never pasted
        assert paste[i].any() and not paste[i].all()
    assert np.array_equal(wt.item_map(lab, partner, off, rank, Cn), np.arange(B, dtype=np.uint8)[:, None, None] * np.ones_like(lab, dtype=np.uint8))
    mixed = np.arange(B) % 2 == 0
    mm = wt.item_map(lab, partner, mixed, rank, Cn)
    for i in range(B):
        assert np.array_equal(mm[i], m[i]) if mixed[i] else (mm[i] == i).all()
    # the mixed batch is the batch gathered by the map: labels and pixels come from the item the map names
    xb = rng.integers(-2 ** 31, 2 ** 31 - 1, (B, 3, h, w)).astype(np.int32)
    xo, lo = cm.mix(xb, lab, on, rank, Cn)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.array_equal(lo, lab[m, yy, xx]) and all(np.array_equal(xo[:, ch], xb[:, ch][m, yy, xx]) for ch in range(3))
    # another partner table than the loader's
    other = [(i + B - 1) % B for i in range(B)]
    mo = wt.item_map(lab, other, on, rank, Cn)
    assert all(set(np.unique(mo[i])) <= {i, other[i]} for i in range(B))


# ---- the losses ---------------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(B, K, h, w, H, W, seed=5):
    Cn, Q = 19, 19 + K
    g = torch.Generator().manual_seed(seed)
    p1, p2 = torch.randn(B, Q, h, w, generator=g) * 3, torch.randn(B, Q, h, w, generator=g) * 3
    f2 = torch.randn(B, Cn, h, w, generator=g) * 4
    _, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=11, block=8)
    T = [so.sig_ntm_forward(so.ntm_init(Cn, K, s), CD, Cn) for s in (1, 2)]
    Wm = [so.sig_w_forward(so.w_init(Cn, K)) for _ in range(2)]
    return p1, p2, f2, lab, T, Wm, so.Hyper(num_classes=Cn, open_classes=K)


def test_view_losses_with_the_identity_map_is_simt_losses_exactly():
    B, K, h, w, H, W = 3, 3, 5, 7, 33, 49
    p1, p2, f2, lab, T, Wm, hp = _loss_inputs(B, K, h, w, H, W)
    want = so.simt_losses(p1, p2, f2, lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W))
    ident = np.arange(B, dtype=np.uint8)[:, None, None] * np.ones((B, H, W), np.uint8)
    for item in (None, ident):
        got = wt.view_losses(p1, p2, f2, lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W), item=item)
        assert got.keys() == want.keys()
        for k in want:
            assert torch.equal(got[k], want[k]), k
    up = so.upsample(p2, (H, W))
    prob = so.upsample(torch.softmax(f2, 1), (H, W))
    want1 = so.simt_losses_single(up, prob, lab, T[1], Wm[1], hp)
    for item in (None, ident):
        got1 = wt.view_losses_single(up, prob, lab, T[1], Wm[1], hp, item=item)
        assert got1.keys() == want1.keys() and all(torch.equal(got1[k], want1[k]) for k in want1)


def test_view_losses_with_a_rolled_map_is_simt_losses_on_the_rolled_frozen_logits_and_a_mixed_map_moves_the_labels():
    B, K, h, w, H, W = 3, 3, 5, 7, 33, 49
    p1, p2, f2, lab, T, Wm, hp = _loss_inputs(B, K, h, w, H, W)
    roll = [(i + 1) % B for i in range(B)]
    rolled = np.array(roll, dtype=np.uint8)[:, None, None] * np.ones((B, H, W), np.uint8)
    want = so.simt_losses(p1, p2, f2[roll], lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W))
    got = wt.view_losses(p1, p2, f2, lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W), item=rolled)
    assert all(torch.equal(got[k], want[k]) for k in want)
    base = so.simt_losses(p1, p2, f2, lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W))
    blocks = (np.add.outer(np.arange(H) // 8, np.arange(W) // 8) % 2).astype(bool)
    mixed = np.where(blocks[None], rolled, np.arange(B, dtype=np.uint8)[:, None, None])
    got = wt.view_losses(p1, p2, f2, lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W), item=mixed)
    sel = torch.from_numpy(np.broadcast_to(blocks[None], (B, H, W)).copy())
    assert torch.equal(got["conf0"], torch.where(sel, want["conf0"], base["conf0"]))
    assert not torch.equal(got["conf0"], base["conf0"]) and not torch.equal(got["conf0"], want["conf0"])
    # an out-of-range byte reads the last item
    high = mixed.copy()
    high[mixed == B - 1] = 200
    again = wt.view_losses(p1, p2, f2, lab, T[0], T[1], Wm[0], Wm[1], hp, (H, W), item=high)
    assert all(torch.equal(again[k], got[k]) for k in got)


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------
def test_loader_refuses_teacher_view_without_an_augmentation():
    from simt_amd.data.pipeline import GpuLoader

    class Ds:
        crop_size, mean, files = (8, 8), (0.0, 0.0, 0.0), []
        class_mix = photometric = scale_crop = None
        teacher_view = True

        def __len__(self):
            return 4
    with pytest.raises(ValueError) as e:
        GpuLoader(Ds(), 2, device="cpu")
    assert all(f in str(e.value) for f in ("--class-mix", "--colour-jitter", "--gaussian-blur", "teacher_view"))
    ds = Ds()
    ds.teacher_view = False
    assert GpuLoader(ds, 2, device="cpu").teacher_view is False
    for kw in ({"class_mix": (19, 1.0)}, {"photometric": (0.2, None)}):
        ds = Ds()
        for k, v in kw.items():
            setattr(ds, k, v)
        assert GpuLoader(ds, 2, device="cpu").teacher_view is True


# ---- train state on fake trainers ---------------------------------------------------------------------------------------------------------------
def _FakeView(teacher_view=False, seed=0):
    """test_ema_cpu._Fake with the keyword's attribute, as the SimT trainers set it (same class: the state names its trainer)."""
    tr = _Fake(seed=seed)
    tr.teacher_view = teacher_view
    return tr


def test_load_training_state_refuses_the_keyword_added_or_dropped(no_device_sync):
    with_v = _advanced(_FakeView(True)).training_state()
    without = _advanced(_FakeView(False)).training_state()
    assert with_v["hyper"]["teacher_view"] is True and "teacher_view" not in without["hyper"]
    assert "teacher_view" in tsf.SWITCH_FIELDS and "teacher_view" not in tsf.CHECKED_FIELDS
    assert {k: v for k, v in with_v["hyper"].items() if k != "teacher_view"} == without["hyper"]          # the views are inputs: nothing else is stored
    assert with_v.keys() == without.keys()
    _refused(_FakeView(False, seed=1), with_v, "teacher_view", "state: True", "this trainer: None")      # dropped
    _refused(_FakeView(True, seed=1), without, "teacher_view", "state: None", "this trainer: True")      # added
    _refused(_Fake(seed=1), with_v, "teacher_view")                                                       # a trainer from before the keyword
    for ts, tr in ((with_v, _FakeView(True, seed=1)), (without, _FakeView(False, seed=1)), (without, _Fake(seed=1))):
        tr.load_training_state(ts)
        assert tr.it_done == 3
    assert tsf.switch_mismatches({}, {}) == [] and tsf.switch_mismatches({"teacher_view": False}, {}) == []
    assert tsf.switch_mismatches({"teacher_view": True}, {}) == ["teacher_view"] == tsf.switch_mismatches({}, {"teacher_view": True})
