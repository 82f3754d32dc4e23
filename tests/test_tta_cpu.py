"""CPU checks of test-time augmentation (simt_tta_label's host side; no GPU): the float64 restatement tests/_tta_ref.py the GPU tests
use as their yardstick, against torch's bilinear interpolate; the term list; both command lines; the argument checks that must come
before any plan is built; the ctypes mirrors of the two descriptors against the header."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tta_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("hw", [(5, 7), (9, 12), (1, 3)])
def test_reference_one_term_is_interpolate_align_corners(hw):
    rng = np.random.default_rng(0)
    l = rng.standard_normal((2, *hw, 19))
    for (H, W) in ((17, 23), (1, 1), (4, 40)):
        ref = _nhwc(F.interpolate(_nchw(l), size=(H, W), mode="bilinear", align_corners=True))
        assert np.abs(R.term_value(l, H, W) - ref).max() <= 1e-12
        s, arg, top, gap = R.combine([(l, False, (0, 0))], H, W, 0)
        assert np.array_equal(s, R.term_value(l, H, W)) and np.array_equal(arg, np.argmax(ref, 3)) and np.all(gap >= 0)


def test_reference_flipped_term_on_reversed_map_is_the_plain_term():
    rng = np.random.default_rng(1)
    l = rng.standard_normal((2, 6, 9, 19))
    rev = np.ascontiguousarray(l[:, :, ::-1])
    assert np.array_equal(R.term_value(rev, 17, 23, flip=True), R.term_value(l, 17, 23))
    # mirroring the label-size result instead is the same map up to rounding only (the weights of pixel x and W-1-x round differently)
    assert np.abs(R.term_value(l, 17, 23, flip=True) - R.term_value(l, 17, 23)[:, :, ::-1]).max() < 1e-12


def test_reference_two_resample_flip_mirrors_the_virtual_map():
    """Two-resample family: a flipped term is the one-resample flipped term applied to the virtual [hi][wi] map."""
    rng = np.random.default_rng(4)
    l = rng.standard_normal((1, 6, 9, 5))
    v = R.resample_half(l, 13, 18)
    assert np.array_equal(R.term_value(l, 17, 23, flip=True, hiwi=(13, 18)), R.term_value(np.ascontiguousarray(v[:, :, ::-1]), 17, 23))


@pytest.mark.parametrize("geo", [((5, 7), (11, 15)), ((9, 12), (19, 25)), ((6, 9), (4, 5))])
def test_reference_two_resamples_are_interpolate_twice(geo):
    (h, w), (hi, wi) = geo
    rng = np.random.default_rng(2)
    l = rng.standard_normal((2, h, w, 19))
    mid = F.interpolate(_nchw(l), size=(hi, wi), mode="bilinear", align_corners=False)
    ref = _nhwc(F.interpolate(mid, size=(17, 23), mode="bilinear", align_corners=True))
    assert np.abs(R.term_value(l, 17, 23, hiwi=(hi, wi)) - ref).max() <= 1e-12


def test_reference_combination_order_and_mean():
    rng = np.random.default_rng(3)
    ls = [rng.standard_normal((1, 5, 7, 4)), rng.standard_normal((1, 6, 9, 4)), rng.standard_normal((1, 9, 12, 4))]
    terms = [(ls[0], False, (0, 0)), (ls[1], True, (0, 0)), (ls[2], False, (0, 0))]
    s0 = R.combine(terms, 8, 9, 0)[0]
    assert np.array_equal(s0, (R.term_value(ls[0], 8, 9) + R.term_value(ls[1], 8, 9, True)) + R.term_value(ls[2], 8, 9))
    s1, arg, top, gap = R.combine(terms, 8, 9, 1)
    assert np.array_equal(s1, s0 * (1.0 / 3)) and np.array_equal(top, s1.max(3)) and np.array_equal(arg, s1.argmax(3))


def test_shared_inputs_are_usable():
    """What tests/test_gpu_tta.py asserts on its reference before it looks at the GPU, for the seed it uses: at most 1 of the 782 pixels
    inside a margin, at least 10 labels, pixels on both sides of the 0.8 threshold."""
    maps = R.make_logits(5)
    assert [m.shape for m in maps] == [(2, 5, 7, 19), (2, 6, 9, 19), (2, 9, 12, 19), (2, 5, 7, 19), (2, 6, 9, 19)]
    for n in (1, 3, 5):
        for fam2 in (False, True):
            terms = [(maps[i], R.FLIPS[i], R.HIWI[i % 3] if fam2 else (0, 0)) for i in range(n)]
            s, arg, top, gap = R.combine(terms, R.H, R.W, 0)
            assert (gap < 1e-4 * (1 + np.abs(top))).sum() <= 1 and len(np.unique(arg)) >= 10
    for n in (2, 4):
        terms = [(R.softmax32(maps[i]), R.FLIPS[i], (0, 0)) for i in range(n)]
        s, arg, top, gap = R.combine(terms, R.H, R.W, 1)
        assert ((gap < 1e-5) | (np.abs(top - 0.8) < 1e-5)).sum() <= 1
        assert 20 <= (top > 0.8).sum() <= top.size - 20 and top.min() < 0.35 and top.max() > 0.95      # both sides of the threshold occur


# ---- term list and command lines -----------------------------------------------------------------------------------------------------
def test_tta_terms_order_and_limit():
    from simt_amd import _lib, ops
    assert ops.TTA_MAX == _lib.TTA_MAX == 8
    assert ops.tta_terms([(512, 1024), (640, 1280)]) == [(512, 1024, False), (640, 1280, False)]
    assert ops.tta_terms([(512, 1024), (640, 1280)], True) == [(512, 1024, False), (512, 1024, True), (640, 1280, False), (640, 1280, True)]
    assert len(ops.tta_terms([(8, 8)] * 8)) == 8 and len(ops.tta_terms([(8, 8)] * 4, True)) == 8
    for scales, flip in (([(8, 8)] * 9, False), ([(8, 8)] * 5, True), ([], False)):
        with pytest.raises(ValueError):
            ops.tta_terms(scales, flip)


def test_make_pseudo_labels_command_line():
    from simt_amd.tools import make_pseudo_labels as mpl
    base = ["--restore-from", "x.pth"]
    a = mpl.get_arguments(base)
    assert not a.tta and not a.tta_flip
    a = mpl.get_arguments(base + ["--tta", "--input-size", "96,48", "--input-size", "128,64", "--input-size", "160,80", "--threshold", "0.8"])
    assert a.tta and not a.tta_flip and len(a.input_size) == 3
    a = mpl.get_arguments(base + ["--tta-flip", "--class-balanced", "0.5"])
    assert a.tta and a.tta_flip, "--tta-flip implies --tta"
    with pytest.raises(SystemExit):                      # 5 scales x mirror = 10 terms
        mpl.get_arguments(base + ["--tta-flip"] + [v for i in range(5) for v in ("--input-size", f"{64 + 16 * i},{32 + 8 * i}")])
    with pytest.raises(SystemExit):                      # mode 1 of the two-resample family is not built
        mpl.get_arguments(base + ["--arch", "v3", "--tta", "--threshold", "0.8"])
    assert mpl.get_arguments(base + ["--arch", "v3", "--tta-flip"]).tta


def test_test_tool_command_line():
    from simt_amd.tools import test as tt
    a = tt.get_arguments([])
    assert a.eval_scales is None and not a.eval_flip
    a = tt.get_arguments(["--eval-scales", "1024,512", "1280,640", "1536,768", "--eval-flip", "--model", "DeepLabv3"])
    assert a.eval_scales == [(1024, 512), (1280, 640), (1536, 768)] and a.eval_flip
    with pytest.raises(SystemExit):
        tt.get_arguments(["--eval-scales", "1024x512"])
    with pytest.raises(SystemExit):
        tt.get_arguments(["--eval-flip", "--eval-scales"] + ["64,32"] * 5)


def test_argument_checks_come_before_any_plan():
    """No GPU and no state here: a refusal that came after the plans were built would fail differently."""
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    from simt_amd.tools.make_pseudo_labels import PseudoLabeller
    for mode in ("confidence", "class_balanced"):
        with pytest.raises(ValueError, match="two-resample"):
            PseudoLabeller({}, arch="v3", mode=mode, tta=True, device="cpu")
    with pytest.raises(ValueError, match="tta"):
        PseudoLabeller({}, flip=True, device="cpu")
    with pytest.raises(ValueError, match="at most 8"):
        PseudoLabeller({}, scales=[(32, 64)] * 5, tta=True, flip=True, device="cpu")
    with pytest.raises(ValueError, match="at most 8"):
        Evaluator({}, scales=[(32, 64)] * 9, device="cpu")
    with pytest.raises(ValueError, match="at most 8"):
        Evaluator({}, scales=[(32, 64)] * 5, flip=True, device="cpu")


def test_thresholds_record_lists_the_terms():
    from simt_amd.tools import make_pseudo_labels as mpl
    hist = np.zeros((2, mpl.CONF_BINS), np.int64)
    hist[:, 200] = 5
    kw = dict(portion=0.5, cap=0.9, data_list="l.txt")
    assert "tta_terms" not in mpl.thresholds_record(np.zeros(2, np.float32), [5, 5, 0], hist, **kw)
    rec = mpl.thresholds_record(np.zeros(2, np.float32), [5, 5, 0], hist, terms=[(48, 96, False), (48, 96, True)], **kw)
    assert rec["tta_terms"] == [{"h": 48, "w": 96, "flip": False}, {"h": 48, "w": 96, "flip": True}]


# ---- descriptor layout ----------------------------------------------------------------------------------------------------------------
def test_tta_ctypes_struct_sizes_match_header():
    """sizeof of both descriptors as a C compiler lays out the header's field lists (the probe of tests/test_host_logic.py)."""
    from simt_amd import _lib
    structs = {"simt_tta_term": _lib.TtaTerm, "simt_tta_desc": _lib.TtaDesc}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in structs) + (
        'printf("off_n %zu\\n", offsetof(simt_tta_desc, n));printf("off_thr %zu\\n", offsetof(simt_tta_desc, thr));'
        'printf("off_hist %zu\\n", offsetof(simt_tta_desc, hist));return 0;}')
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "p.c"), os.path.join(td, "p")
        open(cpath, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    for n, cls in structs.items():
        assert C.sizeof(cls) == sizes[n], f"{n}: ctypes {C.sizeof(cls)} vs C {sizes[n]}"
    assert (_lib.TtaDesc.n.offset, _lib.TtaDesc.thr.offset, _lib.TtaDesc.hist.offset) == (sizes["off_n"], sizes["off_thr"], sizes["off_hist"])
    assert [n for n, _ in _lib.TtaTerm._fields_] == ["l", "h", "w", "ld", "hi", "wi", "flip"]
    assert _lib.TTA_MAX == int(re.search(r"#define SIMT_TTA_MAX (\d+)", open(os.path.join(ROOT, "include", "simt_hip.h")).read()).group(1))
    assert "simt_tta_label" in _lib.SIGNATURES
