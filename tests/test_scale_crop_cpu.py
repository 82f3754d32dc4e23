"""Host side of --scale-crop (simt_amd/data/scale_crop.py, the tools' flag, the descriptor's layout): no GPU needed."""
import ctypes as C
import math
import os
import subprocess
import tempfile
import types
from fractions import Fraction

import numpy as np
import pytest

import _scale_crop_ref as ref
from simt_amd.data import resample as rs
from simt_amd.data import scale_crop as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scaled_sizes_come_from_the_decimal_text():
    """floor(n * s + 1/2) in exact arithmetic: 1024 * 0.7 = 716.8 -> 717; 513 * 0.5 = 256.5 -> 257 (the half rounds up); 65 * 1.5 = 97.5
    -> 98; 5 * 0.1 = 0.5 -> 1, where the binary float product 0.5000000000000000277 would agree only by luck; 1000 * 0.0005 -> 1."""
    assert sc.scaled_size(1024, "0.7") == 717 and sc.scaled_size(512, "0.7") == 358
    assert sc.scaled_size(513, "0.5") == 257 and sc.scaled_size(65, "1.5") == 98 and sc.scaled_size(129, "0.5") == 65
    assert sc.scaled_size(5, "0.1") == 1 and sc.scaled_size(1000, "0.0005") == 1 and sc.scaled_size(1000, "0.0004") == 0
    assert sc.scaled_size(1024, "1.0") == 1024 and sc.scaled_size(1024, "1") == 1024
    for n in (1, 7, 72, 513, 1024):
        for c in sc.DEFAULT_CHOICES + ("0.35", "2.5", "0.15"):
            assert sc.scaled_size(n, c) == math.floor(n * Fraction(c) + Fraction(1, 2)) == ref.scaled(n, c)
    # 45 * 0.7 = 31.5 exactly -> 32; the binary float 0.7 lies below 7/10 and 45 * 0.7 + 0.5 = 31.999999999999996: the text decides
    assert sc.scaled_size(45, "0.7") == 32 and math.floor(45 * 0.7 + 0.5) == 31
    assert sc.scaled_size(25, "0.58") == 15 and math.floor(25 * 0.58 + 0.5) == 14


def test_choices_default_limit_and_refusals():
    assert sc.parse_choices([]) == sc.DEFAULT_CHOICES == tuple(f"{k / 10:.1f}" for k in range(5, 16)) and len(sc.DEFAULT_CHOICES) == 11
    assert sc.parse_choices(["0.5", "2"]) == ("0.5", "2")
    assert len(sc.parse_choices(["1.0"] * 16)) == 16
    with pytest.raises(ValueError, match="at most 16"):
        sc.parse_choices(["1.0"] * 17)
    for bad in ("0", "-1", "abc", "1/2", "nan", ""):
        with pytest.raises(ValueError, match="not a positive decimal"):
            sc.parse_choices([bad])


def test_origin_ranges_and_origins_stay_inside():
    assert sc.origin_range(108, 72) == (0, 36) and sc.origin_range(36, 72) == (-36, 0) and sc.origin_range(72, 72) == (0, 0)
    top = 1.0 - 2.0 ** -53                                        # the largest value Generator.random can return
    assert top < 1.0
    for lo, hi in [(0, 36), (-36, 0), (0, 0), (0, 512), (-1023, 0), (0, 2 ** 40), (0, 2 ** 53), (0, 2 ** 60)]:
        assert sc.origin(0.0, lo, hi) == lo
        assert sc.origin(top, lo, hi) == hi or hi - lo >= 2 ** 40            # (a double cannot name every origin of so wide a range)
        for u in (0.25, 0.5, 0.999999, top):
            assert lo <= sc.origin(u, lo, hi) <= hi
    # every origin of a small range is reached, uniformly: u in [k / n, (k + 1) / n) -> lo + k
    assert [sc.origin((k + 0.5) / 5, -2, 2) for k in range(5)] == [-2, -1, 0, 1, 2]


@pytest.mark.parametrize("mirror", [False, True])
def test_skipping_equals_consuming_the_draws(mirror):
    choices, crop, B = ("0.5", "1.0", "1.5"), (72, 40), 3
    a, b = np.random.default_rng(9), np.random.default_rng(9)
    for _ in range(4):
        sc.draw_batch(a, B, choices, crop, mirror)
    sc.skip_scale_crop_draws(b, B, 4, len(choices), mirror)
    assert a.bit_generator.state == b.bit_generator.state
    assert sc.draw_batch(a, B, choices, crop, mirror) == sc.draw_batch(b, B, choices, crop, mirror)
    # the documented order and the test-side restatement of it
    c, d = np.random.default_rng(9), np.random.default_rng(9)
    assert sc.draw_batch(c, B, choices, crop, mirror) == ref.draws(d, B, choices, crop, mirror)


def test_mirror_draw_is_the_first_of_every_batch_and_the_one_the_loader_always_made():
    """One generator serves all draws, in batch order, so the scale-crop draws of batch k lie between the mirror draws of batches k and
    k + 1: with scale-crop on, batch 0's flags ARE those of the loader without it for the same seed, and every later batch's flags are
    what the old draw, `integers(0, 2, B) == 0`, gives at that point of the stream."""
    B = 4
    off = np.random.default_rng(1234)
    on = np.random.default_rng(1234)
    first_off = (off.integers(0, 2, B) == 0).tolist()
    flags, _pick, _ox, _oy = sc.draw_batch(on, B, ("0.5", "1.5"), (72, 40), True)
    assert flags == first_off
    twin = np.random.default_rng(1234)
    sc.skip_scale_crop_draws(twin, B, 1, 2, True)
    expect = (twin.integers(0, 2, B) == 0).tolist()
    assert sc.draw_batch(on, B, ("0.5", "1.5"), (72, 40), True)[0] == expect
    # mirroring off: no mirror draw is made at all
    g, k = np.random.default_rng(5), np.random.default_rng(5)
    fl, pick, _x, _y = sc.draw_batch(g, B, ("0.5", "1.5"), (72, 40), False)
    assert fl == [False] * B and pick == k.integers(0, 2, B).tolist()


@pytest.mark.parametrize("geom", [((96, 160), (72, 40), ("0.5", "1.0", "1.5", "2.0", "2.5")), ((96, 160), (73, 41), ("0.5", "2.5")),
                                  ((96, 192), (129, 65), ("0.5", "1.5")), ((1024, 2048), (1024, 512), ("0.5", "1.0", "1.5"))])
def test_worst_row_span_equals_brute_force_over_tiles(geom):
    (Hs, Ws), (w, h), choices = geom
    t = sc.Tables((Hs, Ws), (w, h), choices)
    worst = 0
    for c in choices:
        hs = ref.scaled(h, c)
        _k, by, _c = rs.bicubic_tables(Hs, hs)
        lo, hi = ref.origin_range(hs, h)
        for oy in range(lo, hi + 1):
            for y0 in range(0, h, 16):
                a, e = max(0, y0 + oy), min(hs, min(y0 + 16, h) + oy)
                if a < e:
                    worst = max(worst, int(by[e - 1, 0] + by[e - 1, 1] - by[a, 0]))
    assert t.max_rows == worst and 0 < worst <= Hs
    if (Hs, Ws) == (1024, 2048):
        assert worst == 76 and t.lds_bytes() == 76 * 192 + 4 * (64 * 17 + 16 * 17) <= 65536      # DESIGN: the Cityscapes arithmetic
    # the offsets tile the one buffer, in order, without gaps
    off = 0
    for e in t.entries:
        for name, n in (("bounds_x", 2 * e["ws"]), ("coef_x", e["ws"] * e["ksx"]), ("bounds_y", 2 * e["hs"]), ("coef_y", e["hs"] * e["ksy"]),
                        ("xtab", e["ws"]), ("ytab", e["hs"])):
            assert e[name] == off
            off += n
    assert off == t.data.size and t.data.dtype == np.int32


def _args(tool, *extra):
    return tool.get_arguments(list(extra))


def test_cli_parses_the_flag_on_both_tools():
    from simt_amd.tools import trainV1_warmup, trainV2_simt
    for tool in (trainV1_warmup, trainV2_simt):
        a = _args(tool)
        assert a.scale_crop is None and trainV2_simt.scale_crop_choices(a) is None and a.random_scale is False
        a = _args(tool, "--scale-crop")
        assert a.scale_crop == [] and trainV2_simt.scale_crop_choices(a) == sc.DEFAULT_CHOICES
        a = _args(tool, "--scale-crop", "0.5", "1.25", "--random-scale", "--batch-size", "2")
        assert trainV2_simt.scale_crop_choices(a) == ("0.5", "1.25") and a.random_scale is True and a.batch_size == 2
        with pytest.raises(SystemExit, match="--scale-crop"):
            trainV2_simt.scale_crop_choices(_args(tool, "--scale-crop", "fast"))
        with pytest.raises(SystemExit, match="at most 16"):
            trainV2_simt.scale_crop_choices(_args(tool, "--scale-crop", *["1.0"] * 17))


def test_run_identity_holds_the_choices_and_a_resume_with_others_is_refused(tmp_path):
    import torch

    from simt_amd import train_state
    from simt_amd.tools import trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    lst = tmp_path / "list.lst"
    lst.write_text("a b\n")
    base = ["--data-list-target", str(lst)]
    off = tool.run_identity(_args(tool, *base), cd)
    on = tool.run_identity(_args(tool, *base, "--scale-crop", "0.5", "1.5"), cd)
    assert "scale_crop" not in off and tool.RUN_DEFAULTS["scale_crop"] is False and on["scale_crop"] == ["0.5", "1.5"]      # absent = False
    assert tool.run_identity(_args(tool, *base, "--scale-crop"), cd)["scale_crop"] == list(sc.DEFAULT_CHOICES)
    assert {k: v for k, v in on.items() if k != "scale_crop"} == {k: v for k, v in off.items() if k != "scale_crop"}
    assert "scale_crop" not in tool.run_identity(_args(tool, *base, "--scale-crop", "0.5", "--synthetic"), cd)      # it does nothing there

    class Tr:
        it_done = 0

        def load_training_state(self, ts):
            self.it_done = ts["it_done"]

    keeper = tool.SnapshotKeeper(str(tmp_path), "x")
    path = str(tmp_path / "run.state")
    train_state.save(path, {"it_done": 3, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": on})
    ok = tool.TrainStateFile(_args(tool, *base, "--scale-crop", "0.5", "1.5", "--train-state", path), 0, 1, cd)
    assert ok.resume(Tr(), keeper) == 3
    for other in (["--scale-crop", "0.5", "1.0"], []):
        with pytest.raises(SystemExit, match=r"differs in: scale_crop \(state: \['0\.5', '1\.5'\]"):
            tool.TrainStateFile(_args(tool, *base, *other, "--train-state", path), 0, 1, cd).resume(Tr(), keeper)
    # a state file from before the key existed lacks it and still loads: it is the state of a run without scale-crop
    assert set(off) == {"random_seed", "random_mirror", "synthetic", "class_dist_sha256", "data_list_sha256"}
    train_state.save(path, {"it_done": 2, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": off})
    assert tool.TrainStateFile(_args(tool, *base, "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 2
    with pytest.raises(SystemExit, match=r"differs in: scale_crop \(state: False"):
        tool.TrainStateFile(_args(tool, *base, "--scale-crop", "--train-state", path), 0, 1, cd).resume(Tr(), keeper)


def test_synthetic_says_once_that_the_flag_does_nothing(capsys):
    from simt_amd.tools import trainV2_simt as tool
    a = _args(tool, "--synthetic", "--scale-crop", "0.5")
    it = tool.batches(a, 1, 8, 8, np.full(19, 1 / 19, np.float32), 0, 1, "cpu")
    assert "--scale-crop does nothing with --synthetic" in capsys.readouterr().out and it is not None
    tool.batches(_args(tool, "--synthetic"), 1, 8, 8, np.full(19, 1 / 19, np.float32), 0, 1, "cpu")
    assert "scale-crop" not in capsys.readouterr().out


def test_descriptor_ctypes_size_matches_the_header():
    """The struct-size pattern of tests/test_host_logic.py for the new descriptors; under 4 KB: it travels as kernel arguments."""
    from simt_amd import _lib as L
    structs = {"simt_scale_crop_desc": L.ScaleCropDesc, "simt_scale_crop_choice": L.ScaleCropChoice}
    src = '#include <stdio.h>\n#include "simt_hip.h"\nint main(void){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in structs) + (
        'printf("max %d %d %d\\n", SIMT_SCALE_CROP_MAX, SIMT_SCALE_CROP_CHOICES, SIMT_SCALE_CROP_LDS_MAX);'
        'printf("tile %d %d\\n", SIMT_SCALE_CROP_TILE_H, SIMT_SCALE_CROP_TILE_W);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe])
        out = dict(ln.split(None, 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    for n, cls in structs.items():
        assert C.sizeof(cls) == int(out[n]), f"{n}: ctypes {C.sizeof(cls)} vs C {out[n]}"
    assert C.sizeof(L.ScaleCropDesc) < 4096
    assert out["max"].split() == [str(L.SCALE_CROP_MAX), str(L.SCALE_CROP_CHOICES), str(L.SCALE_CROP_LDS_MAX)]
    assert out["tile"].split() == [str(sc.TILE_H), str(sc.TILE_W)] and sc.MAX_CHOICES == L.SCALE_CROP_CHOICES
    assert "simt_scale_crop" in L.SIGNATURES and "simt_scale_crop_lds_bytes" in L.SIGNATURES and L.ABI_VERSION == 2
