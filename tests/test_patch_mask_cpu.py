"""Host side of --mask-patches (simt_amd/data/patch_mask.py, the tools' flags, the descriptor's layout, the loader's acceptance, the
restatement's own properties and the limits of the GPU test's cases): no GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch  # noqa: F401  (before any test swaps ctypes.CDLL: _lib.load imports it)

import _patch_mask_ref as ref
from simt_amd.data import patch_mask as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()

# (B, h, w, P) of tests/test_gpu_patch_mask.py: the last one goes through InputPrep.patch_mask_batch, which splits at 16
SHAPES = [(2, 24, 40, 8), (5, 17, 23, 8), (3, 16, 16, 6), (1, 32, 128, 4), (1, 128, 32, 4), (17, 8, 8, 4)]
MASKS = ("random", "kept", "blanked", "checkerboard", "last_patch", "garbage")


def grid(h, w, P):
    return -(-h // P), -(-w // P)


def mask_words(kind, B, h, w, P, seed=9):
    """The row words of one named mask of the GPU test, [B, 32] uint32."""
    gh, gw = grid(h, w, P)
    rng = np.random.default_rng([seed, B, h, w, P])
    m = np.zeros((B, gh, gw), bool)
    if kind in ("random", "garbage"):
        m = rng.random((B, gh, gw)) < 0.7
    elif kind == "blanked":
        m[:] = True
    elif kind == "checkerboard":
        m[:] = (np.add.outer(np.arange(gh), np.arange(gw)) % 2 == 0)[None]
    elif kind == "last_patch":
        m[:, gh - 1, gw - 1] = True
    else:
        assert kind == "kept"
    words = pm.pack_rows(m)
    if kind == "garbage":                  # ones and noise where the contract says "ignored": columns >= gw, rows >= gh
        noise = rng.integers(0, 2 ** 32, (B, ref.GRID), dtype=np.uint64).astype(np.uint32)
        keep = np.uint32((1 << gw) - 1) if gw < 32 else np.uint32(0xFFFFFFFF)
        words[:, :gh] |= noise[:, :gh] & ~keep
        words[:, gh:] = noise[:, gh:] | np.uint32(1)
    return words


def special_bits(B, h, w, seed=4):
    """[B, 3, h, w] uint32: finite values with NaNs of several payloads, -0.0, both infinities and denormals sprinkled in."""
    rng = np.random.default_rng([seed, B, h, w])
    x = (rng.standard_normal((B, 3, h, w)) * 60).astype(np.float32).view(np.uint32).copy()
    special = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000],
                       dtype=np.uint32)
    pick = rng.random(x.shape) < 0.2
    x[pick] = rng.choice(special, size=int(pick.sum()))
    x.reshape(-1)[:special.size] = special          # each of them at least once
    return x


# ---- header and descriptor ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbol_and_the_descriptor_matches_ctypes():
    from simt_amd import _lib as L
    assert re.search(r"int simt_patch_mask\(const simt_patch_mask_desc\* d, simt_stream_t stream\);", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    fields = [n for n, _t in L.PatchMaskDesc._fields_]
    assert fields == ["x", "x_out", "B", "h", "w", "patch", "rows"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(simt_patch_mask_desc));' +
           "".join(f'printf("{n} %zu\\n", offsetof(simt_patch_mask_desc, {n}));' for n in fields) +
           'printf("row %zu\\n", sizeof(((simt_patch_mask_desc*)0)->rows[0]));'
           'printf("max %d %d\\n", SIMT_PATCH_MASK_MAX, SIMT_PATCH_MASK_GRID);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe])
        out = dict(ln.split(None, 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    assert C.sizeof(L.PatchMaskDesc) == int(out["size"]) < 4096          # it travels as kernel arguments
    for n in fields:
        assert getattr(L.PatchMaskDesc, n).offset == int(out[n]), n
    assert int(out["row"]) == 4 * L.PATCH_MASK_GRID
    assert out["max"].split() == [str(L.PATCH_MASK_MAX), str(L.PATCH_MASK_GRID)] == ["16", "32"]
    assert (pm.MAX_ITEMS, pm.MAX_GRID, ref.GRID) == (L.PATCH_MASK_MAX, L.PATCH_MASK_GRID, L.PATCH_MASK_GRID)
    assert L.SIGNATURES["simt_patch_mask"] == (C.c_int, [C.POINTER(L.PatchMaskDesc), C.c_void_p])


def test_a_library_without_the_symbol_names_it(monkeypatch):
    """A libsimt_hip.so built before the symbol was added has the same ABI version: loading must name the symbol and say to rebuild."""
    from simt_amd import _lib as L

    class Old:
        def __getattr__(self, name):
            if name == "simt_patch_mask":
                raise AttributeError(name)
            return lambda *a: L.ABI_VERSION
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(L, "LIB_PATH", __file__)
    with pytest.raises(L.SimtHipError, match=r"simt_patch_mask\b.*rebuild"):
        L.load()


# ---- parse ----------------------------------------------------------------------------------------------------------------------------------
def test_parse_accepts_and_refuses_and_names_what_is_wrong():
    assert pm.parse("0.7", 64, (1024, 512)) == (64, 0.7, 8, 16)
    assert pm.parse(0.5, "32", (1024, 512)) == (32, 0.5, 16, 32)
    assert pm.parse("0.01", 1, (32, 32)) == (1, 0.01, 32, 32) and pm.parse(0.99, 7, (23, 17)) == (7, 0.99, 3, 4)
    assert pm.parse("0.7", 64, (2048, 1024)) == (64, 0.7, 16, 32)
    for ratio, named in [("0", r"--mask-patches '0'"), ("1", r"--mask-patches '1'"), (1.0, r"--mask-patches 1\.0"), ("1.5", r"--mask-patches '1\.5'"),
                         ("-0.2", r"--mask-patches '-0\.2'"), ("nan", r"--mask-patches 'nan'"), ("x", r"--mask-patches 'x' is not a ratio"),
                         (None, r"--mask-patches None")]:
        with pytest.raises(ValueError, match=named):
            pm.parse(ratio, 64, (1024, 512))
    for patch, named in [(0, r"--mask-patch-size 0\b"), ("0", r"--mask-patch-size '0'"), (-4, r"--mask-patch-size -4"),
                         ("x", r"--mask-patch-size 'x' is not an integer"), ("6.5", r"--mask-patch-size '6\.5' is not an integer"),
                         (6.5, r"--mask-patch-size 6\.5 is not an integer")]:
        with pytest.raises(ValueError, match=named):
            pm.parse("0.7", patch, (1024, 512))
    with pytest.raises(ValueError, match=r"--mask-patch-size 32: a crop of 2048 x 1024 needs 64 x 32 patches.*--mask-patch-size 64 or larger would fit"):
        pm.parse("0.7", 32, (2048, 1024))
    with pytest.raises(ValueError, match=r"needs 2 x 33 patches.*--mask-patch-size 17 or larger"):
        pm.parse("0.7", 16, (32, 528))
    assert pm.parse("0.7", 17, (32, 528))[2:] == (32, 2)          # ... and the size the message names does fit


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------
def test_draws_are_deterministic_per_seed_and_rank_and_equal_the_documented_order():
    B, gh, gw = 4, 8, 16
    a = [pm.draw_batch(g, B, gh, gw, 0.7) for g in [pm.generator(7, 0)] for _ in range(3)]
    b = [pm.draw_batch(g, B, gh, gw, 0.7) for g in [pm.generator(7, 0)] for _ in range(3)]
    c = [pm.draw_batch(g, B, gh, gw, 0.7) for g in [pm.generator(7, 1)] for _ in range(3)]
    d = [ref.draws(g, B, gh, gw, 0.7) for g in [ref.generator(7, 0)] for _ in range(3)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and all(np.array_equal(p, q) for p, q in zip(a, d))
    assert not any(np.array_equal(p, q) for p, q in zip(a, c)), "ranks 0 and 1 drew the same masks"
    assert not np.array_equal(pm.draw_batch(pm.generator(8, 0), B, gh, gw, 0.7), a[0])
    assert not np.array_equal(a[0], a[1])
    for words in a + c:
        assert words.dtype == np.uint32 and words.shape == (B, 32)
        assert not (words[:, :gh] >> gw).any() and not words[:, gh:].any()          # unused bits of a row word, unused row words: 0
    share = np.mean([pm.blanked_share(wd, 512, 1024, 64).mean() for wd in a + c])
    assert 0.6 < share < 0.8                                                       # about R of the pixels
    assert pm.draw_batch(pm.generator(1, 0), 2, 32, 32, 0.999).dtype == np.uint32   # bit 31 fits


def test_the_generator_is_nobodys_else():
    """Not the loader's, the mix's or the photometric step's: the same seed and rank give other numbers in each of the four streams."""
    from simt_amd.data import class_mix as cm
    from simt_amd.data import photometric as ph
    first = [g.random(8) for g in (pm.generator(7, 0), cm.generator(7, 0), ph.generator(7, 0), np.random.default_rng(7), np.random.default_rng(7 + 7919 * 0))]
    assert len({cm.STREAM_TAG, ph.STREAM_TAG, pm.STREAM_TAG, ref.STREAM_TAG}) == 3 and pm.STREAM_TAG == ref.STREAM_TAG
    for i in range(1, len(first)):
        assert not np.array_equal(first[0], first[i])
    # ... and drawing masks moves none of the others: they are separate objects seeded apart
    g_mix = cm.generator(7, 0)
    before = g_mix.bit_generator.state
    pm.draw_batch(pm.generator(7, 0), 4, 8, 16, 0.7)
    assert g_mix.bit_generator.state == before


@pytest.mark.parametrize("ratio", [0.7, 0.01, 0.99])
def test_skipping_equals_consuming_the_draws_whatever_the_ratio(ratio):
    B, gh, gw = 3, 5, 9
    for n in (0, 1, 5):
        a, b = pm.generator(11, 2), pm.generator(11, 2)
        drawn = [pm.draw_batch(a, B, gh, gw, ratio) for _ in range(n + 1)]
        pm.skip_draws(b, B, n, gh, gw)
        assert np.array_equal(pm.draw_batch(b, B, gh, gw, ratio), drawn[n])          # skip(n), then a draw = the (n + 1)-th draw
        assert a.bit_generator.state == b.bit_generator.state
    a, b = pm.generator(11, 2), pm.generator(11, 2)
    pm.draw_batch(a, B, gh, gw, 0.01)
    pm.draw_batch(b, B, gh, gw, 0.99)
    assert a.bit_generator.state == b.bit_generator.state                          # the number of draws depends on neither R nor the values


# ---- the restatement and the GPU test's cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_cases_are_within_the_limits_and_the_restatement_agrees_with_itself(shape):
    from simt_amd import _lib as L
    B, h, w, P = shape
    gh, gw = grid(h, w, P)
    assert gh <= L.PATCH_MASK_GRID and gw <= L.PATCH_MASK_GRID and h * w < 2 ** 31
    assert B <= L.PATCH_MASK_MAX or shape == SHAPES[-1]           # the last one is split by InputPrep.patch_mask_batch: 16 + 1
    assert pm.parse("0.7", P, (w, h)) == (P, 0.7, gh, gw)
    x = special_bits(B, h, w)
    assert {0x7FC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001} <= set(x.reshape(-1).tolist())
    for kind in MASKS:
        words = mask_words(kind, B, h, w, P)
        want = ref.out_of_place(x, words, P)
        assert np.array_equal(ref.in_place(x.copy(), words, P), want)              # in place = out of place
        m = ref.mask_pixels(words, h, w, P)
        assert m.shape == (B, h, w)
        for p in range(3):
            assert not want[:, p][m].any() and np.array_equal(want[:, p][~m], x[:, p][~m])
        if kind == "kept":
            assert not m.any() and np.array_equal(want, x)
        elif kind == "blanked":
            assert m.all() and not want.any()
        elif kind == "last_patch":
            assert m[:, (gh - 1) * P:, (gw - 1) * P:].all() and int(m[0].sum()) == (h - (gh - 1) * P) * (w - (gw - 1) * P)
        elif kind == "checkerboard":
            assert m[:, 0, 0].all() and (gw < 2 or not m[:, 0, P].any())
        elif kind == "garbage":                                                     # the ignored bits are ignored
            clean = mask_words("random", B, h, w, P)
            assert not np.array_equal(words, clean) and np.array_equal(ref.mask_pixels(clean, h, w, P), m)
        else:
            assert m.any() and not m.all()
    if shape == (1, 32, 128, 4):
        assert (mask_words("blanked", *shape)[:, :8] >> 31).all()                  # bit 31 of a row word is used
    if shape == (1, 128, 32, 4):
        assert mask_words("blanked", *shape)[:, 31].all() and ref.mask_pixels(mask_words("last_patch", *shape), 128, 32, 4)[0, 127, 31]
    if shape == (5, 17, 23, 8):
        assert (h - (gh - 1) * P, w - (gw - 1) * P) == (1, 7)                      # a one-row and a seven-column edge patch


def test_restatement_against_a_per_pixel_loop():
    rng = np.random.default_rng(3)
    for _ in range(20):
        B, h, w, P = int(rng.integers(1, 4)), int(rng.integers(1, 20)), int(rng.integers(1, 20)), int(rng.integers(1, 9))
        if max(-(-h // P), -(-w // P)) > 32:
            continue
        words = rng.integers(0, 2 ** 32, (B, 32), dtype=np.uint64).astype(np.uint32)
        x = rng.integers(1, 2 ** 32, (B, 3, h, w), dtype=np.uint64).astype(np.uint32)
        want = x.copy()
        for i in range(B):
            for y in range(h):
                for xx in range(w):
                    if (int(words[i, y // P]) >> (xx // P)) & 1:
                        want[i, :, y, xx] = 0
        assert np.array_equal(ref.out_of_place(x, words, P), want)


# ---- the tools' flags --------------------------------------------------------------------------------------------------------------------------
def _args(tool, *extra):
    return tool.get_arguments(list(extra))


def test_both_tools_parse_the_flags_and_refuse_bad_values(capsys):
    from simt_amd.tools import trainV1_warmup, trainV2_simt
    for tool in (trainV1_warmup, trainV2_simt):
        a = _args(tool)
        assert a.mask_patches is None and a.mask_patch_size is None and trainV2_simt.patch_mask_setting(a) is None
        assert trainV2_simt.patch_mask_setting(_args(tool, "--mask-patches")) == (64, 0.7)                       # MIC's defaults
        assert trainV2_simt.patch_mask_setting(_args(tool, "--mask-patches", "0.5", "--mask-patch-size", "32")) == (32, 0.5)
        assert trainV2_simt.patch_mask_setting(_args(tool, "--mask-patches", "--input-size-target", "2048,1024")) == (64, 0.7)
        for extra, named in [(["--mask-patch-size", "32"], "--mask-patch-size needs --mask-patches"),
                             (["--mask-patches", "0"], "--mask-patches '0'"), (["--mask-patches", "1"], "--mask-patches '1'"),
                             (["--mask-patches", "nan"], "--mask-patches 'nan'"), (["--mask-patches", "x"], "--mask-patches 'x'"),
                             (["--mask-patches", "--mask-patch-size", "0"], "--mask-patch-size '0'"),
                             (["--mask-patches", "--mask-patch-size", "32", "--input-size-target", "2048,1024"], "--mask-patch-size 64 or larger"),
                             (["--mask-patches", "--mask-patch-size", "8"], "--mask-patch-size 32 or larger")]:
            with pytest.raises(SystemExit) as e:
                _args(tool, *extra)
            err = capsys.readouterr().err
            assert e.value.code == 2 and named in err, (extra, err)


def test_weak_teacher_is_satisfied_by_the_mask_alone_and_its_refusal_keeps_the_sentence(capsys):
    from simt_amd.tools import trainV2_simt as tool
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        a = _args(tool, "--model", model, "--weak-teacher", "--mask-patches")
        assert a.weak_teacher is True and a.mask_patches == "0.7"
    for argv in (["--weak-teacher"], ["--weak-teacher", "--mask-patches", "--synthetic"]):
        with pytest.raises(SystemExit) as e:
            _args(tool, *argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--weak-teacher needs --class-mix, --colour-jitter or --gaussian-blur" in err and "--mask-patches" in err
    tool.weak_teacher_line(_args(tool, "--weak-teacher", "--mask-patches"))
    out = capsys.readouterr().out
    assert "--mask-patches" in out and "no item map" in out
    tool.patch_mask_line(_args(tool, "--weak-teacher", "--mask-patches"))
    assert capsys.readouterr().out == ""
    tool.patch_mask_line(_args(tool, "--mask-patches"))
    assert "both models see the masked image" in capsys.readouterr().out
    tool.patch_mask_line(_args(tool))
    tool.patch_mask_line(_args(tool, "--mask-patches", "--synthetic"))
    assert capsys.readouterr().out == ""


def test_synthetic_says_once_that_the_flag_does_nothing(capsys):
    from simt_amd.tools import trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    assert tool.batches(_args(tool, "--synthetic", "--mask-patches", "0.5"), 2, 8, 8, cd, 0, 1, "cpu") is not None
    assert "--mask-patches does nothing with --synthetic" in capsys.readouterr().out
    tool.batches(_args(tool, "--synthetic"), 1, 8, 8, cd, 0, 1, "cpu")
    assert "mask-patches" not in capsys.readouterr().out


def test_run_identity_holds_the_pair_and_a_resume_that_differs_is_refused(tmp_path):
    import torch

    from simt_amd import train_state
    from simt_amd.tools import trainV1_warmup, trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    lst = tmp_path / "list.lst"
    lst.write_text("a b\n")
    base = ["--data-list-target", str(lst), "--batch-size", "2"]
    off = tool.run_identity(_args(tool, *base), cd)
    on = tool.run_identity(_args(tool, *base, "--mask-patches", "0.5", "--mask-patch-size", "32"), cd)
    assert "patch_mask" not in off and tool.RUN_DEFAULTS["patch_mask"] is False and on["patch_mask"] == [32, 0.5]      # absent = False
    assert tool.run_identity(_args(tool, *base, "--mask-patches"), cd)["patch_mask"] == [64, 0.7]
    assert {k: v for k, v in on.items() if k != "patch_mask"} == off
    assert "patch_mask" not in tool.run_identity(_args(tool, *base, "--mask-patches", "0.5", "--synthetic"), cd)        # it does nothing there
    assert tool.run_identity(_args(trainV1_warmup, *base, "--mask-patches"), cd)["patch_mask"] == [64, 0.7]

    class Tr:
        it_done = 0

        def load_training_state(self, ts):
            self.it_done = ts["it_done"]

    keeper = tool.SnapshotKeeper(str(tmp_path), "x")
    path = str(tmp_path / "run.state")
    flags = ["--mask-patches", "0.5", "--mask-patch-size", "32"]
    train_state.save(path, {"it_done": 3, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": on})
    assert tool.TrainStateFile(_args(tool, *base, *flags, "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 3
    for other in (["--mask-patches", "0.25", "--mask-patch-size", "32"], ["--mask-patches", "0.5"], ["--mask-patches", "0.5", "--mask-patch-size", "128"], []):
        with pytest.raises(SystemExit, match=r"differs in: patch_mask \(state: \[32, 0\.5\]"):           # another R, another P, dropped
            tool.TrainStateFile(_args(tool, *base, *other, "--train-state", path), 0, 1, cd).resume(Tr(), keeper)
    # a state file from before the key existed lacks it and still loads with the flag off; with the flag added it is refused
    train_state.save(path, {"it_done": 2, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": off})
    assert tool.TrainStateFile(_args(tool, *base, "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 2
    with pytest.raises(SystemExit, match=r"differs in: patch_mask \(state: False, this run: \[64, 0\.7\]"):
        tool.TrainStateFile(_args(tool, *base, "--mask-patches", "--train-state", path), 0, 1, cd).resume(Tr(), keeper)


# ---- datasets and loader ----------------------------------------------------------------------------------------------------------------------
def test_datasets_store_the_pair(tmp_path):
    from simt_amd.dataset.cityscapes_dataset import cityscapesDataSet, cityscapesPseudo
    lst = tmp_path / "l.lst"
    lst.write_text("a.png b.png\n")
    assert cityscapesPseudo(str(tmp_path), str(lst)).patch_mask is None
    assert cityscapesPseudo(str(tmp_path), str(lst), patch_mask=("64", "0.7")).patch_mask == (64, 0.7)
    one = tmp_path / "one.lst"
    one.write_text("a.png\n")
    assert cityscapesDataSet(str(tmp_path), str(one)).patch_mask is None
    assert cityscapesDataSet(str(tmp_path), str(one), patch_mask=(32, 0.5)).patch_mask == (32, 0.5)


def test_loader_accepts_teacher_view_with_the_mask_alone_and_its_refusal_keeps_its_words():
    from simt_amd.data.pipeline import GpuLoader

    class Ds:
        crop_size, mean, files = (40, 24), (0.0, 0.0, 0.0), []
        class_mix = photometric = scale_crop = patch_mask = None
        teacher_view = True

        def __len__(self):
            return 4
    with pytest.raises(ValueError) as e:
        GpuLoader(Ds(), 2, device="cpu")
    assert all(f in str(e.value) for f in ("--class-mix", "--colour-jitter", "--gaussian-blur", "teacher_view", "--mask-patches"))
    ds = Ds()
    ds.patch_mask = (8, 0.7)
    loader = GpuLoader(ds, 2, device="cpu")
    assert loader.teacher_view is True and loader.patch_mask == (8, 0.7, 3, 5) and loader.class_mix is None and loader.photometric is None
    ds.teacher_view = False
    assert GpuLoader(ds, 2, device="cpu").patch_mask == (8, 0.7, 3, 5)
    # start_batch skips the mask's draws: the loader's generator stands where n batches' draws leave it
    skipped = GpuLoader(ds, 2, device="cpu", start_batch=3)._mask_rng
    assert skipped.bit_generator.state == pm.skip_draws(pm.generator(1234, 0), 2, 3, 3, 5).bit_generator.state
    assert skipped.bit_generator.state != pm.generator(1234, 0).bit_generator.state
    for bad, named in (((1, 0.7), "--mask-patch-size 1:"), ((8, 1.0), "--mask-patches 1.0")):
        ds.patch_mask = bad
        with pytest.raises(ValueError, match=named):
            GpuLoader(ds, 2, device="cpu")
