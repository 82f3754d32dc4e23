"""Host side of --colour-jitter / --gaussian-blur (simt_amd/data/photometric.py, the tools' flags, the descriptor's layout, the
restatement's own properties): no GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _photometric_ref as ref
from simt_amd.data import photometric as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
MEAN = (104.00698793, 116.66876762, 122.67891434)
F = np.float32
U = 2.0 ** -24          # the unit roundoff of float32


def test_header_declares_the_symbols_and_the_descriptor_matches_ctypes():
    """sizeof / offsetof of simt_photometric_desc from a compiled C program against the ctypes mirror; symbols added, the ABI version stays."""
    from simt_amd import _lib as L
    assert re.search(r"int\s+simt_grey_mean_parts\s*\(", HDR) and re.search(r"int\s+simt_photometric\s*\(", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    fields = [n for n, _t in L.PhotometricDesc._fields_]
    assert fields == ["x", "x_out", "part", "inv", "B", "h", "w", "mean", "fb", "fc", "omfc", "A", "wk", "jit", "blur"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(simt_photometric_desc));' +
           "".join(f'printf("{n} %zu\\n", offsetof(simt_photometric_desc, {n}));' for n in fields) +
           'printf("max %d %d\\n", SIMT_PHOTOMETRIC_MAX, SIMT_PHOTOMETRIC_PARTS);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe])
        out = dict(ln.split(None, 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    assert C.sizeof(L.PhotometricDesc) == int(out["size"]) < 4096          # it travels as kernel arguments
    for n in fields:
        assert getattr(L.PhotometricDesc, n).offset == int(out[n]), n
    assert out["max"].split() == [str(L.PHOTOMETRIC_MAX), str(L.PHOTOMETRIC_PARTS)] == ["32", "64"]
    assert ph.MAX_ITEMS == L.PHOTOMETRIC_MAX and ph.RADIUS == ref.RADIUS == 5
    assert "simt_grey_mean_parts" in L.SIGNATURES and "simt_photometric" in L.SIGNATURES
    assert L.PhotometricDesc.A.size == 32 * 36 and L.PhotometricDesc.wk.size == 32 * 24


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def test_parse_refuses_bad_values_and_names_them():
    assert ph.parse() is None and ph.parse(None, None) is None
    assert ph.parse("0.2", None) == (0.2, None) and ph.parse(None, "0.5") == (None, 0.5) and ph.parse(0.5, 1) == (0.5, 1.0)
    for jit, blur, named in [("0", None, r"--colour-jitter '0'"), ("0.6", None, r"--colour-jitter '0\.6'.*\(0, 0\.5\]"),
                             ("x", None, r"--colour-jitter 'x' is not a strength"), ("nan", "0.5", r"--colour-jitter 'nan'"),
                             ("-0.1", None, r"--colour-jitter '-0\.1'"), (None, "0", r"--gaussian-blur '0'"),
                             ("0.2", "1.5", r"--gaussian-blur '1\.5'.*\(0, 1\]"), (None, "p", r"--gaussian-blur 'p' is not a probability"),
                             (None, "nan", r"--gaussian-blur 'nan'")]:
        with pytest.raises(ValueError, match=named):
            ph.parse(jit, blur)


def _args(tool, *extra):
    return tool.get_arguments(list(extra))


def test_cli_parses_the_flags_on_both_tools_and_exits_on_bad_values():
    from simt_amd.tools import trainV1_warmup, trainV2_simt
    for tool in (trainV1_warmup, trainV2_simt):
        a = _args(tool)
        assert a.colour_jitter is None and a.gaussian_blur is None and trainV2_simt.photometric_setting(a) is None
        assert trainV2_simt.photometric_setting(_args(tool, "--colour-jitter")) == (0.2, None)          # either flag alone
        assert trainV2_simt.photometric_setting(_args(tool, "--gaussian-blur")) == (None, 0.5)
        assert trainV2_simt.photometric_setting(_args(tool, "--colour-jitter", "0.5", "--gaussian-blur", "1")) == (0.5, 1.0)
        for extra, named in [(["--colour-jitter", "0"], r"--colour-jitter '0'"), (["--colour-jitter", "0.51"], r"--colour-jitter '0\.51'"),
                             (["--gaussian-blur", "0"], r"--gaussian-blur '0'"), (["--gaussian-blur", "1.01"], r"--gaussian-blur '1\.01'"),
                             (["--colour-jitter", "--gaussian-blur", "x"], r"--gaussian-blur 'x'")]:
            with pytest.raises(SystemExit, match=named):
                trainV2_simt.photometric_setting(_args(tool, *extra))


def test_synthetic_says_once_that_the_flags_do_nothing(capsys):
    from simt_amd.tools import trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    assert tool.batches(_args(tool, "--synthetic", "--gaussian-blur"), 1, 8, 8, cd, 0, 1, "cpu") is not None
    assert "--colour-jitter / --gaussian-blur do nothing with --synthetic" in capsys.readouterr().out
    tool.batches(_args(tool, "--synthetic"), 1, 8, 8, cd, 0, 1, "cpu")
    assert "jitter" not in capsys.readouterr().out


def test_run_identity_holds_the_pair_and_a_resume_that_differs_is_refused(tmp_path):
    import torch

    from simt_amd import train_state
    from simt_amd.tools import trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    lst = tmp_path / "list.lst"
    lst.write_text("a b\n")
    base = ["--data-list-target", str(lst)]
    both = ["--colour-jitter", "--gaussian-blur"]
    off = tool.run_identity(_args(tool, *base), cd)
    on = tool.run_identity(_args(tool, *base, *both), cd)
    assert "photometric" not in off and tool.RUN_DEFAULTS["photometric"] is False and on["photometric"] == [0.2, 0.5]       # absent = False
    assert tool.run_identity(_args(tool, *base, "--colour-jitter", "0.3"), cd)["photometric"] == [0.3, None]
    assert tool.run_identity(_args(tool, *base, "--gaussian-blur", "1"), cd)["photometric"] == [None, 1.0]
    assert {k: v for k, v in on.items() if k != "photometric"} == off
    assert "photometric" not in tool.run_identity(_args(tool, *base, *both, "--synthetic"), cd)                            # they do nothing there

    class Tr:
        it_done = 0

        def load_training_state(self, ts):
            self.it_done = ts["it_done"]

    keeper = tool.SnapshotKeeper(str(tmp_path), "x")
    path = str(tmp_path / "run.state")
    train_state.save(path, {"it_done": 3, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": on})
    assert tool.TrainStateFile(_args(tool, *base, *both, "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 3
    for other in (["--colour-jitter", "0.3", "--gaussian-blur"], ["--colour-jitter"], ["--gaussian-blur"], []):
        with pytest.raises(SystemExit, match=r"differs in: photometric \(state: \[0\.2, 0\.5\]"):
            tool.TrainStateFile(_args(tool, *base, *other, "--train-state", path), 0, 1, cd).resume(Tr(), keeper)
    # a state file from before the key existed lacks it and still loads with the flags off
    train_state.save(path, {"it_done": 2, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": off})
    assert tool.TrainStateFile(_args(tool, *base, "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 2
    with pytest.raises(SystemExit, match=r"differs in: photometric \(state: False, this run: \[None, 0\.5\]"):
        tool.TrainStateFile(_args(tool, *base, "--gaussian-blur", "--train-state", path), 0, 1, cd).resume(Tr(), keeper)


def test_dataset_stores_the_pair(tmp_path):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    lst = tmp_path / "l.lst"
    lst.write_text("a.png b.png\n")
    assert cityscapesPseudo(str(tmp_path), str(lst)).photometric is None
    assert cityscapesPseudo(str(tmp_path), str(lst), photometric=("0.2", None)).photometric == (0.2, None)


# ---- draws -----------------------------------------------------------------------------------------------------------------------------
SETTINGS = [(0.2, 0.5), (0.5, None), (None, 1.0)]


def _same_draws(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


def test_draws_are_seven_per_item_whatever_the_settings_and_equal_the_documented_order():
    B = 5
    states = []
    for st in SETTINGS:
        g, r, plain = ph.generator(7, 0), ref.generator(7, 0), ref.generator(7, 0)
        for _ in range(3):
            d = ph.draw_batch(g, B, st)
            assert _same_draws(d, ref.draws(r, B, *st))
            u = plain.random((7, B))                                            # exactly 7 * B doubles, in this order
            S, P = st
            s = S or 0.0
            assert np.array_equal(d["jit"], (u[0] < 0.8) & (S is not None)) and np.array_equal(d["blur"], (u[5] < P) if P else np.zeros(B, bool))
            assert np.array_equal(d["fb"], (1 - s) + 2 * s * u[1]) and np.array_equal(d["theta"], -s + 2 * s * u[4])
            assert np.array_equal(d["sigma"], 0.15 + u[6])
            assert d["jit"].dtype == np.bool_ and d["blur"].dtype == np.bool_ and all(d[k].shape == (B,) for k in d)
            if S is not None:
                assert ((d["fb"] >= 1 - S) & (d["fb"] <= 1 + S) & (d["fc"] >= 1 - S) & (d["fc"] <= 1 + S) & (d["fs"] >= 1 - S)
                        & (d["fs"] <= 1 + S) & (np.abs(d["theta"]) <= S)).all()
            assert ((d["sigma"] >= 0.15) & (d["sigma"] <= 1.15)).all()
        assert g.bit_generator.state == plain.bit_generator.state
        states.append(g.bit_generator.state)
    assert states[0] == states[1] == states[2]
    a, b = ph.draw_batch(ph.generator(7, 0), B, SETTINGS[0]), ph.draw_batch(ph.generator(7, 1), B, SETTINGS[0])
    assert not np.array_equal(a["fb"], b["fb"]), "ranks 0 and 1 drew the same factors"
    assert not np.array_equal(ph.draw_batch(ph.generator(8, 0), B, SETTINGS[0])["fb"], a["fb"])
    off_jit = ph.draw_batch(ph.generator(7, 0), 64, (None, 1.0))
    assert not off_jit["jit"].any() and off_jit["blur"].all()
    on = ph.draw_batch(ph.generator(7, 0), 64, (0.2, None))
    assert on["jit"].any() and not on["jit"].all() and not on["blur"].any()


@pytest.mark.parametrize("settings", SETTINGS)
def test_skipping_equals_consuming_the_draws(settings):
    B = 3
    for n in (0, 1, 5):
        a, b = ph.generator(11, 2), ph.generator(11, 2)
        for _ in range(n):
            ph.draw_batch(a, B, settings)
        ph.skip_draws(b, B, n)
        assert a.bit_generator.state == b.bit_generator.state
        assert _same_draws(ph.draw_batch(a, B, settings), ph.draw_batch(b, B, settings))


def test_the_class_mix_and_loader_generators_are_untouched_by_the_flag():
    """The photometric generator is a third stream: for one seed and rank its numbers are neither the loader's nor the mix's, and drawing
    from it moves neither."""
    from simt_amd.data import class_mix as cm
    assert ph.STREAM_TAG == ref.TAG != cm.STREAM_TAG
    mix, loader, photo = cm.generator(7, 0), np.random.default_rng(7), ph.generator(7, 0)
    before = (mix.bit_generator.state, loader.bit_generator.state)
    first = photo.random(4)
    ph.draw_batch(photo, 4, (0.2, 0.5))
    assert (mix.bit_generator.state, loader.bit_generator.state) == before
    assert not np.array_equal(first, mix.random(4)) and not np.array_equal(first, loader.random(4))


# ---- parameters ------------------------------------------------------------------------------------------------------------------------
def test_blur_weights():
    for sigma in (0.15, 0.3, 0.6, 0.9, 1.15):
        wk = ph.blur_weights(sigma)
        assert wk.dtype == F and wk.shape == (6,) and (wk >= 0).all() and (np.diff(wk) <= 0).all()
        # six roundings of at most U relative each, of terms that sum to 1: within one float32 rounding of 1
        assert abs(float(wk[0].astype(np.float64) + 2.0 * wk[1:].astype(np.float64).sum()) - 1.0) <= 2 * U
        e = np.exp(-np.arange(6.0) ** 2 / (2 * sigma * sigma))
        assert np.array_equal(wk == 0, e < 2.0 ** -24), "a weight under 2^-24 is exactly 0, every other one is not"
        assert not ((wk != 0) & (wk < 2.0 ** -26)).any()                # (normalising divides by at most 1 + 2 * 5: nothing near a denormal)
        assert np.array_equal(wk, ref.params(1, 1, 1, 0, sigma)[4])
    assert np.array_equal(ph.blur_weights(0.15), np.array([1, 0, 0, 0, 0, 0], F))      # exp(-1 / 0.045) = 2.2e-10 < 2^-24: the identity
    e = np.exp(-np.arange(6.0) ** 2 / (2 * 1.15 ** 2))
    assert (e >= 2.0 ** -24).all()
    assert np.array_equal(ph.blur_weights(1.15), (e / (e[0] + 2 * e[1:].sum())).astype(F))
    assert abs(float(ph.blur_weights(1.15)[0]) - 0.346907) < 1e-6 and abs(float(ph.blur_weights(1.15)[5]) - 2.7249e-05) < 1e-9


def test_colour_matrix():
    assert np.array_equal(ph.colour_matrix(1.0, 0.0), np.eye(3, dtype=F))              # exactly the identity
    wg = np.array([0.114, 0.587, 0.299])
    grid = [(fs, th) for fs in (0.5, 0.8, 1.0, 1.2, 1.5) for th in (-0.5, -0.2, -0.01, 0.0, 0.13, 0.5)]
    for fs, th in grid:
        A = ph.colour_matrix(fs, th)
        assert A.dtype == F and A.shape == (3, 3)
        assert np.array_equal(A, ref.params(1, 1, fs, th, 1)[3]), (fs, th)
        assert np.abs(A.astype(np.float64) @ np.ones(3) - 1.0).max() <= 4 * U, "grey maps to grey"      # three roundings per row
        H = ph.hue_matrix(th)
        assert np.abs(wg @ H - wg).max() < 1e-12, "the hue turn keeps the grey value"
        assert np.abs(H @ ph.hue_matrix(-th) - np.eye(3)).max() < 1e-12
    assert np.abs(ph.hue_matrix(0.25) @ ph.hue_matrix(0.25) - ph.hue_matrix(0.5)).max() < 1e-12
    assert np.abs(ph.hue_matrix(0.5) - (2 * np.outer(np.ones(3), wg) - np.eye(3))).max() < 1e-12          # half a turn: v -> 2 grey(v) - v
    assert np.abs(ph.hue_matrix(1.0) - np.eye(3)).max() < 1e-12
    # fs = 0 would be grey: every row of A(0, 0) is wg (not reachable, S <= 0.5, but it says what fs means)
    assert np.abs(ph.colour_matrix(0.0, 0.0) - np.tile(wg, (3, 1))).max() <= U
    # planes are B, G, R: a positive turn moves pure red (plane 2) towards YIQ's +Q side exactly as the RGB-order matrix does
    rgb = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
    a = 2 * np.pi * 0.1
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    want = (np.linalg.inv(rgb) @ rot @ rgb)[::-1, ::-1]
    assert np.abs(ph.hue_matrix(0.1) - want).max() < 1e-12


def test_item_params_are_float32_and_omfc_is_of_the_rounded_fc():
    rng = np.random.default_rng(3)
    for _ in range(50):
        fb, fc, fs, th, sg = 0.5 + rng.random(), 0.5 + rng.random(), 0.5 + rng.random(), rng.random() - 0.5, 0.15 + rng.random()
        got, want = ph.item_params(fb, fc, fs, th, sg), ref.params(fb, fc, fs, th, sg)
        for g, w in zip(got, want):
            assert np.asarray(g).dtype == F and np.array_equal(g, w)
        assert got[0] == F(fb) and got[1] == F(fc) and got[2] == F(1.0 - float(F(fc))) and got[2] == F(1) - F(fc)
    assert ph.inv_pixels(37, 41) == 1.0 / (65536.0 * 37 * 41)


# ---- the restatement means what it claims --------------------------------------------------------------------------------------------
def _frame(rng, h, w):
    """uint8 colours minus the mean, a zero border as scale-crop leaves one, a few values far outside (every clamp)."""
    x = rng.integers(0, 256, (3, h, w)).astype(F) - np.array(MEAN, F)[:, None, None]
    x[:, :1, :] = 0
    x[:, :, -1:] = 0
    x[:, h // 2, w // 2] = -300
    x[:, h // 2, w // 2 - 1] = 400
    return x


def _bound(x, fb, fc, omfc, A, jit):
    """|restatement - float64| per output value, from the operation count.  Each float32 operation adds at most U times the magnitude of
    its result; clamps, and a blur pass (weights >= 0 that sum to 1), do not amplify an error; brightness amplifies by fb, contrast by fc,
    the matrix by its largest absolute row sum LA.  The 16-bit grey mean adds its own 2^-17 through |omfc|."""
    vmax = float(np.abs(x.astype(np.float64) + np.array(MEAN)[:, None, None]).max()) / 255.0
    e = 2 * U * max(vmax, 1.0)                              # x + mean, then * c255
    if jit:
        fb, fc, om = float(fb), float(fc), abs(float(omfc))
        LA = float(np.abs(A).sum(axis=1).max())
        e = fb * e + U * fb                                 # brightness: one product of at most fb
        em = e + 5 * U + 2.0 ** -17 + U                     # grey: 3 products, 2 adds of values <= 1; the rounding to 16 bits; m's own rounding
        e = fc * e + om * em + 3 * U * (fc + om)            # two products, one add
        e = LA * e + 5 * U * LA                             # three products, two adds of partial sums <= LA
    e = e + 2 * 31 * U                                      # per pass: 5 x (neighbour sum <= 2, product, add) + the first product, all <= 2
    return 255.0 * e + 2 * 255.0 * U                        # v * 255, then - mean


@pytest.mark.parametrize("hw", [(6, 6), (13, 22), (37, 41)], ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_float64(hw):
    h, w = hw
    rng = np.random.default_rng([4, h, w])
    worst = 0.0
    for fb, fc, fs, th, sg in [(0.5, 0.5, 0.5, -0.5, 0.15), (1.5, 1.5, 1.5, 0.5, 1.15), (1, 1, 1, 0, 0.6), (0.8, 1.2, 0.9, 0.07, 0.9),
                               (1.2, 0.8, 1.5, -0.3, 0.4)]:
        x = _frame(rng, h, w)
        p = ref.params(fb, fc, fs, th, sg)
        for jit, blur in ((1, 0), (0, 1), (1, 1)):
            got, S, m = ref.item(x, MEAN, jit, blur, *p)
            want = ref.float64_item(x, MEAN, jit, blur, *p)
            assert got.dtype == F and got.shape == x.shape
            err, bound = float(np.abs(got.astype(np.float64) - want).max()), _bound(x, *p[:4], jit)
            assert err <= bound, (fb, fc, fs, th, sg, jit, blur, err, bound)
            worst = max(worst, err / bound)
            assert (got.astype(np.float64) + np.array(MEAN)[:, None, None] >= -1e-4).all()          # clamped: a colour in [0, 255]
            assert (got.astype(np.float64) + np.array(MEAN)[:, None, None] <= 255 + 1e-4).all()
            if jit:
                assert 0 <= S <= 65537 * h * w and m == F(S / (65536.0 * h * w))
    assert worst > 1e-4, "the bound is not vacuous"


def test_restatement_copies_constant_frames_and_blur_only_identity():
    rng = np.random.default_rng(9)
    mean = np.array(MEAN, F)[:, None, None]
    ident = ref.params(1, 1, 1, 0, 0.15)
    # neither flag: the input, bit for bit -- NaN payloads and -0.0 included
    bits = rng.integers(-2 ** 31, 2 ** 31, (3, 9, 11), dtype=np.int64).astype(np.int32)
    bits[0, 0, 0], bits[1, 2, 3] = np.int32(-2 ** 31), np.int32(0x7FC12345)
    out, S, m = ref.item(bits.view(F), MEAN, 0, 0, *ident)
    assert np.array_equal(out.view(np.int32), bits) and S is None and m is None
    # a constant frame stays constant under blur, to the blur's own rounding: per pass 31 operations of at most 2 U each (see _bound)
    for sigma in (0.15, 0.6, 1.15):
        for colour in ((10.0, 200.0, 90.0), (0.0, 255.0, 128.0)):
            x = np.broadcast_to(np.array(colour, F)[:, None, None], (3, 12, 17)) - mean
            out, _S, _m = ref.item(np.ascontiguousarray(x), MEAN, 0, 1, *ref.params(1, 1, 1, 0, sigma))
            want = ref.item(np.ascontiguousarray(x), MEAN, 0, 1, *ident)[0]          # sigma 0.15: weights (1, 0, ...): normalise + back only
            assert np.abs(out.astype(np.float64) - want).max() <= 255.0 * 2 * 31 * 2 * U + 2 * 255.0 * U
            for p in range(3):
                assert np.ptp(out[p]) <= 255.0 * 2 * 31 * 2 * U + 255.0 * U
    # the identity parameters with jitter on change a frame by rounding only (m drops out: omfc = 0)
    x = _frame(rng, 8, 9)
    x[:, 4, 4], x[:, 4, 3] = 7.0, -9.0
    got = ref.item(x, MEAN, 1, 0, *ident)[0]
    want = ref.item(x, MEAN, 0, 1, *ident)[0]
    assert np.array_equal(got, want)
    # reflection without repeating the edge: a frame that is a ramp along x blurs to the mirror-extended ramp's blur
    wk = ref.params(1, 1, 1, 0, 1.15)[4]
    ramp = np.tile(np.arange(8, dtype=F) / F(8), (6, 1))
    left = ref.blur_pass(ramp, wk, 1)[0, 0]
    acc = wk[0] * ramp[0, 0]
    for k in range(1, 6):
        acc = acc + wk[k] * (ramp[0, k] + ramp[0, k])
    assert left == acc


def test_loader_validates_the_pair_like_the_flags():
    """GpuLoader passes dataset.photometric through `parse`: a strength or probability outside its range is refused by name, before any
    device work."""
    from simt_amd.data.pipeline import GpuLoader

    class Dataset:
        crop_size, mean = (8, 8), MEAN

        def __init__(self, photometric):
            self.photometric = photometric

        def __len__(self):
            return 4
    assert GpuLoader(Dataset((0.5, 1.0)), 2, device="cpu").photometric == (0.5, 1.0)
    assert GpuLoader(Dataset(("0.2", None)), 2, device="cpu").photometric == (0.2, None)
    assert GpuLoader(Dataset(None), 2, device="cpu").photometric is None
    for pair, named in [((0.9, None), r"--colour-jitter 0\.9"), ((0.2, 1.5), r"--gaussian-blur 1\.5"), ((None, None), r"\(None, None\)")]:
        with pytest.raises(ValueError, match=named):
            GpuLoader(Dataset(pair), 2, device="cpu")
