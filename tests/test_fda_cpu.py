"""--fda without a GPU: the band identity behind csrc/fda.hip, the band and the tables of simt_amd/data/fda.py, the bindings, the
tool's flag, its refusals and its place in the run identity, and that the GPU test's comparator (tests/_fda_ref.py) rejects planted mistakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _fda_ref as fr
from simt_amd import _lib as L
from simt_amd.data import fda

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "simt_hip.h")).read()
MEAN = fr.IMG_MEAN


@pytest.fixture(scope="module")
def cases():
    """Per geometry, computed once: the uniform inputs of the GPU test and a dark source / bright target pair, with the published result and
    the fp32 restatement's error for each."""
    out = {}
    for g in fr.GEOMETRIES:
        B, h, w, _beta, b, seed = g
        for kind, rng in (("uniform", (0, 256, 0, 256)), ("dark-bright", (0, 100, 100, 256))):
            xs, xt = fr.inputs(B, h, w, seed, *rng)
            full = fr.fda_full(xs, xt, MEAN, b)
            err32 = float(np.abs(fr.fda_band(xs, xt, MEAN, b, np.float32) - full).max())
            out[fr.geo_id(g), kind] = (xs, xt, full, err32)
    return out


@pytest.mark.parametrize("g", fr.GEOMETRIES, ids=fr.geo_id)
def test_band_form_is_the_published_form(cases, g):
    """The source plus a band-limited polynomial IS fft2 / swap / ifft2: 1e-9 grey levels in float64, and the sequential fp32 restatement
    lies a few 1e-5 away -- the scale of the GPU test's bar."""
    B, h, w, beta, b, _seed = g
    assert fda.band(h, w, beta) == b
    for kind in ("uniform", "dark-bright"):
        xs, xt, full, err32 = cases[fr.geo_id(g), kind]
        assert np.abs(fr.fda_band(xs, xt, MEAN, b) - full).max() <= 1e-9
        assert 0 < err32 < 1e-3, err32


@pytest.mark.parametrize("g", fr.GEOMETRIES, ids=fr.geo_id)
def test_seeds_are_well_conditioned(g):
    B, h, w, _beta, b, seed = g
    xs, xt = fr.inputs(B, h, w, seed)
    assert fr.kappa(xs, xt, MEAN, b) <= fr.KAPPA_MAX


@pytest.mark.parametrize("fault", fr.FAULTS)
@pytest.mark.parametrize("g", [g for g in fr.GEOMETRIES if g[4] >= 1], ids=fr.geo_id)
def test_the_comparator_bites(cases, g, fault):
    """Each planted mistake lies far outside the GPU test's bar, 4 * err32 + 2^-22 * max|out|, at every geometry with b >= 1.  The uniform inputs
    of the GPU test show four of them.  The fifth, the mean not added back, they CANNOT show: it only moves the DC coefficient, whose swap is
    |F_T| * sign(F_S) - F_S, and a plane of uniform grey levels minus the mean has a positive DC on both sides, for which that is F_T - F_S with
    or without the mean.  A dark source beside a bright target (DC below the mean on one side, above it on the other) shows all five."""
    B, h, w, _beta, b, _seed = g
    for kind in ("uniform", "dark-bright"):
        if fault == "no_mean" and kind == "uniform":
            continue
        xs, xt, full, err32 = cases[fr.geo_id(g), kind]
        wrong = float(np.abs(fr.fda_band(xs, xt, MEAN, b, np.float32, fault) - full).max())
        assert wrong > 100 * fr.bar(err32, full), (kind, wrong, fr.bar(err32, full))


def test_zero_amplitude_rule():
    """A plane with S = T = 0 comes back bit for bit with no NaN (p = 1 where |F_S| == 0), in both forms."""
    xs, xt = fr.inputs(1, 24, 40, 5)
    m = np.asarray(MEAN, dtype=np.float32)
    xs[0, 1], xt[0, 1] = -m[1], -m[1]
    out = fr.fda_band(xs, xt, MEAN, 2, np.float32)
    assert np.isfinite(out).all() and np.array_equal(out[0, 1], xs[0, 1])
    assert np.abs(fr.fda_full(xs, xt, MEAN, 2)[0, 1] - xs[0, 1]).max() < 1e-9


def test_band_and_tables():
    assert fda.band(768, 768, 0.01) == 7 and fda.band(512, 1024, 0.09) == 46 and fda.band(65, 129, 0.01) == 0 and fda.band(9, 516, 0.2) == 1
    for h, w in ((9, 516), (33, 47), (64, 64)):
        tw_h, tw_w = fda.twiddle_tables(h, w)
        assert tw_h.dtype == tw_w.dtype == np.float32 and tw_h.shape == (h, 2) and tw_w.shape == (w, 2)
        ref_h, ref_w = fr.tables(h, w)
        assert np.array_equal(tw_h, ref_h) and np.array_equal(tw_w, ref_w)
        assert tw_w[0, 0] == 1.0 and tw_w[0, 1] == 0.0
        # indexed by the integer (v y) mod w: the entry is the float64 value of the REDUCED angle, rounded once
        v, y = 3, w - 2
        k = (v * y) % w
        assert tw_w[k, 0] == np.float32(np.cos(2.0 * np.pi * k / w)) and tw_w[k, 1] == np.float32(np.sin(2.0 * np.pi * k / w))
        assert abs(float(tw_w[k, 0]) - np.cos(2.0 * np.pi * v * y / w)) < 1e-7


def test_bindings():
    assert C.sizeof(L.FdaDesc) == 80
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} simt_fda_desc;", HDR).group(1))
    names = [re.sub(r"\[\d+\]", "", n).strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split()[-1:] + decl.split(",")[:-1]]
    names = [n.split()[-1].strip("*") for n in names]
    assert sorted(names) == sorted(f[0] for f in L.FdaDesc._fields_), names
    assert [f[0] for f in L.FdaDesc._fields_] == ["xs", "xt", "x_out", "tw_h", "tw_w", "work", "B", "h", "w", "b", "mean", "reserved_"]
    assert L.SIGNATURES["simt_fda_transfer"] == (C.c_int, [C.POINTER(L.FdaDesc), C.c_void_p])
    assert L.SIGNATURES["simt_fda_workspace_bytes"] == (C.c_long, [C.c_int] * 4)
    assert L.FDA_MAX_ITEMS == fda.MAX_ITEMS == int(re.search(r"#define SIMT_FDA_MAX_ITEMS (\d+)", HDR).group(1))
    assert L.FDA_MAX_BAND == fda.MAX_BAND == 64 == int(re.search(r"#define SIMT_FDA_MAX_BAND\s+(\d+)", HDR).group(1))
    assert L.ABI_VERSION == 2 == int(re.search(r"#define SIMT_ABI_VERSION (\d+)", HDR).group(1))


# ---- the tool's flag ---------------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from simt_amd.tools import trainV1_warmup as tool
    return tool.get_arguments(list(argv))


ON = ["--online-labels", "--online-source"]


def test_cli_flag():
    assert _parse().fda is None and _parse(*ON).fda is None
    assert _parse(*ON, "--fda").fda == "0.01" and _parse(*ON, "--fda", "0.05").fda == "0.05"
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        assert _parse(*ON, "--fda", "--model", model, "--synthetic").fda == "0.01"
    assert fda.parse("0.01", (1024, 512)) == (0.01, 5) and fda.parse("0.01", (768, 768)) == (0.01, 7)


@pytest.mark.parametrize("argv,msg", [
    (["--fda"], "--fda needs --online-source"),
    (["--online-labels", "--fda"], "--fda needs --online-source"),
    (ON + ["--fda", "0"], "beta must lie in (0, 1)"),
    (ON + ["--fda", "-0.1"], "beta must lie in (0, 1)"),
    (ON + ["--fda", "nan"], "beta must lie in (0, 1)"),
    (ON + ["--fda", "x"], "is not a share of the spectrum"),
    (ON + ["--fda", "0.5"], "a band of 513 x 513 frequencies does not fit a crop of 1024 x 512"),
    (ON + ["--fda", "0.6", "--input-size-target", "129,65"], "a band of 79 x 79 frequencies does not fit a crop of 129 x 65"),
    (ON + ["--fda", "0.09", "--input-size-target", "768,768"], "the launch holds b <= 64"),
    (ON + ["--fda", "--batch-size", "33"], "one launch takes 1 to 32 items"),
])
def test_cli_refusals(capsys, argv, msg):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_a_band_that_does_not_fit():
    """2b + 1 <= min(h, w) for every beta < 0.5 (b = floor(min * beta)), for none above 0.5; the band limit of the launch comes on top."""
    for h, w, beta in ((9, 516, 0.49), (2, 2, 0.49), (130, 136, 0.4999), (65, 129, 0.4999)):
        assert fda.parse(beta, (w, h))[1] == fda.band(h, w, beta) and 2 * fda.band(h, w, beta) + 1 <= min(h, w)
    for h, w, beta in ((9, 516, 0.6), (8, 12, 0.5), (65, 129, 0.6)):
        with pytest.raises(ValueError, match="does not fit"):
            fda.parse(beta, (w, h))
    with pytest.raises(ValueError, match="the launch holds b <= 64"):
        fda.parse("0.2", (1024, 512))


def test_run_identity_carries_beta():
    from simt_amd.tools.trainV2_simt import RUN_DEFAULTS, run_identity
    cd = np.full(19, 1.0 / 19, dtype=np.float32)
    off = run_identity(_parse(*ON, "--synthetic"), cd)
    a = run_identity(_parse(*ON, "--synthetic", "--fda"), cd)
    b = run_identity(_parse(*ON, "--synthetic", "--fda", "0.05"), cd)
    assert "fda" not in off and RUN_DEFAULTS["fda"] is False
    assert a["fda"] == 0.01 and b["fda"] == 0.05 and a != b
    assert {k: v for k, v in a.items() if k != "fda"} == off
