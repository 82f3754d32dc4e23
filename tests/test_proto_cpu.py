"""The prototype weights without a GPU: the identities of the restatement in tests/_proto_ref.py, the package's own `proto_step`
held to it, the step size against literals, the comparator of the GPU tests against seven planted mistakes, the inputs' exclusion share, and the
host side -- keyword checks, flag parsing, run identity, train-state fields, record sizes."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _proto_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("family", [0, 1])
def test_no_class_seen_gives_a_copy(dt, family):
    k = pr.make_case(40, 16, 5, family=family, ldp=8, seed=11)
    r = pr.rectify_ref(pr.features(k), k["P"], k["eta"], np.zeros(5, np.int32), k["temp"], k["thr"], family, dt)
    assert np.array_equal(r["out"].astype(F32).view(np.uint32), k["P"].view(np.uint32)) and r["changed"] == 0


@pytest.mark.parametrize("dt", [F32, F64])
def test_equal_prototypes_leave_the_posterior(dt):
    k0, k1 = pr.make_case(30, 16, 6, family=0, unseen=0, seed=12), pr.make_case(30, 16, 6, family=1, unseen=0, seed=12)
    eta = np.repeat(k0["eta"][:1], 6, axis=0)
    r0 = pr.rectify_ref(pr.features(k0), k0["P"], eta, k0["n"], 1.0, 0.5, 0, dt)
    p = k0["P"].astype(dt)
    want = p / p.sum(axis=1, keepdims=True) if dt == F64 else (p / pr._seq_sum(p, dt)[:, None]).astype(dt)
    assert np.array_equal(r0["out"], want)
    r1 = pr.rectify_ref(pr.features(k1), k1["P"], eta, k1["n"], 1.0, 0.5, 1, dt)
    assert np.array_equal(r1["out"], k1["P"].astype(dt))


def test_the_logit_form_is_the_posterior_form():
    """softmax(family-1 out) == family-0 out on softmax(the same logits), to 1e-12 in float64: adding log-weights to logits IS weighing the
    softmax and renormalising."""
    k = pr.make_case(60, 32, 7, family=1, seed=13)
    v = k["P"].astype(F64)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    o1 = pr.rectify_ref(pr.features(k), v, k["eta"], k["n"], 0.7, 0.5, 1, F64)["out"]
    o0 = pr.rectify_ref(pr.features(k), p, k["eta"], k["n"], 0.7, 0.5, 0, F64)["out"]
    e1 = np.exp(o1 - o1.max(axis=1, keepdims=True))
    assert np.abs(e1 / e1.sum(axis=1, keepdims=True) - o0).max() <= 1e-12


def test_the_first_update_is_the_mean_and_a_later_one_moves_by_a():
    rng = np.random.default_rng(5)
    Fm = rng.standard_normal((50, 8))
    lab = rng.integers(0, 3, size=50).astype(np.uint8)
    lab[:5] = 255
    S, cnt = pr.accumulate_ref(Fm, lab, 4, F64)
    assert cnt.tolist() == [int((lab == c).sum()) for c in range(4)] and cnt[3] == 0
    eta = rng.standard_normal((4, 8))
    n = np.array([0, 3, 200, 7], np.int32)
    eta2, n2 = pr.update_ref(S, cnt, eta, n, 0.99, F64)
    mean = np.stack([Fm[lab == c].mean(axis=0) for c in range(3)])
    assert np.allclose(eta2[0], mean[0], rtol=0, atol=1e-15) and n2.tolist() == [1, 4, 201, 7]
    assert np.allclose(eta2[1] - eta[1], 0.25 * (mean[1] - eta[1]), rtol=0, atol=1e-15)      # 1 / (3 + 1) > 1 - 0.99
    assert np.allclose(eta2[2] - eta[2], (1.0 - 0.99) * (mean[2] - eta[2]), rtol=0, atol=1e-15)      # 1 / 201 < 0.01
    assert np.array_equal(eta2[3], eta[3])          # absent from the batch: untouched


def test_alpha_against_literals():
    from simt_amd import proto
    for (m, n, want) in [(0.9999, 1, 0.5), (0.9999, 3, 0.25), (0.9999, 9999, 1e-4), (0.9999, 20000, 1.0 - 0.9999), (0.9, 1, 0.5), (0.9, 9, 0.1),
                         (0.9, 10, 1.0 - 0.9), (0.0, 5, 1.0), (0.5, 1, 0.5)]:
        assert pr.alpha(m, n) == pytest.approx(want, rel=1e-12) and proto.alpha(m, n) == pr.alpha(m, n)
    assert pr.alpha(0.9, 1, F32) == F32(0.5) and pr.alpha(0.9, 100, F32) == F32(1.0 - 0.9)


@pytest.mark.parametrize("name", list(pr.CASES))
def test_the_package_restatement_is_the_tests_restatement(name):
    from simt_amd import proto
    k = pr.case(name)
    for dt in (F32, F64):
        a = pr.step_ref(pr._core(k), dt)
        b = proto.proto_step(pr.features(k), k["P"], k["eta"], k["n"], k["temp"], k["thr"], k["family"], k["momentum"], dt)
        for q in ("out", "lab", "S", "cnt", "eta", "n"):
            assert np.array_equal(a[q], b[q], equal_nan=True), (name, dt, q)
        assert a["changed"] == b["changed"]


@pytest.mark.parametrize("name", list(pr.CASES))
def test_the_inputs_keep_the_float32_restatement_inside_the_cap(name):
    """The float32 restatement alone passes the GPU comparator on every shared case -- the excluded share is a property of the inputs -- and
    the cases exercise what they are there for: moved cells, ignored cells, a class absent from the batch where there are classes to spare."""
    k = pr.case(name)
    r32 = pr.step_ref(pr._core(k), F32)
    pr.check_step(pr.as_got(r32, k), k, report=name)
    if k["M"] > 9:
        assert r32["changed"] > 0 and (r32["lab"] == 255).any() and (r32["lab"] != 255).any()


@pytest.mark.parametrize("mistake", pr.MISTAKES)
def test_comparator_rejects_the_planted_mistakes(mistake):
    """Squared distance without the root, an unseen class at distance 0, an unseen class at weight 0, update before rectify, M where 1 - M
    belongs, the mean over all M cells, family 0 not renormalised: each one, planted in the float32 restatement, fails check_step."""
    for name in ("bf16_2x5x7_2048_19", "f32_3x9x9_1024_19"):          # family 0, two unseen classes, n > 0 elsewhere
        k = pr.case(name)
        bad = pr.step_ref(pr._core(k), F32, mistake=mistake)
        with pytest.raises(AssertionError):
            pr.check_step(pr.as_got(bad, k), k)
    if mistake != "no_renorm":          # (family 1 has no sum to forget)
        k = pr.case("f32_2x8x16_256_25_logits")
        with pytest.raises(AssertionError):
            pr.check_step(pr.as_got(pr.step_ref(pr._core(k), F32, mistake=mistake), k), k)


def test_nan_and_inf_rows_are_ignored_cells():
    k = dict(pr.case("f32_3x9x9_1024_19"))
    Fm = pr.features(k).copy()
    Fm[3, 5], Fm[10, 0] = np.nan, np.inf
    for dt in (F32, F64):
        r = pr.rectify_ref(Fm, k["P"], k["eta"], k["n"], k["temp"], -np.inf, 0, dt)
        assert r["lab"][3] == 255 and r["lab"][10] == 255 and (np.delete(r["lab"], [3, 10]) != 255).all()
        assert np.isnan(r["out"][[3, 10], :k["C"]]).all() and not np.isnan(np.delete(r["out"], [3, 10], axis=0)).any()


# ---- the host side ---------------------------------------------------------------------------------------------------------------------------------------
def test_check_proto():
    from simt_amd.proto import DEFAULT_MOMENTUM, DEFAULT_TEMP, check_proto
    assert (DEFAULT_TEMP, DEFAULT_MOMENTUM) == (1.0, 0.9999)
    assert check_proto(None, None, None) == (None, 0.9999) and check_proto(None, 0.9999, 0.9) == (None, 0.9999)
    assert check_proto(1.0, None, 0.0) == (1.0, 0.9999) and check_proto(2, 0.5, 0.9, 19) == (2.0, 0.5) and check_proto(0.5, 0, 0.9) == (0.5, 0.0)
    for args, named in [((1.0, None, None), "proto_denoise needs online_labels"), ((0, None, 0.9), "proto_denoise 0"),
                        ((-1.0, None, 0.9), "proto_denoise -1.0"), ((float("nan"), None, 0.9), "proto_denoise nan"),
                        ((float("inf"), None, 0.9), "proto_denoise inf"), ((True, None, 0.9), "proto_denoise True"),
                        (("warm", None, 0.9), "proto_denoise 'warm'"), ((1.0, 1.0, 0.9), "proto_momentum 1.0"),
                        ((1.0, -0.1, 0.9), "proto_momentum -0.1"), ((1.0, float("nan"), 0.9), "proto_momentum nan"),
                        ((1.0, True, 0.9), "proto_momentum True"), ((None, 0.9, 0.9), "proto_momentum needs proto_denoise"),
                        ((1.0, None, 0.9, 65), "proto_denoise with num_classes = 65"), ((1.0, None, 0.9, 1), "proto_denoise with num_classes = 1")]:
        with pytest.raises(ValueError, match=named):
            check_proto(*args)


def test_flags_defaults_refusals_and_run_identity(capsys):
    from oracle import simt_oracle as so
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools.trainV2_simt import RUN_DEFAULTS, run_identity
    cd = so.load_class_dist().numpy()
    base = ["--synthetic", "--online-labels", "0.9"]
    off = tool.get_arguments(base)
    assert (off.proto_denoise, off.proto_momentum) == (None, None) and tool.proto_kwargs(off) == {}
    ident = run_identity(off, cd)
    assert "proto_denoise" not in ident and RUN_DEFAULTS["proto_denoise"] is False
    tool.proto_line(off)
    assert capsys.readouterr().out == ""
    bare = tool.get_arguments(base + ["--proto-denoise"])
    assert tool.proto_kwargs(bare) == {"proto_denoise": 1.0, "proto_momentum": 0.9999}
    assert run_identity(bare, cd)["proto_denoise"] == [1.0, 0.9999]
    assert {k: v for k, v in run_identity(bare, cd).items() if k != "proto_denoise"} == ident
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        full = tool.get_arguments(base + ["--model", model, "--proto-denoise", "0.5", "--proto-momentum", "0.99"])
        assert tool.proto_kwargs(full) == {"proto_denoise": 0.5, "proto_momentum": 0.99}
        assert run_identity(full, cd)["proto_denoise"] == [0.5, 0.99]
    tool.proto_line(full)
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and "/ 0.5)" in line and "momentum 0.99" in line and "per rank" in line and "no dataset pass" in line
    assert tool.proto_text(full, {"proto_seen": 17, "proto_changed": 0.03125}) == " proto = 17/19 moved 0.0312" or \
        tool.proto_text(full, {"proto_seen": 17, "proto_changed": 0.03125}) == " proto = 17/19 moved 0.0313"
    assert tool.proto_text(full, {"loss_seg": 1.0}) == ""
    for bad, named in [(["--synthetic", "--proto-denoise"], "--proto-denoise needs --online-labels"),
                       (base + ["--proto-denoise", "0"], "--proto-denoise 0.0"), (base + ["--proto-denoise", "nan"], "--proto-denoise nan"),
                       (base + ["--proto-denoise", "-1"], "--proto-denoise -1.0"), (base + ["--proto-denoise", "--proto-momentum", "1"], "--proto-momentum 1.0"),
                       (base + ["--proto-momentum", "0.9"], "--proto-momentum needs --proto-denoise")]:
        with pytest.raises(SystemExit) as e:
            tool.get_arguments(bad)
        assert e.value.code == 2 and named in capsys.readouterr().err, (bad, named)


def test_train_state_fields():
    from simt_amd import train_state as tsf
    assert tsf.PROTO_FIELDS == ("proto_denoise", "proto_momentum")
    on = {"proto_denoise": 1.0, "proto_momentum": 0.9999}
    assert tsf.value_mismatches({}, {}, fields=tsf.PROTO_FIELDS) == [] and tsf.value_mismatches(on, dict(on), fields=tsf.PROTO_FIELDS) == []
    assert tsf.value_mismatches({}, on, fields=tsf.PROTO_FIELDS) == list(tsf.PROTO_FIELDS)          # added
    assert tsf.value_mismatches(on, {}, fields=tsf.PROTO_FIELDS) == list(tsf.PROTO_FIELDS)          # dropped
    assert tsf.value_mismatches(on, dict(on, proto_denoise=0.5), fields=tsf.PROTO_FIELDS) == ["proto_denoise"]
    assert tsf.value_mismatches(on, dict(on, proto_momentum=0.9), fields=tsf.PROTO_FIELDS) == ["proto_momentum"]


def test_bindings_match_the_header():
    from simt_amd import _lib as L
    structs = {"simt_proto_rectify_desc": L.ProtoRectifyDesc, "simt_proto_acc_desc": L.ProtoAccDesc, "simt_proto_update_desc": L.ProtoUpdateDesc}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in structs) + (
        'printf("thr %zu\\n", offsetof(simt_proto_rectify_desc, thr));printf("momentum %zu\\n", offsetof(simt_proto_update_desc, momentum));'
        'printf("maxc %d\\n", SIMT_PROTO_MAX_CLASSES);printf("maxd %d\\n", SIMT_PROTO_MAX_DIM);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "p.c"), os.path.join(td, "p")
        open(cpath, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    for n, cls in structs.items():
        assert ctypes.sizeof(cls) == got[n], (n, ctypes.sizeof(cls), got[n])
    assert L.ProtoRectifyDesc.thr.offset == got["thr"] and L.ProtoUpdateDesc.momentum.offset == got["momentum"]
    assert (L.PROTO_MAX_CLASSES, L.PROTO_MAX_DIM) == (got["maxc"], got["maxd"]) == (64, 4096)
    for name in ("simt_proto_parts", "simt_proto_ws_floats", "simt_proto_rectify", "simt_proto_accumulate", "simt_proto_update"):
        assert name in L.SIGNATURES
