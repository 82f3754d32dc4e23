"""ClassMix behind the teacher without a GPU: the three descriptors against the header, the signatures, the flag of
trainV1_warmup and its refusals, the texts, the run identity, the keywords' checks, the train state on fake trainers, and the order of the
draws against tests/_class_mix_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as ref
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import online_labels as ol
from simt_amd import train_state as tsf
from simt_amd.data import class_mix
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)
from test_online_labels_cb_cpu import _FakeBalanced, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
CD = so.load_class_dist()
NEW = ["simt_online_label_parts", "simt_online_label_u8", "simt_online_label_cb_u8", "simt_class_mix_u8"]


# ---- header and descriptors -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols_and_the_descriptors_match_ctypes():
    assert re.search(r"int simt_online_label_parts\(const simt_online_label_u8_desc\* d\);", HDR)
    assert re.search(r"int simt_online_label_u8\(const simt_online_label_u8_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_online_label_cb_u8\(const simt_online_label_cb_u8_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_class_mix_u8\(const simt_class_mix_u8_desc\* d, simt_stream_t stream\);", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    assert L.ONLINE_LABEL_MAX_PARTS == 1024 == int(re.search(r"#define SIMT_ONLINE_LABEL_MAX_PARTS (\d+)", HDR).group(1))
    geo = ["B", "h", "w", "ld", "H", "W", "C", "family"]
    for struct, cls, names, size in (
            ("simt_online_label_u8_desc", L.OnlineLabelU8Desc, ["fix", "lab8", "counts", "part"] + geo + ["threshold"], 72),
            ("simt_online_label_cb_u8_desc", L.OnlineLabelCbU8Desc, ["fix", "lab8", "counts", "hist", "thr", "part"] + geo, 80),
            ("simt_class_mix_u8_desc", L.ClassMixU8Desc,
             ["x", "lab8", "x_out", "lab_out", "part", "B", "h", "w", "n_classes", "rows", "partner", "apply", "rank"], 40 + 20 + 32 + 32 + 1024 + 4)):
        assert [n for n, _t in cls._fields_] == names
        out = _layout(struct, names)
        assert C.sizeof(cls) == out["size"] == size, (struct, C.sizeof(cls), out["size"])
        for n in names:
            assert getattr(cls, n).offset == out[n], (struct, n)
    assert L.ClassMixU8Desc.rank.offset % 4 == 0          # the kernel reads a rank row as 8 dwords
    # the descriptors that existed stay what they were
    assert C.sizeof(L.OnlineLabelDesc) == 64 and C.sizeof(L.OnlineLabelCbDesc) == 72 and C.sizeof(L.ClassMixDesc) == 40 + 16 + 32 + 32 + 1024


def test_signatures():
    assert L.SIGNATURES["simt_online_label_parts"] == (C.c_int, [C.POINTER(L.OnlineLabelU8Desc)])
    assert L.SIGNATURES["simt_online_label_u8"] == (C.c_int, [C.POINTER(L.OnlineLabelU8Desc), C.c_void_p])
    assert L.SIGNATURES["simt_online_label_cb_u8"] == (C.c_int, [C.POINTER(L.OnlineLabelCbU8Desc), C.c_void_p])
    assert L.SIGNATURES["simt_class_mix_u8"] == (C.c_int, [C.POINTER(L.ClassMixU8Desc), C.c_void_p])


@pytest.mark.parametrize("symbol", NEW)
def test_a_library_without_a_symbol_names_it(monkeypatch, symbol):
    class Old:
        def __getattr__(self, name):
            if name == symbol:
                raise AttributeError(name)
            return lambda *a: L.ABI_VERSION
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(L, "LIB_PATH", __file__)
    with pytest.raises(L.SimtHipError, match=symbol + r"\b.*rebuild"):
        L.load()


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults():
    from simt_amd.tools.trainV1_warmup import balanced_kwargs, get_arguments
    a = get_arguments([])
    assert a.online_mix is None and "online_mix" not in balanced_kwargs(a)
    a = get_arguments(["--online-labels", "--online-mix", "--batch-size", "2"])
    assert a.online_mix == 1.0                             # bare: 1.0, like --class-mix
    assert balanced_kwargs(a) == {"online_labels_balanced": None, "online_labels_momentum": None, "online_mix": 1.0, "online_mix_seed": 1234}
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        a = get_arguments(["--model", model, "--online-labels", "0.9", "--online-mix", "0.25", "--batch-size", "32", "--num-classes", "32",
                           "--random-seed", "7", "--synthetic", "--ema", "--online-labels-every", "2", "--online-labels-balanced", "--scale-crop",
                           "--cache-dataset", "device", "--iter-size", "2", "--colour-jitter", "--gaussian-blur", "--mask-patches"])
        assert a.online_mix == 0.25 and balanced_kwargs(a)["online_mix_seed"] == 7
    assert get_arguments(["--online-labels", "--online-mix", "1", "--batch-size", "2", "--num-classes", "1"]).online_mix == 1.0


@pytest.mark.parametrize("argv,named", [
    (["--online-mix", "--batch-size", "2"], "--online-mix needs --online-labels"),
    (["--online-mix", "0.5", "--batch-size", "2", "--ema"], "--online-mix needs --online-labels"),
    (["--online-labels", "--online-mix"], "--online-mix with --batch-size 1"),
    (["--online-labels", "--online-mix", "--batch-size", "33"], "--online-mix with --batch-size 33"),
    (["--online-labels", "--online-mix", "--batch-size", "2", "--num-classes", "33"], "--online-mix with --num-classes 33"),
    (["--online-labels", "--online-mix", "0", "--batch-size", "2"], "argument --online-mix"),
    (["--online-labels", "--online-mix", "-0.5", "--batch-size", "2"], "argument --online-mix"),
    (["--online-labels", "--online-mix", "1.01", "--batch-size", "2"], "argument --online-mix"),
    (["--online-labels", "--online-mix", "nan", "--batch-size", "2"], "argument --online-mix"),
    (["--online-labels", "--online-mix", "x", "--batch-size", "2"], "argument --online-mix"),
    (["--online-labels", "--online-mix", "--class-mix", "--batch-size", "2"], "--online-labels cannot be combined with --class-mix"),
])
def test_flag_refusals_exit_2_and_name_the_flag(capsys, argv, named):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and named in err, (argv, err)


def test_the_class_mix_refusal_now_points_at_the_flag(capsys):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit):
        get_arguments(["--online-labels", "--class-mix", "--batch-size", "2"])
    err = capsys.readouterr().err
    assert "--online-labels cannot be combined with --class-mix" in err and "--online-mix" in err


def test_the_simt_tool_gets_no_such_flag(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(["--online-mix"])
    assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_start_up_line_on_and_off(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    one = tool.get_arguments(["--online-labels"])
    on = tool.get_arguments(["--online-labels", "0.9", "--online-mix", "0.5", "--batch-size", "2"])
    views = tool.get_arguments(["--online-labels", "0.9", "--online-mix", "--batch-size", "2", "--colour-jitter", "--mask-patches"])
    shared.online_label_line(one)
    out = capsys.readouterr().out
    assert out.endswith("the same batch as the student\n") and "online mix" not in out          # the line it was
    shared.online_label_line(on)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "; online mix: with probability 0.5 an item receives" in out and "strong views" not in out
    shared.online_label_line(views)
    out = capsys.readouterr().out
    assert "the teacher sees the batch before --colour-jitter, --mask-patches (the weak view)" in out
    assert "the mix selects from the students' strong views: a pasted region carries its partner's --colour-jitter, --mask-patches" in out
    assert shared.mix_clause(one, []) == ""


# ---- run identity -----------------------------------------------------------------------------------------------------------------------------------
def test_run_identity_carries_the_flag_only_when_it_is_on():
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    off = shared.run_identity(tool.get_arguments([]), cd)
    one = shared.run_identity(tool.get_arguments(["--online-labels", "--batch-size", "2"]), cd)
    on = shared.run_identity(tool.get_arguments(["--online-labels", "--online-mix", "0.25", "--batch-size", "2"]), cd)
    syn = shared.run_identity(tool.get_arguments(["--online-labels", "--online-mix", "--batch-size", "2", "--synthetic"]), cd)
    assert "online_mix" not in off and "online_mix" not in one and on["online_mix"] == 0.25 and syn["online_mix"] == 1.0
    assert {k: v for k, v in on.items() if k != "online_mix"} == one
    assert shared.RUN_DEFAULTS["online_mix"] is False


def test_train_state_file_refuses_the_flag_added_dropped_or_changed(tmp_path, no_device_sync):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    base = ["--ema", "0.9", "--train-state", str(tmp_path / "s.state"), "--online-labels", "0.9", "--batch-size", "2"]

    class Keeper:
        def state(self):
            return {}

        def load_state(self, s):
            pass
    on, other = ["--online-mix"], ["--online-mix", "0.5"]
    for first, others in ((on, ([], other)), ([], (on,))):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(_advanced(_Fake(ema_decay=0.9)), Keeper())
        assert shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper()) == 3
        for second in others:
            with pytest.raises(SystemExit, match="online_mix"):
                shared.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper())


# ---- the keywords ---------------------------------------------------------------------------------------------------------------------------------
def test_keyword_checks_start_with_the_keyword():
    assert ol.check_mix(None, 0, None, 1, 300) == (None, 0) == ol.check_mix(None, None, 0.5, 2, 19)
    assert ol.check_mix(0.5, 0, 0.9, 2, 19) == (0.5, 0) and ol.check_mix(1, 7, 0.0, 32, 32) == (1.0, 7)
    assert ol.check_mix("0.25", np.int64(3), 0.9, 2, 1) == (0.25, 3)
    for p in (0, 0.0, -0.5, 1.01, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match=r"^online_mix "):
            ol.check_mix(p, 0, 0.9, 2, 19)
    for s in (1.5, "1", True, -1):
        with pytest.raises(ValueError, match=r"^online_mix_seed "):
            ol.check_mix(0.5, s, 0.9, 2, 19)
    with pytest.raises(ValueError, match=r"^online_mix needs online_labels"):
        ol.check_mix(0.5, 0, None, 2, 19)
    with pytest.raises(ValueError, match=r"^online_mix_seed needs online_mix"):
        ol.check_mix(None, 5, 0.9, 2, 19)
    for b in (1, 33):
        with pytest.raises(ValueError, match=rf"^online_mix with a batch of {b}\b"):
            ol.check_mix(0.5, 0, 0.9, b, 19)
    with pytest.raises(ValueError, match=r"^online_mix with num_classes = 33"):
        ol.check_mix(0.5, 0, 0.9, 2, 33)
    # the pinned functions are what they were
    assert ol.check_settings(0.5, None, None) == (0.5, None) and ol.check_balanced(None, None, 0.5, 300) == (None, None)


# ---- the draws ------------------------------------------------------------------------------------------------------------------------------------
def test_draws_are_the_loaders_contract_in_order():
    """The trainer's generator and per-micro-batch call are simt_amd.data.class_mix's; held to the restatement of tests/_class_mix_ref.py."""
    for seed, rank, B, Cn, P in ((0, 0, 2, 19, 0.5), (1234, 3, 5, 32, 1.0), (7, 1, 32, 1, 0.25)):
        a, b = class_mix.generator(seed, rank), ref.generator(seed, rank)
        for _ in range(4):
            ap, rk = class_mix.draw_batch(a, B, Cn, P)
            ap2, rk2 = ref.draws(b, B, Cn, P)
            assert ap.tolist() == ap2.tolist() and rk.dtype == np.uint8 and (rk == rk2).all()
        assert a.bit_generator.state == b.bit_generator.state


# ---- train state on fake trainers -----------------------------------------------------------------------------------------------------------------
def _FakeMix(P=None, S=0, seed=0, balanced=None):
    tr = _FakeBalanced(balanced, seed=seed)
    tr.online_mix, tr.online_mix_seed = P, S
    if P is not None:
        tr._mix_rng = class_mix.generator(S, 0)
    return tr


def test_hyper_and_state_carry_the_mix_only_when_on(no_device_sync):
    legacy = _advanced(_FakeBalanced()).training_state()          # a fake from before the keyword: no attribute at all
    off = _advanced(_FakeMix()).training_state()
    assert legacy["hyper"] == off["hyper"] and legacy.keys() == off.keys() and "mix_rng" not in off
    assert not set(off["hyper"]) & set(tsf.MIX_FIELDS)
    assert tsf.MIX_FIELDS == ("online_mix", "online_mix_seed")
    assert tsf.VALUE_FIELDS == ("online_labels", "online_labels_every") and tsf.BALANCE_FIELDS == ("online_labels_balanced", "online_labels_momentum")
    on_tr = _advanced(_FakeMix(0.5, 7))
    for _ in range(3):
        class_mix.draw_batch(on_tr._mix_rng, 2, 19, 0.5)
    on = on_tr.training_state()
    assert on["hyper"]["online_mix"] == 0.5 and on["hyper"]["online_mix_seed"] == 7
    assert {k: v for k, v in on["hyper"].items() if k not in tsf.MIX_FIELDS} == off["hyper"]
    assert set(on) == set(off) | {"mix_rng"} and on["mix_rng"] == on_tr._mix_rng.bit_generator.state
    # added, dropped, P or S differing: the field is named with both values
    _refused(_FakeMix(seed=1), on, "online_mix (state: 0.5, this trainer: None)", "online_mix_seed (state: 7, this trainer: None)")
    _refused(_FakeBalanced(seed=1), on, "online_mix (state: 0.5, this trainer: None)")          # a trainer from before the keyword
    _refused(_FakeMix(0.5, 7, seed=1), off, "online_mix (state: None, this trainer: 0.5)")
    _refused(_FakeMix(0.5, 7, seed=1), legacy, "online_mix (state: None, this trainer: 0.5)")
    _refused(_FakeMix(0.25, 7, seed=1), on, "online_mix (state: 0.5, this trainer: 0.25)")
    _refused(_FakeMix(0.5, 8, seed=1), on, "online_mix_seed (state: 7, this trainer: 8)")
    _refused(_FakeMix(0.5, 7, seed=1), {k: v for k, v in on.items() if k != "mix_rng"}, "mix_rng")
    # what fits loads: the next draws are the saved run's next draws
    tr = _FakeMix(0.5, 7, seed=1)
    tr.load_training_state(on)
    want, got = class_mix.draw_batch(on_tr._mix_rng, 2, 19, 0.5), class_mix.draw_batch(tr._mix_rng, 2, 19, 0.5)
    assert tr.it_done == 3 and want[0].tolist() == got[0].tolist() and (want[1] == got[1]).all()
    # a file round trip keeps the generator's state
    import io
    buf = io.BytesIO()
    torch.save(on, buf)
    buf.seek(0)
    assert torch.load(buf, weights_only=False)["mix_rng"] == on["mix_rng"]
    for ts, t in ((legacy, _FakeMix(seed=1)), (off, _FakeBalanced(seed=1))):
        t.load_training_state(ts)
        assert t.it_done == 3
    assert tsf.value_mismatches({"online_mix": 0.5}, {}) == []          # the default fields are the two they were
    assert tsf.value_mismatches({"online_mix": 0.5}, {}, fields=tsf.MIX_FIELDS) == ["online_mix"]
