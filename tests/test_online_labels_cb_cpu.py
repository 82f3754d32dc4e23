"""Class-balanced online labels without a GPU: the two descriptors against the header, the flags of trainV1_warmup and their
refusals, the texts, the run identity, the keywords' checks, the train state on fake trainers, and `balanced_update` -- the numpy restatement of
simt_class_thresholds -- on crafted histograms against values worked out by hand."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import online_labels as ol
from simt_amd import train_state as tsf
from simt_amd.tools.make_pseudo_labels import class_thresholds
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)
from test_online_labels_cpu import _FakeOnline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
CD = so.load_class_dist()
f32 = np.float32


# ---- header and descriptors -------------------------------------------------------------------------------------------------------------------------
def _layout(struct, fields):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(void){'
           f'printf("size %zu\\n", sizeof({struct}));' +
           "".join(f'printf("{n} %zu\\n", offsetof({struct}, {n}));' for n in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe])
        return {k: int(v) for k, v in (ln.split(None, 1) for ln in subprocess.check_output([exe]).decode().splitlines())}


def test_header_declares_both_symbols_and_the_descriptors_match_ctypes():
    assert re.search(r"int simt_online_label_cb\(const simt_online_label_cb_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_class_thresholds\(const simt_class_thresholds_desc\* d, simt_stream_t stream\);", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    for struct, cls, names, size in (
            ("simt_online_label_cb_desc", L.OnlineLabelCbDesc, ["fix", "label", "counts", "hist", "thr", "B", "h", "w", "ld", "H", "W", "C", "family"], 72),
            ("simt_class_thresholds_desc", L.ClassThresholdsDesc, ["hist", "thr", "t_out", "drop", "C", "cap", "omd"], 48)):
        assert [n for n, _t in cls._fields_] == names
        out = _layout(struct, names)
        assert C.sizeof(cls) == out["size"] == size
        for n in names:
            assert getattr(cls, n).offset == out[n], (struct, n)
    assert L.SIGNATURES["simt_online_label_cb"] == (C.c_int, [C.POINTER(L.OnlineLabelCbDesc), C.c_void_p])
    assert L.SIGNATURES["simt_class_thresholds"] == (C.c_int, [C.POINTER(L.ClassThresholdsDesc), C.c_void_p])
    # the descriptor of the one-threshold launch stays what it was
    assert C.sizeof(L.OnlineLabelDesc) == 64 and L.CONF_BINS == 256 == int(re.search(r"#define SIMT_CONF_BINS (\d+)", HDR).group(1))


@pytest.mark.parametrize("symbol", ["simt_online_label_cb", "simt_class_thresholds"])
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


# ---- the flags --------------------------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_default():
    from simt_amd.tools.trainV1_warmup import balanced_kwargs, get_arguments
    a = get_arguments([])
    assert a.online_labels_balanced is None and a.online_labels_momentum is None
    assert balanced_kwargs(a) == {"online_labels_balanced": None, "online_labels_momentum": None}
    a = get_arguments(["--online-labels", "--online-labels-balanced"])
    assert a.online_labels_balanced == 0.5 == ol.DEFAULT_PORTION and a.online_labels_momentum is None and ol.DEFAULT_MOMENTUM == 0.9
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        a = get_arguments(["--model", model, "--online-labels", "0.9", "--online-labels-balanced", "0.25", "--online-labels-momentum", "0",
                           "--ema", "--online-labels-every", "3"])
        assert (a.online_labels, a.online_labels_balanced, a.online_labels_momentum, a.online_labels_every) == (0.9, 0.25, 0.0, 3)
        assert balanced_kwargs(a) == {"online_labels_balanced": 0.25, "online_labels_momentum": 0.0}
    assert get_arguments(["--online-labels", "--online-labels-balanced", "1"]).online_labels_balanced == 1.0
    assert get_arguments(["--online-labels", "--online-labels-balanced", "--num-classes", "64"]).num_classes == 64


@pytest.mark.parametrize("argv,named", [
    (["--online-labels-balanced"], "--online-labels-balanced needs --online-labels"),
    (["--online-labels-balanced", "0.5", "--ema"], "--online-labels-balanced needs --online-labels"),
    (["--online-labels", "--online-labels-momentum", "0.5"], "--online-labels-momentum needs --online-labels-balanced"),
    (["--online-labels-momentum", "0.5"], "--online-labels-momentum needs --online-labels-balanced"),
    (["--online-labels", "--online-labels-balanced", "0"], "argument --online-labels-balanced"),
    (["--online-labels", "--online-labels-balanced", "1.01"], "argument --online-labels-balanced"),
    (["--online-labels", "--online-labels-balanced", "-0.5"], "argument --online-labels-balanced"),
    (["--online-labels", "--online-labels-balanced", "nan"], "argument --online-labels-balanced"),
    (["--online-labels", "--online-labels-balanced", "x"], "argument --online-labels-balanced"),
    (["--online-labels", "--online-labels-balanced", "--online-labels-momentum"], "argument --online-labels-momentum: expected one argument"),
    (["--online-labels", "--online-labels-balanced", "--online-labels-momentum", "1"], "argument --online-labels-momentum"),
    (["--online-labels", "--online-labels-balanced", "--online-labels-momentum", "-0.1"], "argument --online-labels-momentum"),
    (["--online-labels", "--online-labels-balanced", "--online-labels-momentum", "nan"], "argument --online-labels-momentum"),
    (["--online-labels", "--online-labels-balanced", "--num-classes", "65"], "--online-labels-balanced with --num-classes 65"),
    (["--online-labels", "--online-labels-balanced", "--class-mix", "--batch-size", "2"], "--online-labels cannot be combined with --class-mix"),
])
def test_flag_refusals_exit_2_and_name_the_flag(capsys, argv, named):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and named in err, (argv, err)


def test_the_simt_tool_gets_no_such_flag(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    for flag in (["--online-labels-balanced"], ["--online-labels-momentum", "0.5"]):
        with pytest.raises(SystemExit) as e:
            get_arguments(flag)
        assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_start_up_line_and_loss_line_text_on_and_off(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    off, one = tool.get_arguments([]), tool.get_arguments(["--online-labels"])
    on = tool.get_arguments(["--online-labels", "0.9", "--online-labels-balanced"])
    on2 = tool.get_arguments(["--online-labels", "0.9", "--online-labels-balanced", "0.25", "--online-labels-momentum", "0.5"])
    shared.online_label_line(off)
    assert capsys.readouterr().out == ""
    shared.online_label_line(one)
    out = capsys.readouterr().out
    assert out.endswith("the same batch as the student\n") and "class-balanced" not in out          # the line it was
    shared.online_label_line(on)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "kept where its confidence is > 0.9;" in out
    assert "; class-balanced: one threshold per class, from 0.9 towards the value that keeps the share 0.5 of" in out and "(momentum 0.9), never above 0.9" in out
    shared.online_label_line(on2)
    out = capsys.readouterr().out
    assert "keeps the share 0.25 of" in out and "(momentum 0.5)" in out
    assert shared.balanced_clause(off) == shared.balanced_clause(one) == ""
    l = {"labelled": 0.51249, "label_thresholds": [0.9, 0.31249, 0.75]}
    assert tool.thresholds_text(off, {}) == "" and tool.thresholds_text(one, {"labelled": 0.5}) == ""
    assert tool.thresholds_text(on, l) == " thr = 0.312..0.900"
    assert tool.labelled_text(on, l) + tool.thresholds_text(on, l) == " labelled = 0.512 thr = 0.312..0.900"
    assert tool.labelled_text(one, l) == " labelled = 0.512"


# ---- run identity -----------------------------------------------------------------------------------------------------------------------------------
def test_run_identity_carries_the_flag_only_when_it_is_on():
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    off = shared.run_identity(tool.get_arguments([]), cd)
    one = shared.run_identity(tool.get_arguments(["--online-labels"]), cd)
    on = shared.run_identity(tool.get_arguments(["--online-labels", "--online-labels-balanced"]), cd)
    on2 = shared.run_identity(tool.get_arguments(["--online-labels", "--online-labels-balanced", "0.25", "--online-labels-momentum", "0"]), cd)
    assert "online_labels_balanced" not in off and "online_labels_balanced" not in one
    assert on["online_labels_balanced"] == [0.5, 0.9] and on2["online_labels_balanced"] == [0.25, 0.0]
    assert {k: v for k, v in on.items() if k != "online_labels_balanced"} == one and on["online_labels"] == [0.968, None]
    assert shared.RUN_DEFAULTS["online_labels_balanced"] is False and shared.RUN_DEFAULTS["online_labels"] is False


def test_train_state_file_refuses_the_flag_added_dropped_or_changed(tmp_path, no_device_sync):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    base = ["--ema", "0.9", "--train-state", str(tmp_path / "s.state"), "--online-labels", "0.9"]

    class Keeper:
        def state(self):
            return {}

        def load_state(self, s):
            pass
    on, other_p, other_m = ["--online-labels-balanced"], ["--online-labels-balanced", "0.25"], ["--online-labels-balanced", "--online-labels-momentum", "0.5"]
    for first, others in ((on, ([], other_p, other_m)), ([], (on,)), (other_m, (on,))):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(_advanced(_Fake(ema_decay=0.9)), Keeper())
        assert shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper()) == 3
        for second in others:
            with pytest.raises(SystemExit, match="online_labels_balanced"):
                shared.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper())


# ---- the keywords ---------------------------------------------------------------------------------------------------------------------------------
def test_keyword_checks_start_with_the_keyword():
    assert ol.check_balanced(None, None, None, 19) == (None, None) == ol.check_balanced(None, None, 0.5, 300)
    assert ol.check_balanced(0.5, None, 0.9, 19) == (0.5, 0.9) and ol.check_balanced(1, 0, 0.0, 64) == (1.0, 0.0)
    assert ol.check_balanced("0.25", np.float32(0.5), 0.9, 1) == (0.25, 0.5)
    for p in (0, 0.0, -0.5, 1.01, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match=r"^online_labels_balanced "):
            ol.check_balanced(p, None, 0.9, 19)
    for m in (1, 1.0, -0.1, float("nan"), "x", True):
        with pytest.raises(ValueError, match=r"^online_labels_momentum "):
            ol.check_balanced(0.5, m, 0.9, 19)
    with pytest.raises(ValueError, match=r"^online_labels_balanced needs online_labels"):
        ol.check_balanced(0.5, None, None, 19)
    with pytest.raises(ValueError, match=r"^online_labels_momentum needs online_labels_balanced"):
        ol.check_balanced(None, 0.9, 0.9, 19)
    with pytest.raises(ValueError, match=r"^online_labels_balanced with num_classes = 65"):
        ol.check_balanced(0.5, None, 0.9, 65)
    # the pinned function is what it was
    assert ol.check_settings(0.5, None, None) == (0.5, None)


# ---- balanced_update on crafted histograms ---------------------------------------------------------------------------------------------------------
def _row(**bins):
    r = np.zeros(256, np.int64)
    for b, n in bins.items():
        r[int(b[1:])] = n
    return r


# (name, row, P, the bin b worked out by hand -- None: the class has no pixel)
CRAFTED = [
    ("empty", _row(), 0.5, None),
    ("n = 1", _row(b200=1), 0.5, 200),                                    # k = min(round(0.5), 0) = 0
    ("the cap binds", _row(b250=10), 0.5, 250),                           # 250 / 256 = 0.9765625 > T
    ("P = 1", _row(b3=1, b77=5, b255=9), 1.0, 3),                         # k = 0: the lowest occupied bin, every pixel kept
    ("P = 1 from bin 0", _row(b0=2, b255=9), 1.0, 0),
    ("k on a bin's last element", _row(b100=4, b150=4), 0.625, 100),      # n = 8, k = round(3.0) = 3: cum[100] = 4 > 3
    ("k on the next bin's first", _row(b100=4, b150=4), 0.5, 150),        # k = 4: cum[100] = 4 is not > 4
    ("2.5 rounds to 2", _row(b10=2, b20=1, b30=2), 0.5, 20),              # n = 5: half to even; half up (3) would give bin 30
    ("3.5 rounds to 4", _row(b10=3, b20=1, b30=3), 0.5, 30),              # n = 7: half to even; half down (3) would give bin 20
    ("k = n - 1", _row(b40=1, b41=1), 0.01, 41),                          # round(1.98) = 2 -> min(2, 1) = 1
    ("counts beyond 2^32", _row(b5=2 ** 33 + 1, b200=2 ** 33), 0.5, 5),   # n = 2^34 + 1, n / 2 = 2^33 + 0.5 -> k = 2^33 (even) < cum[5]
    ("counts beyond 2^32, the other side", _row(b5=2 ** 33, b200=2 ** 33 + 2), 0.5, 200),      # k = 2^33 + 1 > cum[5] = 2^33
    ("all in the last bin", _row(b255=7), 0.5, 255),
]
T = 0.9


def _fold(thr, t, M):
    """thr + omd * (t - thr), three float32 roundings, written out."""
    omd = f32(1.0 - M)
    diff = f32(f32(t) - f32(thr))
    step = f32(omd * diff)
    return f32(f32(thr) + step)


@pytest.mark.parametrize("name,row,P,b", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_balanced_update_on_a_crafted_row(name, row, P, b):
    for start in (T, 0.3):
        thr, t = ol.balanced_update(np.array([start], f32), row[None], P, T, 0.9)
        assert thr.dtype == t.dtype == np.float32 and thr.shape == t.shape == (1,)
        if b is None:
            assert thr[0] == f32(start) and t[0] == 0.0
            continue
        want_t = min(f32(b / 256.0), f32(T))
        assert t[0] == want_t and (b / 256.0 <= T or t[0] == f32(T))
        assert thr[0] == _fold(start, want_t, 0.9)
        assert t[0] == class_thresholds(row[None], P, cap=T)[0]
        # M = 0: the batch's own thresholds
        thr0, _ = ol.balanced_update(np.array([start], f32), row[None], P, T, 0.0)
        assert thr0[0] == want_t


def test_balanced_update_values_by_hand():
    """One table, C = 4, thr = [0.9, 0.9, 0.5, 0.25], M = 0.5 (omd = 0.5 exactly, so the fold is exact on dyadic values)."""
    hist = np.stack([_row(b128=4, b192=4), _row(), _row(b64=3), _row(b250=2)])
    thr, t = ol.balanced_update(np.array([0.9, 0.9, 0.5, 0.25], f32), hist, 0.5, T, 0.5)
    assert t.tolist() == [0.75, 0.0, 0.25, float(f32(0.9))]
    assert thr[1] == f32(0.9) and thr[2] == f32(0.375)                      # 0.5 + 0.5 * (0.25 - 0.5)
    assert thr[0] == f32(f32(0.9) + f32(f32(0.5) * f32(f32(0.75) - f32(0.9))))
    assert thr[3] == f32(f32(0.25) + f32(f32(0.5) * f32(f32(0.9) - f32(0.25))))
    # with cap = T the thresholds never rise above T
    assert (thr <= f32(T)).all()
    # the inputs are left as they were, and a float64 start is taken as float32
    start = np.array([0.9, 0.9, 0.5, 0.25])
    again, _ = ol.balanced_update(start, hist, 0.5, T, 0.5)
    assert start.dtype == np.float64 and (again == thr).all()
    with pytest.raises(ValueError):
        ol.balanced_update(np.zeros(4, f32), hist, 0.0, T, 0.5)


# ---- train state on fake trainers -----------------------------------------------------------------------------------------------------------------
def _FakeBalanced(P=None, M=0.9, tau=0.9, seed=0):
    tr = _FakeOnline(tau, seed=seed)
    if P is not None:
        tr.online_labels_balanced, tr.online_labels_momentum = P, M
        tr.label_thr = torch.full((3,), tau)
    return tr


def test_hyper_and_accumulators_carry_the_thresholds_only_when_on(no_device_sync):
    one = _advanced(_FakeOnline(0.9)).training_state()           # a fake from before the keyword: no attribute at all
    off = _advanced(_FakeBalanced()).training_state()
    assert one["hyper"] == off["hyper"] and set(one["accumulators"]) == set(off["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported"}
    assert not set(off["hyper"]) & set(tsf.BALANCE_FIELDS)
    on_tr = _advanced(_FakeBalanced(0.5))
    on_tr.label_thr.copy_(torch.tensor([0.9, 0.4, 0.65]))
    on = on_tr.training_state()
    assert on["hyper"]["online_labels_balanced"] == 0.5 and on["hyper"]["online_labels_momentum"] == 0.9
    assert {k: v for k, v in on["hyper"].items() if k not in tsf.BALANCE_FIELDS} == off["hyper"]
    assert set(on["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported", "label_thresholds"}
    assert torch.equal(on["accumulators"]["label_thresholds"], torch.tensor([0.9, 0.4, 0.65])) and "label_hist" not in on["accumulators"]
    assert tsf.VALUE_FIELDS == ("online_labels", "online_labels_every") and tsf.BALANCE_FIELDS == ("online_labels_balanced", "online_labels_momentum")
    # added, dropped, P or M differing: the field is named with both values
    _refused(_FakeBalanced(seed=1), on, "online_labels_balanced (state: 0.5, this trainer: None)", "online_labels_momentum (state: 0.9, this trainer: None)")
    _refused(_FakeOnline(0.9, seed=1), on, "online_labels_balanced (state: 0.5, this trainer: None)")          # a trainer from before the keyword
    _refused(_FakeBalanced(0.5, seed=1), off, "online_labels_balanced (state: None, this trainer: 0.5)")
    _refused(_FakeBalanced(0.5, seed=1), one, "online_labels_balanced (state: None, this trainer: 0.5)")         # a state from before the keyword
    _refused(_FakeBalanced(0.25, seed=1), on, "online_labels_balanced (state: 0.5, this trainer: 0.25)")
    _refused(_FakeBalanced(0.5, 0.5, seed=1), on, "online_labels_momentum (state: 0.9, this trainer: 0.5)")
    # what fits loads: the thresholds come back
    tr = _FakeBalanced(0.5, seed=1)
    tr.load_training_state(on)
    assert tr.it_done == 3 and torch.equal(tr.label_thr, torch.tensor([0.9, 0.4, 0.65]))
    for ts, t in ((one, _FakeBalanced(seed=1)), (off, _FakeOnline(0.9, seed=1)), (one, _FakeOnline(0.9, seed=1))):
        t.load_training_state(ts)
        assert t.it_done == 3
    assert tsf.value_mismatches({"online_labels_balanced": 0.5}, {}) == []          # the default fields are the two they were
    assert tsf.value_mismatches({"online_labels_balanced": 0.5}, {}, fields=tsf.BALANCE_FIELDS) == ["online_labels_balanced"]
    assert tsf.value_mismatches({"online_labels_balanced": 0.5, "online_labels_momentum": 0.9},
                                {"online_labels_balanced": 0.5, "online_labels_momentum": 0.5}, fields=tsf.BALANCE_FIELDS) == ["online_labels_momentum"]


def test_losses_reports_the_thresholds_only_with_the_keyword():
    class Tr(ol.OnlineLabelMixin):
        pass
    tr = Tr()
    tr.online_labels, tr.label_counts, tr._counts_reported = 0.9, torch.tensor([3, 0, 5, 8]), [0, 0]          # as the existing fakes: no new attribute
    assert tr._labelled({}) == {"labelled": 0.5}
    tr.online_labels_balanced, tr.label_thr = 0.5, torch.tensor([0.5, 0.25, 0.875])
    assert tr._labelled({}) == {"labelled": 0.0, "label_thresholds": [0.5, 0.25, 0.875]}
    tr.online_labels = None
    assert tr._labelled({"x": 1}) == {"x": 1}
