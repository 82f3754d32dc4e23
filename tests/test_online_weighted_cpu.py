"""Quality-weighted online labels without a GPU: the three descriptors against the header, the signatures, the keyword's checks,
the numpy restatement of the quality rule, the flag of trainV1_warmup, the run identity, the train state on fake trainers, and the float64
restatement of the weighted cross-entropy (tests/_weighted_ref.py) held to the bars the GPU test uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _head_bar as hb
import _weighted_ref as wr
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import online_labels as ol
from simt_amd import train_state as tsf
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)
from test_online_labels_cb_cpu import _FakeBalanced, _layout
from test_online_mix_cpu import _FakeMix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
CD = so.load_class_dist()
NEW = ["simt_online_label_w", "simt_online_label_w_u8", "simt_label_quality", "simt_head_loss_weighted", "simt_head_grad_weighted",
       "simt_class_mix_u8_items"]


# ---- header and descriptors -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols_and_the_descriptors_match_ctypes():
    assert re.search(r"int simt_online_label_w\(const simt_online_label_w_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_online_label_w_u8\(const simt_online_label_w_u8_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_label_quality\(const simt_label_quality_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_head_loss_weighted\(const simt_head_desc\* d, const float\* w, const uint8_t\* w_item, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_head_grad_weighted\(const simt_head_desc\* d, const float\* w, const uint8_t\* w_item, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_class_mix_u8_items\(const simt_class_mix_u8_desc\* d, uint8_t\* item_out, simt_stream_t stream\);", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    geo = ["B", "h", "w", "ld", "H", "W", "C", "family"]
    for struct, cls, names, size in (
            ("simt_online_label_w_desc", L.OnlineLabelWDesc, ["fix", "label", "counts", "conf_part"] + geo + ["threshold"], 72),
            ("simt_online_label_w_u8_desc", L.OnlineLabelWU8Desc, ["fix", "lab8", "counts", "part", "conf_part"] + geo + ["threshold"], 80),
            ("simt_label_quality_desc", L.LabelQualityDesc, ["conf_part", "q", "B", "rows", "H", "W", "mode"], 40)):
        assert [n for n, _t in cls._fields_] == names
        out = _layout(struct, names)
        assert C.sizeof(cls) == out["size"] == size, (struct, C.sizeof(cls), out["size"])
        for n in names:
            assert getattr(cls, n).offset == out[n], (struct, n)
    # the descriptors that existed stay what they were
    assert C.sizeof(L.OnlineLabelDesc) == 64 and C.sizeof(L.OnlineLabelU8Desc) == 72 and C.sizeof(L.OnlineLabelCbDesc) == 72
    assert C.sizeof(L.OnlineLabelCbU8Desc) == 80 and C.sizeof(L.ClassMixU8Desc) == 40 + 20 + 32 + 32 + 1024 + 4
    assert L.LABEL_QUALITY_MODES == {"item": 0, "batch": 1}


def test_signatures():
    p = C.c_void_p
    assert L.SIGNATURES["simt_online_label_w"] == (C.c_int, [C.POINTER(L.OnlineLabelWDesc), p])
    assert L.SIGNATURES["simt_online_label_w_u8"] == (C.c_int, [C.POINTER(L.OnlineLabelWU8Desc), p])
    assert L.SIGNATURES["simt_label_quality"] == (C.c_int, [C.POINTER(L.LabelQualityDesc), p])
    assert L.SIGNATURES["simt_head_loss_weighted"] == (C.c_int, [C.POINTER(L.HeadDesc), p, p, p]) == L.SIGNATURES["simt_head_grad_weighted"]
    assert L.SIGNATURES["simt_class_mix_u8_items"] == (C.c_int, [C.POINTER(L.ClassMixU8Desc), p, p])


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


# ---- the keyword ------------------------------------------------------------------------------------------------------------------------------------
def test_check_weighted_starts_with_the_keyword():
    assert ol.check_weighted(None, None, None, 300) is None and ol.check_weighted(None, 0.5, 0.5, 2) is None
    assert ol.check_weighted("batch", 0.9, None, 1) == "batch" and ol.check_weighted("item", 0.0, None, 32) == "item"
    assert ol.WEIGHTED_MODES == ("batch", "item") and ol.MAX_WEIGHTED_ITEMS == L.CLASS_MIX_MAX == 32
    for m in ("", "Batch", "both", True, 1, 0.5, b"item"):
        with pytest.raises(ValueError, match=r"^online_labels_weighted "):
            ol.check_weighted(m, 0.9, None, 2)
    with pytest.raises(ValueError, match=r"^online_labels_weighted needs online_labels"):
        ol.check_weighted("batch", None, None, 2)
    with pytest.raises(ValueError, match=r"^online_labels_weighted cannot be combined with online_labels_balanced in this version"):
        ol.check_weighted("item", 0.9, 0.5, 2)
    with pytest.raises(ValueError, match=r"^online_labels_weighted with a batch of 33\b"):
        ol.check_weighted("batch", 0.9, None, 33)
    # the pinned functions are what they were
    assert ol.check_settings(0.5, None, None) == (0.5, None) and ol.check_mix(None, 0, None, 1, 300) == (None, 0)


# ---- the quality rule -------------------------------------------------------------------------------------------------------------------------------
def test_label_quality_restatement_on_hand_made_counts():
    N = 5000 * 5000                                        # 25e6 > 2^24: the counts below do not fit a float32 exactly
    n = [0, N, (1 << 24) + 1, 12345677, 1]
    item = ol.label_quality(n, N, "item")
    assert item.dtype == np.float32 and item.shape == (5,)
    assert item[0] == 0.0 and item[1] == 1.0
    # one conversion, one division, one rounding: what exact rational arithmetic rounds to
    from fractions import Fraction
    for v, q in zip(n, item):
        want = Fraction(v, N)
        lo, hi = np.nextafter(q, np.float32(-1)), np.nextafter(q, np.float32(2))
        assert abs(Fraction(float(q)) - want) <= min(abs(Fraction(float(lo)) - want), abs(Fraction(float(hi)) - want))
    assert item[2] == np.float32(np.float64((1 << 24) + 1) / np.float64(N))
    batch = ol.label_quality(n, N, "batch")
    assert batch.dtype == np.float32 and len(set(batch.tolist())) == 1
    assert batch[0] == np.float32(np.float64(sum(n)) / np.float64(5 * N))
    assert ol.label_quality([7], 7, "batch").tolist() == [1.0] == ol.label_quality([7], 7, "item").tolist()          # B = 1
    assert ol.label_quality([0, 0], 9, "batch").tolist() == [0.0, 0.0] == ol.label_quality([0, 0], 9, "item").tolist()
    assert ol.label_quality(np.array([3, 1], dtype=np.uint32), 4, "item").tolist() == [0.75, 0.25]
    assert ol.label_quality(np.array([3, 1], dtype=np.uint32), 4, "batch").tolist() == [0.5, 0.5]
    # integer sums: three counts near 2^32 must not wrap or round before the division
    big = [(1 << 31) - 1] * 3
    assert ol.label_quality(big, 1 << 31, "batch")[0] == np.float32(np.float64(3 * ((1 << 31) - 1)) / np.float64(3 * (1 << 31)))
    with pytest.raises(ValueError):
        ol.label_quality([1], 1, "image")


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults():
    from simt_amd.tools.trainV1_warmup import balanced_kwargs, get_arguments, quality_text
    a = get_arguments([])
    assert a.online_labels_weighted is None and "online_labels_weighted" not in balanced_kwargs(a)
    assert quality_text(a, {}) == ""
    a = get_arguments(["--online-labels", "--online-labels-weighted"])
    assert a.online_labels_weighted == "batch"              # bare: the published rule
    assert balanced_kwargs(a) == {"online_labels_balanced": None, "online_labels_momentum": None, "online_labels_weighted": "batch"}
    assert quality_text(a, {"label_quality": [0.25, 0.5]}) == " q = 0.250..0.500"
    a = get_arguments(["--online-labels", "0.9", "--online-labels-weighted", "--batch-size", "2"])      # the next flag is not its value
    assert a.online_labels_weighted == "batch" and a.batch_size == 2
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        a = get_arguments(["--model", model, "--online-labels", "0.9", "--online-labels-weighted", "item", "--online-mix", "0.25",
                           "--batch-size", "32", "--synthetic", "--ema", "--online-labels-every", "2", "--iter-size", "2"])
        assert a.online_labels_weighted == "item"
        assert balanced_kwargs(a) == {"online_labels_balanced": None, "online_labels_momentum": None, "online_mix": 0.25,
                                      "online_mix_seed": 1234, "online_labels_weighted": "item"}


@pytest.mark.parametrize("argv,named", [
    (["--online-labels-weighted"], "--online-labels-weighted needs --online-labels"),
    (["--online-labels-weighted", "item", "--ema"], "--online-labels-weighted needs --online-labels"),
    (["--online-labels", "--online-labels-weighted", "--online-labels-balanced"],
     "--online-labels-weighted cannot be combined with --online-labels-balanced in this version"),
    (["--online-labels", "--online-labels-weighted", "--batch-size", "33"], "--online-labels-weighted with --batch-size 33"),
    (["--online-labels", "--online-labels-weighted", "image"], "argument --online-labels-weighted"),
    (["--online-labels", "--online-labels-weighted", "0.5"], "argument --online-labels-weighted"),
])
def test_flag_refusals_exit_2_and_name_the_flag(capsys, argv, named):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and named in err, (argv, err)


def test_the_simt_tool_gets_no_such_flag(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(["--online-labels-weighted"])
    assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_start_up_line_on_and_off(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    one = tool.get_arguments(["--online-labels"])
    shared.online_label_line(one)
    out = capsys.readouterr().out
    assert out.endswith("the same batch as the student\n") and "quality weights" not in out          # the line it was
    assert shared.weighted_clause(one) == ""
    shared.online_label_line(tool.get_arguments(["--online-labels", "0.9", "--online-labels-weighted"]))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "; quality weights (batch): every pixel keeps the teacher's arg-max" in out and "the batch's pixels" in out
    assert "confidence is > 0.9" in out
    shared.online_label_line(tool.get_arguments(["--online-labels", "0.9", "--online-labels-weighted", "item", "--online-mix", "--batch-size", "2"]))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "; online mix:" in out and out.index("; online mix:") < out.index("; quality weights (item):")
    assert "its image's pixels" in out
    assert "--online-labels-weighted [batch|item]" in tool.__doc__ and " q = <min>..<max>" in tool.__doc__


# ---- run identity and the train-state file ------------------------------------------------------------------------------------------------------------
def test_run_identity_carries_the_flag_only_when_it_is_on():
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    off = shared.run_identity(tool.get_arguments([]), cd)
    one = shared.run_identity(tool.get_arguments(["--online-labels"]), cd)
    on = shared.run_identity(tool.get_arguments(["--online-labels", "--online-labels-weighted"]), cd)
    item = shared.run_identity(tool.get_arguments(["--online-labels", "--online-labels-weighted", "item", "--synthetic"]), cd)
    assert "online_labels_weighted" not in off and "online_labels_weighted" not in one
    assert on["online_labels_weighted"] == "batch" and item["online_labels_weighted"] == "item"
    assert {k: v for k, v in on.items() if k != "online_labels_weighted"} == one
    assert shared.RUN_DEFAULTS["online_labels_weighted"] is False


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
    on, other = ["--online-labels-weighted"], ["--online-labels-weighted", "item"]
    for first, others in ((on, ([], other)), ([], (on,))):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(_advanced(_Fake(ema_decay=0.9)), Keeper())
        assert shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper()) == 3
        for second in others:
            with pytest.raises(SystemExit, match="online_labels_weighted"):
                shared.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper())


# ---- train state on fake trainers -----------------------------------------------------------------------------------------------------------------
def _FakeWeighted(mode=None, seed=0, mix=None):
    tr = _FakeMix(mix, 7 if mix is not None else 0, seed=seed)
    tr.online_labels_weighted = mode
    if mode is not None:
        tr.label_q = torch.zeros(tr.B)
    return tr


def test_hyper_and_accumulators_carry_the_mode_only_when_on(no_device_sync):
    legacy = _advanced(_FakeMix()).training_state()          # a fake from before the keyword: no attribute at all
    off = _advanced(_FakeWeighted()).training_state()
    assert legacy["hyper"] == off["hyper"] and legacy.keys() == off.keys()
    assert set(legacy["accumulators"]) == set(off["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported"}
    assert not set(off["hyper"]) & set(tsf.WEIGHTED_FIELDS) and tsf.WEIGHTED_FIELDS == ("online_labels_weighted",)
    # the field lists that existed are what they were
    assert tsf.MIX_FIELDS == ("online_mix", "online_mix_seed") and tsf.VALUE_FIELDS == ("online_labels", "online_labels_every")
    assert tsf.BALANCE_FIELDS == ("online_labels_balanced", "online_labels_momentum")
    on_tr = _advanced(_FakeWeighted("batch"))
    on_tr.label_q.copy_(torch.tensor([0.25, 0.75]))
    on = on_tr.training_state()
    assert on["hyper"]["online_labels_weighted"] == "batch"
    assert {k: v for k, v in on["hyper"].items() if k != "online_labels_weighted"} == off["hyper"]
    assert set(on["accumulators"]) == set(off["accumulators"]) | {"label_quality"} and set(on) == set(off)
    # added, dropped or changed: the field is named with both values
    _refused(_FakeWeighted(seed=1), on, "online_labels_weighted (state: 'batch', this trainer: None)")
    _refused(_FakeMix(seed=1), on, "online_labels_weighted (state: 'batch', this trainer: None)")          # a trainer from before the keyword
    _refused(_FakeWeighted("batch", seed=1), off, "online_labels_weighted (state: None, this trainer: 'batch')")
    _refused(_FakeWeighted("batch", seed=1), legacy, "online_labels_weighted (state: None, this trainer: 'batch')")
    _refused(_FakeWeighted("item", seed=1), on, "online_labels_weighted (state: 'batch', this trainer: 'item')")
    tr = _FakeWeighted("batch", seed=1)
    tr.load_training_state(on)
    assert tr.it_done == 3 and tr.label_q.tolist() == [0.25, 0.75]
    for ts, t in ((legacy, _FakeWeighted(seed=1)), (off, _FakeMix(seed=1))):
        t.load_training_state(ts)
        assert t.it_done == 3
    both = _advanced(_FakeWeighted("item", mix=0.5)).training_state()
    assert both["hyper"]["online_mix"] == 0.5 and both["hyper"]["online_labels_weighted"] == "item" and "mix_rng" in both
    assert tsf.value_mismatches({"online_labels_weighted": "item"}, {}) == []          # the default fields are the two they were
    assert tsf.value_mismatches({"online_labels_weighted": "item"}, {}, fields=tsf.WEIGHTED_FIELDS) == ["online_labels_weighted"]


# ---- the float64 restatement of the weighted cross-entropy, on the inputs of the GPU test ------------------------------------------------------------
def test_weighted_ref_with_unit_weights_is_the_warmup_reference():
    """w = 1 and no map: the restatement is tests/_head_bar.warmup_ref, the reference the unweighted launches are held to."""
    p1, p2, lab, _w, _item = wr.inputs("straddle", CD)
    B = p2.shape[0]
    for half in (False, True):
        a = wr.weighted_ref(p1, p2, lab, np.ones(B, np.float32), None, 0.1, half, torch.float64)
        b = hb.warmup_ref(p1, p2, lab, 0.1, half, torch.float64)
        assert torch.allclose(a["total"], b["total"], rtol=1e-13, atol=0) and torch.allclose(a["l1"], b["l1"], rtol=1e-13, atol=0)
        assert torch.allclose(a["dpred2"], b["dpred2"], rtol=1e-10, atol=1e-18) and torch.allclose(a["dpred1"], b["dpred1"], rtol=1e-10, atol=1e-18)
        assert a["N"] == int(((lab >= 0) & (lab < 19)).sum())


@pytest.mark.parametrize("case,half,single", [("straddle", False, False), ("straddle", True, True), ("rows", False, False)])
def test_references_stay_within_the_cap_and_the_bar_rejects_a_shifted_map(case, half, single):
    """The fp32 restatement against the float64 one on the GPU test's inputs: the elements where the references themselves disagree are at
    most CAP of each tensor (so the bar of tests/_head_bar.py has room for nothing but the kernel), the fp32 restatement itself passes the
    bar, and the same restatement reading the weights through a map that is off by one item does not."""
    B, h, w, H, W, Q, Cn = wr.CASES[case]
    p1, p2, lab, wt, item = wr.inputs(case, CD)
    if single:
        p1 = None
    r64 = wr.weighted_ref(p1, p2, lab, wt, item, 0.1, half, torch.float64, Cn)
    r32 = wr.weighted_ref(p1, p2, lab, wt, item, 0.1, half, torch.float32, Cn)
    wrong = wr.weighted_ref(p1, p2, lab, wt, wr.shifted(item, B), 0.1, half, torch.float32, Cn)
    assert len(set(np.asarray(wt).tolist())) == B, "equal weights: a shifted map would change nothing"
    for k in ("dpred2",) if single else ("dpred1", "dpred2"):
        m = hb.measure(r64[k], r32[k])
        assert int(m["excl"].sum()) <= hb.CAP * r64[k].numel(), (k, int(m["excl"].sum()), r64[k].numel())
        hb.grad_bar(r32[k], r64[k], r32[k], f"{case} {k}: the fp32 restatement")
        with pytest.raises(AssertionError, match="beyond tau"):
            hb.grad_bar(wrong[k], r64[k], r32[k], f"{case} {k}: weights from the wrong item")
    assert abs(float(r32["total"]) - float(r64["total"])) <= 1e-4 * (1 + abs(float(r64["total"])))
    assert abs(float(wrong["total"]) - float(r64["total"])) > 1e-4 * (1 + abs(float(r64["total"])))
