"""Online labels without a GPU: the descriptor of simt_online_label against the header, the flags of trainV1_warmup and their
refusals, the run identity, the label-less dataset, the keywords' checks, the `labelled` read-out and the train-state refusals on fake
trainers."""
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
from simt_amd.ema_teacher import refresh_due
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
CD = so.load_class_dist()


# ---- header and descriptor ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbol_and_the_descriptor_matches_ctypes():
    assert re.search(r"int simt_online_label\(const simt_online_label_desc\* d, simt_stream_t stream\);", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    fields = [n for n, _t in L.OnlineLabelDesc._fields_]
    assert fields == ["fix", "label", "counts", "B", "h", "w", "ld", "H", "W", "C", "family", "threshold"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(simt_online_label_desc));' +
           "".join(f'printf("{n} %zu\\n", offsetof(simt_online_label_desc, {n}));' for n in fields) +
           'printf("label %zu\\n", sizeof(*((simt_online_label_desc*)0)->label));return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe])
        out = dict(ln.split(None, 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    assert C.sizeof(L.OnlineLabelDesc) == int(out["size"]) == 64 and int(out["label"]) == 8
    for n in fields:
        assert getattr(L.OnlineLabelDesc, n).offset == int(out[n]), n
    assert L.SIGNATURES["simt_online_label"] == (C.c_int, [C.POINTER(L.OnlineLabelDesc), C.c_void_p])
    # the export kernels it is held to keep their prototypes
    assert len(L.SIGNATURES["simt_pseudo_label_u8"][1]) == 17 and len(L.SIGNATURES["simt_pseudo_label2_u8"][1]) == 21


def test_a_library_without_the_symbol_names_it(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name == "simt_online_label":
                raise AttributeError(name)
            return lambda *a: L.ABI_VERSION
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(L, "LIB_PATH", __file__)
    with pytest.raises(L.SimtHipError, match=r"simt_online_label\b.*rebuild"):
        L.load()


# ---- the flags --------------------------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_default():
    from simt_amd.tools.trainV1_warmup import get_arguments
    a = get_arguments([])
    assert a.online_labels is None and a.online_labels_every is None
    assert get_arguments(["--online-labels"]).online_labels == 0.968 == ol.DEFAULT_THRESHOLD
    assert get_arguments(["--online-labels", "0"]).online_labels == 0.0 and get_arguments(["--online-labels", "0.5"]).online_labels == 0.5
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        a = get_arguments(["--model", model, "--online-labels", "0.9", "--ema", "--online-labels-every", "3", "--colour-jitter", "--mask-patches"])
        assert (a.online_labels, a.online_labels_every, a.ema) == (0.9, 3, 0.999)
    assert get_arguments(["--online-labels", "--synthetic"]).online_labels == 0.968          # --synthetic: the flag works, labels are ignored
    assert get_arguments(["--online-labels", "--ema", "0.9", "--online-labels-every", "1"]).online_labels_every == 1


@pytest.mark.parametrize("argv,named", [
    (["--online-labels-every", "2", "--online-labels"], "--online-labels-every needs --ema"),
    (["--online-labels-every", "2", "--ema"], "--online-labels-every needs --online-labels"),
    (["--online-labels-every", "2"], "--online-labels-every needs --online-labels"),
    (["--online-labels", "1"], "argument --online-labels"), (["--online-labels", "1.5"], "argument --online-labels"),
    (["--online-labels", "-0.1"], "argument --online-labels"), (["--online-labels", "nan"], "argument --online-labels"),
    (["--online-labels", "x"], "argument --online-labels"),
    (["--online-labels", "--ema", "--online-labels-every"], "argument --online-labels-every: expected one argument"),          # a bare N
    (["--online-labels", "--ema", "--online-labels-every", "0"], "argument --online-labels-every"),
    (["--online-labels", "--ema", "--online-labels-every", "1.5"], "argument --online-labels-every"),
    (["--online-labels", "--class-mix", "--batch-size", "2"], "--online-labels cannot be combined with --class-mix"),
])
def test_flag_refusals_exit_2_and_name_the_flag(capsys, argv, named):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and named in err, (argv, err)


def test_the_simt_tool_gets_no_such_flag(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    for flag in (["--online-labels"], ["--online-labels-every", "2"]):
        with pytest.raises(SystemExit) as e:
            get_arguments(flag)
        assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_start_up_line_says_who_labels(capsys):
    from simt_amd.tools import trainV2_simt as shared
    from simt_amd.tools.trainV1_warmup import get_arguments
    shared.online_label_line(get_arguments([]))
    assert capsys.readouterr().out == ""
    shared.online_label_line(get_arguments(["--online-labels"]))
    out = capsys.readouterr().out
    assert "a fixed teacher" in out and "> 0.968" in out and "the same batch as the student" in out
    shared.online_label_line(get_arguments(["--online-labels", "0.9", "--ema", "0.99", "--online-labels-every", "4", "--gaussian-blur", "--mask-patches"]))
    out = capsys.readouterr().out
    assert "follows the weight EMA (decay 0.99), refreshed every 4 update(s)" in out and "> 0.9;" in out
    assert "the batch before --gaussian-blur, --mask-patches (the weak view)" in out
    shared.online_label_line(get_arguments(["--online-labels", "--colour-jitter", "--synthetic"]))          # with --synthetic they do nothing
    assert "the same batch as the student" in capsys.readouterr().out


def test_step_args_and_the_loss_line_text():
    from simt_amd.tools import trainV1_warmup as tool
    off, on, on2 = tool.get_arguments([]), tool.get_arguments(["--online-labels"]), tool.get_arguments(["--online-labels", "--iter-size", "2"])
    assert tool.step_args(off, [("i", "l")]) == (("i", "l"), {})
    assert tool.step_args(on, [("i", None, None)]) == (("i", None), {})
    assert tool.step_args(on, [("i", None, "w")]) == (("i", None), {"teacher_image": "w"})
    assert tool.step_args(on2, [("i", None, "w"), ("j", None, "v")]) == ((["i", "j"], None), {"teacher_image": ["w", "v"]})
    assert tool.step_args(on2, [("i", None, None), ("j", None, None)]) == ((["i", "j"], None), {})
    assert tool.labelled_text(off, {}) == "" and tool.labelled_text(on, {"labelled": 0.51249}) == " labelled = 0.512"


# ---- run identity -----------------------------------------------------------------------------------------------------------------------------------
def test_run_identity_carries_the_flag_only_when_it_is_on():
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    off = shared.run_identity(tool.get_arguments([]), cd)
    on = shared.run_identity(tool.get_arguments(["--online-labels"]), cd)
    moving = shared.run_identity(tool.get_arguments(["--online-labels", "0.9", "--ema", "--online-labels-every", "2"]), cd)
    assert "online_labels" not in off and on["online_labels"] == [0.968, None] and moving["online_labels"] == [0.9, 2]
    assert {k: v for k, v in on.items() if k != "online_labels"} == off
    assert shared.RUN_DEFAULTS["online_labels"] is False
    assert shared.run_identity(tool.get_arguments(["--online-labels", "--synthetic"]), cd)["online_labels"] == [0.968, None]


def test_train_state_file_refuses_the_flag_added_dropped_or_changed(tmp_path, no_device_sync):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    base = ["--ema", "0.9", "--train-state", str(tmp_path / "s.state")]

    class Keeper:
        def state(self):
            return {}

        def load_state(self, s):
            pass
    on, moving = ["--online-labels", "0.9"], ["--online-labels", "0.9", "--online-labels-every", "2"]
    for first, others in ((on, ([], ["--online-labels", "0.8"], moving)), ([], (on,)), (moving, (on, ["--online-labels", "0.9", "--online-labels-every", "3"]))):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(_advanced(_Fake(ema_decay=0.9)), Keeper())
        assert shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper()) == 3
        for second in others:
            with pytest.raises(SystemExit, match="online_labels"):
                shared.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper())


# ---- the label-less dataset -----------------------------------------------------------------------------------------------------------------------
def _files(tmp_path, lines):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    (tmp_path / "img").mkdir()
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (8, 12, 3), dtype=np.uint8)).save(tmp_path / "img" / f"f{i}.png")
    (tmp_path / "list.lst").write_text("\n".join(lines) + "\n")
    return str(tmp_path), str(tmp_path / "list.lst")


def test_dataset_without_labels_parses_one_and_two_columns_and_opens_no_label_file(tmp_path):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    root, lst = _files(tmp_path, ["img/f0.png", "img/f1.png lab/f1_pseudo.png", "", "img/f2.png"])          # no lab/ directory exists
    ds = cityscapesPseudo(root, lst, crop_size=(12, 8), labels=False, photometric=(0.2, None), teacher_view=True)
    assert len(ds) == 3 and ds.labels is False and ds.teacher_view and ds.photometric == (0.2, None)
    assert [f["name"] for f in ds.files] == ["f0", "f1", "f2"] and all("label" not in f for f in ds.files)          # the name: from the IMAGE path
    for i in range(3):
        rgb, lab, name = ds.decode(i)
        assert rgb.shape == (8, 12, 3) and rgb.dtype == np.uint8 and lab is None and name == f"f{i}"
        assert ds.cache_key(i) == (os.path.join(root, f"img/f{i}.png"), None)                                          # the image alone
    assert len(cityscapesPseudo(root, lst, max_iters=7, labels=False)) == 9
    # with labels (the default) the same list is what it always was: two columns per line, the label file opened
    with pytest.raises(ValueError):
        cityscapesPseudo(root, lst, crop_size=(12, 8))
    root2, lst2 = root, str(tmp_path / "pairs.lst")
    open(lst2, "w").write("img/f1.png lab/f1_pseudo.png\n")
    with_labels = cityscapesPseudo(root2, lst2, crop_size=(12, 8))
    assert with_labels.labels is True and with_labels.files[0]["name"] == "f1_pseudo"
    with pytest.raises(FileNotFoundError):
        with_labels.decode(0)
    open(lst, "w").write("img/f0.png a b\n")
    with pytest.raises(ValueError, match=r"list\.lst:1: .*3 columns"):
        cityscapesPseudo(root, lst, labels=False)
    with pytest.raises(ValueError, match="class_mix"):
        cityscapesPseudo(root, lst2, labels=False, class_mix=(19, 1.0))


# ---- the keywords ---------------------------------------------------------------------------------------------------------------------------------
def test_keyword_checks_name_the_keyword():
    assert ol.check_settings(None, None, None) == (None, None) and ol.check_settings(None, None, 0.9) == (None, None)
    assert ol.check_settings(0.5, None, None) == (0.5, None) and ol.check_settings(0, 2, 0.9) == (0.0, 2)
    assert ol.check_settings("0.968", np.int64(1), 0.0) == (0.968, 1)
    for tau in (1.0, 1, -0.01, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match=r"^online_labels "):
            ol.check_settings(tau, None, None)
    for every in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match=r"^online_labels_every "):
            ol.check_settings(0.5, every, 0.9)
    with pytest.raises(ValueError, match="online_labels_every needs online_labels"):
        ol.check_settings(None, 2, 0.9)
    with pytest.raises(ValueError, match="online_labels_every needs ema_decay"):
        ol.check_settings(0.5, 2, None)


def test_refresh_due_is_reused_as_it_is():
    """The moving teacher is ema_teacher's: behind every N-th EMA update, never before the first (TeacherMixin._teacher_follows)."""
    assert ol.OnlineLabelMixin._teacher_follows is __import__("simt_amd.ema_teacher", fromlist=["x"]).TeacherMixin._teacher_follows
    assert [u for u in range(0, 9) if refresh_due(u, 1)] == list(range(1, 9))
    assert [u for u in range(0, 9) if refresh_due(u, 3)] == [3, 6]
    ran = []

    class Tr(ol.OnlineLabelMixin):
        pass
    tr = Tr()
    tr.ema = type("E", (), {"updates": 0})()
    tr.teacher = type("T", (), {"every": 2, "run": lambda self, st: ran.append(tr.ema.updates)})()
    for u in range(1, 7):
        tr.ema.updates = u
        tr._teacher_follows(None)
    assert ran == [2, 4, 6]


def test_labelled_share_diffs_the_cumulative_counts():
    share, rep = ol.labelled_share([3, 0, 5, 8], [0, 0])            # classes 0..2, then the 255s
    assert share == 0.5 and rep == [8, 16]
    share, rep = ol.labelled_share([3, 1, 5, 17], rep)              # since then: 1 labelled of 10
    assert share == 0.1 and rep == [9, 26]
    assert ol.labelled_share([3, 1, 5, 17], rep) == (0.0, [9, 26])          # nothing counted since


# ---- train state on fake trainers -----------------------------------------------------------------------------------------------------------------
class _FakeTeacher:
    def __init__(self, every, seed):
        self.every, self.refreshes = every, 0
        self.fixed_params = {"conv.weight": torch.randn(4, 3, generator=torch.Generator().manual_seed(100 + seed))}
        self.copied = {"conv.weight": 12}

    def state(self):
        return {"every": self.every, "refreshes": self.refreshes, "params": {k: v.clone() for k, v in self.fixed_params.items()}}

    def load_state(self, saved):
        self.fixed_params["conv.weight"].copy_(saved["params"]["conv.weight"])
        self.refreshes = int(saved["refreshes"])


def _FakeOnline(tau=None, every=None, seed=0, start=7):
    """test_ema_cpu._Fake with what the warm-up trainers set for the keywords (same class: the state names its trainer)."""
    tr = _Fake(ema_decay=0.9, seed=seed)
    tr.online_labels, tr.teacher = tau, None
    if tau is not None:
        tr.frozen_sha256 = tsf.state_sha256({"w": torch.full((2,), float(start))})
        tr.label_counts, tr._counts_reported = torch.zeros(4, dtype=torch.int64), [0, 0]
        if every is not None:
            tr.teacher = _FakeTeacher(every, seed)
    return tr


def test_hyper_carries_the_keywords_only_when_on_and_mismatches_name_the_field(no_device_sync):
    plain = _advanced(_FakeOnline()).training_state()
    legacy = _advanced(_Fake(ema_decay=0.9)).training_state()
    assert plain["hyper"] == legacy["hyper"] and plain.keys() == legacy.keys() and set(plain["accumulators"]) == {"hout", "bad_labels"}
    assert not any(k.startswith("online") for k in plain["hyper"]) and "frozen_sha256" not in plain
    fixed_tr = _advanced(_FakeOnline(0.9))
    fixed_tr.label_counts += torch.tensor([5, 0, 2, 9])
    fixed_tr._counts_reported = [3, 6]
    fixed = fixed_tr.training_state()
    assert fixed["hyper"]["online_labels"] == 0.9 and "online_labels_every" not in fixed["hyper"] and "teacher" not in fixed
    assert {k: v for k, v in fixed["hyper"].items() if k != "online_labels"} == plain["hyper"]
    assert fixed["accumulators"]["label_counts"].tolist() == [5, 0, 2, 9] and fixed["accumulators"]["counts_reported"] == [3, 6]
    moving_tr = _advanced(_FakeOnline(0.9, 2))
    moving_tr.teacher.refreshes = 1
    moving = moving_tr.training_state()
    assert moving["hyper"]["online_labels_every"] == 2 and moving["teacher"]["every"] == 2 and moving["teacher"]["refreshes"] == 1
    assert tsf.VALUE_FIELDS == ("online_labels", "online_labels_every") and not set(tsf.VALUE_FIELDS) & set(tsf.CHECKED_FIELDS + tsf.SWITCH_FIELDS)
    # the keyword added, dropped, tau or N differing: the field is named with both values
    _refused(_FakeOnline(seed=1), fixed, "online_labels (state: 0.9, this trainer: None)")
    _refused(_Fake(ema_decay=0.9, seed=1), fixed, "online_labels (state: 0.9, this trainer: None)")          # a trainer from before the keyword
    _refused(_FakeOnline(0.9, seed=1), plain, "online_labels (state: None, this trainer: 0.9)")
    _refused(_FakeOnline(0.8, seed=1), fixed, "online_labels (state: 0.9, this trainer: 0.8)")
    _refused(_FakeOnline(0.9, 2, seed=1), fixed, "online_labels_every (state: None, this trainer: 2)")
    _refused(_FakeOnline(0.9, seed=1), moving, "online_labels_every (state: 2, this trainer: None)")
    _refused(_FakeOnline(0.9, 3, seed=1), moving, "online_labels_every (state: 2, this trainer: 3)")
    _refused(_FakeOnline(0.9, seed=1, start=8), fixed, "frozen_sha256 differs")
    # what fits loads: the counts and their host twin come back, and a moving teacher with its refresh count
    tr = _FakeOnline(0.9, seed=1)
    tr.load_training_state(fixed)
    assert tr.it_done == 3 and tr.label_counts.tolist() == [5, 0, 2, 9] and tr._counts_reported == [3, 6]
    tr = _FakeOnline(0.9, 2, seed=1)
    tr.load_training_state(moving)
    assert tr.teacher.refreshes == 1 and torch.equal(tr.teacher.fixed_params["conv.weight"], moving["teacher"]["params"]["conv.weight"])
    for ts, t in ((plain, _FakeOnline(seed=1)), (legacy, _FakeOnline(seed=1)), (plain, _Fake(ema_decay=0.9, seed=1))):
        t.load_training_state(ts)
        assert t.it_done == 3
    assert tsf.value_mismatches({}, {}) == [] and tsf.value_mismatches({"online_labels": 0.5}, {"online_labels": 0.5}) == []
    assert tsf.value_mismatches({"online_labels": 0.5}, {}) == ["online_labels"] == tsf.value_mismatches({}, {"online_labels": 0.5})
    assert tsf.value_mismatches({"online_labels": 0.5, "online_labels_every": 1}, {"online_labels": 0.5, "online_labels_every": 2}) == ["online_labels_every"]
