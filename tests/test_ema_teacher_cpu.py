"""The EMA teacher without a GPU (simt_amd/ema_teacher.py): the --ema-teacher flag's parsing, the C ABI's structs and signature,
the refresh schedule as a pure function of (updates, N), which shadow feeds which frozen tensor, and the train-state entry with its refusals on
fake trainers (CPU tensors; no launch is made: the refresh list is built, never run)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

from simt_amd import _lib, ema, ema_teacher
from simt_amd import train_state as tsf
from simt_amd.engine import LaunchList
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_as_specified(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    assert get_arguments([]).ema_teacher is None and get_arguments(["--ema", "0.9"]).ema_teacher is None          # default: off
    assert get_arguments(["--ema", "0.9", "--ema-teacher"]).ema_teacher == 1                                       # a bare flag: N = 1
    assert get_arguments(["--ema-teacher", "--ema"]).ema_teacher == 1 and get_arguments(["--ema-teacher", "--ema"]).ema == 0.999
    a = get_arguments(["--ema", "0.9", "--ema-teacher", "3", "--model", "DeepLabVGG"])
    assert a.ema_teacher == 3 and isinstance(a.ema_teacher, int) and a.ema == 0.9
    for argv, word in ((["--ema-teacher"], "--ema"), (["--ema-teacher", "2"], "--ema"), (["--ema", "0.9", "--ema-teacher", "0"], "integer >= 1"),
                       (["--ema", "0.9", "--ema-teacher", "-2"], None), (["--ema", "0.9", "--ema-teacher", "1.5"], "integer >= 1"),
                       (["--ema", "0.9", "--ema-teacher", "often"], "integer >= 1")):
        with pytest.raises(SystemExit) as e:
            get_arguments(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2, argv
        assert word is None or word in err, (argv, err)


def test_the_warmup_tool_has_no_such_flag(capsys):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(["--ema", "0.9", "--ema-teacher"])
    assert e.value.code == 2 and "--ema-teacher" in capsys.readouterr().err


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_symbol_signature_and_struct_sizes_match_the_header():
    header = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
    assert re.search(r"int simt_bn_fold_multi\(const simt_bn_fold_desc\* d, simt_stream_t stream\);", header)
    assert re.search(r"#define SIMT_ABI_VERSION 2\b", header) and _lib.ABI_VERSION == 2
    res, args = _lib.SIGNATURES["simt_bn_fold_multi"]
    assert res is C.c_int and args == [C.POINTER(_lib.BnFoldDesc), C.c_void_p]
    structs = {"simt_bn_fold_seg": (_lib.BnFoldSeg, ["gamma", "beta", "running_mean", "running_var", "scale", "shift", "C", "reserved_"]),
               "simt_bn_fold_desc": (_lib.BnFoldDesc, ["segs", "segs_host", "chunks", "nsegs", "nchunks", "chunk", "eps"])}
    assert all([f[0] for f in cls._fields_] == fields for cls, fields in structs.values())
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(){'
    for n, (_cls, fields) in structs.items():
        prog += f'printf("%zu", sizeof({n}));' + "".join(f'printf(" %zu", offsetof({n}, {f}));' for f in fields) + 'printf("\\n");'
    prog += "return 0;}"
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "p.c"), os.path.join(td, "p")
        open(cpath, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
        lines = subprocess.check_output([exe]).decode().splitlines()
    for line, (n, (cls, fields)) in zip(lines, structs.items()):
        out = list(map(int, line.split()))
        assert out[0] == C.sizeof(cls), f"{n}: ctypes {C.sizeof(cls)} vs C {out[0]}"
        assert out[1:] == [getattr(cls, f).offset for f in fields], n
    assert C.sizeof(_lib.BnFoldSeg) == 56 and "/* 56 bytes */" in header


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------------
def test_refresh_schedule_is_every_nth_update_and_never_before_the_first():
    for n in (1, 2, 3, 7):
        due = [u for u in range(0, 30) if ema_teacher.refresh_due(u, n)]
        assert due == list(range(n, 30, n)), (n, due)
    assert not ema_teacher.refresh_due(0, 1)                 # a fresh trainer (no update yet) and a resumed one at a multiple alike: only
    assert ema_teacher.refresh_due(4, 2) and not ema_teacher.refresh_due(3, 2)          # the update that REACHES the multiple refreshes
    # a run of 6 steps with N = 2 refreshes behind steps 2, 4, 6; cut at 3, the resumed half refreshes behind 4 and 6
    assert [u for u in range(4, 7) if ema_teacher.refresh_due(u, 2)] == [4, 6]
    for bad in (0, -1, 1.0, 2.5, "2", None, True):
        with pytest.raises(ValueError, match="ema_teacher_every"):
            ema_teacher.check_every(bad)
    assert ema_teacher.check_every(1) == 1 and ema_teacher.check_every(5) == 5


def test_which_shadow_feeds_which_frozen_tensor():
    student = {"conv1.weight": (64, 3, 7, 7), "bn1.running_var": (64,), "layer6.w": (19, 8, 3, 3), "layer6_1.w": (3, 8, 3, 3),
               "classifier.w": (22, 8, 3, 3), "classifier.b": (22,)}
    frozen = {"conv1.weight": (64, 3, 7, 7), "bn1.running_var": (64,), "layer6.w": (19, 8, 3, 3)}
    served, problems = ema_teacher.teacher_sources(frozen, student)
    assert not problems and served == {"conv1.weight": 64 * 147, "bn1.running_var": 64, "layer6.w": 19 * 72}          # layer6_1: no counterpart
    # the one-classifier model: the frozen model's 19 rows are the leading rows of a 19 + 3 row shadow -- only with prefix_rows = 3
    vgg = {"classifier.w": (19, 8, 3, 3), "classifier.b": (19,)}
    served, problems = ema_teacher.teacher_sources(vgg, student, prefix_rows=3)
    assert not problems and served == {"classifier.w": 19 * 72, "classifier.b": 19}
    for rows in (0, 2, 4):
        served, problems = ema_teacher.teacher_sources(vgg, student, prefix_rows=rows)
        assert not served and len(problems) == 2 and all(k in " ".join(problems) for k in vgg)
    served, problems = ema_teacher.teacher_sources({"ghost.weight": (2,), "conv1.weight": (64, 3, 7, 6)}, student, prefix_rows=3)
    assert not served and "ghost.weight: no shadow" in problems and any(p.startswith("conv1.weight: shadow of shape") for p in problems)


# ---- train state on fake trainers ---------------------------------------------------------------------------------------------------------------
class _FrozenPlan:
    """What TeacherRefresh asks of the frozen plan: its pack lists (empty: nothing is folded or packed here), its device, repack()."""
    dev = torch.device("cpu")

    def __init__(self):
        self._pack_items_raw, self.pack_list, self.repacks = [], LaunchList(), 0

    def repack(self):
        self.repacks += 1


class _FakeSimT(_Fake, ema_teacher.TeacherMixin):
    """test_ema_cpu._Fake with a frozen model (the closed-set part of its parameters, drawn from another seed) and the teacher keyword."""

    def __init__(self, ema_decay=None, every=None, seed=0, frozen=None):
        super().__init__(ema_decay=ema_decay, seed=seed)
        g = torch.Generator().manual_seed(77)
        self.fixed_params = frozen or {"conv.weight": torch.randn(4, 3, generator=g), "bn.running_mean": torch.randn(3, generator=g),
                                       "bn.num_batches_tracked": torch.tensor(5)}
        self.frozen_sha256 = tsf.state_sha256(self.fixed_params)
        self.lout = torch.zeros(16)
        self.fixed = _FrozenPlan()
        self._init_teacher(every)


def _refresh_on_host(tr):
    """The host twin of the refresh's first launch (the word copy); counts like TeacherRefresh.run."""
    for k in tr.teacher.copied:
        tr.fixed_params[k].copy_(tr.ema.shadow[k])
    tr.teacher.refreshes += 1


def _run(tr, steps):
    for _ in range(steps):
        _advanced(tr, 1)
        if ema_teacher.refresh_due(tr.ema.updates, tr.teacher.every):
            _refresh_on_host(tr)
    return tr


def test_constructor_refusals():
    with pytest.raises(ValueError, match="ema_decay"):
        _FakeSimT(every=1)
    for bad in (0, -3, 1.5, "1"):
        with pytest.raises(ValueError, match="ema_teacher_every"):
            _FakeSimT(ema_decay=0.9, every=bad)
    frozen = {"conv.weight": torch.zeros(4, 2), "ghost.bias": torch.zeros(2), "bn.running_mean": torch.zeros(3)}
    with pytest.raises(ValueError) as e:
        _FakeSimT(ema_decay=0.9, every=1, frozen=frozen)
    assert "conv.weight" in str(e.value) and "ghost.bias" in str(e.value) and "bn.running_mean" not in str(e.value)
    off = _FakeSimT(ema_decay=0.9)
    assert off.teacher is None
    for what in ("teacher_refreshes", "teacher_params"):
        with pytest.raises(RuntimeError, match="ema_teacher_every"):
            getattr(off, what)
    with pytest.raises(RuntimeError, match="ema_teacher_every"):
        off.teacher_state_dict()


def test_refresh_list_is_built_once_and_copies_floating_tensors_only():
    tr = _FakeSimT(ema_decay=0.9, every=2)
    t = tr.teacher
    assert list(t.copied) == ["conv.weight", "bn.running_mean"] and t.elements == 15            # no num_batches_tracked
    assert [fn for fn, _a in t.launches] == [_lib.load().simt_ema_multi] and t.fold_desc is None          # nothing to fold, nothing to pack here
    assert t.copy_desc.omd == 1.0 and t.copy_desc.nchunks == 2 and t.copy_desc.skip_if is None
    assert tr.teacher_params is tr.fixed_params and tr.teacher_refreshes == 0
    sd = tr.teacher_state_dict()
    assert list(sd) == list(tr.fixed_params) and int(sd["bn.num_batches_tracked"]) == 5


def test_train_state_carries_the_teacher_between_refreshes(no_device_sync):
    tr = _run(_FakeSimT(ema_decay=0.9, every=2), 3)
    assert tr.teacher_refreshes == 1 and tr.ema_updates == 3
    ts = tr.training_state()
    assert set(ts["teacher"]) == {"every", "refreshes", "params"} and ts["teacher"]["every"] == 2 and ts["teacher"]["refreshes"] == 1
    assert set(ts["teacher"]["params"]) == {"conv.weight", "bn.running_mean"}
    # the cut falls between refreshes: the teacher is the shadow of update 2, not the current one, and not the model the run started beside
    assert not torch.equal(ts["teacher"]["params"]["conv.weight"], ts["ema"]["shadow"]["conv.weight"])
    assert ts["frozen_sha256"] == tr.frozen_sha256 != tsf.state_sha256(tr.fixed_params)
    other = _FakeSimT(ema_decay=0.9, every=2, seed=1)
    assert other.frozen_sha256 == tr.frozen_sha256
    other.load_training_state(ts)
    assert other.teacher_refreshes == 1 and other.fixed.repacks == 1 and other.frozen_sha256 == tr.frozen_sha256
    assert all(torch.equal(other.fixed_params[k], tr.fixed_params[k]) for k in tr.fixed_params)
    _run(tr, 3), _run(other, 3)
    assert tr.teacher_refreshes == other.teacher_refreshes == 3
    assert all(torch.equal(other.fixed_params[k], tr.fixed_params[k]) for k in tr.fixed_params)
    # without the keyword the state has no such entry
    assert "teacher" not in _advanced(_FakeSimT(ema_decay=0.9)).training_state()


def test_load_training_state_refuses_each_teacher_mismatch_and_names_the_field(no_device_sync):
    with_t = _run(_FakeSimT(ema_decay=0.9, every=2), 3).training_state()
    without = _advanced(_FakeSimT(ema_decay=0.9)).training_state()

    def refused(tr, ts, *names):
        frozen = {k: v.clone() for k, v in tr.fixed_params.items()}
        _refused(tr, ts, *names)
        assert all(torch.equal(frozen[k], tr.fixed_params[k]) for k in frozen) and tr.fixed.repacks == 0, "a refused load changed the frozen model"

    refused(_FakeSimT(ema_decay=0.9, seed=1), with_t, "ema_teacher", "every 2", "does not move")                  # the flag is dropped
    refused(_FakeSimT(ema_decay=0.9, every=2, seed=1), without, "ema_teacher", "every 2", "written with a frozen model that does not move")   # added
    refused(_FakeSimT(ema_decay=0.9, every=1, seed=1), with_t, "ema_teacher every", "state: 2", "this trainer: 1")      # N differs
    params = with_t["teacher"]["params"]
    short = dict(with_t, teacher=dict(with_t["teacher"], params={k: v for k, v in params.items() if k != "bn.running_mean"}))
    refused(_FakeSimT(ema_decay=0.9, every=2, seed=1), short, "ema_teacher params", "bn.running_mean: missing")
    shaped = dict(with_t, teacher=dict(with_t["teacher"], params=dict(params, **{"conv.weight": torch.zeros(5)})))
    refused(_FakeSimT(ema_decay=0.9, every=2, seed=1), shaped, "ema_teacher params", "conv.weight: shape (5,)")
    # and the pure function, on its own
    assert ema_teacher.state_mismatch(None, None) is None
    assert ema_teacher.state_mismatch(_FakeSimT(ema_decay=0.9, every=2).teacher, with_t["teacher"]) is None
