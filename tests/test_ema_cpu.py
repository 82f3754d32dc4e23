"""The weight EMA without a GPU: the numpy restatement of the contract (tests/_ema_ref.py) against float64, the schedule, the C ABI's
struct and signature, the train-state refusals on fake trainers and the --ema flag's parsing."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _ema_ref as ref
from simt_amd import _lib, ema
from simt_amd import train_state as tsf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24             # unit roundoff of binary32, round to nearest
TINY = 2.0 ** -149           # the smallest subnormal: what gradual underflow may cost one multiply (half of it) -- additions are exact there


def _bound(e, w, o):
    """|restatement - exact| for x = e + o * (w - e) evaluated without rounding, from the operation count: three float32 operations,
    t = (w - e)(1 + d1), u = o t (1 + d2) + eta, r = (e + u)(1 + d3), |d_i| <= EPS, |eta| <= TINY / 2 (underflow of the product only).
    With U = o (w - e):  u = U + U th + eta, |th| <= 2 EPS + EPS^2, and r - x = U th + eta + (e + u) d3 with |e + u| <= |x| + |U th| + |eta|,
    so |r - x| <= |U| (2 EPS + EPS^2)(1 + EPS) + EPS |x| + (1 + EPS) |eta|  <=  EPS (|x| + 3 |U|) + TINY."""
    e, w, o = e.astype(np.float64), w.astype(np.float64), float(o)
    U = o * (w - e)
    return EPS * (np.abs(e + U) + 3.0 * np.abs(U)) + TINY


@pytest.mark.parametrize("o", [0.5, 2.0 ** -10, float(np.float32(1 - 0.999)), float(np.float32(0.1)), float(np.float32(1 / 3))])
def test_restatement_is_within_three_roundings_of_float64(o):
    rng = np.random.default_rng(11)
    n = 20000
    w = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 6, n)).astype(np.float32)
    e = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 6, n)).astype(np.float32)
    e[::5] = w[::5] * np.float32(1 + 2.0 ** -20)            # close pairs: cancellation in w - e
    got = ref.update(e, w, np.float32(o)).astype(np.float64)
    # D_t e + (1 - D_t) w with D_t = 1 - o, in float64 (its own rounding, ~2^-53 relative, is far below the bound)
    exact = (1.0 - o) * e.astype(np.float64) + o * w.astype(np.float64)
    err, bound = np.abs(got - exact), _bound(e, w, o) + 4 * 2.0 ** -53 * (np.abs(e.astype(np.float64)) + np.abs(w.astype(np.float64)))
    worst = int(np.argmax(err / bound))
    print(f"omd {o}: worst error / bound {err[worst] / bound[worst]:.3f}")
    assert np.all(err <= bound), (worst, err[worst], bound[worst])


def test_equal_values_do_not_move_and_minus_zero_becomes_plus_zero():
    rng = np.random.default_rng(2)
    w = rng.standard_normal(4096).astype(np.float32)
    w[:6] = [0.0, -0.0, 1e-41, -1e-41, 3.4e38, -1.1754944e-38]
    for o in (0.5, 2.0 ** -10, float(np.float32(0.001))):
        got = ref.update(w.copy(), w, np.float32(o))
        assert np.array_equal(got, w)                                       # as numbers
        same = ref.words(got) == ref.words(w)
        assert same[0] and not same[1] and same[2:].all() and ref.words(got)[1] == 0       # only -0.0 changes its word: it becomes +0.0
    # e = -0.0 beside w = +0.0 as well (the contract's documented case)
    assert ref.words(ref.update(np.array([-0.0], np.float32), np.array([0.0], np.float32), np.float32(0.5)))[0] == 0


def test_update_zero_copies_bits():
    w, e = ref.planted(64, np.random.default_rng(3))
    assert np.isnan(w).sum() >= 2 and (ref.words(w) == 0x80000000).any()
    assert ref.omd(0.999, 0) == np.float32(1.0)
    got = ref.update(e, w, ref.omd(0.999, 0))
    assert np.array_equal(ref.words(got), ref.words(w))
    assert got is not w and not np.shares_memory(got, w)


@pytest.mark.parametrize("D", [0.9, 0.99])
def test_running_mean_phase_equals_the_float64_mean(D):
    """After n <= 1 / (1 - D) updates the shadow is the running mean of the iterates: within the per-update bound times n (each update adds at most
    its own bound and scales what came before by 1 - omd <= 1).  The per-update bound is _bound's with one more EPS |U| for the schedule's own
    rounding of 1 / (t + 1) to float32, taken at the largest magnitudes of the sequence: |x| <= M, |U| <= 2 M."""
    n = int(round(1.0 / (1.0 - D)))
    rng = np.random.default_rng(5)
    seq = [rng.standard_normal(3000).astype(np.float32) for _ in range(n)]
    sh = ref.Shadow({"w": seq[0]}, D)
    for w in seq:
        sh.update({"w": w})
    assert sh.updates == n
    mean = np.mean(np.stack(seq).astype(np.float64), axis=0)
    M = max(float(np.abs(s).max()) for s in seq)
    bound = n * (EPS * (M + 4.0 * 2.0 * M) + TINY)
    err = np.abs(sh.e["w"].astype(np.float64) - mean)
    print(f"D {D}: n {n}, worst error {err.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound


@pytest.mark.parametrize("D", [0.0, 0.5, 0.9, 0.999, 0.9999])
def test_schedule(D):
    vals = [ref.omd(D, t) for t in range(20050)]
    assert all(v.dtype == np.float32 for v in vals[:3])
    assert vals[0] == np.float32(1.0) and ref.words(np.array([vals[0]]))[0] == 0x3F800000
    assert all(a >= b for a, b in zip(vals, vals[1:]))                       # monotone
    first = next(t for t in range(20050) if 1.0 / (t + 1) <= 1.0 - D)
    assert all(v == np.float32(1.0 - D) for v in vals[first:])
    assert all(np.float32(0) < v <= np.float32(1) for v in vals)
    # the library's schedule is the restatement's
    assert all(ema.omd_schedule(D, t) == vals[t] and ema.omd_schedule(D, t).dtype == np.float32 for t in list(range(40)) + [first, 20000])


def test_decay_must_lie_in_zero_one():
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema decay"):
            ema.check_decay(bad)
    assert ema.check_decay("0.9") == 0.9 and ema.check_decay(0) == 0.0


def test_symbol_signature_and_struct_size_match_the_header():
    header = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
    assert re.search(r"int simt_ema_multi\(const simt_ema_desc\* d, simt_stream_t stream\);", header)
    assert re.search(r"#define SIMT_ABI_VERSION 2\b", header) and _lib.ABI_VERSION == 2
    res, args = _lib.SIGNATURES["simt_ema_multi"]
    assert res is C.c_int and args == [C.POINTER(_lib.EmaDesc), C.c_void_p]
    fields = ["segs", "chunks", "nchunks", "chunk", "omd", "skip_if"]
    assert [f[0] for f in _lib.EmaDesc._fields_] == fields
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(){printf("%zu", sizeof(simt_ema_desc));' +
            "".join(f'printf(" %zu", offsetof(simt_ema_desc, {f}));' for f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "p.c"), os.path.join(td, "p")
        open(cpath, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
        out = list(map(int, subprocess.check_output([exe]).decode().split()))
    assert out[0] == C.sizeof(_lib.EmaDesc)
    assert out[1:] == [getattr(_lib.EmaDesc, f).offset for f in fields]
    # the segment record the host builds (simt_amd/ema.py) is the 24 bytes the header documents
    assert "(24 bytes each)" in header


# ---- train state on fake trainers ------------------------------------------------------------------------------------------------------------
class _Plan:
    layers = (1, 1, 2, 1)
    fbn_err = None

    def raise_on_fbn_error(self):
        pass

    def repack(self):
        self.repacked = True


class _Hp:
    def __init__(self):
        self.lr, self.iter_size = 1e-3, 1


class _Fake(tsf.TrainStateMixin, ema.EmaMixin):
    """A trainer's host side with CPU tensors: what training_state() / load_training_state() touch, nothing else."""

    def __init__(self, ema_decay=None, seed=0, extra=False, shape=(4, 3)):
        g = torch.Generator().manual_seed(seed)
        self.hp, self.B, self.H, self.W, self.dtype, self.dev, self.plan = _Hp(), 2, 8, 8, torch.float32, torch.device("cpu"), _Plan()
        self.params = {"conv.weight": torch.randn(*shape, generator=g), "bn.running_mean": torch.randn(3, generator=g),
                       "bn.num_batches_tracked": torch.tensor(0)}
        if extra:
            self.params["more.bias"] = torch.randn(2, generator=g)
        self.mom = {k: torch.zeros_like(v) for k, v in self.params.items() if k.endswith("weight") or k.endswith("bias")}
        self.it_done, self._bad_reported = 0, 0
        self.hout, self.bad_labels = torch.zeros(16), torch.zeros(1)
        self._init_ema(ema_decay)

    def _nbt_steps(self, key):
        return self.it_done

    def state_dict(self):
        return {k: (v.clone() if v.dtype != torch.long else torch.tensor(int(v) + self.it_done)) for k, v in self.params.items()}


def _snap(tr):
    out = {f"p {k}": v.clone() for k, v in tr.params.items()}
    if tr.ema is not None:
        out.update({f"e {k}": v.clone() for k, v in tr.ema.shadow.items()})
        out["updates"] = torch.tensor(tr.ema.updates)
    out["it_done"] = torch.tensor(tr.it_done)
    return out


def _refused(tr, ts, *names):
    before = _snap(tr)
    with pytest.raises(ValueError) as e:
        tr.load_training_state(ts)
    for n in names:
        assert n in str(e.value), (n, str(e.value))
    after = _snap(tr)
    assert all(torch.equal(before[k], after[k]) for k in before), "a refused load changed the trainer"


@pytest.fixture
def no_device_sync(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *_a, **_k: None)


def _advanced(tr, n=3):
    for i in range(n):
        for k, v in tr.params.items():
            if v.is_floating_point():
                v.add_(0.25 * (i + 1))
        if tr.ema is not None:                      # the host twin of the launch: the restatement
            o = ema.omd_schedule(tr.ema.decay, tr.ema.updates)
            for k, e in tr.ema.shadow.items():
                e.copy_(torch.from_numpy(ref.update(e.numpy(), tr.params[k].numpy(), o)))
            tr.ema.updates += 1
        tr.it_done += 1
    return tr


def test_train_state_carries_the_ema_and_round_trips(no_device_sync):
    tr = _advanced(_Fake(ema_decay=0.9))
    ts = tr.training_state()
    assert set(ts["ema"]) == {"decay", "updates", "shadow"} and ts["ema"]["decay"] == 0.9 and ts["ema"]["updates"] == 3
    assert set(ts["ema"]["shadow"]) == {"conv.weight", "bn.running_mean"}          # floating tensors only: no num_batches_tracked
    assert not torch.equal(ts["ema"]["shadow"]["conv.weight"], ts["model"]["conv.weight"])
    other = _Fake(ema_decay=0.9, seed=1)
    other.load_training_state(ts)
    assert other.ema_updates == 3 and other.it_done == 3
    a, b = _snap(tr), _snap(other)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    sd, esd = other.state_dict(), other.ema_state_dict()
    assert list(sd) == list(esd) and all(sd[k].dtype == esd[k].dtype and sd[k].shape == esd[k].shape for k in sd)
    assert int(esd["bn.num_batches_tracked"]) == int(sd["bn.num_batches_tracked"]) == 3
    assert set(other.ema_params) == set(other.params) and other.ema_params["bn.num_batches_tracked"] is other.params["bn.num_batches_tracked"]


def test_train_state_without_ema_round_trips_unchanged(no_device_sync):
    tr = _advanced(_Fake())
    ts = tr.training_state()
    assert "ema" not in ts and set(ts) == {"model", "momentum", "it_done", "bad_reported", "hyper", "accumulators"}
    assert "ema_decay" not in ts["hyper"] and "ema_decay" not in tsf.CHECKED_FIELDS
    other = _Fake(seed=1)
    other.load_training_state(ts)
    a, b = _snap(tr), _snap(other)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(RuntimeError, match="ema_decay"):
        other.ema_params
    with pytest.raises(RuntimeError, match="ema_decay"):
        other.ema_state_dict()


def test_load_training_state_refuses_each_ema_mismatch_and_names_it(no_device_sync):
    with_ema = _advanced(_Fake(ema_decay=0.9)).training_state()
    without = _advanced(_Fake()).training_state()
    _refused(_Fake(seed=1), with_ema, "ema", "this trainer has none")                      # the state has one, the trainer does not
    _refused(_Fake(ema_decay=0.9, seed=1), without, "ema", "written without one")           # the trainer has one, the state does not
    _refused(_Fake(ema_decay=0.99, seed=1), with_ema, "ema decay", "0.9", "0.99")           # both values named
    shadow = with_ema["ema"]["shadow"]
    short = dict(with_ema, ema=dict(with_ema["ema"], shadow={k: v for k, v in shadow.items() if k != "bn.running_mean"}))
    _refused(_Fake(ema_decay=0.9, seed=1), short, "ema shadow", "bn.running_mean: missing")
    more = dict(with_ema, ema=dict(with_ema["ema"], shadow=dict(shadow, **{"ghost.weight": torch.zeros(2)})))
    _refused(_Fake(ema_decay=0.9, seed=1), more, "ema shadow", "ghost.weight: unknown")
    shaped = dict(with_ema, ema=dict(with_ema["ema"], shadow=dict(shadow, **{"conv.weight": torch.zeros(5)})))
    _refused(_Fake(ema_decay=0.9, seed=1), shaped, "ema shadow", "conv.weight: shape (5,)")


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool", ["trainV2_simt", "trainV1_warmup"])
def test_ema_flag_parsing(tool, capsys):
    import importlib
    get = importlib.import_module("simt_amd.tools." + tool).get_arguments
    assert get([]).ema is None
    assert get(["--ema"]).ema == 0.999
    assert get(["--ema", "--synthetic"]).ema == 0.999
    assert get(["--ema", "0.9"]).ema == 0.9 and get(["--ema", "0"]).ema == 0.0
    for bad in ("1.0", "-0.1", "x"):
        with pytest.raises(SystemExit):
            get(["--ema", bad])
        assert "--ema" in capsys.readouterr().err


def test_second_rotation_travels_in_the_train_state_file(tmp_path, capsys):
    from simt_amd.tools.trainV2_simt import EmaSnapshots, SnapshotKeeper, TrainStateFile, get_arguments

    class Tr:
        it_done, ema_params = 4, {}

        def __init__(self, on):
            self.ema = object() if on else None

        def training_state(self):
            return {"it_done": 4, "hyper": {}}

        def load_training_state(self, ts):
            pass

        def state_dict(self):
            return {"w": torch.zeros(1)}

        def ema_state_dict(self):
            return {"w": torch.ones(1)}

    f = str(tmp_path / "run.state")
    args = get_arguments(["--train-state", f, "--snapshot-dir", str(tmp_path)])
    # off: the file's loop part is what it always was, EmaSnapshots does nothing
    tr, keeper, rf = Tr(False), SnapshotKeeper(str(tmp_path), "GTA5_iter"), TrainStateFile(args, 0, 1)
    snap = EmaSnapshots(tr, keeper, rf, 0)
    snap.rolling(2), snap.final(str(tmp_path), 4), snap.evaluated(lambda p: 1 / 0, 2)
    rf.write(tr, keeper)
    assert tsf.load(f)[2] == {"world": 1, "run": {}} and sorted(os.listdir(tmp_path)) == ["run.state"]
    # on: a keeper `GTA5_ema_iter`, carried and continued
    tr, keeper, rf = Tr(True), SnapshotKeeper(str(tmp_path), "GTA5_BAPA_warmup_iter"), TrainStateFile(args, 0, 1)
    snap = EmaSnapshots(tr, keeper, rf, 0)
    assert snap.keeper.stem == "GTA5_BAPA_warmup_ema_iter"
    snap.rolling(2)
    snap.final(str(tmp_path), 4)
    rf.write(tr, keeper)
    assert tsf.load(f)[2]["ema_keeper"] == {"best_mIoU": 0, "best_iter": 0, "rolling_iter": 2}
    assert sorted(os.listdir(tmp_path)) == ["GTA5_4_ema.pth", "GTA5_BAPA_warmup_ema_iter2.pth", "run.state"]
    keeper2, rf2 = SnapshotKeeper(str(tmp_path), "GTA5_BAPA_warmup_iter"), TrainStateFile(args, 0, 1)
    snap2 = EmaSnapshots(tr, keeper2, rf2, 0)
    assert rf2.resume(tr, keeper2) == 4 and snap2.keeper.rolling_iter == 2
    snap2.rolling(4)                                                          # removes the file the first half left
    assert sorted(os.listdir(tmp_path)) == ["GTA5_4_ema.pth", "GTA5_BAPA_warmup_ema_iter4.pth", "run.state"]
    snap2.evaluated(lambda params: 41.5, 6)
    assert "EMA mIoU:  41.5" in capsys.readouterr().out and os.path.exists(tmp_path / "GTA5_BAPA_warmup_ema_iter6_mIoU41.5.pth")
