"""Resuming a run: k steps, `training_state()`, a trip through the train-state file, a NEW trainer, `load_training_state()`, n - k steps
== n steps.  Every comparison is between two executions of the same arithmetic and therefore BITWISE (torch.equal); no tolerance anywhere.

  1. trainer level, all four trainers: the losses of steps 4-6, every tensor of state_dict() (num_batches_tracked included), every momentum
     buffer, NTM, W and Adam moment; straight after the load the plan's packed operands equal a fresh plan's (tests/_operand_coherence.py).
     A CONTROL runs the uninterrupted trainer twice and asks the same: if it fails, the resume cases mean nothing.
  2. what load_training_state refuses, and the bad-label accumulator across a resume.
  3. GpuLoader(start_batch=n): the tail of the default loader's batches, no skipped item decoded.
  4. both tools x three models: `--num-steps-stop 3 --train-state F`, then the same command with `--num-steps-stop 6`, against one run of 6.
"""
import contextlib
import glob
import os
import re

import pytest
import torch

import _operand_coherence as oc
from oracle import simt_oracle as so
from simt_amd import train_state as tsf
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import GpuLoader
from simt_amd.engine_v3 import v3_state_shapes
from simt_amd.step import Hyper, SimTTrainer, WarmupTrainer
from simt_amd.step_single import SimTSingleTrainer, WarmupSingleTrainer
from test_gpu_dataset_cache import _assert_same_batches, _collect, _Counting, _dataset, _tool_files, _write_files
from test_gpu_single import VGG_SMALL, _v3_state, _vgg_state
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF, F32 = torch.bfloat16, torch.float32
SMALL = (1, 1, 2, 1)
K = 3
# num_steps = 20: the poly learning rate falls by ~5 % per step, so a resumed trainer that counts its iterations from 0 again is far off
HP = dict(lr=6e-4, lr_T=6e-3, num_steps=20)
# The reduced VGG has no BatchNorm and its optimiser lists every tensor: six bf16 steps at 6e-4 on its random state overflow (every loss NaN, in
# the uninterrupted run already).  A tenth of the 2.5e-4 the three-step VGG tests of tests/test_gpu_single.py use keeps six steps finite.
VGG_LR = 2.5e-5

# case -> (trainer kind, keyword arguments)
CASES = {
    "SimTTrainer": ("simt", {}),                                              # the default schedule: early SGD on the side stream
    "SimTTrainer-late_sgd": ("simt", {"late": True}),
    "SimTTrainer-iter_size2": ("simt", {"iter_size": 2}),                       # the _grad_acc path, early SGD off
    "SimTTrainer-fp32_512": ("simt", {"dtype": F32, "size": (1, 512, 512)}),    # configs[0]'s size, reduced depth
    "SimTTrainer-rccl_one_rank": ("simt", {"dp": True}),
    "WarmupTrainer": ("warmup", {}),
    "WarmupTrainer-iter_size2": ("warmup", {"iter_size": 2}),
    "SimTSingleTrainer-v3": ("simt1", {"model": "v3"}),
    "SimTSingleTrainer-vgg": ("simt1", {"model": "vgg", "lr": VGG_LR}),
    "WarmupSingleTrainer-v3": ("warmup1", {"model": "v3"}),
    "WarmupSingleTrainer-vgg": ("warmup1", {"model": "vgg", "lr": VGG_LR}),
    "WarmupSingleTrainer-v3-iter_size2": ("warmup1", {"model": "v3", "iter_size": 2}),
}


def _size(kind, kw):
    return kw.get("size", (2, 97, 97) if kind in ("simt", "warmup") else (2, 96, 128))


def make(kind, kw, dev, pg=None, seed=0, hp_kw=None, frozen_seed=0, size=None):
    """The trainer of a case.  `seed` moves the weights and NTMs the trainer is GIVEN (a resumed trainer is built from other ones: the load
    replaces them); the frozen model stays (`frozen_seed` moves it, for the refusal test)."""
    B, H, W = size or _size(kind, kw)
    dtype = kw.get("dtype", BF)
    hkw = dict(HP, iter_size=kw.get("iter_size", 1))
    if "lr" in kw:
        hkw["lr"] = kw["lr"]
    hkw.update(hp_kw or {})
    if kind in ("simt", "warmup"):
        Kx = K if kind == "simt" else 0
        st = so.recipe_state(so.state_shapes(19, Kx, kind == "simt", layers=SMALL), seed=31 + seed, head_scale=8.0)
        if kind == "warmup":
            return WarmupTrainer(st, Hyper(open_classes=0, **hkw), B, H, W, dtype=dtype, device=dev, layers=SMALL, process_group=pg)
        fst = so.recipe_state(so.state_shapes(19, 0, False, layers=SMALL), seed=32 + frozen_seed, head_scale=8.0)
        return SimTTrainer(st, fst, so.ntm_init(19, K, 911 + seed), so.ntm_init(19, K, 912 + seed), Hyper(open_classes=K, **hkw), CD.numpy(),
                           B, H, W, dtype=dtype, device=dev, layers=SMALL, process_group=pg)
    model, warm = kw["model"], kind == "warmup1"
    if model == "v3":
        Kx, layers, width, ac = (0 if warm else 6), (1, 2, 2), 64, 64
        st = _v3_state(v3_state_shapes(19, Kx, not warm, layers, width, ac), 3 + 10 * seed)
        fst = _v3_state(v3_state_shapes(19, 0, False, layers, width, ac), 4 + 10 * frozen_seed)
        arch = {"layers": layers, "width": width, "assp_ch": ac}
    else:
        Kx = 0 if warm else 3
        lay = [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in VGG_SMALL]
        st, fst = _vgg_state(19 + Kx, lay, 5 + 10 * seed), _vgg_state(19, lay, 6 + 10 * frozen_seed)
        arch = {"vgg_layers": lay}
    if warm:
        return WarmupSingleTrainer(model, st, Hyper(open_classes=0, **hkw), B, H, W, dtype=dtype, device=dev, arch=arch, process_group=pg)
    return SimTSingleTrainer(model, st, fst, so.ntm_init(19, Kx, 9 + seed), Hyper(open_classes=Kx, **hkw), CD.numpy(), B, H, W, dtype=dtype,
                             device=dev, arch=arch, process_group=pg)


def batches(kind, kw, dev, n=6, bad_at=None):
    B, H, W = _size(kind, kw)
    its = kw.get("iter_size", 1)
    out = []
    for i in range(n):
        mb = [so.synthetic_batch(B, H, W, CD.numpy(), seed=700 + 10 * i + j, block=8) for j in range(its)]
        mb = [(img.to(dev), lab.to(dev)) for img, lab in mb]
        if bad_at == i:
            mb[-1][1][0, 3, 4:7] = 200                     # three label values outside [0, 19) that are not 255
        out.append(mb[0] if its == 1 else ([m[0] for m in mb], [m[1] for m in mb]))
    return out


def scalars(tr):
    """The device scalars `losses()` reads, as they are after the last step -- as bit patterns: the warm-up head leaves NaN in slots of `hout`
    that no one reads, and the comparison is bitwise."""
    return (tr.lout if hasattr(tr, "lout") else tr.hout[:16]).clone().view(torch.int32)


def finite_losses(tr, what):
    l = tr.losses()                                        # (raises for a bad label or a BatchNorm time-out)
    assert l and all(v == v and abs(v) != float("inf") for v in l.values()), f"{what}: losses {l}"
    return l


def full_state(tr):
    """Everything a resume must reproduce, on the host."""
    torch.cuda.synchronize()
    out = {f"model {k}": v for k, v in tr.state_dict().items()}
    out.update({f"momentum {k}": v.cpu() for k, v in tr.mom.items()})
    for f in tsf.NTM_FIELDS:
        if hasattr(tr, f):
            v = getattr(tr, f)
            out.update({f"{f}[{i}]": t.cpu() for i, t in enumerate(v)} if isinstance(v, list) else {f: v.cpu()})
    out["it_done"] = torch.tensor(tr.it_done)
    for i, dsts in enumerate(oc.snapshot(tr.plan)):        # what the NEXT step would read: every destination of the plan's pack list
        out.update({f"packed operand {i}.{j}": t.cpu() for j, t in enumerate(dsts)})
    return out


def straight(kind, kw, dev, pg, data):
    tr = make(kind, kw, dev, pg)
    louts = []
    for b in data:
        tr.step(*b)
        louts.append(scalars(tr))
    finite_losses(tr, "uninterrupted run, step 6")
    res = louts, full_state(tr)
    del tr
    torch.cuda.empty_cache()
    return res


def split(kind, kw, dev, pg, data, path, k=3):
    tr = make(kind, kw, dev, pg)
    louts = []
    for b in data[:k]:
        tr.step(*b)
        louts.append(scalars(tr))
    ts = tr.training_state()
    seen = finite_losses(tr, f"step {k}")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    torch.cuda.empty_cache()
    ts, _keeper, _loop = tsf.load(path)
    assert ts["it_done"] == k and all(not t.is_cuda for t in list(ts["model"].values()) + list(ts["momentum"].values()))
    tr = make(kind, kw, dev, pg, seed=1)                   # other weights, other NTMs: the load replaces them
    tr.load_training_state(ts)
    assert tr.it_done == k and tr.losses() == seen, "losses() straight after the load differ from the losses() of the trainer that was saved"
    fresh = oc.fresh_plan(tr.plan, oc.device_state(tr.state_dict(), dev))
    bad, _ = oc.compare(tr.plan, fresh, "a fresh plan built from the loaded masters (STALE)")
    assert not bad, "operands after load_training_state: " + "; ".join(bad[:8])
    del fresh
    loaded, m0 = oc.snapshot(tr.plan), oc.masters(tr)
    for b in data[k:]:
        tr.step(*b)
        louts.append(scalars(tr))
    # the steps after the load re-pack what they update: not vacuous only if packed weight operands really moved between step 3 and step 6
    moved, ents = oc.compare(tr.plan, loaded, "the operands straight after the load")
    weights = [e.label for e in ents if e.fn in ("simt_pack_weight", "simt_stem7_pack") and any(n in tr.sgd_names for n in e.sources)]
    moved_w = [w for w in weights if any(m.startswith(w + ":") for m in moved)]
    m1 = oc.masters(tr)
    print(f"after the load: {len(moved_w)} of {len(weights)} packed operands of applied weights changed in steps {k + 1}-6; "
          f"{sum(not torch.equal(m0[n], m1[n]) for n in m0)} of {len(m0)} applied masters changed")
    assert all(not torch.equal(m0[n], m1[n]) for n in m0 if n.endswith(".weight")), "an applied weight did not move after the load"
    assert weights and moved_w, "no packed operand of an applied weight changed after the load: the case does not exercise the re-pack"
    finite_losses(tr, "resumed run, step 6")
    res = louts, full_state(tr)
    del tr
    torch.cuda.empty_cache()
    return res


def assert_same_run(a, b, what, first=0):
    (la, sa), (lb, sb) = a, b
    assert len(la) == len(lb) == 6
    for i in range(first, 6):
        assert torch.equal(la[i], lb[i]), (f"{what}: the scalars of step {i + 1} differ: {la[i].view(torch.float32).tolist()} vs "
                                           f"{lb[i].view(torch.float32).tolist()}")
    assert sa.keys() == sb.keys()
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{what}: {len(diff)} of {len(sa)} tensors differ after step 6: {diff[:8]}"


# ---- 1. trainer level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["control", "resume"])
@pytest.mark.parametrize("case", list(CASES))
def test_resumed_trainer_continues_bit_for_bit(dev, tmp_path, monkeypatch, case, mode):
    """control: the uninterrupted 6 steps twice.  resume: 3 steps, training_state(), save / load on disk, a new trainer built from OTHER weights,
    load_training_state(), 3 more steps."""
    kind, kw = CASES[case]
    monkeypatch.setenv("SIMT_EARLY_SGD", "0" if kw.get("late") else "1")
    with (one_rank_group(dev, 29564) if kw.get("dp") else contextlib.nullcontext()) as pg:
        probe = make(kind, kw, dev, pg)
        if kind == "simt":
            assert probe._early_sgd == (not kw.get("late") and kw.get("iter_size", 1) == 1), "the schedule under test is not the one the case names"
            assert (probe._grad_acc is not None) == (kw.get("iter_size", 1) > 1)
        assert (probe.reducer is not None) == bool(kw.get("dp")) and probe.dtype == kw.get("dtype", BF)
        del probe
        data = batches(kind, kw, dev)
        a = straight(kind, kw, dev, pg, data)
        moved = [k for k in a[1] if k.startswith("momentum ") and float(a[1][k].abs().max()) > 0]
        assert len(moved) > 0 and int(a[1]["it_done"]) == 6
        nbt = [int(v) for k, v in a[1].items() if k.endswith("num_batches_tracked")]
        assert not nbt or max(nbt) == 6 * kw.get("iter_size", 1)
        if mode == "control":
            assert_same_run(a, straight(kind, kw, dev, pg, data), f"CONTROL {case} (two uninterrupted runs)")
        else:
            assert_same_run(a, split(kind, kw, dev, pg, data, str(tmp_path / "run.state")), f"{case} resumed after step 3", first=3)


def test_resume_test_sees_a_trainer_that_forgets_its_iteration(dev, tmp_path, monkeypatch):
    """Red: a load that leaves the iteration counter at 0 (what --restore-from of a snapshot amounts to) must fail the comparison."""
    kind, kw = CASES["SimTTrainer"]
    data = batches(kind, kw, dev)
    a = straight(kind, kw, dev, None, data)
    orig = SimTTrainer.load_training_state

    def forgetful(self, ts):
        orig(self, dict(ts, it_done=0, model={k: (v - 3 if k.endswith("num_batches_tracked") else v) for k, v in ts["model"].items()}))
        self.it_done = 0
    monkeypatch.setattr(SimTTrainer, "load_training_state", forgetful)
    tr = make(kind, kw, dev)
    for b in data[:3]:
        tr.step(*b)
    ts = tr.training_state()
    del tr
    tr = make(kind, kw, dev, seed=1)
    tr.load_training_state(ts)
    for b in data[3:]:
        tr.step(*b)
    assert not torch.equal(scalars(tr), a[0][5])


def test_no_train_state_while_the_fused_batchnorm_error_word_is_set(dev, tmp_path, monkeypatch):
    """losses() reads one more device word than the scalars: the plan's sticky fused-BatchNorm error word.  While it is set the optimiser
    launches skip their updates and `it_done` still counts, so the trainer holds no state of the run: training_state() raises what losses()
    raises, and --train-state keeps the file it wrote before (the last good state).  The word is set by hand (tests/test_gpu_bn_fused.py);
    nothing times out."""
    from simt_amd.tools.trainV2_simt import SnapshotKeeper, TrainStateFile, get_arguments
    monkeypatch.setenv("SIMT_BN_GRID", "3")
    kind, kw = CASES["SimTTrainer"]
    size = (4, 768, 768)                                   # (large enough for the plan to fuse BatchNorm launches at this reduced depth)
    tr = make(kind, kw, dev, size=size)
    assert tr.plan.fbn_launches > 0 and tr.plan.fbn_err is not None
    img, lab = so.synthetic_batch(*size, CD.numpy(), seed=1, block=8)
    img, lab = img.to(dev), lab.to(dev)
    path = str(tmp_path / "run.state")
    flag = TrainStateFile(get_arguments(["--train-state", path, "--train-state-every", "1"]), 0, 1, CD.numpy())
    keeper = SnapshotKeeper(str(tmp_path), "GTA5_iter")
    tr.step(img, lab)
    flag.after_iteration(0, tr, keeper)
    good = tsf.load(path)[0]
    assert good["it_done"] == 1
    tr.plan.fbn_err.fill_(1)                               # what a timed-out fused launch leaves behind
    tr.step(img, lab)
    assert tr.it_done == 2
    with pytest.raises(RuntimeError, match="SIMT_BN_GRID=0"):
        tr.training_state()
    with pytest.raises(RuntimeError, match="SIMT_BN_GRID=0"):
        flag.after_iteration(1, tr, keeper)
    again = tsf.load(path)[0]
    assert again["it_done"] == 1 and all(torch.equal(again["model"][k], good["model"][k]) for k in good["model"])
    assert not os.path.exists(path + ".tmp")
    with pytest.raises(RuntimeError, match="SIMT_BN_GRID=0"):
        tr.losses()
    # the file resumes the last good state
    tr.plan.fbn_err.zero_()
    del tr
    torch.cuda.empty_cache()
    tr = make(kind, kw, dev, seed=1, size=size)
    assert flag.resume(tr, keeper) == 1
    tr.step(img, lab)
    finite_losses(tr, "resumed from the last good state")


# ---- 2. refusals, accumulators -----------------------------------------------------------------------------------------------------------------
def test_load_training_state_refuses_and_names_what_differs(dev):
    kind, kw = CASES["SimTTrainer"]
    tr = make(kind, kw, dev)
    data = batches(kind, kw, dev, n=1)
    tr.step(*data[0])
    ts = tr.training_state()
    assert set(ts) >= {"model", "momentum", "ntm", "ntm_m", "ntm_v", "wraw", "w_m", "w_v", "it_done", "hyper", "frozen_sha256", "accumulators"}
    assert set(ts["momentum"]) == set(tr.mom) and len(ts["ntm"]) == 2 and ts["hyper"]["format_version"] == tsf.FORMAT_VERSION
    assert ts["frozen_sha256"] == tsf.state_sha256(tr.fixed_params) and "fixed" not in "".join(ts)

    def refused(other, state, *names):
        before = full_state(other)
        with pytest.raises(ValueError) as e:
            other.load_training_state(state)
        for n in names:
            assert n in str(e.value), (n, str(e.value))
        after = full_state(other)
        assert all(torch.equal(before[k], after[k]) for k in before), "a refused load changed the trainer"
        return str(e.value)

    msg = refused(make(kind, kw, dev, hp_kw={"lr": 1e-3, "lambda_anchor": 0.25}), ts, "lr ", "lambda_anchor")
    assert "momentum" not in msg and "th_high" not in msg
    refused(make(kind, kw, dev, hp_kw={"iter_size": 2}), ts, "iter_size")
    refused(make(kind, kw, dev, size=(2, 65, 97)), ts, "H (")
    refused(make(kind, dict(kw, dtype=F32), dev), ts, "dtype")
    refused(make(kind, kw, dev, frozen_seed=1), ts, "frozen_sha256")
    refused(make(*CASES["WarmupTrainer"], dev), ts, "trainer", "open_classes")
    same = make(kind, kw, dev, seed=1)
    short = dict(ts, momentum={k: v for k, v in ts["momentum"].items() if k != tr.sgd_names[0]})
    refused(same, short, f"momentum {tr.sgd_names[0]}: missing")
    shaped = dict(ts, momentum=dict(ts["momentum"], **{tr.sgd_names[1]: torch.zeros(3)}))
    refused(same, shaped, f"momentum {tr.sgd_names[1]}: shape")
    refused(same, dict(ts, hyper=dict(ts["hyper"], format_version=tsf.FORMAT_VERSION + 1)), "format_version")
    # what may differ: a trainer that skips the gradients no optimiser applies follows the same trajectory
    make(kind, kw, dev, hp_kw={"skip_unapplied_grads": True}).load_training_state(ts)
    same.load_training_state(ts)
    a, b = full_state(tr), full_state(same)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", ["SimTTrainer", "WarmupTrainer", "SimTSingleTrainer-vgg", "WarmupSingleTrainer-v3"])
@pytest.mark.parametrize("reported", [False, True], ids=["not_yet_reported", "already_reported"])
def test_bad_label_count_survives_a_resume(dev, case, reported):
    """Out-of-range label values in step 2 of 3.  Saved before losses() has raised for them: the resumed trainer raises what the saved one
    would have raised.  Saved after: it does not raise again (the device counter is cumulative; its host twin travels with it)."""
    kind, kw = CASES[case]
    data = batches(kind, kw, dev, n=4, bad_at=1)
    tr = make(kind, kw, dev)
    for b in data[:3]:
        tr.step(*b)
    if reported:
        with pytest.raises(ValueError, match="label value"):
            tr.losses()
    ts = tr.training_state()
    assert (ts["bad_reported"] > 0) == reported
    expected = None
    if not reported:
        with pytest.raises(ValueError, match="label value") as e:
            tr.losses()                                    # (after the state was taken: what the saved trainer would have raised)
        expected = str(e.value)
    del tr
    tr = make(kind, kw, dev, seed=1)
    tr.load_training_state(ts)
    if not reported:
        with pytest.raises(ValueError) as e:
            tr.losses()
        assert str(e.value) == expected
    tr.losses()
    tr.step(*data[3])
    tr.losses()


# ---- 3. loader ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
@pytest.mark.parametrize("rank", [0, 1])
def test_gpu_loader_start_batch_yields_the_tail(dev, tmp_path, rank, cached):
    """11 files, B = 2, two ranks' shards (3 and 2 batches per epoch), shuffle + mirror, 4 epochs: from a batch inside epoch 0, on an epoch
    boundary and inside epoch 2 the batches equal the default loader's tail, and only the items of those batches are decoded (cached: each
    once -- the cache starts empty after a resume and refills)."""
    Image = pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, Image, 11)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=4, rank=rank, world=2)
    ds0 = _dataset(root, lst)
    assert ds0.is_mirror
    ref = _collect(GpuLoader(ds0, 2, **kw))
    per_epoch = (3, 2)[rank]
    assert len(ref) == 4 * per_epoch
    for n in (1, per_epoch, 2 * per_epoch + 1):
        ds = _dataset(root, lst)
        cnt = _Counting(ds)
        cache = DatasetCache((48, 24), slab_slots=4, device=dev) if cached else None
        got = _collect(GpuLoader(ds, 2, cache=cache, start_batch=n, **kw))
        assert len(got) == len(ref) - n
        _assert_same_batches(ref[n:], got)
        dealt = [name for (_x, _l, _s, names) in ref[n:] for name in names]
        decoded = [os.path.splitext(os.path.basename(k[0] if isinstance(k, tuple) else k))[0] for k in cnt.calls]
        assert sorted(decoded) == (sorted(set(dealt)) if cached else sorted(dealt)), (n, sorted(decoded), sorted(dealt))
    assert not _collect(GpuLoader(_dataset(root, lst), 2, start_batch=4 * per_epoch, **kw))


# ---- 4. tools ----------------------------------------------------------------------------------------------------------------------------------
def _loss_lines(out):
    """The `iter = ...` lines without the wall-clock rate (tests/test_gpu_dataset_cache.py)."""
    return [re.sub(r"\s*\([0-9.]+ img/s\)", "", ln) for ln in out.splitlines() if ln.startswith("iter = ")]


def _tool(which):
    if which == "warmup":
        from simt_amd.tools import trainV1_warmup as tool
        return tool, ["--learning-rate", "2.5e-4"]
    from simt_amd.tools import trainV2_simt as tool
    return tool, ["--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3"]


def _same_snapshot(a, b):
    sa, sb = torch.load(a), torch.load(b)
    assert set(sa) == set(sb) and len(sa) > 0
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{os.path.basename(a)}: {len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


def _resume_case(tmp_path, capsys, which, model, source, every=(), split_at=3, save_pred_every="100"):
    tool, extra = _tool(which)
    common = extra + ["--model", model, "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--save-pred-every", save_pred_every,
                      "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2"] + source

    def run(tag, stop, *flags):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(flags))
        return capsys.readouterr().out, snap

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6)
    assert "resumed" not in out_a and len(_loss_lines(out_a)) == 6
    out_b1, snap_b = run("b", split_at, "--train-state", state, *every)
    assert "resumed" not in out_b1 and len(_loss_lines(out_b1)) == split_at and os.path.exists(state) and not os.path.exists(state + ".tmp")
    assert _loss_lines(out_b1) == _loss_lines(out_a)[:split_at]
    out_b2, _ = run("b", 6, "--train-state", state, *every)
    assert re.search(rf"resumed \w+ from .* at iteration {split_at}\b", out_b2), out_b2
    assert _loss_lines(out_b2) == _loss_lines(out_a)[split_at:], (out_a, out_b2)
    _same_snapshot(os.path.join(snap_a, "GTA5_6.pth"), os.path.join(snap_b, "GTA5_6.pth"))
    assert tsf.load(state)[0]["it_done"] == 6
    before = {f: os.path.getmtime(os.path.join(snap_b, f)) for f in os.listdir(snap_b)}
    out_b3, _ = run("b", 6, "--train-state", state, *every)
    assert "the run is complete" in out_b3 and not _loss_lines(out_b3) and "save model" not in out_b3
    assert {f: os.path.getmtime(os.path.join(snap_b, f)) for f in os.listdir(snap_b)} == before
    return snap_a, snap_b, (out_a, out_b1, out_b2)


@pytest.mark.parametrize("model", ["DeepLab", "DeepLabv3", "DeepLabVGG"])
@pytest.mark.parametrize("which", ["simt", "warmup"])
def test_tools_resume_from_train_state_equals_one_run(dev, tmp_path, capsys, which, model):
    """--synthetic, 6 steps in one run against 3 + 3 through --train-state: loss lines of iterations 3-5, every tensor of GTA5_6.pth; a third
    invocation takes no step.  A run without the flag leaves what it always left: the final snapshot, nothing else."""
    snap_a, snap_b, _ = _resume_case(tmp_path, capsys, which, model, ["--synthetic"])
    assert os.listdir(snap_a) == ["GTA5_6.pth"]
    assert sorted(os.listdir(snap_b)) == ["GTA5_3.pth", "GTA5_6.pth"]
    assert sorted(os.listdir(tmp_path)) == ["a", "b", "run.state"]


def test_tool_resumes_on_files_with_mirror_and_cache_across_epochs(dev, tmp_path, capsys):
    """4 PNG pairs, B = 2: two batches per epoch.  The first half ends inside epoch 1 (batches 0-2), the second starts at its second batch
    and runs into epoch 2; --random-mirror (the generator is advanced past three batches' draws) and --cache-dataset device (the cache
    starts empty again and refills)."""
    Image = pytest.importorskip("PIL.Image")
    _tool_files(tmp_path / "data", Image)
    src = ["--data-dir-target", str(tmp_path / "data"), "--data-list-target", str(tmp_path / "data" / "pseudo.lst"), "--random-mirror",
           "--cache-dataset", "device"]
    _a, _b, (_out_a, _o1, out_b2) = _resume_case(tmp_path, capsys, "simt", "DeepLab", src)
    # the resumed half decodes what it is dealt first (2 misses in what is left of epoch 1), then lives on its cache
    lines = re.findall(r"dataset cache: rank 0 epoch (\d+): (\d+) hits, (\d+) misses", out_b2)
    assert [tuple(map(int, l)) for l in lines[:2]] == [(1, 0, 2), (2, 2, 2)], out_b2


def test_tool_rotation_continues_after_a_resume(dev, tmp_path, capsys):
    """--save-pred-every 2, no validation set: the rolling snapshot.  The first half (4 steps) leaves iter2, the resumed half writes iter4 and
    removes iter2 -- one rolling file remains, the one the uninterrupted run leaves, with the same tensors.  --train-state-every 1 on top."""
    snap_a, snap_b, _ = _resume_case(tmp_path, capsys, "warmup", "DeepLabVGG", ["--synthetic"], every=["--train-state-every", "1"], split_at=4,
                                     save_pred_every="2")
    assert sorted(os.listdir(snap_a)) == ["GTA5_6.pth", "GTA5_BAPA_warmup_iter4.pth"]
    assert sorted(os.listdir(snap_b)) == ["GTA5_4.pth", "GTA5_6.pth", "GTA5_BAPA_warmup_iter4.pth"]
    rolling = glob.glob(os.path.join(snap_b, "GTA5_BAPA_warmup_iter*.pth"))
    assert len(rolling) == 1
    _same_snapshot(os.path.join(snap_a, "GTA5_BAPA_warmup_iter4.pth"), rolling[0])


def test_tool_refuses_a_train_state_of_another_run(dev, tmp_path, capsys):
    tool, extra = _tool("simt")
    state = str(tmp_path / "run.state")
    common = ["--model", "DeepLabVGG", "--synthetic", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
              "--num-steps-stop", "1", "--snapshot-dir", str(tmp_path / "s"), "--train-state", state]
    tool.main(common + extra)
    with pytest.raises(SystemExit, match="lr_T"):
        tool.main(common + extra[:-1] + ["5e-3", "--num-steps-stop", "2"])
    with pytest.raises(SystemExit, match="B \\("):
        tool.main(common + extra + ["--batch-size", "1", "--num-steps-stop", "2"])
    capsys.readouterr()
