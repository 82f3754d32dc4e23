"""`optimizer="adamw"` and `lr_warmup` in the four trainers and both tools, on the small geometries of tests/test_gpu_resume.py.

  1. keywords at their defaults: the keyword-less trainer, bit for bit;
  2. AdamW against the float64 restatement (tests/_adamw_ref.py): every element of every applied tensor, step by step, from the masters, moments
     and gradients the device holds; the segment table lists every applied tensor once; the early placement equals the late one;
  3. operand coherence after a step that is visible in bf16 (tests/_operand_coherence.py);
  4. resume: 3 + 3 steps == 6 steps with the warm-up ramp crossing the save, iter_size 2, a one-rank RCCL group; what a load refuses;
  5. the weight EMA still follows tests/_ema_ref.py;
  6. the warm-up alone, against a keyword-less trainer whose learning rate is the hand-computed one;
  7. both tools: `--optimizer adamw --lr-warmup 2` resumed equals the uninterrupted run.

Comparisons between two executions of the same arithmetic are bitwise; the one against float64 uses the derived bar of tests/_adamw_ref.py."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import _adamw_ref as ref
import _ema_ref as ema_ref
import _operand_coherence as oc
import test_gpu_resume as R
from simt_amd import step as step_mod
from simt_amd import step_single as step_single_mod
from simt_amd import train_state as tsf
from simt_amd.step import lr_poly
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
TRAINERS = ("SimTTrainer", "WarmupTrainer", "SimTSingleTrainer", "WarmupSingleTrainer")
CONFIGS = ["SimTTrainer", "WarmupTrainer", "SimTSingleTrainer-v3", "SimTSingleTrainer-vgg", "WarmupSingleTrainer-v3", "WarmupSingleTrainer-vgg"]
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
SEG_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("pad", "<i4")])
ADAMW = dict(optimizer="adamw")


@contextlib.contextmanager
def keywords(**kw):
    """tests/test_gpu_resume.make builds the four trainers by name: give every one of them the keywords for the duration (the pattern of
    tests/test_gpu_ema.ema_on); its full_state() also reports Adam's second moment where a trainer has one."""
    saved = {n: getattr(R, n) for n in TRAINERS}
    full = R.full_state

    def full_state(tr):
        out = full(tr)
        out.update({f"momentum2 {k}": v.cpu() for k, v in getattr(tr, "mom2", {}).items()})
        return out
    try:
        if kw:
            for n, cls in saved.items():
                setattr(R, n, functools.partial(cls, **kw))
        R.full_state = full_state
        yield
    finally:
        R.full_state = full
        for n, cls in saved.items():
            setattr(R, n, cls)


@contextlib.contextmanager
def placement(late):
    before = os.environ.get("SIMT_EARLY_SGD")
    os.environ["SIMT_EARLY_SGD"] = "0" if late else "1"          # read by the constructor
    try:
        yield
    finally:
        if before is None:
            os.environ.pop("SIMT_EARLY_SGD", None)
        else:
            os.environ["SIMT_EARLY_SGD"] = before


def case_of(config, dtype, **more):
    kind, kw = R.CASES[config]
    return kind, dict(kw, dtype=dtype, **more)


def build(config, dtype, dev, late=False, pg=None, seed=0, hp_kw=None, **opt):
    kind, kw = case_of(config, dtype)
    with placement(late), keywords(**opt):
        tr = R.make(kind, kw, dev, pg, seed=seed, hp_kw=hp_kw)
    if kind == "simt":
        assert tr._early_sgd == (not late), "the placement under test is not the one the case names"
    return tr


def run(config, dtype, dev, n, late=False, **opt):
    """n steps -> (loss scalars per step, full state with both moments)."""
    kind, kw = case_of(config, dtype)
    data = R.batches(kind, kw, dev, n=n)
    tr = build(config, dtype, dev, late=late, **opt)
    louts = []
    for b in data:
        tr.step(*b)
        louts.append(R.scalars(tr))
    R.finite_losses(tr, f"{config} step {n}")
    with keywords():
        state = R.full_state(tr)
    del tr
    torch.cuda.empty_cache()
    return louts, state


def same(a, b, what):
    (la, sa), (lb, sb) = a, b
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), f"{what}: the scalars of step {i + 1} differ"
    assert sa.keys() == sb.keys(), f"{what}: {sorted(set(sa) ^ set(sb))[:6]}"
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{what}: {len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


# ---- 1. keywords at their defaults -------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("config", CONFIGS)
def test_default_keywords_are_the_trainer_it_was(dev, config, dtype):
    plain = run(config, dtype, dev, 3)
    named = run(config, dtype, dev, 3, optimizer="sgd", adam_betas=(0.9, 0.999), adam_eps=1e-8, lr_warmup=0, lr_warmup_ratio=1e-6)
    same(plain, named, f'{config}: optimizer="sgd", lr_warmup=0 against no keyword')
    tr = build(config, dtype, dev, optimizer="sgd", lr_warmup=0)
    assert not hasattr(tr, "mom2") and not hasattr(tr, "adamw_desc"), "the default allocates nothing"
    hy = tr._hyper_state()
    assert not set(hy) & set(tsf.OPTIMIZER_FIELDS), "the flag-off hyper dict is what it was"
    assert "momentum2" not in tr.training_state()


# ---- 2. AdamW against the restatement ----------------------------------------------------------------------------------------------------------
def _expected_groups(tr):
    """{applied tensor: AdamW group}: the SGD table's group (0 trunk, 1 heads at 10x), + 2 for a BatchNorm's gamma / beta (no decay)."""
    base = oc.sgd_groups(tr)
    return {n: base[n][0] + (2 if n.rsplit(".", 1)[0] + ".running_mean" in tr.params else 0) for n in tr.sgd_names}


def _cat(d, names):
    return torch.cat([d[n].detach().flatten() for n in names])      # (on the device: the float64 restatement runs there too)


def _expected_lr(hp, it, warmup, ratio):
    lr = lr_poly(hp.lr, it, hp.num_steps, hp.power)
    return lr * (1 - (1 - it / warmup) * (1 - ratio)) if warmup and it < warmup else lr


@DTYPES
@pytest.mark.parametrize("config", CONFIGS)
def test_adamw_step_every_element_vs_float64(dev, config, dtype):
    """Late placement, three steps, lr_warmup = 2 so that the learning rate changes in kind as well.  Before each step the masters and both
    moments are read, after it the gradients the plan still holds; the restatement is applied to them and every element of p, m and v of
    every applied tensor must lie within the bar.  The moments are NaN before the first step: it must not read them."""
    betas, eps, warm, ratio = (0.9, 0.99), 1e-7, 2, 0.125
    opt = dict(ADAMW, adam_betas=betas, adam_eps=eps, lr_warmup=warm, lr_warmup_ratio=ratio)
    kind, kw = case_of(config, dtype)
    data = R.batches(kind, kw, dev, n=3)
    tr = build(config, dtype, dev, late=True, **opt)
    names = list(tr.sgd_names)
    groups = _expected_groups(tr)
    # ---- the device's table: every applied tensor once, its own pointers, the expected group
    segs = np.frombuffer(tr.adamw_segs.cpu().numpy().tobytes(), dtype=SEG_DT)
    assert len(segs) == len(names) == len(set(names)) and len({int(s["p"]) for s in segs}) == len(segs), "every applied tensor is listed ONCE"
    for s, n in zip(segs, names):
        assert (int(s["p"]), int(s["g"]), int(s["m"]), int(s["v"]), int(s["n"]), int(s["group"])) == \
            (tr.params[n].data_ptr(), tr.plan.grads[n].data_ptr(), tr.mom[n].data_ptr(), tr.mom2[n].data_ptr(), tr.params[n].numel(), groups[n]), n
    assert tr.adamw_desc.nchunks == sum((tr.params[n].numel() + 65535) // 65536 for n in names) and tr.adamw_desc.chunk == 65536
    group = torch.cat([torch.full((tr.params[n].numel(),), groups[n], dtype=torch.int64) for n in names]).to(dev)
    print(f"{config}: {len(names)} applied tensors, {group.numel()} elements, per group {torch.bincount(group, minlength=4).tolist()}")
    others = [n for n, t in tr.params.items() if t.is_floating_point() and n not in names and not n.endswith(("running_mean", "running_var"))]
    for t in list(tr.mom.values()) + list(tr.mom2.values()):
        t.fill_(float("nan"))
    wd = tr.hp.weight_decay
    worst = 0.0
    for k, b in enumerate(data):
        torch.cuda.synchronize()
        p0, m0, v0 = _cat(tr.params, names), _cat(tr.mom, names), _cat(tr.mom2, names)
        o0 = {n: tr.params[n].clone() for n in others}
        tr.step(*b)
        torch.cuda.synchronize()
        lr = _expected_lr(tr.hp, k, warm, ratio)
        c = ref.constants([lr, lr * 10.0, lr, lr * 10.0], [wd, wd, 0.0, 0.0], betas, k + 1)
        assert (np.float32(tr.adamw_desc.step_size[0]), np.float32(tr.adamw_desc.step_size[1])) == (c["step_size"][0], c["step_size"][1]), \
            f"step {k}: the launch received another learning rate than lr_at's"
        want = ref.adamw_ref(ref.exact(p0), ref.exact(_cat(tr.plan.grads, names)), None if k == 0 else ref.exact(m0), None if k == 0 else ref.exact(v0),
                             ref.per_element(c["step_size"], group), ref.per_element(c["decay"], group), c["beta2"], c["omb1"], c["omb2"],
                             c["bc2s"], eps, k == 0)
        for what, got, w in (("p", tr.params, want[0]), ("m", tr.mom, want[1]), ("v", tr.mom2, want[2])):
            worst = max(worst, ref.ratio(_cat(got, names), w, f"{config} step {k} {what}"))
        assert float((_cat(tr.params, names) != p0).double().mean()) > (0.5 if k else 0.0), f"step {k}: the applied masters did not move"
        moved = [n for n in others if not torch.equal(tr.params[n], o0[n])]
        assert not moved, f"step {k}: tensors the optimiser does not apply changed: {moved[:6]}"
    R.finite_losses(tr, f"{config} step 3")
    print(f"{config}: worst |stored - float64| / bound = {worst:.3f} (allowed {ref.SLACK})")


def test_adamw_early_placement_equals_late(dev):
    """SimTTrainer is the trainer with two placements: simt_adamw_multi on the side stream at the early cut against behind the backward."""
    for dtype in (BF, F32):
        late = run("SimTTrainer", dtype, dev, 3, late=True, lr_warmup=2, **ADAMW)
        early = run("SimTTrainer", dtype, dev, 3, late=False, lr_warmup=2, **ADAMW)
        assert any(k.startswith("momentum2 ") and float(v.abs().max()) > 0 for k, v in late[1].items())
        same(late, early, f"SimTTrainer {dtype}: AdamW early against late")


# ---- 3. operand coherence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,late", [(c, False) for c in CONFIGS] + [("SimTTrainer", True)],
                         ids=CONFIGS + ["SimTTrainer-late"])      # (SimTTrainer has two placements; its default is the early one)
def test_adamw_operands_coherent_after_a_visible_step(dev, config, late):
    """A decay of 1 - 2^-5 (lr 1e-5 x weight decay 3125; heads 1 - 10 x 2^-5) moves every decayed element by 3 % relative, far more than Adam's
    own term of 1e-5 (which could cancel it only where |p| is about 3e-4): the update is visible in bf16 on >= 99 % of the elements of every
    conv weight (the condition is computed from the fp32 masters alone).  Then every packed operand equals a fresh plan's."""
    kind, kw = case_of(config, BF)
    data = R.batches(kind, kw, dev, n=2)
    tr = build(config, BF, dev, late=late, hp_kw={"lr": 1e-5, "weight_decay": 3125.0}, **ADAMW)
    tr.step(*data[0])
    R.finite_losses(tr, f"{config} step 1")
    torch.cuda.synchronize()
    m0, ops0 = oc.masters(tr), oc.snapshot(tr.plan)
    frozen0 = oc.snapshot(tr.fixed) if getattr(tr, "fixed", None) is not None else None
    tr.step(*data[1])
    R.finite_losses(tr, f"{config} step 2")
    fr = oc.rounding_changed(m0, oc.masters(tr))
    oc.assert_visible({n: f for n, f in fr.items() if m0[n].dim() == 4}, f"AdamW {config}")
    fresh = oc.fresh_plan(tr.plan, oc.device_state(tr.state_dict(), dev))
    bad = oc.check_coherent(tr.plan, fresh, tr.sgd_names, ops0)
    if frozen0 is not None:
        bad += oc.compare(tr.fixed, frozen0, "the frozen plan's operands before the step (it is never re-packed)")[0]
    assert not bad, f"{config}: " + "; ".join(bad[:8])


# ---- 4. resume ---------------------------------------------------------------------------------------------------------------------------------
RESUME = [("SimTTrainer", BF), ("SimTTrainer", F32), ("SimTTrainer-late_sgd", BF), ("SimTTrainer-iter_size2", BF), ("SimTTrainer-rccl_one_rank", BF),
          ("WarmupTrainer", BF), ("WarmupTrainer", F32), ("WarmupTrainer-iter_size2", BF), ("SimTSingleTrainer-v3", BF), ("SimTSingleTrainer-vgg", BF),
          ("SimTSingleTrainer-v3", F32), ("WarmupSingleTrainer-v3", BF), ("WarmupSingleTrainer-vgg", BF), ("WarmupSingleTrainer-vgg", F32)]


@pytest.mark.parametrize("config,dtype", RESUME, ids=[f"{c}-{'bf16' if d == BF else 'fp32'}" for c, d in RESUME])
def test_adamw_resumed_trainer_continues_bit_for_bit(dev, tmp_path, config, dtype):
    """3 steps, training_state(), the file, a NEW trainer built from other weights, load_training_state(), 3 steps == 6 steps; lr_warmup = 4: the
    ramp crosses the save, a trainer that forgot the iteration or the second moment is far off."""
    kind, kw = case_of(config, dtype)
    # DAFormer's 6e-5 (heads 6e-4): Adam moves every element by about lr per step whatever the gradient, and at the 6e-4 the SGD cases use the
    # random bf16 SimT model has a NaN place loss by step 6, in the uninterrupted run already
    kw["lr"] = min(kw.get("lr", 6e-5), 6e-5)
    with placement(bool(kw.get("late"))), keywords(lr_warmup=4, **ADAMW), \
            (one_rank_group(dev, 29571) if kw.get("dp") else contextlib.nullcontext()) as pg:
        data = R.batches(kind, kw, dev)
        a = R.straight(kind, kw, dev, pg, data)
        assert any(k.startswith("momentum2 ") and float(v.abs().max()) > 0 for k, v in a[1].items()) and int(a[1]["it_done"]) == 6
        R.assert_same_run(a, R.split(kind, kw, dev, pg, data, str(tmp_path / "run.state")), f"{config} with AdamW resumed after step 3", first=3)
    ts = tsf.load(str(tmp_path / "run.state"))[0]
    assert set(ts["momentum2"]) == set(ts["momentum"]) and ts["hyper"]["optimizer"] == "adamw" and ts["hyper"]["lr_warmup"] == 4


def test_adamw_state_is_refused_by_a_trainer_that_differs(dev):
    config, dtype = "WarmupTrainer", BF
    kind, kw = case_of(config, dtype)
    on = dict(ADAMW, lr_warmup=4)
    tr = build(config, dtype, dev, **on)
    tr.step(*R.batches(kind, kw, dev, n=1)[0])
    ts = tr.training_state()
    assert ts["hyper"]["adam_betas"] == [0.9, 0.999] and ts["hyper"]["adam_eps"] == 1e-8 and ts["hyper"]["lr_warmup_ratio"] == 1e-6
    for opt, named in ((dict(lr_warmup=4), ("optimizer", "adam_betas", "adam_eps")), (dict(on, adam_betas=(0.9, 0.99)), ("adam_betas",)),
                       (dict(on, adam_eps=1e-6), ("adam_eps",)), (dict(ADAMW), ("lr_warmup", "lr_warmup_ratio")), (dict(on, lr_warmup=5), ("lr_warmup",)),
                       (dict(on, lr_warmup_ratio=0.5), ("lr_warmup_ratio",))):
        other = build(config, dtype, dev, seed=1, **opt)
        with keywords():
            before = R.full_state(other)
        with pytest.raises(ValueError) as e:
            other.load_training_state(ts)
        assert all(n + " (" in str(e.value) for n in named), (named, str(e.value))
        assert ("adam_eps (" in str(e.value)) == ("adam_eps" in named) and "momentum " not in str(e.value)
        with keywords():
            after = R.full_state(other)
        assert all(torch.equal(before[k], after[k]) for k in before), "a refused load changed the trainer"
    plain = build(config, dtype, dev)
    plain.step(*R.batches(kind, kw, dev, n=1)[0])
    with pytest.raises(ValueError, match=r"optimizer \("):      # and the other way round: an SGD state into an AdamW trainer
        build(config, dtype, dev, seed=1, **on).load_training_state(plain.training_state())
    short = dict(ts, momentum2={k: v for k, v in ts["momentum2"].items() if k != tr.sgd_names[0]})
    with pytest.raises(ValueError, match=f"momentum2 {tr.sgd_names[0]}: missing"):
        build(config, dtype, dev, seed=1, **on).load_training_state(short)


# ---- 5. the weight EMA -------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("config", CONFIGS)
def test_adamw_ema_shadow_follows_the_restatement(dev, config, dtype):
    kind, kw = case_of(config, dtype)
    data = R.batches(kind, kw, dev, n=3)
    tr = build(config, dtype, dev, ema_decay=0.9, lr_warmup=2, **ADAMW)
    masters = lambda: {k: v.cpu().numpy() for k, v in tr.params.items() if v.is_floating_point()}
    torch.cuda.synchronize()
    sh = ema_ref.Shadow(masters(), 0.9)
    for k, b in enumerate(data):
        tr.step(*b)
        torch.cuda.synchronize()
        sh.update(masters())
        bad = [n for n, v in tr.ema.shadow.items() if not np.array_equal(v.cpu().numpy().view(np.uint32), ema_ref.words(sh.e[n]))]
        assert not bad, f"{config} step {k}: {len(bad)} shadow tensors differ from the restatement: {bad[:6]}"
    live = masters()
    assert any(not np.array_equal(ema_ref.words(live[n]), ema_ref.words(sh.e[n])) for n in tr.sgd_names), "the shadow is an average by now"


# ---- 6. the warm-up alone ----------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("config", CONFIGS)
def test_lr_warmup_alone_is_sgd_at_the_hand_computed_rate(dev, monkeypatch, config, dtype):
    """optimizer="sgd", lr_warmup=4, ratio 0.25, five steps (the ramp and the first step past it) against a keyword-less trainer whose model
    learning rate is replaced by the hand-computed one; the rates the launches received are read from the descriptor."""
    warm, ratio, n = 4, 0.25, 5
    kind, kw = case_of(config, dtype)
    data = R.batches(kind, kw, dev, n=n)
    tr = build(config, dtype, dev, lr_warmup=warm, lr_warmup_ratio=ratio)
    hand = [lr_poly(tr.hp.lr, it, tr.hp.num_steps, tr.hp.power) * ((1 - (1 - it / 4) * (1 - 0.25)) if it < 4 else 1.0) for it in range(n)]
    assert hand[0] == pytest.approx(0.25 * tr.hp.lr) and hand[4] == lr_poly(tr.hp.lr, 4, tr.hp.num_steps, tr.hp.power)
    louts = []
    for it, b in enumerate(data):
        tr.step(*b)
        louts.append(R.scalars(tr))
        assert (np.float32(tr.sgd_desc.lr[0]), np.float32(tr.sgd_desc.lr[1])) == (np.float32(hand[it]), np.float32(hand[it] * 10.0)), f"step {it}"
    R.finite_losses(tr, f"{config} step {n}")
    got = louts, R.full_state(tr)
    del tr
    torch.cuda.empty_cache()
    seen = []

    def patched(base, it, max_iter, power, warmup=0, warmup_ratio=1e-6):
        assert warmup == 0, "the reference trainer has no warm-up of its own"
        seen.append(it)
        return hand[it]
    monkeypatch.setattr(step_mod, "lr_at", patched)
    monkeypatch.setattr(step_single_mod, "lr_at", patched)
    ref_tr = build(config, dtype, dev)
    louts = []
    for b in data:
        ref_tr.step(*b)
        louts.append(R.scalars(ref_tr))
    assert seen == list(range(n))
    same(got, (louts, R.full_state(ref_tr)), f"{config}: lr_warmup=4 against the hand-computed learning rate")


# ---- 7. the tools ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["DeepLab", "DeepLabv3", "DeepLabVGG"])
@pytest.mark.parametrize("which", ["simt", "warmup"])
def test_tools_resume_with_adamw_and_warmup(dev, tmp_path, capsys, which, model):
    """--synthetic, 6 steps in one run against 3 + 3 through --train-state (tests/test_gpu_resume._resume_case): the loss lines of iterations
    3-5 and every tensor of GTA5_6.pth; the start-up line names what is on; the file carries the optimiser."""
    flags = ["--synthetic", "--optimizer", "adamw", "--lr-warmup", "2"]
    _a, _b, (out_a, _o1, out_b2) = R._resume_case(tmp_path, capsys, which, model, flags)
    assert "optimiser: adamw, betas 0.9 0.999, eps 1e-08" in out_a and "learning-rate warm-up: linear over the first 2 iterations" in out_a
    lrs = [ln.split("lr = ")[1].split()[0] for ln in R._loss_lines(out_a)]
    assert float(lrs[0]) < 1e-3 * float(lrs[2]) and float(lrs[1]) == pytest.approx(0.5 * float(lrs[2]), rel=0.05), lrs      # the printed rate is lr_at's
    hy = tsf.load(str(tmp_path / "run.state"))[0]["hyper"]
    assert hy["optimizer"] == "adamw" and hy["lr_warmup"] == 2
    if model != "DeepLabVGG":
        return
    tool, extra = R._tool(which)
    with pytest.raises(SystemExit, match="optimizer"):      # the same command line without the flags: refused, by name
        tool.main(extra + ["--model", model, "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--synthetic", "--from-scratch",
                           "--restore-from", "", "--num-workers", "2", "--snapshot-dir", str(tmp_path / "c"), "--num-steps-stop", "7",
                           "--train-state", str(tmp_path / "run.state")])
    capsys.readouterr()
