"""The state BETWEEN two steps: after an optimiser step, does every trainer's next forward / backward read the weights it just wrote?

  1. Operand coherence (tests/_operand_coherence.py): after a step whose update is VISIBLE in bf16 (seeded momentum; the 99 % condition is
     computed from the fp32 masters alone), the destination of every pack-list entry equals, bit for bit, a fresh plan built from the
     current masters; operands of parameters the stage does not apply, and every operand of the frozen plan, are bit-identical to before.
     Then the checkpoint round trip: a plan built from state_dict() computes the running trainer's logits, flat gradient and BatchNorm
     running statistics bit for bit.  Red tests plant a stale operand and must name it.
  2. Early against late optimiser step at the production size (full depth, B = 4, 768 x 768, bf16), single GPU and over a one-rank RCCL
     group: three iterations on distinct images, everything bit-identical, both schedules coherent.
  3. The cut point of the early step as a checked property (tests/_step_hazards.py) on the real byte ranges of the full-depth plans.
  4. Evaluator.load and the nn.Module facades: a second cached plan sees the new weights and BatchNorm statistics.

Every case prints, per applied tensor, the fraction of elements whose bf16 rounding changed."""
import contextlib
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import _launch_oracle as lo
import _operand_coherence as oc
import _step_hazards as sh
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import model_spec as ms
from simt_amd.engine import TrunkPlan
from simt_amd.engine_v3 import v3_state_shapes
from simt_amd.step import Hyper, SimTTrainer, WarmupTrainer, lr_poly
from simt_amd.step_single import SimTSingleTrainer, WarmupSingleTrainer
from test_gpu_single import VGG_SMALL, _v3_state, _vgg_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF = torch.bfloat16
SMALL = (1, 1, 2, 1)
FULL = (3, 4, 23, 3)
K = 3
# The seeded momentum term moves every element by 2^-5 relative whatever the learning rate (seed_momentum divides by it); the gradient term
# lr * g is absolute, and at 2.5e-4 it cancels the seeded term on the ~1-2 % of the elements of some tensors that lie closest to zero.  A
# learning rate 100 times smaller keeps it out of the way; which operands a step re-packs does not depend on it.
LR = 2.5e-6


@contextlib.contextmanager
def one_rank_group(dev, port):
    """A one-rank RCCL group (the pattern of test_dp_hooked_backward_world1_equals_plain)."""
    import torch.distributed as dist
    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        yield dist.group.WORLD
    finally:
        torch.cuda.synchronize()
        if created:
            dist.destroy_process_group()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sh_job_dt():
    """Record layout of simt_pack_weight_multi's job table (engine.LaunchList.coalesce_packs)."""
    return np.dtype([("w", "<u8"), ("dst", "<u8"), ("cscale", "<u8"), ("ldk", "<i8"), ("total", "<i8"), ("Cout", "<i4"), ("Cin", "<i4"),
                     ("RS", "<i4"), ("row_off", "<i4"), ("tap_off", "<i4"), ("Ck", "<i4"), ("mode", "<i4"), ("dtype", "<i4")])


def finite_losses(tr, what):
    l = tr.losses()
    assert all(np.isfinite(v) for v in l.values()), f"{what}: losses {l}"


def batches(B, H, W, n, seed, iter_size=1):
    out = []
    for i in range(n):
        mb = [so.synthetic_batch(B, H, W, CD.numpy(), seed=seed + 10 * i + j, block=8) for j in range(iter_size)]
        out.append(mb[0] if iter_size == 1 else ([m[0] for m in mb], [m[1] for m in mb]))
    return out


def to_dev(b, dev):
    return tuple([t.to(dev) for t in x] if isinstance(x, list) else x.to(dev) for x in b)


def seeded_step(tr, data, dev, what, sabotage=None, seed=77):
    """A plain first step, then the step under test with seeded momentum.  -> (mismatches, fresh plan built from state_dict())."""
    frozen0 = oc.snapshot(tr.fixed) if getattr(tr, "fixed", None) is not None else None
    tr.step(*to_dev(data[0], dev), 0)
    finite_losses(tr, f"{what} step 0")
    oc.seed_momentum(tr, lr_poly(tr.hp.lr, 1, tr.hp.num_steps, tr.hp.power), seed)
    torch.cuda.synchronize()
    m0, ops0 = oc.masters(tr), oc.snapshot(tr.plan)
    if sabotage is not None:
        sabotage(tr)
    tr.step(*to_dev(data[1], dev), 1)
    finite_losses(tr, f"{what} step 1")
    oc.assert_visible(oc.rounding_changed(m0, oc.masters(tr)), what)
    fresh = oc.fresh_plan(tr.plan, oc.device_state(tr.state_dict(), dev))
    bad = oc.check_coherent(tr.plan, fresh, tr.sgd_names, ops0)
    if frozen0 is not None:
        bad += oc.compare(tr.fixed, frozen0, "the frozen plan's operands at construction (it is never re-packed)")[0]
    return bad, fresh


def coherence_case(tr, data, dev, what):
    """First step, seeded step, coherence, checkpoint round trip, one more step on what was re-packed."""
    bad, fresh = seeded_step(tr, data, dev, what)
    assert not bad, f"{what}: " + "; ".join(bad[:8])
    img = data[1][0][-1] if isinstance(data[1][0], list) else data[1][0]
    a, b = oc.forward_backward(tr.plan, img.to(dev)), oc.forward_backward(fresh, img.to(dev))
    rt = oc.round_trip_mismatches(a, b)
    assert not rt, f"{what}: " + "; ".join(rt[:8])
    assert float(a["flat_grad"].abs().max()) > 0
    del fresh, a, b
    tr.step(*to_dev(data[2], dev), 2)
    finite_losses(tr, f"{what} step 2")


def small_simt(dev, hp_kw=None, pg=None, B=2, H=97, W=97, layers=SMALL):
    st = so.recipe_state(so.state_shapes(19, K, True, layers=layers), seed=31, head_scale=8.0)
    fst = so.recipe_state(so.state_shapes(19, 0, False, layers=layers), seed=32, head_scale=8.0)
    hp = Hyper(open_classes=K, lr=LR, lr_T=6e-3, **(hp_kw or {}))
    return SimTTrainer(st, fst, so.ntm_init(19, K, 911), so.ntm_init(19, K, 912), hp, CD.numpy(), B, H, W, dtype=BF, device=dev, layers=layers,
                       process_group=pg)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. operand coherence, small trunks
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["early", "late", "skip_unapplied_grads", "iter_size2", "rccl_one_rank"])
def test_simt_trainer_operands_coherent_after_step(dev, monkeypatch, case):
    monkeypatch.setenv("SIMT_EARLY_SGD", "0" if case == "late" else "1")
    kw = {"skip_unapplied_grads": True} if case == "skip_unapplied_grads" else {"iter_size": 2} if case == "iter_size2" else {}
    with (one_rank_group(dev, 29561) if case == "rccl_one_rank" else contextlib.nullcontext()) as pg:
        tr = small_simt(dev, kw, pg)
        assert tr._early_sgd == (case not in ("late", "iter_size2")), "the schedule under test is not the one this case names"
        assert (tr.reducer is not None) == (case == "rccl_one_rank")
        unapplied = [n for n in tr.plan.p if n.endswith(".weight") and n.split(".")[0] in ("conv1", "layer1", "layer2") and tr.plan.p[n].dim() == 4]
        assert unapplied and not set(unapplied) & set(tr.sgd_names)
        coherence_case(tr, batches(2, 97, 97, 3, 900, iter_size=tr.hp.iter_size), dev, f"SimTTrainer {case}")


def test_warmup_trainer_every_operand_changes_and_is_coherent(dev):
    st = so.recipe_state(so.state_shapes(19, 0, False, layers=SMALL), seed=77, head_scale=8.0)
    tr = WarmupTrainer(st, Hyper(open_classes=0, lr=LR), 2, 97, 97, dtype=BF, device=dev, layers=SMALL)
    ops0 = oc.snapshot(tr.plan)
    coherence_case(tr, batches(2, 97, 97, 3, 300), dev, "WarmupTrainer")
    # the warm-up stage applies every conv weight: every weight operand must have changed over the three steps
    ents = oc.pack_entries(tr.plan)
    same, _ = oc.compare(tr.plan, ops0, "x")
    changed = {s.split(":")[0] for s in same}
    still = [e.label for e in ents if e.fn in ("simt_pack_weight", "simt_stem7_pack") and e.label not in changed]
    assert not still, f"operands unchanged although the warm-up stage applies every layer: {still[:6]}"


def _single(model, dev, warmup):
    Cn, B, H, W = 19, 2, 96, 128
    if model == "v3":
        Kx, layers, width, ac = (0 if warmup else 6), (1, 2, 2), 64, 64
        st = _v3_state(v3_state_shapes(Cn, Kx, not warmup, layers, width, ac), 3)
        fst = _v3_state(v3_state_shapes(Cn, 0, False, layers, width, ac), 4)
        arch = {"layers": layers, "width": width, "assp_ch": ac}
    else:
        Kx = 0 if warmup else 3
        lay = [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in VGG_SMALL]
        st, fst = _vgg_state(Cn + Kx, lay, 5), _vgg_state(Cn, lay, 6)
        arch = {"vgg_layers": lay}
    if warmup:
        return WarmupSingleTrainer(model, st, Hyper(open_classes=0, lr=LR), B, H, W, dtype=BF, device=dev, arch=arch)
    return SimTSingleTrainer(model, st, fst, so.ntm_init(Cn, Kx, 9), Hyper(open_classes=Kx, lr=LR, lr_T=6e-3), CD.numpy(), B, H, W, dtype=BF,
                             device=dev, arch=arch)


@pytest.mark.parametrize("model", ["v3", "vgg"])
@pytest.mark.parametrize("warmup", [False, True], ids=["simt", "warmup"])
def test_single_trainers_operands_coherent_after_step(dev, model, warmup):
    tr = _single(model, dev, warmup)
    coherence_case(tr, batches(2, 96, 128, 3, 500), dev, f"{type(tr).__name__} {model}")


# ---- red: a stale operand must be found and named
def test_red_dropped_dgrad_job_of_the_subset_repack_is_named(dev, monkeypatch):
    """pack_subset loses the dgrad-operand job of one applied conv: the early step leaves that operand stale, everything else fresh."""
    victim = "layer4.0.conv2.weight"
    orig = TrunkPlan.pack_subset

    def lossy(self, names):
        raw, lib = self._pack_items_raw, L.load()
        ptr = self.p[victim].data_ptr()
        self._pack_items_raw = [it for it in raw if not (it.fn is lib.simt_pack_weight and it.args[0] == ptr and (it.args[9] & 0xFF) == 1)]
        assert len(self._pack_items_raw) == len(raw) - 1
        try:
            return orig(self, names)
        finally:
            self._pack_items_raw = raw
    monkeypatch.setattr(TrunkPlan, "pack_subset", lossy)
    monkeypatch.setenv("SIMT_EARLY_SGD", "1")
    tr = small_simt(dev)
    assert tr._early_sgd
    bad, _fresh = seeded_step(tr, batches(2, 97, 97, 2, 900), dev, "red: dropped dgrad job")
    print(bad)
    assert len(bad) == 1 and bad[0].startswith(f"{victim} (dgrad operand)") and "STALE" in bad[0], bad


@pytest.mark.parametrize("model", ["v3", "vgg"])
def test_red_missing_repack_of_single_trainer_is_named(dev, model):
    """SimTSingleTrainer's plan.repack does nothing for the step under test: every operand of an applied parameter is stale and named."""
    tr = _single(model, dev, warmup=False)

    def sabotage(t):
        t.plan.repack = lambda: None
    bad, _fresh = seeded_step(tr, batches(2, 96, 128, 2, 500), dev, f"red: no repack {model}", sabotage=sabotage)
    del tr.plan.repack
    print(len(bad), bad[:4])
    stale = {b.split(" (")[0] for b in bad if "STALE" in b}
    weights = {n for n in tr.sgd_names if tr.params[n].dim() == 4}
    assert weights and weights <= stale, f"stale operands not reported for {sorted(weights - stale)[:6]}"
    assert any("dgrad operand" in b for b in bad) and any("fprop operand" in b for b in bad)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. early against late at the production size (also part 1's full-depth case of the default schedule)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_states():
    return (ms.trained_like_init(ms.state_shapes(19, K, True), seed=1234), ms.trained_like_init(ms.state_shapes(19, 0, False), seed=1234))


def full_simt(dev, B, H, W, pg=None, **hp_kw):
    st, fst = full_states()
    return SimTTrainer(st, fst, ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), Hyper(open_classes=K, lr=LR, lr_T=6e-3, **hp_kw), CD.numpy(),
                       B, H, W, dtype=BF, device=dev, process_group=pg)


@pytest.mark.parametrize("dp", [False, True], ids=["single_gpu", "rccl_one_rank"])
def test_early_against_late_at_production_size(dev, monkeypatch, dp):
    """Three iterations of SimTTrainer at full depth, B = 4, 768 x 768, bf16, on three distinct images, SIMT_EARLY_SGD 1 against 0: losses of
    every iteration, every parameter, every momentum buffer, NTM and W state bit-identical; after the second iteration (momentum seeded so
    that the update is visible in bf16) both schedules are coherent and pass the checkpoint round trip.  One run each."""
    B, H, W = 4, 768, 768
    data = [ms.synthetic_batch(B, H, W, CD.numpy(), seed=5 + i, device=dev) for i in range(3)]
    runs = []
    with (one_rank_group(dev, 29562) if dp else contextlib.nullcontext()) as pg:
        for early in ("1", "0"):
            monkeypatch.setenv("SIMT_EARLY_SGD", early)
            tr = full_simt(dev, B, H, W, pg)
            assert tr._early_sgd == (early == "1") and tr.plan.layers == FULL and (tr.reducer is not None) == dp
            what = f"production size, SIMT_EARLY_SGD={early}{', one-rank RCCL group' if dp else ''}"
            bad, fresh = seeded_step(tr, data, dev, what)
            assert not bad, f"{what}: " + "; ".join(bad[:8])
            louts = [tr.lout.clone()]
            tr.step(*data[2], 2)
            finite_losses(tr, f"{what} step 2")
            louts.append(tr.lout.clone())
            state = dict(lout=louts, params={k: v.clone() for k, v in tr.params.items()}, mom={k: v.clone() for k, v in tr.mom.items()},
                         ntm=[t.clone() for t in tr.ntm + tr.ntm_m + tr.ntm_v], w=[t.clone() for t in tr.wraw + tr.w_m + tr.w_v])
            # checkpoint round trip, after the trajectory has been recorded (it moves the BatchNorm running statistics once more)
            fresh2 = oc.fresh_plan(tr.plan, oc.device_state(tr.state_dict(), dev))
            del fresh
            rt = oc.round_trip_mismatches(oc.forward_backward(tr.plan, data[1][0]), oc.forward_backward(fresh2, data[1][0]))
            assert not rt, f"{what}: " + "; ".join(rt[:8])
            runs.append(state)
            del tr, fresh2
            torch.cuda.empty_cache()
    a, b = runs
    assert all(torch.equal(x, y) for x, y in zip(a["lout"], b["lout"])), "losses differ between the early and the late schedule"
    for grp in ("params", "mom"):
        diff = [k for k in a[grp] if not torch.equal(a[grp][k], b[grp][k])]
        assert not diff, f"{grp} differ between the early and the late schedule: {diff[:6]}"
    assert all(torch.equal(x, y) for x, y in zip(a["ntm"], b["ntm"])) and all(torch.equal(x, y) for x, y in zip(a["w"], b["w"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the cut point, on the real byte ranges
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2, 161, 161), (4, 768, 768)], ids=["small_input", "768x768"])
@pytest.mark.parametrize("variant", ["default", "skip_unapplied_grads", "data_parallel", "two_pass_batchnorm"])
def test_early_cut_has_no_hazard_on_the_full_depth_plan(dev, monkeypatch, size, variant):
    """The byte ranges every backward launch of the full-depth (3, 4, 23, 3) SimT plan reads and writes (tests/_launch_oracle.prepare; the
    descriptors for launches with a fused BatchNorm; nothing is launched or checked numerically) against what SGD and the subset re-pack
    read and write on the side stream from `_early_cut` on: no violation.  With the cut one hook point earlier the checker must object."""
    B, H, W = size
    monkeypatch.setenv("SIMT_EARLY_SGD", "1")
    if variant == "two_pass_batchnorm":
        monkeypatch.setenv("SIMT_BN_GRID", "0")
    with (one_rank_group(dev, 29563) if variant == "data_parallel" else contextlib.nullcontext()) as pg:
        tr = full_simt(dev, B, H, W, pg, skip_unapplied_grads=(variant == "skip_unapplied_grads"))
        assert tr._early_sgd and tr._pack_applied is not None and tr.plan.layers == FULL
        assert tr.plan.data_parallel == (variant == "data_parallel")
        fused = sum(1 for it in tr.plan.bwd_list.items if it.fn is not None and lo.fn_name(it) == "simt_conv_fprop" and it.keep.fbn)
        assert fused == 0 if variant == "two_pass_batchnorm" else (fused > 0 or size != (4, 768, 768)), "the production plans fuse BatchNorm backward"
        launches, unhandled = sh.plan_launches(tr.plan, tr.plan.bwd_list, others=(tr.fixed,))
        assert not unhandled, f"backward launches without known ranges: {unhandled[:6]}"
        sgd_reads, sgd_writes, pack_writes = sh.trainer_ranges(tr)
        # trainer_ranges derives the re-pack's destinations from the plan's raw pack list: the list the trainer really runs agrees with it
        dsts = []
        for it in tr._pack_applied.items:
            if lo.fn_name(it) == "simt_pack_weight_multi":
                raw = it.keep[0].cpu().numpy().view(sh_job_dt())
                dsts += [int(j["dst"]) for j in raw]
            elif lo.fn_name(it) == "simt_pack_weight":
                dsts.append(it.args[1])
        nweight = sum(1 for w in pack_writes if w[0].endswith("operand)"))
        assert len(dsts) == nweight > 0 and all(any(w[1] <= d < w[1] + w[2] for w in pack_writes) for d in dsts)
        cut = tr._early_cut
        assert cut in set(tr.plan.grad_ready.values()), "the cut is a hook point of TrunkPlan.backward: the early step fires exactly there"
        v = sh.check_cut(launches, cut, sgd_reads, sgd_writes, pack_writes)
        print(f"{variant} {size}: {len(launches)} launches ({fused} with a fused BatchNorm), cut {cut} of {len(tr.plan.bwd_list.items)}, "
              f"{len(sgd_reads)} applied gradients, {len(pack_writes)} re-pack destinations, {len(v)} violations")
        assert not v, "; ".join(f"{x.kind} [{x.index}] {x.name}: {x.what}" for x in v[:8])
        early = sh.earlier_cut(cut, tr.plan.grad_ready.values())
        assert early is not None
        ve = sh.check_cut(launches, early, sgd_reads, sgd_writes, pack_writes)
        print(f"    cut one hook point earlier ({early}): {len(ve)} violations, kinds {sorted({x.kind for x in ve})}; first: "
              + (f"[{ve[0].index}] {ve[0].name}: {ve[0].what}" if ve else "none"))
        assert ve, "the cut could move one hook point earlier without a hazard: it is later than it needs to be"
        del tr
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. Evaluator.load and the nn.Module facades
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _trained_state(tr, data, dev):
    """The trainer's state_dict() after two steps, the second with seeded momentum: weights AND BatchNorm running statistics moved."""
    tr.step(*to_dev(data[0], dev), 0)
    oc.seed_momentum(tr, lr_poly(tr.hp.lr, 1, tr.hp.num_steps, tr.hp.power), 5)
    tr.step(*to_dev(data[1], dev), 1)
    finite_losses(tr, "state B")
    return tr.state_dict()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("model", ["v2", "v3", "vgg"])
def test_evaluator_load_refreshes_both_plans(dev, model, dtype):
    """The tools' periodic evaluation: one Evaluator (two scales = two plans over one set of parameters) given state A, then load(B): labels
    and histogram equal a fresh Evaluator given B, bitwise.  B = a trainer's state_dict() after its steps."""
    g = torch.Generator().manual_seed(11)
    if model == "v2":
        A = so.recipe_state(so.state_shapes(19, K, True, layers=SMALL), seed=31, head_scale=8.0)
        B_ = _trained_state(small_simt(dev), batches(2, 97, 97, 2, 900), dev)
        kw, s1, s2, HW = dict(open_classes=K, layers=SMALL), (65, 97), (81, 113), (130, 194)
    elif model == "v3":
        layers = (1, 2, 2)
        A = _v3_state(v3_state_shapes(19, 6, True, layers, 64, 256), 3)
        fst = _v3_state(v3_state_shapes(19, 0, False, layers, 64, 256), 4)
        tr = SimTSingleTrainer("v3", A, fst, so.ntm_init(19, 6, 9), Hyper(open_classes=6, lr=LR, lr_T=6e-3), CD.numpy(), 2, 96, 128, dtype=BF,
                               device=dev, arch={"layers": layers, "width": 64, "assp_ch": 256})
        B_ = _trained_state(tr, batches(2, 96, 128, 2, 500), dev)
        kw, s1, s2, HW = dict(open_classes=6, layers=layers), (96, 128), (128, 160), (192, 256)
    else:
        lay = [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in VGG_SMALL]      # (bf16: at least 64 channels)
        A, fst = _vgg_state(19 + K, lay, 5), _vgg_state(19, lay, 6)
        tr = SimTSingleTrainer("vgg", A, fst, so.ntm_init(19, K, 9), Hyper(open_classes=K, lr=LR, lr_T=6e-3), CD.numpy(), 2, 96, 128, dtype=BF,
                               device=dev, arch={"vgg_layers": lay})
        B_ = _trained_state(tr, batches(2, 96, 128, 2, 500), dev)
        kw, s1, s2, HW = dict(open_classes=K, layers=lay), (96, 128), (128, 160), (192, 256)
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    moved = [k for k in A if A[k].dtype != torch.long and not torch.equal(A[k], B_[k])]
    assert any(k.endswith(".weight") for k in moved) and (model == "vgg" or any(k.endswith("running_var") for k in moved))
    img1 = torch.randn(1, 3, *s1, generator=g) * 50
    img2 = torch.nn.functional.interpolate(img1, size=s2, mode="bilinear", align_corners=True)
    gt = torch.randint(0, 19, (1, *HW), generator=g)
    ev = Evaluator(A, num_classes=19, batch=1, label_hw=HW, scales=(s1, s2), dtype=dtype, device=dev, model=model, **kw)
    ev.add(img1, img2, gt)
    pred_a = ev.pred.clone()
    ev.load(B_)
    ev.add(img1, img2, gt)
    fresh = Evaluator(B_, num_classes=19, batch=1, label_hw=HW, scales=(s1, s2), dtype=dtype, device=dev, model=model, **kw)
    fresh.add(img1, img2, gt)
    torch.cuda.synchronize()
    assert torch.equal(ev.pred, fresh.pred), f"{int((ev.pred != fresh.pred).sum())} labels differ between load(B) and a fresh Evaluator(B)"
    assert torch.equal(ev.hist, fresh.hist) and int(ev.hist.sum()) == gt.numel()
    for p_old, p_new in zip(ev.plans, fresh.plans):
        bad, _ = oc.compare(p_old, p_new, "a fresh Evaluator's operand (STALE)")
        assert not bad, "; ".join(bad[:6])
    assert not torch.equal(pred_a, ev.pred), "vacuous: states A and B give the same labels"


def _facade(model, dev):
    if os.path.join(ROOT, "simt_amd") not in sys.path:          # the drop-in package names (`model`, `utils`), as tests/test_gpu_modules.py
        sys.path.insert(0, os.path.join(ROOT, "simt_amd"))
    if model == "v2":
        from model.deeplab_multi import Bottleneck, ResNetMulti
        make = lambda: ResNetMulti(Bottleneck, list(SMALL), 19, K, True)
        m = make()
        m.load_state_dict(so.recipe_state(so.state_shapes(19, K, True, layers=SMALL), seed=21))
    elif model == "v3":
        from model.deeplabv3 import DeepLabv3
        make = lambda: DeepLabv3(19, 6, True)
        torch.manual_seed(3)
        m = make()
    else:
        from model.deeplab_vgg import DeeplabVGG
        make = lambda: DeeplabVGG(19 + K)
        torch.manual_seed(4)
        m = make()
    return m.to(dev), make


@pytest.mark.parametrize("model", ["v2", "v3", "vgg"])
def test_module_facade_second_cached_plan_sees_the_optimiser_step(dev, model):
    """compute_dtype = bfloat16: an eval forward at size b (its plan is cached), a train forward + backward at size a, torch.optim.SGD.step()
    (weight decay 3 at lr 1e-2: a 3 % relative update per listing, visible in bf16), then the eval forward at size b again equals a fresh
    module loaded from state_dict(), bitwise -- weights and (v2, v3) the BatchNorm statistics the train forward moved."""
    m, make = _facade(model, dev)
    assert m.compute_dtype == BF
    g = torch.Generator().manual_seed(2)
    xa, xb = (torch.randn(2, 3, 96, 128, generator=g) * 50).to(dev), (torch.randn(1, 3, 128, 160, generator=g) * 50).to(dev)
    m.eval()
    with torch.no_grad():
        e0 = m(xb)
    m.train()
    out = m(xa)
    (1e-6 * sum((o.float() ** 2).mean() for o in (out if isinstance(out, tuple) else (out,)))).backward()      # (the decay term is the update)
    args = type("A", (), {"learning_rate": 1e-2})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = torch.optim.SGD(m.optim_parameters(args), lr=1e-2, weight_decay=3.0, foreach=False)
    listed = {id(p) for grp in opt.param_groups for p in grp["params"]}
    before = {n: p.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None and id(p) in listed}
    opt.step()
    fr = oc.rounding_changed(before, {n: p.detach().cpu() for n, p in m.named_parameters() if n in before})
    oc.assert_visible({n: f for n, f in fr.items() if before[n].dim() == 4}, f"facade {model}")
    m.eval()
    with torch.no_grad():
        e1 = m(xb)
    m2 = make()
    m2.load_state_dict(m.state_dict())
    m2 = m2.to(dev).eval()
    with torch.no_grad():
        e2 = m2(xb)
    torch.cuda.synchronize()
    for a, b, z in zip(*[(t if isinstance(t, tuple) else (t,)) for t in (e1, e2, e0)]):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ from a fresh module"
        assert not torch.equal(a, z), "vacuous: the step did not change the eval output"
