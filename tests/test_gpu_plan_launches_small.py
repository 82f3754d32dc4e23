"""Small, odd-shaped plans of the three models, fp32 AND bf16, launch by launch against float64.

tests/test_gpu_plan_launches.py and _v2.py hold the three bf16 plans bench.py times.  This file points the same replay (tests/_plan_replay.py)
and the same descriptor-driven float64 oracle (tests/_launch_oracle.py) at the plans the tile planner builds AWAY from those sizes, in both
storage dtypes: the fp32 parity plans (conv_igemm.hip / conv_wgrad.hip on the fp32 MFMA, the im2col stem, the multi-tap ASPP heads with bias,
ungrouped weight gradients, the stand-alone first pass of the BatchNorm backward, the <float> instantiations of the pools, scatters, column
sums and upsamplers) and bf16 plans with M below one 128-row tile, fewer tiles than workgroups, ragged direct-stem tiles and dilations larger
than the map.

Per case (model x dtype x geometry), under SIMT_SINGLE_STREAM=1 and SIMT_BN_GRID=0: the trainable plan's pack list, the frozen partner's pack
list, the trainable forward, the frozen forward, then -- the upstream gradient seeded -- the trainable backward, ONE LAUNCH AT A TIME, inputs
snapshotted and outputs poisoned before each launch, every stored element held to its derived bound right after.  Asserted per case, as
_assert_model of tests/test_gpu_plan_launches.py does: no launch outside its bar, no uncovered launch (NOT_HERE is empty), every conv launch's
weight operand traced to its parameter with that layer's geometry (tests/_plan_layers.py), every layer launched in each direction.

  DeepLab-v2   layers (1, 1, 2, 1), multi_heads(19, 3, True) trainable + multi_heads(19, 0, False) frozen (stem_from= the trainable plan):
               B=1  65x81   stride-8 map  9x11, M =  99  one partial tile in layers 2-4, fewer tiles than workgroups everywhere
               B=3  97x129  stride-8 map 13x17, M = 663  ragged last tile, B not a power of two
               B=2  33x193  stride-8 map  5x25, M = 250  map height below layer 4's dilation and both ASPP dilations
               and, eval only: single_head(19) (the 4-branch, 36-tap head of model/deeplab.py), layers (1, 1, 1, 1), B=1 65x81
  DeepLabv3    layers (1, 2, 2), Q = 19 + 6 trainable + closed-set frozen, width = assp_ch = 32 (fp32) / 64 (bf16): B=2 65x97, B=1 96x160
  DeepLab-VGG  Q = 19 + 3 trainable + 19 frozen, test_gpu_vgg.SMALL (fp32) / its 64-channel widening (bf16):     B=2 64x80, B=3 40x72
No plan constructor refused a size: none is substituted.

On top of that:
  * red tests: copies of real results of these plans are perturbed (an element moved by 4 x ITS OWN bound, two columns swapped, a border row
    zeroed, a statistics slot scaled by 1 + 1e-3 in fp32; the 2-ulp set of the existing files on a bf16 launch with M < 128) and the checker
    must raise for every one;
  * the serial replay equals the schedule the trainers run: the same plans built under the default environment (default SIMT_BN_GRID, two
    streams), forward and backward on the same weights, image and seeded gradients, must give the replay's logits, gradients and BatchNorm
    running statistics bit for bit.
"""
import time

import pytest
import torch

import _launch_oracle as lo
import test_gpu_v3 as tv3
import test_gpu_vgg as tvgg
from _plan_layers import v2_layers, v3_layers, vgg_layers
from _plan_replay import Run, _env, _perturb, _two_ulps, match_layers, replay
from oracle import simt_oracle as so

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32

# tag -> the test that holds launches of that tag instead.  Empty: every entry point of these plans has a handler.
NOT_HERE = {}

V2_LAYERS, V2_K = (1, 1, 2, 1), 3
V3_LAYERS, V3_K = (1, 2, 2), 6
VGG_K = 3
CASES = ([("v2", dt, B, H, W) for (B, H, W) in ((1, 65, 81), (3, 97, 129), (2, 33, 193)) for dt in (F32, BF)]
         + [("v2single", dt, 1, 65, 81) for dt in (F32, BF)]
         + [("v3", dt, B, H, W) for (B, H, W) in ((2, 65, 97), (1, 96, 160)) for dt in (F32, BF)]
         + [("vgg", dt, B, H, W) for (B, H, W) in ((2, 64, 80), (3, 40, 72)) for dt in (F32, BF)])
TRAINABLE = [c for c in CASES if c[0] != "v2single"]
RED_F32, RED_BF16 = ("v2", F32, 1, 65, 81), ("v2", BF, 1, 65, 81)


def _id(case):
    m, dt, B, H, W = case
    return f"{m}-{'bf16' if dt == BF else 'fp32'}-b{B}-{H}x{W}"


def _params(st, dev):
    return {k: v.detach().to(dev, torch.float32 if v.dtype != torch.long else torch.long).clone() for k, v in st.items()}


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def _vgg_table(dtype):
    return tvgg.SMALL if dtype == F32 else [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in tvgg.SMALL]


def _v3_width(dtype):
    return 32 if dtype == F32 else 64


class _Model:
    """How one case builds its plans, seeds its upstream gradient and names its layers."""

    def __init__(self, case):
        self.model, self.dtype, self.B, self.H, self.W = case
        m, dt = self.model, self.dtype
        if m == "v2":
            self.st = so.recipe_state(so.state_shapes(19, V2_K, True, layers=V2_LAYERS), seed=77)
            self.fst = so.recipe_state(so.state_shapes(19, 0, False, layers=V2_LAYERS), seed=78)
        elif m == "v2single":
            self.st, self.fst = None, so.recipe_state(so.state_shapes(19, layers=(1, 1, 1, 1), single_head=True), seed=79)
        elif m == "v3":
            wd = _v3_width(dt)
            self.st = tv3.make_state(tv3.v3_state_shapes(19, V3_K, True, V3_LAYERS, wd, wd), 5)
            self.fst = tv3.make_state(tv3.v3_state_shapes(19, 0, False, V3_LAYERS, wd, wd), 6)
        else:
            self.st = tvgg.make_state(tvgg.vgg_state_shapes(19 + VGG_K, _vgg_table(dt)), 5)
            self.fst = tvgg.make_state(tvgg.vgg_state_shapes(19, _vgg_table(dt)), 6)
        g = torch.Generator().manual_seed(7)
        self.img = torch.randn(self.B, 3, self.H, self.W, generator=g) * (50.0 if m.startswith("v2") else 1.0)

    def plans(self, dev):
        """(trainable or None, frozen), built as the trainers build them."""
        m, dt, B, H, W = self.model, self.dtype, self.B, self.H, self.W
        if m == "v2":
            from simt_amd.engine import TrunkPlan, multi_heads
            tr = TrunkPlan(_params(self.st, dev), B, H, W, multi_heads(19, V2_K, True), dtype=dt, train=True, layers=V2_LAYERS)
            fr = TrunkPlan(_params(self.fst, dev), B, H, W, multi_heads(19, 0, False), dtype=dt, train=False, layers=V2_LAYERS, stem_from=tr)
            return tr, fr
        if m == "v2single":
            from simt_amd.engine import TrunkPlan, single_head
            return None, TrunkPlan(_params(self.fst, dev), B, H, W, single_head(19), dtype=dt, train=False, layers=(1, 1, 1, 1))
        if m == "v3":
            from simt_amd.engine_v3 import V3Plan
            wd = _v3_width(dt)
            tr = V3Plan(_params(self.st, dev), B, H, W, 19, V3_K, True, dtype=dt, train=True, layers=V3_LAYERS, width=wd, assp_ch=wd)
            fr = V3Plan(_params(self.fst, dev), B, H, W, 19, 0, False, dtype=dt, train=False, layers=V3_LAYERS, width=wd, assp_ch=wd)
            return tr, fr
        from simt_amd.engine_vgg import VggPlan
        tr = VggPlan(_params(self.st, dev), B, H, W, 19 + VGG_K, dtype=dt, train=True, vgg_layers=_vgg_table(dt))
        fr = VggPlan(_params(self.fst, dev), B, H, W, 19, dtype=dt, train=False, vgg_layers=_vgg_table(dt))
        return tr, fr

    def tables(self):
        """(trainable table or None, frozen table)"""
        m, dt, B, H, W = self.model, self.dtype, self.B, self.H, self.W
        if m == "v2":
            return v2_layers(B, H, W, V2_K, V2_LAYERS, dt), v2_layers(B, H, W, 0, V2_LAYERS, dt)
        if m == "v2single":
            from simt_amd.engine import single_head
            return None, v2_layers(B, H, W, 0, (1, 1, 1, 1), dt, heads=single_head(19))
        if m == "v3":
            wd = _v3_width(dt)
            return v3_layers(B, H, W, V3_LAYERS, 19 + V3_K, wd, wd, dt), v3_layers(B, H, W, V3_LAYERS, 19, wd, wd, dt)
        return vgg_layers(B, H, W, 19 + VGG_K, _vgg_table(dt), dt), vgg_layers(B, H, W, 19, _vgg_table(dt), dt)

    def seed_grad(self, tr):
        """N(0, 1) / (h w) upstream gradient, as the two existing files seed it: dout_full (DeepLabv3) or the Q live columns of dlogits."""
        g = torch.Generator().manual_seed(8)
        if self.model == "v3":
            tr.dout_full.copy_((torch.randn(tr.dout_full.shape, generator=g) / (tr.H * tr.W)).to(tr.dout_full.device))
            return
        for dl in tr.dlogits.values():
            hd = tr.heads[0]
            dl.zero_()
            dl[:, :hd.Q] = (torch.randn(dl.shape[0], hd.Q, generator=g) / (hd.h * hd.w)).to(dl.dtype).to(dl.device)

    def feed(self, tr, fr, dev):
        for pl in (tr, fr):
            if pl is not None:
                pl.x_in.copy_(self.img.to(dev))

    def snapshot(self, tr, fr):
        """What the tie compares: both networks' logits, the trainable flat gradient buffer, the BatchNorm running statistics."""
        out = {}
        for n, pl in (("trainable", tr), ("frozen", fr)):
            if self.model == "v3":
                out[f"logits {n}"], out[f"logits {n} (low resolution)"] = pl.out_full.clone(), pl.logits.clone()
            else:
                out.update({f"logits {n} {k}": pl.out[k].clone() for k in pl.out})
        out["flat_grad"] = tr.flat_grad.clone()
        for k, v in tr.p.items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                out[k] = v.clone()
        return out


# ---- red hooks -------------------------------------------------------------------------------------------------------------------------------
def _move(t, idx, bound, k=4.0):
    """Move t[idx] away from zero by k x `bound` (a 0-dim float64 tensor: that element's own bound)."""
    v = t[idx].double()
    t[idx] = (v + k * bound * (1 if v >= 0 else -1)).to(t.dtype)


def _swap01(t):
    t.copy_(t[..., [1, 0] + list(range(2, t.shape[-1]))])


def _conv_cases_f32(chk, got, stats):
    y = got["y"]
    rows, tol = chk.bounds["rows"], chk.bounds["y"]
    r0 = int(rows[0])
    col = int(y[r0].abs().argmax())
    border = int(rows[min(10, rows.numel() - 1)])
    cases = [("4 x its bound", lambda g: _move(g["y"], (r0, col), tol[0, col])),
             ("columns swapped", lambda g: _swap01(g["y"])),
             ("border row zeroed", lambda g: g["y"][border].zero_())]
    if stats:
        cases.append(("stats slot 1e-3", lambda g: g["stats"][0].mul_(1.0 + 1e-3)))
    return cases


def _red_hook(run, dtype, frozen=False):
    def take(key, it, chk, got, cases):
        run.red[key] = (f"{it.tag} {it.shape or ''}", [c[0] for c in cases], _perturb(chk, got, key, cases))

    def hook(lname, it, chk, got):
        name = lo.fn_name(it)
        d = it.keep
        if dtype == BF:
            # the existing 2-ulp set on a conv launch with M < 128 (3x3 dilated, statistics)
            if not frozen and "conv" not in run.red and name == "simt_conv_fprop" and d.stats and d.ntaps == 9 and d.B * d.Ho * d.Wo < 128:
                col = int(got["y"][0].float().abs().argmax())
                cases = [("2 ulps", lambda g: _two_ulps(g["y"], (0, col))),
                         ("columns swapped", lambda g: _swap01(g["y"])),
                         ("border row zeroed", lambda g: g["y"][10].zero_()),
                         ("stats slot 1e-3", lambda g: g["stats"][0].mul_(1.0 + 1e-3))]
                take("conv", it, chk, got, cases)
            return
        if frozen:
            if "frozen conv" not in run.red and name == "simt_conv_fprop" and d.bias and d.res and d.relu:
                take("frozen conv", it, chk, got, _conv_cases_f32(chk, got, False))
            return
        if "conv" not in run.red and name == "simt_conv_fprop" and d.stats and d.ntaps == 9 and int(d.dy[0]) < -1:
            take("conv", it, chk, got, _conv_cases_f32(chk, got, True))
        if "wgrad" not in run.red and name == "simt_conv_wgrad" and d.ntaps == 9 and int(d.dy_[0]) < -1:
            s, tol = got["slab0"], chk.bounds["slab0"]
            flat = int(s.double().sum(0).abs().argmax())
            co, kk = flat // s.shape[2], flat % s.shape[2]
            cases = [("4 x its bound", lambda g: _move(g["slab0"], (0, co, kk), tol[co, kk])),
                     ("columns swapped", lambda g: _swap01(g["slab0"])),
                     ("edge-tap row zeroed", lambda g: g["slab0"][:, 0, :d.Cin].zero_())]
            take("wgrad", it, chk, got, cases)
        if "bn_bwd" not in run.red and name == "simt_bn_bwd" and "part" in got and not d.y2:
            dy, tol, ctol = got["dy"], chk.bounds["dy"], chk.bounds["coef"]
            col = int(dy[0].abs().argmax())
            ccol = int(got["coef"][1].abs().argmax())
            cases = [("dy: 4 x its bound", lambda g: _move(g["dy"], (0, col), tol[0, col])),
                     ("coef: 4 x its bound", lambda g: _move(g["coef"], (1, ccol), ctol[1, ccol])),
                     ("dy: columns swapped", lambda g: _swap01(g["dy"])),
                     ("dy: border row zeroed", lambda g: g["dy"][10].zero_()),
                     ("statistics slot 1e-3", lambda g: g["part"][0].mul_(1.0 + 1e-3))]
            take("bn_bwd", it, chk, got, cases)
    return hook


# ---- one case ---------------------------------------------------------------------------------------------------------------------------------
_DONE = {}


def _run_case(case, dev):
    """Serial replay under the oracle, then (trainable cases) the default schedule on fresh plans.  Cached: the red and tie tests read it."""
    if case in _DONE:
        return _DONE[case]
    from simt_amd import engine as eng
    mdl = _Model(case)
    res = {"id": _id(case)}
    t0, f0 = time.time(), lo.GEMM_FLOPS[0]
    with pytest.MonkeyPatch.context() as mp:
        _env(mp)
        tr, fr = mdl.plans(dev)
        run, run_f = Run(), Run()
        red = case in (RED_F32, RED_BF16)                       # (the red cases are taken on the way through those two replays)
        hook, hook_f = (_red_hook(run, mdl.dtype), _red_hook(run_f, mdl.dtype, frozen=True)) if red else (None, None)
        mdl.feed(tr, fr, dev)
        ttab, ftab = mdl.tables()
        pre = mdl.model
        if tr is not None:
            replay(tr, [(pre + ".pack", tr.pack_list)], run, hook, others=(fr,), not_here=NOT_HERE)
        replay(fr, [(pre + "f.pack", fr.pack_list)], run_f, hook_f, others=(tr,) if tr is not None else (), not_here=NOT_HERE)
        if tr is not None:
            replay(tr, [(pre + ".fwd", tr.fwd_list)], run, hook, others=(fr,), not_here=NOT_HERE)
        replay(fr, [(pre + "f.fwd", fr.fwd_list)], run_f, hook_f, others=(tr,) if tr is not None else (), not_here=NOT_HERE)
        if tr is not None:
            mdl.seed_grad(tr)
            replay(tr, [(pre + ".bwd", tr.bwd_list)], run, hook, others=(fr,), not_here=NOT_HERE)
        torch.cuda.synchronize()
        # a shared direct-stem launch's second weight set is the frozen network's conv1
        stem_f = [c for c in run.convs if c[0].endswith(" set 1")]
        run.convs = [c for c in run.convs if not c[0].endswith(" set 1")]
        run_f.convs += stem_f
        if tr is not None:
            match_layers(tr, run, ttab, True)
            res["serial"] = mdl.snapshot(tr, fr)
        match_layers(fr, run_f, ftab, False)
        del tr, fr
        torch.cuda.empty_cache()
    res["secs"], res["tflop"] = time.time() - t0, (lo.GEMM_FLOPS[0] - f0) / 1e12
    res["run"], res["run_f"] = run, run_f
    if mdl.st is not None and not run.fail:
        # ---- the schedule the trainers run: default environment (default SIMT_BN_GRID, two streams), same weights / image / gradients
        t1 = time.time()
        with pytest.MonkeyPatch.context() as mp:
            mp.delenv("SIMT_SINGLE_STREAM", raising=False)
            mp.delenv("SIMT_BN_GRID", raising=False)
            eng._SIDE_STREAMS.clear()
            tr, fr = mdl.plans(dev)
            res["fbn_launches"] = tr.fbn_launches
            mdl.feed(tr, fr, dev)
            tr.fwd_list.run()
            fr.fwd_list.run()
            mdl.seed_grad(tr)
            tr.bwd_list.run()
            torch.cuda.synchronize()
            res["fbn_error"] = tr.fbn_error()
            res["prod"] = mdl.snapshot(tr, fr)
            del tr, fr
            torch.cuda.empty_cache()
        res["prod_secs"] = time.time() - t1
    eng._SIDE_STREAMS.clear()
    _DONE[case] = res
    return res


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_small_plan_launches_hold_float64(dev, case):
    """Every launch of the trainable (pack, forward, backward) and frozen (pack, forward) plans within its float64 bar; no launch uncovered;
    every conv launch has its layer's geometry and every layer is launched in each direction."""
    res = _run_case(case, dev)
    run, run_f = res["run"], res["run_f"]
    name = res["id"]
    worst = dict(run.worst)
    for k, v in run_f.worst.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n{name}: {run.n + run_f.n} launches checked in {res['secs']:.1f} s wall (plans built, replayed and checked; {res['tflop']:.3f} TFLOP "
          f"of float64 GEMM in the oracle); {len(worst)} distinct (tag, shape), worst error / bound:")
    for (tag, shape), r in sorted(worst.items()):
        print(f"  {r:6.3f}  {tag}  {shape}")
    fails = run.fail + run_f.fail
    assert not fails, f"{name}: {len(fails)} launch(es) outside their float64 bar:\n  " + "\n  ".join(fails[:40])
    unc = run.uncovered + run_f.uncovered
    assert not unc, f"{name}: {len(unc)} launch(es) neither checked by a handler nor listed in NOT_HERE:\n  " + "\n  ".join(unc[:40])
    bad = run.layer_bad + run_f.layer_bad
    assert not bad, f"{name}: {len(bad)} conv launch(es) not matching their layer:\n  " + "\n  ".join(bad[:20])
    for what, r in (("trainable", run), ("frozen", run_f)):
        assert not r.layer_missing, f"{name} {what} plan: layers never launched {r.layer_missing[:6]}"
    assert run_f.n > 0 and (case[0] == "v2single" or run.n > 0)
    if case[0].startswith("v2"):
        assert ("conv1", "fwd") in run_f.layer_seen and (case[0] == "v2single" or ("conv1", "fwd") in run.layer_seen)
    assert all(r <= 1.0 for r in worst.values())


@pytest.mark.parametrize("case", [RED_F32, RED_BF16], ids=_id)
def test_small_oracle_is_red_on_perturbed_results(dev, case):
    """The checker must fail on perturbed copies of real stored results of these plans.  fp32 (one element moved by 4 x its own bound, read
    from the bound tensor of the check; two output columns swapped; one border row zeroed; one statistics slot scaled by 1 + 1e-3): a 3x3
    dilated conv with statistics and its weight-gradient slab on the first-generation fp32 kernels, a simt_bn_bwd launch (dy and coef), and a
    frozen-plan bias + residual + ReLU conv.  bf16: the 2-ulp set of the existing files on a conv launch with M = 99 < 128."""
    res = _run_case(case, dev)
    red = dict(res["run"].red)
    red.update(res["run_f"].red)
    want = {"conv", "wgrad", "bn_bwd", "frozen conv"} if case[1] == F32 else {"conv"}
    assert set(red) == want, f"red cases found: {sorted(red)}"
    for what, (launch, cases, caught) in red.items():
        print(f"{what}: {launch}: caught {caught}")
        assert caught == cases, f"{what} ({launch}): the checker missed {sorted(set(cases) - set(caught))}"


@pytest.mark.parametrize("case", TRAINABLE, ids=_id)
def test_small_default_schedule_matches_the_replay_bitwise(dev, case):
    """The default schedule (two streams, the default SIMT_BN_GRID) against the serial two-pass replay: both networks' logits, every gradient
    and the BatchNorm running statistics bit for bit."""
    res = _run_case(case, dev)
    assert "prod" in res, "the serial replay failed: see test_small_plan_launches_hold_float64"
    print(f"\n{res['id']} default schedule: {res['fbn_launches']} fused BatchNorm launches, {res['prod_secs']:.1f} s wall")
    assert not res["fbn_error"], "a fused BatchNorm launch timed out waiting for co-residency (another process held CUs)"
    s, p = res["serial"], res["prod"]
    assert set(s) == set(p)
    diff = []
    for k in s:
        ne = int((_bits(s[k]) != _bits(p[k])).sum())
        if ne:
            diff.append(f"{k}: {ne} of {s[k].numel()} elements differ")
    assert not diff, "default schedule differs from the serial replay:\n  " + "\n  ".join(diff[:20])
