"""The two other benchmarked models, launch by launch, against float64 (bench.py --model v3 / --model vgg, bf16).

DeepLabv3 (B=4, 512x1024, layers (3, 4, 6), Q = 19 + 6) and DeepLab-VGG16 (B=8, 512x512, Q = 19 + 3): the trainable plan (pack list,
forward, backward) and the frozen plan (pack list, forward) at the sizes bench.py times, Kaiming weights.  Every launch of those lists is
replayed ONE AT A TIME on one stream (SIMT_SINGLE_STREAM=1; SIMT_BN_GRID=0: the two-pass BatchNorm, whose fused forms
tests/test_gpu_bn_fused.py ties bit for bit to these; the replay is tests/_plan_replay.py), its inputs snapshotted and its outputs poisoned
before it runs, and checked right after by the descriptor-driven float64 oracle of tests/_launch_oracle.py; the chain then continues on the
kernel's own result.

Coverage is enforced: a launch that no handler checks and whose tag is not in NOT_HERE fails the test by name.  Each conv launch's weight
operand is traced to the parameter(s) the pack jobs wrote into that buffer, and the launch's geometry (Cin, Cout, stride, taps, H / W) must
be that layer's as v3_block_specs / ASSP_BRANCHES / VGG_LAYERS describe it; every layer must be launched in each direction.  With the
packing check (packed operand == bf16 of the parameter) this ties every conv's weight operand to its own parameter.  The activation
operand is not traced here: it is whatever the previous launch of the chain wrote, checked there (tests/test_gpu_plan_launches_v2.py
traces DeepLab-v2's to their last writer).
"""
import time

import pytest
import torch
import torch.nn.functional as F

import _launch_oracle as lo
from _plan_layers import v3_layers, vgg_layers
from _plan_replay import Run, _env, _perturb, _two_ulps, match_layers, replay
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import model_spec as ms
from simt_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CD = so.load_class_dist()

# tag -> the test that holds launches of that tag instead.  Empty: with SIMT_BN_GRID=0 the plans carry no fused-BatchNorm launch (the only
# form this oracle refuses), and every other entry point has a handler.
NOT_HERE = {}


def _seed_and_backward(plan, lists_bwd, run, red, B, Q, dev, v3):
    g = torch.Generator().manual_seed(8)
    if v3:
        plan.dout_full.copy_((torch.randn(plan.dout_full.shape, generator=g) / (plan.H * plan.W)).to(dev))
    else:
        for dl in plan.dlogits.values():
            hd = plan.heads[0]
            dl.zero_()
            dl[:, :Q] = (torch.randn(dl.shape[0], Q, generator=g) / (hd.h * hd.w)).to(BF).to(dev)
    replay(plan, lists_bwd, run, red, not_here=NOT_HERE)


def _red_hook(run):
    def hook(lname, it, chk, got):
        name = lo.fn_name(it)
        if "conv" not in run.red and name == "simt_conv_fprop" and it.keep.stats and it.keep.ntaps == 9 and it.keep.stride == 1 \
                and it.keep.B * it.keep.Ho * it.keep.Wo == 8192:
            y = got["y"]
            col = int(y[0].float().abs().argmax())
            border = 10                                           # pixel (b 0, row 0, col 10): its top taps read outside the image
            cases = [("2 ulps", lambda g: _two_ulps(g["y"], (0, col))),
                     ("columns swapped", lambda g: g["y"].copy_(g["y"][:, [1, 0] + list(range(2, g["y"].shape[1]))])),
                     ("border row zeroed", lambda g: g["y"][border].zero_()),
                     ("stats slot 1e-3", lambda g: g["stats"][3].mul_(1.0 + 1e-3))]
            run.red["conv"] = (f"{it.tag} {it.shape}", [c[0] for c in cases], _perturb(chk, got, "conv", cases))
        if "wgrad" not in run.red and name == "simt_conv_wgrad" and it.keep.ntaps == 9 and int(it.keep.dy_[0]) == -18:
            s = got["slab0"]
            flat = int(s[0].abs().argmax())
            co, kk = flat // s.shape[2], flat % s.shape[2]
            cases = [("2 ulps", lambda g: _two_ulps(g["slab0"], (0, co, kk))),
                     ("columns swapped", lambda g: g["slab0"].copy_(g["slab0"][:, :, [1, 0] + list(range(2, s.shape[2]))])),
                     ("edge-tap row zeroed", lambda g: g["slab0"][:, 0, :it.keep.Cin].zero_())]
            run.red["wgrad"] = (f"{it.tag} {it.shape}", [c[0] for c in cases], _perturb(chk, got, "wgrad", cases))
        if "maxpool2_bwd" not in run.red and name == "simt_maxpool2_bwd":
            da = got["da"]
            nz = (da[0, 0] != 0).nonzero()
            assert nz.shape[0] > 0
            e = (0, 0) + tuple(int(v) for v in nz[0])
            cases = [("2 ulps", lambda g: _two_ulps(g["da"], e)),
                     ("columns swapped", lambda g: g["da"].copy_(g["da"][..., [1, 0] + list(range(2, da.shape[-1]))])),
                     ("border row zeroed", lambda g: g["da"][0, 0].zero_())]
            run.red["maxpool2_bwd"] = (f"{it.tag} {it.args[4:8]}", [c[0] for c in cases], _perturb(chk, got, "maxpool2_bwd", cases))
    return hook


@pytest.fixture(scope="module")
def runs(dev):
    """Both models replayed once (the red cases are taken on the way); every test below reads its part."""
    from simt_amd.engine_v3 import V3Plan, v3_state_shapes
    from simt_amd.engine_vgg import VggPlan, vgg_state_shapes
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        _env(mp)
        # ---- DeepLabv3, bench.py --model v3: B=4, 512x1024, layers (3, 4, 6), Q = 19 + 6
        t0, f0 = time.time(), lo.GEMM_FLOPS[0]
        K, B, H, W, lay = 6, 4, 512, 1024, (3, 4, 6)
        run = Run()
        hook = _red_hook(run)
        img, _ = ms.synthetic_batch(B, H, W, CD.numpy(), seed=7, device=dev)
        st = ms.kaiming_init(v3_state_shapes(19, K, True, layers=lay), seed=1234)
        p = {k: v.to(dev) for k, v in st.items()}
        tr = V3Plan(p, B, H, W, 19, K, True, dtype=BF, train=True, layers=lay)
        tr.x_in.copy_(img)
        replay(tr, [("v3.pack", tr.pack_list), ("v3.fwd", tr.fwd_list)], run, hook, not_here=NOT_HERE)
        _seed_and_backward(tr, [("v3.bwd", tr.bwd_list)], run, hook, B, 19 + K, dev, True)
        match_layers(tr, run, v3_layers(B, H, W, lay, 19 + K), True)
        del tr, p
        torch.cuda.empty_cache()
        fst = ms.kaiming_init(v3_state_shapes(19, 0, False, layers=lay), seed=1234)
        fp = {k: v.to(dev) for k, v in fst.items()}
        fr = V3Plan(fp, B, H, W, 19, 0, False, dtype=BF, train=False, layers=lay)
        fr.x_in.copy_(img)
        run_f = Run()
        replay(fr, [("v3f.pack", fr.pack_list), ("v3f.fwd", fr.fwd_list)], run_f, not_here=NOT_HERE)
        match_layers(fr, run_f, v3_layers(B, H, W, lay, 19), False)
        del fr, fp
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        out["v3"] = (run, run_f, time.time() - t0, lo.GEMM_FLOPS[0] - f0)
        # ---- DeepLab-VGG16, bench.py --model vgg: B=8, 512x512, Q = 19 + 3
        t0, f0 = time.time(), lo.GEMM_FLOPS[0]
        K, B, H, W = 3, 8, 512, 512
        run = Run()
        hook = _red_hook(run)
        img, _ = ms.synthetic_batch(B, H, W, CD.numpy(), seed=7, device=dev)
        st = ms.kaiming_init(vgg_state_shapes(19 + K), seed=1234)
        p = {k: v.to(dev) for k, v in st.items()}
        tr = VggPlan(p, B, H, W, 19 + K, dtype=BF, train=True)
        tr.x_in.copy_(img)
        replay(tr, [("vgg.pack", tr.pack_list), ("vgg.fwd", tr.fwd_list)], run, hook, not_here=NOT_HERE)
        _seed_and_backward(tr, [("vgg.bwd", tr.bwd_list)], run, hook, B, 19 + K, dev, False)
        match_layers(tr, run, vgg_layers(B, H, W, 19 + K), True)
        del tr, p
        torch.cuda.empty_cache()
        fst = ms.kaiming_init(vgg_state_shapes(19), seed=1234)
        fp = {k: v.to(dev) for k, v in fst.items()}
        fr = VggPlan(fp, B, H, W, 19, dtype=BF, train=False)
        fr.x_in.copy_(img)
        run_f = Run()
        replay(fr, [("vggf.pack", fr.pack_list), ("vggf.fwd", fr.fwd_list)], run_f, not_here=NOT_HERE)
        match_layers(fr, run_f, vgg_layers(B, H, W, 19), False)
        del fr, fp
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        out["vgg"] = (run, run_f, time.time() - t0, lo.GEMM_FLOPS[0] - f0)
    import simt_amd.engine as eng
    eng._SIDE_STREAMS.clear()
    return out


def _assert_model(name, runs):
    run, run_f, secs, flops = runs[name]
    worst = dict(run.worst)
    for k, v in run_f.worst.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n{name}: {run.n + run_f.n} launches checked in {secs:.1f} s wall (plans built, replayed and checked; "
          f"{flops / 1e12:.2f} TFLOP of float64 GEMM in the oracle); {len(worst)} distinct (tag, shape), worst error / bound:")
    for (tag, shape), r in sorted(worst.items()):
        print(f"  {r:6.3f}  {tag}  {shape}")
    fails = run.fail + run_f.fail
    assert not fails, f"{name}: {len(fails)} launch(es) outside their float64 bar:\n  " + "\n  ".join(fails[:40])
    unc = run.uncovered + run_f.uncovered
    assert not unc, f"{name}: {len(unc)} launch(es) neither checked by a handler nor listed in NOT_HERE:\n  " + "\n  ".join(unc[:40])
    # every conv launch has the geometry of the layer whose parameter was packed into its weight operand, and every layer is launched
    bad = run.layer_bad + run_f.layer_bad
    assert not bad, f"{name}: {len(bad)} conv launch(es) not matching their layer:\n  " + "\n  ".join(bad[:20])
    for what, r in (("trainable", run), ("frozen", run_f)):
        assert not r.layer_missing, f"{name} {what} plan: layers never launched {r.layer_missing[:6]}"
    assert all(r <= 1.0 for r in worst.values())


def test_v3_plan_launches_hold_float64_b4_512x1024(runs):
    """DeepLabv3 + SimT(K=6) bf16 at bench.py's size: every launch of the trainable (pack, forward, backward) and frozen (pack, forward)
    plans within its float64 bar; each conv launch has the geometry of its layer (v3_block_specs / ASSP_BRANCHES)."""
    _assert_model("v3", runs)


def test_vgg_plan_launches_hold_float64_b8_512x512(runs):
    """DeepLab-VGG16 + SimT(K=3) bf16 at bench.py's size (M = 2 097 152 in layer 0): every launch within its float64 bar; each conv launch has
    the geometry of its layer (VGG_LAYERS, the tap-expanded head)."""
    _assert_model("vgg", runs)


def test_launch_oracle_is_red_on_perturbed_results(runs):
    """The checker must fail on a copy of a real launch's stored result with one element moved by 2 bf16 ulps, two output columns swapped, one
    border row zeroed and (conv) one statistics slot off by 1e-3 relative: a conv launch at M = 8192 (3x3, statistics), the dilation-18 ASSP
    weight gradient and a VGG max-pool backward.  Stored data only is perturbed; the descriptors are untouched."""
    red = {}
    for name in ("v3", "vgg"):
        red.update(runs[name][0].red)
    assert set(red) == {"conv", "wgrad", "maxpool2_bwd"}, f"red cases found: {sorted(red)}"
    for what, (launch, cases, caught) in red.items():
        print(f"{what}: {launch}: caught {caught}")
        assert caught == cases, f"{what} ({launch}): the checker missed {sorted(set(cases) - set(caught))}"


def test_maxpool2_ties_follow_torch(dev):
    """simt_maxpool2 on bf16 with planted ties (equal values in 2x2 windows, all-zero windows, a negative-zero tie) against CPU
    torch.max_pool2d(return_indices=True), which keeps the FIRST maximum in scan order; and the oracle's restatement of that rule
    (_launch_oracle.maxpool2_expect) against the same."""
    B, H, W, Cn = 2, 64, 96, 64
    g = torch.Generator().manual_seed(5)
    y = torch.randn(B, H, W, Cn, generator=g).round().to(BF)          # integers in about [-4, 4]: many exact ties
    y[:, 0:8] = 0.0                                                   # all-zero windows
    y[0, 8, 0, :] = 3.0
    y[0, 9, 1, :] = 3.0                                               # tie between (0, 0) and (1, 1)
    y[1, 10, 2, :] = -0.0
    y[1, 10, 3, :] = 0.0
    y[1, 11, 2:4, :] = -1.0                                           # +0 / -0 tie
    yd = y.to(dev)
    Hp, Wp = H // 2, W // 2
    p = torch.empty(B, Hp, Wp, Cn, device=dev, dtype=BF)
    idx = torch.empty(B, Hp, Wp, Cn, device=dev, dtype=torch.uint8)
    L.call("simt_maxpool2", yd.data_ptr(), p.data_ptr(), idx.data_ptr(), B, H, W, Cn, L.SIMT_BF16, ops.stream_ptr())
    torch.cuda.synchronize()
    rv, ri = F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2, return_indices=True)
    ri = ri.permute(0, 2, 3, 1)                                       # flat index iy * W + ix in the plane
    r_idx = ((ri // W) % 2) * 2 + (ri % W) % 2
    assert torch.equal(p.cpu(), rv.permute(0, 2, 3, 1))
    assert torch.equal(idx.cpu().long(), r_idx), "arg-max index differs from torch's first maximum"
    best, bi = lo.maxpool2_expect(y)
    assert torch.equal(best, rv.permute(0, 2, 3, 1)) and torch.equal(bi.long(), r_idx)
