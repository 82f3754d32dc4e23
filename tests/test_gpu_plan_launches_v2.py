"""DeepLab-v2 + SimT(K=3), bench.py's headline plan (B=4, 768x768, bf16, ResNet-101), launch by launch against float64.

The trainable TrunkPlan (multi_heads(19, 3, True), train=True) and the frozen one (multi_heads(19, 0, False), train=False, stem_from= the
trainable plan) are built as SimTTrainer builds them, with seeded weights, and replayed ONE LAUNCH AT A TIME (tests/_plan_replay.py) under the
float64 oracle of tests/_launch_oracle.py: trainable pack list, frozen pack list, trainable forward (its direct-stem launch writes both
networks' stem outputs), frozen forward, then -- dlogits seeded -- the trainable backward.  SIMT_SINGLE_STREAM=1 and SIMT_BN_GRID=0 (the
two-pass BatchNorm); every other switch keeps its default, and the test asserts that the plan really is the production one (direct stem and
stem weight gradient, grouped weight gradients, operand-path BatchNorm, bit-mask residuals, the row-streaming 1x1 and 256-column 3x3 tiles).

On top of the per-launch bars:
  * every conv launch's weight operand is traced to its parameter and has that layer's geometry (v2_layers), every layer is launched in each
    direction, and no launch is uncovered (NOT_HERE is empty);
  * the activation operands are traced to their last writer (tests/_plan_trace.py, rules R1-R3): a weight gradient that reads a dY buffer set
    another Bottleneck has overwritten, or a saved activation a backward launch reused, fails even though its arithmetic is right;
  * the red test perturbs real stem results and requires the checker to fail;
  * the production schedule (two streams, the fused BatchNorm backward as the default selects it, same weights / image / dlogits) must give
    the serial replay's logits, gradients and BatchNorm running statistics bit for bit, which carries the per-launch evidence over to the
    schedule bench.py times.
The step-level launches outside TrunkPlan: the SimT head and the NTM gradients are held element by element on their own scale against the
float64 oracle (tests/_head_bar.py) by test_head_production_size_vs_oracle and, in the form the trainers launch it (bf16 gradient at the plan's
pitch, gscale, byte maps), by test_head_production_form_v2_simt / _v2_warmup; softmax and the optimisers by tests/test_gpu_bn_pool.py and
tests/test_gpu_optim.py.
"""
import time

import pytest
import torch

import _launch_oracle as lo
from _plan_layers import v2_layers
from _plan_replay import Run, _env, _perturb, _two_ulps, match_layers, replay
from _plan_trace import Tracer, check_rules
from oracle import simt_oracle as so
from simt_amd import model_spec as ms

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CD = so.load_class_dist()
B, H, W, K = 4, 768, 768, 3
Q = 19 + K

# tag -> the test that holds launches of that tag instead.  Empty: every entry point of the two plans has a handler.
NOT_HERE = {}


def _params(st, dev):
    return {k: v.detach().to(dev, torch.float32 if v.dtype != torch.long else torch.long).clone() for k, v in st.items()}


def _plans(st, fst, dev):
    from simt_amd.engine import TrunkPlan, multi_heads
    tr = TrunkPlan(_params(st, dev), B, H, W, multi_heads(19, K, True), dtype=BF, train=True)
    fr = TrunkPlan(_params(fst, dev), B, H, W, multi_heads(19, 0, False), dtype=BF, train=False, stem_from=tr)
    return tr, fr


def _seed_dlogits(plan):
    """As test_gpu_plan_launches._seed_and_backward seeds the DeepLab-v2-style heads: N(0, 1) / (h w) on the Q live columns, zero padding."""
    g = torch.Generator().manual_seed(8)
    for dl in plan.dlogits.values():
        hd = plan.heads[0]
        dl.zero_()
        dl[:, :Q] = (torch.randn(dl.shape[0], Q, generator=g) / (hd.h * hd.w)).to(BF).to(dl.device)


def _production_coverage(tr, fr):
    """The plan under test is the production one: a changed default must not quietly shrink what this file checks."""
    fns = [(lst, lo.fn_name(it), it) for lst in ("fwd", "bwd") for it in getattr(tr, lst + "_list").items if it.fn is not None]
    names = {n for (_l, n, _i) in fns}
    tags = {it.tag for (_l, _n, it) in fns}
    missing = [n for n in ("simt_stem7_fwd", "simt_stem7_wgrad", "simt_conv_wgrad_multi") if n not in names]
    assert not missing, f"production plan lacks {missing}"
    assert tr.fwd_list.items[0].tag == "simt_stem7_fwd" and tr.stem_desc.nsets == 2, "the direct stem launch must carry both networks"
    convs = [it.keep for (_l, n, it) in fns if n == "simt_conv_fprop"]
    assert any(d.in_scale for d in convs), "no conv with the operand-path BatchNorm (in_scale)"
    assert any(d.res_bits for d in convs), "no conv with a bit-mask residual (res_bits)"
    assert "conv1x1_rows_kernel" in tags, "no row-streaming 1x1 conv"
    assert any(t.startswith("conv_igemm2_kernel<256, 5, 3,") for t in tags), "no conv_igemm2_kernel<256, 5, 3, ...> tile"
    assert not any(lo.fn_name(it) in ("simt_stem7_fwd", "simt_im2col_stem") for it in fr.fwd_list.items)


def _red_hook(run):
    def hook(lname, it, chk, got):
        name = lo.fn_name(it)
        if "stem7_fwd" not in run.red and name == "simt_stem7_fwd":
            col = int(got["y0"][0].float().abs().argmax())              # row 0: pixel (b 0, 0, 0), its window leaves the image
            col1 = int(got["y1"][0].float().abs().argmax())
            border = 10                                                 # pixel (b 0, row 0, col 10): its top taps read outside the image
            cases = [("2 ulps", lambda g: _two_ulps(g["y0"], (0, col))),
                     ("channels swapped", lambda g: g["y0"].copy_(g["y0"][:, [1, 0] + list(range(2, 64))])),
                     ("border row zeroed", lambda g: g["y0"][border].zero_()),
                     ("stats slot 1e-3", lambda g: g["stats0"][3].mul_(1.0 + 1e-3)),
                     ("set 1: 2 ulps", lambda g: _two_ulps(g["y1"], (0, col1)))]
            run.red["stem7_fwd"] = (f"{it.tag} {it.shape}", [c[0] for c in cases], _perturb(chk, got, "stem7_fwd", cases))
        if "stem7_wgrad" not in run.red and name == "simt_stem7_wgrad":
            # the partials are perturbed and dw re-derived from them in the kernel's fixed order, so only the float64 bar can catch the case
            dw = got["dw"]
            o, c, r, s = (int(v) for v in torch.unravel_index(dw.abs().argmax().cpu(), dw.shape))
            v = float(dw[o, c, r, s])
            delta = 2.5 * float(lo.ulp_bf16(torch.tensor(abs(v), dtype=torch.float64), 1e-30)) * (1 if v >= 0 else -1)

            def redo(g):
                g["dw"].copy_(lo.stem7_wgrad_reduce_expect(g["part"]))

            def bump(g):
                g["part"][0, o, r, s * 3 + c] += delta
                redo(g)

            def swap(g):
                g["part"].copy_(g["part"][:, [1, 0] + list(range(2, 64))])
                redo(g)

            def edge(g):
                g["part"][:, 0, 0, :].zero_()                             # filter row 0 of channel 0: taps outside the image for the top rows
                redo(g)
            cases = [("2 ulps", bump), ("channels swapped", swap), ("edge-tap row zeroed", edge)]
            run.red["stem7_wgrad"] = (f"{it.tag} {it.shape}", [c_[0] for c_ in cases], _perturb(chk, got, "stem7_wgrad", cases))
    return hook


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def _snapshot(tr, fr):
    """What the tie compares: both networks' logits, the trainable flat gradient buffer, the BatchNorm running statistics."""
    out = {f"logits {n} {k}": pl.out[k].clone() for n, pl in (("trainable", tr), ("frozen", fr)) for k in pl.out}
    out["flat_grad"] = tr.flat_grad.clone()
    for k, v in tr.p.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out[k] = v.clone()
    return out


@pytest.fixture(scope="module")
def v2(dev):
    from simt_amd import engine as eng
    res = {}
    t0, f0 = time.time(), lo.GEMM_FLOPS[0]
    st = ms.trained_like_init(ms.state_shapes(19, K, True), seed=5)
    fst = ms.trained_like_init(ms.state_shapes(19, 0, False), seed=6)
    img, _ = ms.synthetic_batch(B, H, W, CD.numpy(), seed=7, device=dev)
    with pytest.MonkeyPatch.context() as mp:
        _env(mp)
        tr, fr = _plans(st, fst, dev)
        _production_coverage(tr, fr)
        run, run_f = Run(), Run()
        hook = _red_hook(run)
        fwd_starts = [(rec["fwd_start"], rec["name"]) for rec in tr.block_io]

        def block_of(lname, i):
            if lname == "v2.fwd":
                names = [n for (s, n) in fwd_starts if s <= i]
                return names[-1] if names else "stem"
            if lname == "v2.bwd":
                for n, (a, b, *_r) in tr.bwd_marks.items():
                    if a <= i < b:
                        return n
            return None
        trace = Tracer(block_of)
        tr.x_in.copy_(img)
        trace.write("test", 0, "image", tr.x_in.data_ptr(), tr.x_in.numel() * 4)
        replay(tr, [("v2.pack", tr.pack_list)], run, hook, others=(fr,), trace=trace, not_here=NOT_HERE)
        replay(fr, [("v2f.pack", fr.pack_list)], run_f, others=(tr,), trace=trace, not_here=NOT_HERE)
        replay(tr, [("v2.fwd", tr.fwd_list)], run, hook, others=(fr,), trace=trace, not_here=NOT_HERE)
        replay(fr, [("v2f.fwd", fr.fwd_list)], run_f, others=(tr,), trace=trace, not_here=NOT_HERE)
        _seed_dlogits(tr)
        for i, dl in enumerate(tr.dlogits.values()):
            trace.write("test", i, "dlogits", dl.data_ptr(), dl.numel() * dl.element_size())
        replay(tr, [("v2.bwd", tr.bwd_list)], run, hook, others=(fr,), trace=trace, not_here=NOT_HERE)
        torch.cuda.synchronize()
        # the stem launch's second weight set is the frozen network's conv1
        stem_f = [c for c in run.convs if c[0].endswith(" set 1")]
        run.convs = [c for c in run.convs if not c[0].endswith(" set 1")]
        run_f.convs += stem_f
        match_layers(tr, run, v2_layers(B, H, W, K), True)
        match_layers(fr, run_f, v2_layers(B, H, W, 0), False)
        # last-writer rules on the trainable plan
        grads = {tr.grads[n].data_ptr(): n for n in tr.grads if n.endswith(".weight")}
        marks = tr.bwd_marks
        window = {"conv1.weight": (marks["layer1.0"][1], len(tr.bwd_list.items))}
        for rec in tr.block_io:
            for c in ("conv1", "conv2", "conv3") + (("downsample.0",) if rec["down"] else ()):
                window[f"{rec['name']}.{c}.weight"] = marks[rec["name"]][:2]
        for hd in tr.heads:
            li = hd.feat_layer
            lo_i = marks[f"layer{li + 1}.0"][1] if li < 4 else 0
            hi_i = marks[f"layer{li}.{tr.layers[li - 1] - 1}"][0]
            for prefix, _c in hd.groups:
                for i in range(len(hd.dilations)):
                    window[f"{prefix}.conv2d_list.{i}.weight"] = (lo_i, hi_i)
        res["rules"] = check_rules(trace, grads, window, fwd="v2.fwd", bwd="v2.bwd", x_from_test={"conv1.weight"})
        res["traced"] = len(trace.launches)
        res["serial"] = _snapshot(tr, fr)
        res["serial_secs"] = time.time() - t0
        res["tflop"] = (lo.GEMM_FLOPS[0] - f0) / 1e12
        del tr, fr, trace
        torch.cuda.empty_cache()
    # ---- the production schedule: default environment (two streams, fused BatchNorm backward), same weights / image / dlogits
    t1 = time.time()
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("SIMT_SINGLE_STREAM", raising=False)
        mp.delenv("SIMT_BN_GRID", raising=False)
        eng._SIDE_STREAMS.clear()
        tr, fr = _plans(st, fst, dev)
        res["fbn_launches"] = tr.fbn_launches
        tr.forward(img)
        fr.forward()
        _seed_dlogits(tr)
        tr.backward()
        torch.cuda.synchronize()
        res["fbn_error"] = tr.fbn_error()
        res["prod"] = _snapshot(tr, fr)
        del tr, fr
        torch.cuda.empty_cache()
    eng._SIDE_STREAMS.clear()
    res["prod_secs"] = time.time() - t1
    res["run"], res["run_f"] = run, run_f
    return res


def test_v2_plan_launches_hold_float64_b4_768(v2):
    """Every launch of the trainable (pack, forward, backward) and frozen (pack, forward) DeepLab-v2 plans within its float64 bar; no launch
    uncovered; every conv launch has its layer's geometry and every layer is launched in each direction."""
    run, run_f = v2["run"], v2["run_f"]
    worst = dict(run.worst)
    for k, v in run_f.worst.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(f"\nv2: {run.n + run_f.n} launches checked in {v2['serial_secs']:.1f} s wall (plans built, replayed and checked; {v2['tflop']:.2f} TFLOP "
          f"of float64 GEMM in the oracle); {len(worst)} distinct (tag, shape), worst error / bound:")
    for (tag, shape), r in sorted(worst.items()):
        print(f"  {r:6.3f}  {tag}  {shape}")
    fails = run.fail + run_f.fail
    assert not fails, f"v2: {len(fails)} launch(es) outside their float64 bar:\n  " + "\n  ".join(fails[:40])
    unc = run.uncovered + run_f.uncovered
    assert not unc, f"v2: {len(unc)} launch(es) neither checked by a handler nor listed in NOT_HERE:\n  " + "\n  ".join(unc[:40])
    bad = run.layer_bad + run_f.layer_bad
    assert not bad, f"v2: {len(bad)} conv launch(es) not matching their layer:\n  " + "\n  ".join(bad[:20])
    for what, r in (("trainable", run), ("frozen", run_f)):
        assert not r.layer_missing, f"v2 {what} plan: layers never launched {r.layer_missing[:6]}"
    assert ("conv1", "fwd") in run.layer_seen and ("conv1", "fwd") in run_f.layer_seen
    assert all(r <= 1.0 for r in worst.values())


def test_v2_operands_have_the_right_last_writer(v2):
    """R1-R3 of tests/_plan_trace.py on the trainable plan's replay: no activation operand read from memory nobody wrote; every weight
    gradient's dY written inside its own Bottleneck's backward range (the stem: after layer1.0's) and its x by the forward list; the saved
    activations of every BatchNorm backward and fused reduce written by the forward list, their dz by the backward list."""
    print(f"\nv2 trace: {v2['traced']} launches traced, {len(v2['rules'])} rule violation(s)")
    assert not v2["rules"], f"{len(v2['rules'])} operand(s) with the wrong last writer:\n  " + "\n  ".join(v2["rules"][:40])


def test_v2_oracle_is_red_on_perturbed_stem_results(v2):
    """The checker must fail on copies of the real stem results with one element moved by 2 bf16 ulps, two output channels swapped, a border
    row zeroed and one statistics slot off by 1e-3 (forward, both weight sets), and on the weight gradient's partials moved the same ways."""
    red = v2["run"].red
    assert set(red) == {"stem7_fwd", "stem7_wgrad"}, f"red cases found: {sorted(red)}"
    for what, (launch, cases, caught) in red.items():
        print(f"{what}: {launch}: caught {caught}")
        assert caught == cases, f"{what} ({launch}): the checker missed {sorted(set(cases) - set(caught))}"


def test_v2_production_schedule_matches_the_replay_bitwise(v2):
    """The default schedule (two streams, fused BatchNorm backward) against the serial two-pass replay: both networks' logits, every
    gradient and the BatchNorm running statistics bit for bit."""
    print(f"\nv2 production schedule: {v2['fbn_launches']} fused BatchNorm launches, {v2['prod_secs']:.1f} s wall")
    assert not v2["fbn_error"], "a fused BatchNorm launch timed out waiting for co-residency (another process held CUs)"
    assert v2["fbn_launches"] > 0, "the default plan has no fused BatchNorm launch: the tie would not cover it"
    s, p = v2["serial"], v2["prod"]
    assert set(s) == set(p)
    diff = []
    for k in s:
        ne = int((_bits(s[k]) != _bits(p[k])).sum())
        if ne:
            diff.append(f"{k}: {ne} of {s[k].numel()} elements differ")
    assert not diff, "production schedule differs from the serial replay:\n  " + "\n  ".join(diff[:20])
