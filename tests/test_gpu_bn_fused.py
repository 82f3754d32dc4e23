"""Train-mode BatchNorm fused into the producing conv launch behind a grid-wide barrier (round 4; include/simt_hip.h simt_fbn_desc,
csrc/conv2_epilogue.h) -- replaces conv -> simt_bn_finalize -> simt_bn_apply (forward) and dgrad -> simt_bn_bwd (backward) for bn1 / bn2
of the Bottlenecks whose conv grid is one co-resident round of the chip (model/deeplab_multi.py:62-70,81-91).

The fused launch reduces the SAME per-tile slots in the SAME order with the same expressions as the separate kernels, so everything is
compared BIT FOR BIT against the unfused path, at the production shapes (M = 4 x 97 x 97 = 37 636, BASELINE configs[1]):
  * per launch, both directions, 3x3 256 -> 256 (dilation 2) and 1x1 1024 -> 256: y, a = relu(bn(y)), mean / rstd / scale / shift, the
    running statistics; dy and the coefficients of the backward;
  * the whole plan (B=4, 768x768, bf16, 33 Bottlenecks): forward logits, saved activations and the flat gradient buffer with
    SIMT_BN_GRID=1 vs 0, the fused instantiation asserted by launch tag;
  * a two-stream soak: full SimT iterations (frozen forward + weight gradients on the side stream beside the waiting launches), no hang,
    trajectory identical to the unfused build's.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.engine import BN_EPS, BN_MOMENTUM, TrunkPlan, multi_heads

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B4, HW = 4, 97
CD = so.load_class_dist()


def _fbn(mode, out, bar, **kw):
    fd = L.FbnDesc()
    fd.mode, fd.ldo, fd.out, fd.work = mode, out.shape[-1], out.data_ptr(), bar.data_ptr()
    for k, v in kw.items():
        setattr(fd, k, v.data_ptr() if torch.is_tensor(v) else v)
    return fd


@pytest.mark.parametrize("shape", [(256, 256, 3, 2), (1024, 256, 1, 1), (256, 256, 3, 1)], ids=["3x3_d2_256", "1x1_1024_256", "3x3_d1_256"])
def test_fused_bn_forward_and_backward_launch_bitwise(dev, shape):
    Cin, Cout, k, dil = shape
    B, H, W = B4, HW, HW
    M = B * H * W
    g = torch.Generator().manual_seed(Cin + 7 * k + dil)
    x = torch.randn(B, H, W, Cin, generator=g).to(dev, BF)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (1.0 / (Cin * k * k)) ** 0.5).to(dev)
    taps = ops.conv_taps(k, k, dil, dil * (k // 2))
    wp = torch.zeros(Cout, len(taps) * Cin, device=dev, dtype=BF)
    ops.pack_weight(w.contiguous(), wp, Cout=Cout, Cin=Cin, RS=k * k, ldk=len(taps) * Cin, mode=0)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.3).to(dev)
    nblk = (M + 127) // 128

    def run(fused, rounds=3):
        y = torch.full((M, Cout), float("nan"), device=dev, dtype=BF)
        a = torch.full((M, Cout), float("nan"), device=dev, dtype=BF)
        part = torch.full((nblk, 2, Cout), float("nan"), device=dev)
        cst = {n: torch.full((Cout,), float("nan"), device=dev) for n in ("mean", "rstd", "scale", "shift")}
        rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
        d = ops.make_conv_desc(x, wp, y, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, Npad=Cout, tile_n=256, stats=part)
        assert L.load().simt_conv_fbn_ok(C.byref(d)) == 1
        bar = torch.zeros(L.load().simt_conv_fbn_words(C.byref(d)), device=dev, dtype=torch.int64)
        if fused:
            fd = _fbn(1, a, bar, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, momentum=BN_MOMENTUM, eps=BN_EPS, **cst)
            d.fbn = C.addressof(fd)
        for _ in range(rounds):                      # the counters only grow: a launch must find its generation every time
            ops.conv_fprop_desc(d)
            if not fused:
                ops.bn_finalize(part, nblk, Cout, M, gamma, beta, rm, rv, BN_MOMENTUM, BN_EPS, cst["mean"], cst["rstd"], cst["scale"], cst["shift"])
                ops.bn_apply(y, cst["scale"], cst["shift"], a, M=M, Cn=Cout, relu=True)
        torch.cuda.synchronize()
        return dict(y=y, a=a, rm=rm, rv=rv, **cst), int(bar[:128:16].sum().item())
    ref, _ = run(False)
    got, tickets = run(True)
    assert tickets == 3 * L.load().simt_conv_mtiles(C.byref(ops.make_conv_desc(x, wp, ref["y"], B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout,
                                                                                taps=taps, Npad=Cout, tile_n=256)))   # one ticket per workgroup and launch
    for n in ref:
        assert torch.isfinite(got[n].float()).all(), n
        assert torch.equal(got[n], ref[n]), f"forward {n}: fused launch differs from conv + finalize + apply"
    assert (got["a"] > 0).float().mean().item() > 0.2
    # ---- backward: this conv as the dgrad that produces dz of a BatchNorm-ed activation y (saved), mask = y * scale + shift > 0
    ysave = torch.randn(M, Cout, generator=g).to(dev, BF)
    cst = {n: ref[n] for n in ("mean", "rstd", "scale", "shift")}

    def run_bwd(fused, rounds=2):
        dz = torch.full((M, Cout), float("nan"), device=dev, dtype=BF)
        dy = torch.full((M, Cout), float("nan"), device=dev, dtype=BF)
        part = torch.full((nblk + 8, 3, Cout), float("nan"), device=dev)
        coef = torch.full((3, Cout), float("nan"), device=dev)
        bnr = {"y": ysave, "mode": 2, "part": part, **cst}
        d = ops.make_conv_desc(x, wp, dz, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, Npad=Cout, tile_n=256, bnr=bnr)
        bar = torch.zeros(L.load().simt_conv_fbn_words(C.byref(d)), device=dev, dtype=torch.int64)
        if fused:
            fd = _fbn(2, dy, bar, coef=coef)
            d.fbn = C.addressof(fd)
        for _ in range(rounds):
            ops.conv_fprop_desc(d)
            if not fused:
                bd = ops.make_bn_bwd_desc(dz=dz, y=ysave, part=part, coef=coef, dy=dy, M=M, Cn=Cout, mask_mode=2,
                                          reduce_done_nblk=L.load().simt_conv_mtiles(C.byref(d)), **cst)
                L.call("simt_bn_bwd", C.byref(bd), ops.stream_ptr())
        torch.cuda.synchronize()
        return dy, coef, dz
    dy_r, coef_r, _ = run_bwd(False)
    dy_f, coef_f, dz_f = run_bwd(True)
    assert torch.isfinite(dy_f.float()).all() and torch.equal(dy_f, dy_r), "backward dy: fused launch differs from dgrad + simt_bn_bwd"
    assert torch.equal(coef_f, coef_r)
    assert torch.isnan(dz_f.float()).all()                              # the raw dz is never written by the fused launch


def _plan(dev, st, fused, **kw):
    os.environ["SIMT_BN_GRID"] = "1" if fused else "0"
    try:
        p = {k: v.clone().to(dev) for k, v in st.items()}
        return TrunkPlan(p, B4, 768, 768, multi_heads(19, 3, True), dtype=BF, train=True, **kw)
    finally:
        os.environ.pop("SIMT_BN_GRID")


def test_fused_bn_whole_plan_bitwise_b4_768(dev):
    """BASELINE configs[1]'s trainable net: forward + backward with the fused launches == without, bit for bit."""
    st = so.recipe_state(so.state_shapes(19, 3, True), seed=1234, head_scale=8.0)
    img, _ = so.synthetic_batch(B4, 768, 768, CD.numpy(), seed=1234)
    res = []
    for fused in (True, False):
        tr = _plan(dev, st, fused)
        ftags = [it.tag for it in tr.fwd_list.items if it.tag and it.tag.startswith("conv_igemm2_kernel<256, 5, 3, 1,")]
        btags = [it.tag for it in tr.bwd_list.items if it.tag and it.tag.startswith("conv_igemm2_kernel<256, 5, 3, 1,")]
        napply = sum(1 for it in tr.fwd_list.items if it.tag == "simt_bn_apply" or it.fn is L.load().simt_bn_apply)
        # no launch of the production plan runs the generic (run-time-flag, spilling) epilogue of the 2-slot short-K conv: tests/test_host_logic.py
        # test_no_scratch_in_production_kernels exempts exactly those two instantiations
        import re
        assert not [it.tag for lst in (tr.fwd_list, tr.bwd_list) for it in lst.items if it.tag and re.match(r"conv_igemm2_kernel<128, \d, 2, 0, 0>", it.tag)]
        if fused:
            assert len(ftags) == 46 and len(btags) == 46, (len(ftags), len(btags))      # bn1 + bn2 of layer3's 23 Bottlenecks, both directions
        else:
            assert not ftags and not btags
        out = tr.forward(img.to(dev))
        g = torch.Generator().manual_seed(3)
        for name in sorted(tr.dlogits):                 # a seeded upstream gradient of the heads' logits (live columns only)
            t = tr.dlogits[name]
            t.zero_()
            t[:, :22].copy_((torch.randn(t.shape[0], 22, generator=g) * 1e-3).to(dev))
        tr.backward()
        torch.cuda.synchronize()
        rec = tr.block_io[10]
        res.append(dict(x1=out["x1"].clone(), x2=out["x2"].clone(), a1=rec["a1"].clone(), a2=rec["a2"].clone(), y2=rec["y2"].clone(),
                        flat=tr.flat_grad.clone(), rm=tr.p["layer3.5.bn2.running_mean"].clone(), napply=napply))
        del tr
        torch.cuda.empty_cache()
    a, b = res
    # 46 applies ride in the fused launches; in the unfused plan layer 3's 23 bn2 applies run in conv3's operand path instead (round 6), and in
    # BOTH plans so do bn2 of layers 1-2 (their conv2 launches are more than one round: never fused)
    assert a["napply"] == b["napply"] - 23
    for k in ("x1", "x2", "a1", "a2", "y2", "flat", "rm"):
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), f"{k}: plan with fused BatchNorm launches differs from the plan without"
    assert a["flat"].abs().max().item() > 0


def test_fused_bn_two_stream_soak(dev):
    """60 full SimT iterations at the production size with the waiting launches on the main stream and the frozen forward / weight
    gradients beside them on the side stream: completes (the kernel traps after ~2 s of waiting instead of hanging), and the
    trajectory equals the unfused build's bit for bit (losses of the last step and a parameter checksum)."""
    from simt_amd import model_spec as ms
    from simt_amd.step import Hyper, SimTTrainer
    K = 3
    st = ms.trained_like_init(ms.state_shapes(19, K, True), seed=1234)
    fst = ms.trained_like_init(ms.state_shapes(19, 0, False), seed=1234)
    img, lab = ms.synthetic_batch(B4, 768, 768, CD.numpy(), seed=5, device=dev)
    outs = []
    for fused, steps in ((True, 60), (False, 60)):
        os.environ["SIMT_BN_GRID"] = "1" if fused else "0"
        try:
            tr = SimTTrainer(st, fst, ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), Hyper(open_classes=K, lr=2.5e-4, lr_T=6e-3), CD.numpy(),
                             B4, 768, 768, dtype=BF, device=dev)
        finally:
            os.environ.pop("SIMT_BN_GRID")
        assert tr.plan._fbn_on == fused
        for it in range(steps):
            tr.step(img, lab, it)
        torch.cuda.synchronize()
        outs.append((tr.lout.clone(), tr.params["layer3.7.conv2.weight"].clone(), tr.params["layer5.conv2d_list.0.weight"].clone()))
        del tr
        torch.cuda.empty_cache()
    for x, y in zip(*outs):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_fused_bn_both_directions_matches_default_trajectory(dev):
    """The production step with fused BatchNorm in both directions (SIMT_BN_GRID=1) gives the default's (3: backward only) trajectory bit for
    bit over five iterations."""
    from simt_amd import model_spec as ms
    from simt_amd.step import Hyper, SimTTrainer
    K = 3
    st = ms.trained_like_init(ms.state_shapes(19, K, True), seed=1234)
    fst = ms.trained_like_init(ms.state_shapes(19, 0, False), seed=1234)
    img, lab = ms.synthetic_batch(B4, 768, 768, CD.numpy(), seed=5, device=dev)
    outs = []
    for env in ({}, {"SIMT_BN_GRID": "1"}):
        os.environ.update(env)
        try:
            tr = SimTTrainer(st, fst, ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), Hyper(open_classes=K, lr=2.5e-4, lr_T=6e-3), CD.numpy(),
                             B4, 768, 768, dtype=BF, device=dev)
        finally:
            for k in env:
                os.environ.pop(k)
        assert tr.plan._fbn_dirs == ((1, 2) if env.get("SIMT_BN_GRID") == "1" else (2,))
        for it in range(5):
            tr.step(img, lab, it)
        torch.cuda.synchronize()
        outs.append((tr.lout.clone(), tr.params["layer3.7.conv2.weight"].clone()))
        del tr
        torch.cuda.empty_cache()
    for o in outs[1:]:
        assert torch.isfinite(o[0]).all() and torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_fused_bn_backward_v3_plan_bitwise_b4_512x1024(dev):
    """BASELINE configs[3] (model/deeplabv3.py, B = 4, 512 x 1024): on the stride-8 / stride-16 maps a dgrad launch is one co-resident round of
    the chip with the 128- / 64-column tiles too, so bn2's and bn1's backward (trainable affine: d gamma / d beta come from the owner
    workgroups) ride in the conv3 / conv2 dgrad launches.  Same logits, same flat gradient (every conv weight, every BatchNorm weight and
    bias) as the plan without fused launches, bit for bit."""
    import re
    from simt_amd.engine_v3 import V3Plan, v3_state_shapes
    from test_gpu_v3 import make_state              # (tests/ is on sys.path under pytest: rootdir conftest)
    st = make_state(v3_state_shapes(19, 6, True), 11)
    g = torch.Generator().manual_seed(12)
    img = torch.randn(B4, 3, 512, 1024, generator=g)
    res = []
    for grid in ("3", "0"):
        os.environ["SIMT_BN_GRID"] = grid
        try:
            plan = V3Plan({k: v.clone().to(dev) for k, v in st.items()}, B4, 512, 1024, 19, 6, True, dtype=BF, train=True)
        finally:
            os.environ.pop("SIMT_BN_GRID")
        ftags = [it.tag for it in plan.bwd_list.items if it.tag and re.match(r"conv_igemm2_kernel<\d+, \d, 3, 1, 2>", it.tag)]
        nbwd = sum(1 for it in plan.bwd_list.items if it.fn is L.load().simt_bn_bwd)
        if grid == "3":
            # layer2 (4 Bottlenecks, 128 x 256 maps, 128-column tiles) and layer3 (6, 64 x 128 maps after the stride, 64-column tiles): bn2 and bn1 each,
            # except where the launch is more than one round of the chip (layer1; the stride-2 block's conv2 dgrad runs on its input map)
            assert len(ftags) >= 16, ftags
            assert {t.split("<")[1].split(",")[0] for t in ftags} >= {"64"}, ftags
        else:
            assert not ftags
        out = plan.forward(img.to(dev))
        up = (torch.randn(B4, 25, 32, 64, generator=torch.Generator().manual_seed(13)) * 1e-3).to(dev)
        plan.backward(torch.nn.functional.interpolate(up, size=(512, 1024), mode="bilinear"))
        torch.cuda.synchronize()
        res.append(dict(out=out.clone(), flat=plan.flat_grad.clone(), nf=len(ftags), nbwd=nbwd))
        del plan
        torch.cuda.empty_cache()
    a, b = res
    assert a["nbwd"] == b["nbwd"] - a["nf"]
    assert torch.isfinite(a["flat"]).all() and a["flat"].abs().max().item() > 0
    assert torch.equal(a["out"], b["out"])
    assert torch.equal(a["flat"], b["flat"]), "v3 plan with the BatchNorm backward fused into the dgrad launches differs from the plan without"


# ----------------------------------------------------------------------------------------------------------------------
# Round 5 (ADVICE r4 high / VERDICT r4 #5a): a fused launch whose polling cannot complete no longer traps the process.  The poller that times
# out (~2 s) sets the sticky error word, every other poller of the launch leaves at its next check, the launch ENDS; the host reads the word
# (TrunkPlan.fbn_error, the trainers' losses() raise) and the optimiser kernel given the word as `skip_if` leaves the weights untouched.
# ----------------------------------------------------------------------------------------------------------------------
def test_fused_bn_polling_timeout_sets_error_word_and_launch_ends(dev):
    import time
    Cin, Cout, k, dil = 256, 256, 3, 2
    B, H, W = B4, HW, HW
    M = B * H * W
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, Cin, generator=g).to(dev, BF)
    taps = ops.conv_taps(k, k, dil, dil)
    wp = (torch.randn(Cout, len(taps) * Cin, generator=g) * 0.02).to(dev, BF)
    y, a = torch.empty(M, Cout, device=dev, dtype=BF), torch.empty(M, Cout, device=dev, dtype=BF)
    part = torch.zeros((M + 127) // 128, 2, Cout, device=dev)
    cst = {n: torch.zeros(Cout, device=dev) for n in ("mean", "rstd", "scale", "shift")}
    d = ops.make_conv_desc(x, wp, y, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, Npad=Cout, tile_n=256, stats=part)
    bar = torch.zeros(L.load().simt_conv_fbn_words(C.byref(d)), device=dev, dtype=torch.int64)
    fd = _fbn(1, a, bar, momentum=BN_MOMENTUM, eps=BN_EPS, **cst)
    d.fbn = C.addressof(fd)
    ops.conv_fprop_desc(d)                          # a healthy launch first: the word stays clear
    torch.cuda.synchronize()
    assert int(bar[L.FBN_ERR_WORD].item()) == 0
    # Break the protocol the way a starved launch looks from inside: the workgroups of ONE ticket shard (blockIdx % 8 == 0) draw tickets of a
    # different generation, so their granules never carry the tag the owners wait for -- exactly "some workgroups never arrived".
    bar[0] += 1000
    # round 6: a launch that gave up writes NOTHING derived from its incomplete reads: the statistics the healthy launch left
    # (mean / rstd / scale / shift and the running statistics it updates in place) and the rows of `out` of every workgroup whose poll gave up
    rm, rv = torch.full((Cout,), 0.25, device=dev), torch.full((Cout,), 1.5, device=dev)
    fd_r = _fbn(1, a, bar, momentum=BN_MOMENTUM, eps=BN_EPS, running_mean=rm, running_var=rv, **cst)
    d.fbn = C.addressof(fd_r)
    good = {n: v.clone() for n, v in cst.items()}
    a.fill_(-7.0)
    t0 = time.perf_counter()
    ops.conv_fprop_desc(d)
    torch.cuda.synchronize()                        # returns: the launch ended by itself (the old kernel executed s_trap here)
    dt = time.perf_counter() - t0
    assert int(bar[L.FBN_ERR_WORD].item()) == 1, "the poller that timed out must set the error word"
    assert 1.0 < dt < 20.0, f"the launch should end within a poll period of the ~2 s timeout, took {dt:.1f} s"
    for n in cst:
        assert torch.equal(cst[n], good[n]), f"{n} was rewritten by a launch whose owners' polls gave up"
    assert bool((rm == 0.25).all()) and bool((rv == 1.5).all()), "running statistics updated from partial sums"
    assert bool((a.float() == -7.0).all()), "`out` written although no workgroup saw this launch's constants"
    d.fbn = C.addressof(fd)
    # the word is sticky and shared: a later launch that polls in vain leaves at its first check instead of waiting 2 s again
    t0 = time.perf_counter()
    ops.conv_fprop_desc(d)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 1.0 and int(bar[L.FBN_ERR_WORD].item()) == 1
    # a caller-owned word (simt_fbn_desc.err) instead of work[SIMT_FBN_ERR_WORD]
    err = torch.zeros(1, device=dev, dtype=torch.int64)
    bar2 = torch.zeros_like(bar)
    bar2[0] += 1000
    fd2 = _fbn(1, a, bar2, momentum=BN_MOMENTUM, eps=BN_EPS, err=err, **cst)
    d.fbn = C.addressof(fd2)
    ops.conv_fprop_desc(d)
    torch.cuda.synchronize()
    assert int(err.item()) == 1 and int(bar2[L.FBN_ERR_WORD].item()) == 0


def test_fbn_error_word_makes_losses_raise_and_sgd_skip(dev):
    from simt_amd import model_spec as ms
    from simt_amd.step import Hyper, SimTTrainer
    lay = (1, 1, 2, 1)
    st = ms.reference_init(ms.state_shapes(19, 3, True, layers=lay), seed=3)
    fst = ms.reference_init(ms.state_shapes(19, 0, False, layers=lay), seed=3)
    cd = ms.load_class_dist("bapa")
    os.environ["SIMT_BN_GRID"] = "3"
    try:
        tr = SimTTrainer(st, fst, ms.ntm_init(19, 3, 1), ms.ntm_init(19, 3, 2), Hyper(open_classes=3), cd, 4, 768, 768, dtype=BF, device=dev, layers=lay)
    finally:
        os.environ.pop("SIMT_BN_GRID")
    assert tr.plan._fbn_on and tr.plan.fbn_launches > 0 and tr.plan.fbn_err is not None and tr.sgd_desc.skip_if == tr.plan.fbn_err.data_ptr()
    img, lab = ms.synthetic_batch(4, 768, 768, cd, seed=1, device=dev)
    tr.step(img, lab, 0)
    tr.losses()                                     # healthy: no error
    assert not tr.plan.fbn_error()
    n = "layer4.0.conv2.weight"
    w0 = tr.params[n].clone()
    assert tr.inner_desc.skip_if == tr.plan.fbn_err.data_ptr()
    snap = lambda: [t.clone() for k in range(2) for t in (tr.ntm[k], tr.ntm_m[k], tr.ntm_v[k], tr.wraw[k], tr.w_m[k], tr.w_v[k])]
    s0 = snap()
    tr.plan.fbn_err.fill_(1)                        # what a timed-out fused launch leaves behind
    tr.step(img, lab, 1)
    torch.cuda.synchronize()
    assert torch.equal(tr.params[n], w0), "the optimiser must not apply gradients of a step whose fused BatchNorm bailed out"
    # round 6: neither do the two Adam steps on NTM1 / NTM2 nor the W inner loop (parameters AND moments): a state_dict
    # saved after losses() raised holds the last good state
    for t0_, t1_ in zip(s0, snap()):
        assert torch.equal(t0_, t1_), "NTM / W / an Adam moment moved while the fused-BatchNorm error word was set"
    with pytest.raises(RuntimeError, match="SIMT_BN_GRID=0"):
        tr.losses()
    tr.plan.fbn_err.zero_()
    tr.step(img, lab, 2)
    torch.cuda.synchronize()
    assert not torch.equal(tr.params[n], w0)


def test_data_parallel_plans_keep_the_fused_batchnorm_and_can_switch_it_off(dev):
    """Round 6: with 236-workgroup launches (160-row tiles) a data-parallel plan keeps the fused BatchNorm backward (engine.TrunkPlan: the
    collective's kernels get the 20 CUs the tile plan leaves free; no circular wait is possible); SIMT_BN_GRID=0 is the documented switch
    (bench.py forces it when several ranks share one GPU)."""
    st = so.recipe_state(so.state_shapes(19, 3, True, layers=(1, 1, 2, 1)), seed=1, head_scale=8.0)
    p = lambda: {k: v.clone().to(dev) for k, v in st.items()}
    kw = dict(dtype=BF, train=True, layers=(1, 1, 2, 1))
    assert os.environ.get("SIMT_BN_GRID") is None
    solo = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), **kw)
    dp = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), data_parallel=True, **kw)
    assert solo._fbn_on and solo._fbn_dirs == (2,) and solo.fbn_launches > 0
    assert dp._fbn_on and dp._fbn_dirs == (2,) and dp.fbn_launches == solo.fbn_launches and dp.fbn_err is not None and dp.cu_budget == 240
    os.environ["SIMT_BN_GRID"] = "0"
    try:
        dp_off = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), data_parallel=True, **kw)
    finally:
        os.environ.pop("SIMT_BN_GRID")
    assert not dp_off._fbn_on and dp_off.fbn_launches == 0 and dp_off.fbn_err is None


# ----------------------------------------------------------------------------------------------------------------------
# Round 6 (VERDICT r5 #1a): bn2's normalise + ReLU applied in conv3's OPERAND path (conv1x1_rows_kernel FL_STATS_INBN; simt_conv_desc.in_*):
# the store waves rewrite every landed stage in LDS one period before the compute waves multiply it and write the activation out on the way.
# Bitwise the two-pass result: simt_bn_apply -> conv with statistics (model/deeplab_multi.py:88-92).
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 1024, B4, HW, HW), (128, 512, B4, HW, HW), (64, 256, B4, 193, 193), (256, 1024, 1, 9, 13)],
                         ids=["layer3_256_1024", "layer2_128_512", "layer1_64_256", "tiny_ragged"])
def test_operand_path_batchnorm_is_bitwise_the_two_pass(dev, shape):
    Cin, Cout, B, H, W = shape
    M = B * H * W
    g = torch.Generator().manual_seed(Cin + M)
    y2 = (torch.randn(B, H, W, Cin, generator=g) * 1.5).to(dev, BF)
    wp = (torch.randn(Cout, Cin, generator=g) * (1.0 / Cin) ** 0.5).to(dev, BF)
    scale = (torch.rand(Cin, generator=g) + 0.5).to(dev)
    shift = (torch.randn(Cin, generator=g) * 0.4).to(dev)
    nblk = (M + 127) // 128

    def conv(x, inbn):
        y = torch.full((M, Cout), float("nan"), device=dev, dtype=BF)
        part = torch.full((nblk, 2, Cout), float("nan"), device=dev)
        d = ops.make_conv_desc(x, wp, y, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=[(0, 0)], Npad=Cout, tile_n=256, stats=part)
        bn, tm, nst = C.c_int(), C.c_int(), C.c_int()
        assert L.load().simt_conv_variant(C.byref(d), C.byref(bn), C.byref(tm), C.byref(nst)) == 5, "not the row-streaming kernel"
        a = None
        if inbn:
            assert L.load().simt_conv_inbn_ok(C.byref(d)) == 1
            a = torch.full((M, Cin), float("nan"), device=dev, dtype=BF)
            d.in_scale, d.in_shift, d.in_out = scale.data_ptr(), shift.data_ptr(), a.data_ptr()
        for _ in range(2):                          # twice: a persistent kernel must leave nothing behind
            ops.conv_fprop_desc(d)
        torch.cuda.synchronize()
        return y, part, a
    a_ref = torch.empty(M, Cin, device=dev, dtype=BF)
    ops.bn_apply(y2.view(M, Cin), scale, shift, a_ref, M=M, Cn=Cin, relu=True)
    y_ref, p_ref, _ = conv(a_ref.view(B, H, W, Cin), False)
    y, p, a = conv(y2, True)
    assert torch.equal(a, a_ref), f"activation written by the operand path differs from simt_bn_apply: {(a.float() - a_ref.float()).abs().max().item()}"
    assert torch.equal(y, y_ref), f"conv output differs: {(y.float() - y_ref.float()).abs().max().item()}"
    assert torch.equal(p, p_ref), "BatchNorm statistics differ"
    assert float(a.float().min()) == 0.0 and float((a == 0).float().mean()) > 0.2          # the ReLU is live


def test_operand_path_batchnorm_rejected_where_no_kernel_takes_it(dev):
    """in_scale on a launch that is not the row-streaming statistics flavour: refused (SIMT_ERR_INVALID), never silently ignored."""
    B, H, W, Cin, Cout = 1, 9, 13, 256, 256
    x = torch.zeros(B, H, W, Cin, device=dev, dtype=BF)
    taps = ops.conv_taps(3, 3, 2, 2)
    wp = torch.zeros(Cout, len(taps) * Cin, device=dev, dtype=BF)
    y = torch.zeros(B * H * W, Cout, device=dev, dtype=BF)
    part = torch.zeros(1, 2, Cout, device=dev)
    sc = torch.ones(Cin, device=dev)
    d = ops.make_conv_desc(x, wp, y, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, Npad=Cout, tile_n=256, stats=part)
    assert L.load().simt_conv_inbn_ok(C.byref(d)) == 0
    d.in_scale, d.in_shift, d.in_out = sc.data_ptr(), sc.data_ptr(), x.data_ptr()
    assert L.load().simt_conv_fprop(C.byref(d), ops.stream_ptr()) != 0


def test_operand_path_batchnorm_plan_bitwise_b4_768(dev, monkeypatch):
    """The production training plan (B=4, 768 x 768, bf16, full depth) with bn2 in conv3's operand path (default) against the plan with the
    separate simt_bn_apply launches (SIMT_NO_INBN=1): 30 of 33 Bottlenecks take it (layer 4's Cin = 512 tile has a 3-slot ring), 30 launches
    fewer in the forward list; logits of both heads and EVERY gradient bit-identical."""
    st = so.recipe_state(so.state_shapes(19, 3, True), seed=1234, head_scale=8.0)
    img, _ = so.synthetic_batch(B4, 768, 768, CD.numpy(), seed=77)
    res = []
    for off in ("0", "1"):
        monkeypatch.setenv("SIMT_NO_INBN", off)
        plan = TrunkPlan({k: v.clone().to(dev) for k, v in st.items()}, B4, 768, 768, multi_heads(19, 3, True), dtype=BF, train=True)
        n_in = sum(1 for r in plan.block_io if r.get("inbn"))
        n_apply = sum(1 for it in plan.fwd_list.items if it.tag == "simt_bn_apply")
        out = plan.forward(img.to(dev))
        gsd = torch.Generator().manual_seed(3)
        for nm in sorted(plan.dlogits):                # a seeded upstream gradient of the heads' logits (live columns only)
            t = plan.dlogits[nm]
            t.zero_()
            t[:, :22].copy_((torch.randn(t.shape[0], 22, generator=gsd) * 1e-3).to(dev))
        plan.backward()
        torch.cuda.synchronize()
        rec = plan.block_io[10]
        res.append(dict(x1=out["x1"].clone(), x2=out["x2"].clone(), flat=plan.flat_grad.clone(), n_in=n_in, n_apply=n_apply,
                        a2=rec["a2"].clone(), rm=plan.p["layer3.5.bn3.running_mean"].clone()))
        del plan
        torch.cuda.empty_cache()
    a, b = res
    assert a["n_in"] == 30 and b["n_in"] == 0 and b["n_apply"] - a["n_apply"] == 30, (a["n_in"], a["n_apply"], b["n_apply"])
    assert torch.isfinite(a["flat"]).all() and a["flat"].abs().max().item() > 0
    assert torch.equal(a["a2"], b["a2"]) and torch.equal(a["x1"], b["x1"]) and torch.equal(a["x2"], b["x2"]) and torch.equal(a["rm"], b["rm"])
    assert torch.equal(a["flat"], b["flat"]), "gradients differ between the operand-path BatchNorm plan and the two-pass plan"


def test_operand_path_batchnorm_v3_plan_bitwise_b4_512x1024(dev, monkeypatch):
    """BASELINE configs[3] (model/deeplabv3.py, B = 4, 512 x 1024; trainable BatchNorm affine): bn2 in conv3's operand path where the
    row-streaming kernel takes conv3, against the plan with the separate simt_bn_apply launches (SIMT_NO_INBN=1): same logits, same flat
    gradient (conv weights, BatchNorm weights and biases), bit for bit."""
    from simt_amd.engine_v3 import V3Plan, v3_state_shapes
    from test_gpu_v3 import make_state
    st = make_state(v3_state_shapes(19, 6, True), 11)
    g = torch.Generator().manual_seed(12)
    img = torch.randn(B4, 3, 512, 1024, generator=g)
    res = []
    for off in ("0", "1"):
        monkeypatch.setenv("SIMT_NO_INBN", off)
        plan = V3Plan({k: v.clone().to(dev) for k, v in st.items()}, B4, 512, 1024, 19, 6, True, dtype=BF, train=True)
        n_in = sum(1 for r in plan.block_io if r.get("inbn"))
        out = plan.forward(img.to(dev))
        up = (torch.randn(B4, 25, 32, 64, generator=torch.Generator().manual_seed(13)) * 1e-3).to(dev)
        plan.backward(torch.nn.functional.interpolate(up, size=(512, 1024), mode="bilinear"))
        torch.cuda.synchronize()
        res.append(dict(out=out.clone(), flat=plan.flat_grad.clone(), n_in=n_in))
        del plan
        torch.cuda.empty_cache()
    a, b = res
    print(f"DeepLabv3 plan: {a['n_in']} of 13 Bottlenecks apply bn2 in conv3's operand path")
    assert a["n_in"] >= 3 and b["n_in"] == 0
    assert torch.isfinite(a["flat"]).all() and a["flat"].abs().max().item() > 0
    assert torch.equal(a["out"], b["out"])
    assert torch.equal(a["flat"], b["flat"]), "v3 plan with bn2 in conv3's operand path differs from the plan without"
