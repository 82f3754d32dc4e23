"""The NTM micro-solver (csrc/ntm.hip) element by element against float64, through the C ABI (L.NtmInnerDesc, L.NtmPostDesc), from states a
training run reaches -- not only the first step after initialisation.  References, bar and cases: tests/_ntm_ref.py (proven on the CPU by
tests/test_ntm_ref_cpu.py).  Every device buffer sits between two guard regions filled with SENTINEL, checked after every launch.

  inner loop   (Q, C) x state x step0 x steps x single x prior: w, exp_avg, exp_avg_sq (both slots), T_out and ntm_grad under the bar; steps = 0
               leaves w / m / v bit for bit (diagonal of w included, like the reference) and still writes T_out; single: slot 0 NULL or
               sentinel-filled, untouched; 5 + 5 steps == 10 steps bit for bit; two equal launches bit for bit
  post         a synthetic hout: lout[0..11] to 1e-4, ntm_grad under the bar, only the diagonal of w changes (to -1e4), lout[12] accumulates;
               gscale = 0.5 is bitwise half; the pivot-swap input; the volume guard (both NTMs degenerate / one)
  rejections   SIMT_ERR_INVALID, a message, nothing touched
  sig_ntm / sig_w   forward-only, backward-only and both
"""
import ctypes as C

import pytest
import torch

import _ntm_ref as nr
from _launch_oracle import SENTINEL
from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu
GUARD = 64            # floats on either side of every buffer
F32, F64 = torch.float32, torch.float64


class Buf:
    """An fp32 device buffer holding `t`, between two guard regions of SENTINEL.  t = None: n floats of SENTINEL (an output, or a buffer a
    launch must not touch)."""

    def __init__(self, dev, t=None, n=None):
        shape = (n,) if t is None else tuple(t.shape)
        n = n if t is None else t.numel()
        self.raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=F32, device=dev)
        self.t = self.raw[GUARD: GUARD + n].view(shape)
        if t is not None:
            self.t.copy_(t.to(F32))
        self.before = self.raw.cpu().clone()

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        return self.t.cpu().clone()

    def guards_intact(self, what):
        r = self.raw.cpu()
        assert bool((r[:GUARD] == SENTINEL).all()) and bool((r[-GUARD:] == SENTINEL).all()), f"{what}: a guard region was written"

    def untouched(self, what):
        assert torch.equal(self.raw.cpu().view(torch.int32), self.before.view(torch.int32)), f"{what}: the buffer was written"


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_all(bufs, what):
    for name, b in bufs.items():
        for k, x in enumerate(b if isinstance(b, list) else [b]):
            if x is not None:
                x.guards_intact(f"{what} {name}[{k}]")


def launch_inner(dev, st, cd, Q, Cn, *, step0, steps, single, lr=nr.LR_T, slot0="null"):
    """One simt_ntm_inner_loop on the state `st`.  single: slot 0 is NULL ("null") or sentinel-filled buffers ("sentinel") that must come back
    untouched.  -> (dict of Buf lists, return code)"""
    ks = (1,) if single else (0, 1)
    mk = lambda ts, shape: [Buf(dev, ts[k]) if k in ks else (Buf(dev, n=shape[0] * shape[1]) if slot0 == "sentinel" else None) for k in range(2)]
    b = {"ntm": mk(st["ntm"], (Q, Cn)), "w": mk(st["w"], (Q, Q)), "ntm_grad": mk(st["ntm_grad"], (Q, Cn)), "m": mk(st["m"], (Q, Q)),
         "v": mk(st["v"], (Q, Q)), "T": [Buf(dev, n=Q * Cn) if (k in ks or slot0 == "sentinel") else None for k in range(2)], "cd": Buf(dev, cd)}
    ni = L.NtmInnerDesc()
    for k in range(2):
        p = lambda x: None if x is None else x.ptr()
        ni.ntm[k], ni.w[k], ni.ntm_grad[k], ni.w_m[k], ni.w_v[k], ni.T_out[k] = (p(b[f][k]) for f in ("ntm", "w", "ntm_grad", "m", "v", "T"))
    ni.class_dist, ni.Q, ni.C, ni.steps, ni.step0, ni.single = b["cd"].ptr(), Q, Cn, steps, step0, int(single)
    ni.lr, ni.beta1, ni.beta2, ni.eps = lr, 0.9, 0.999, 1e-8
    rc = L.load().simt_ntm_inner_loop(C.byref(ni), ops.stream_ptr())
    torch.cuda.synchronize()
    return b, rc


def run_inner(dev, st, cd, Q, Cn, what, **kw):
    b, rc = launch_inner(dev, st, cd, Q, Cn, **kw)
    L.check(rc)
    _check_all(b, what)
    b["cd"].untouched(f"{what} class_dist")
    for k in range(2):
        if b["ntm"][k] is not None:
            b["ntm"][k].untouched(f"{what} ntm[{k}]")
    if kw["single"] and b["w"][0] is not None:
        for f in ("ntm", "w", "ntm_grad", "m", "v", "T"):
            b[f][0].untouched(f"{what}: single = 1, {f}[0]")
    ks = (1,) if kw["single"] else (0, 1)
    return {f: [b[f][k].cpu().view(Q, -1) if k in ks else None for k in range(2)] for f in ("w", "m", "v", "T", "ntm_grad")}


def hold_inner(tag, got, r64, r32):
    for f in ("w", "m", "v", "T", "ntm_grad"):
        for k in range(2):
            if r64[f][k] is not None:
                r = (nr.square_bar if f in ("w", "m", "v") else nr.bar)(got[f][k], r64[f][k], r32[f][k], f"{tag} {f}[{k}]")
                nr.report(tag, f"{f}[{k}]", r)


@pytest.mark.parametrize("case", nr.INNER_CASES, ids=nr.case_id)
def test_inner_loop_every_element_vs_float64(dev, case):
    Q, Cn, kind, step0, steps, single, _ = case
    tag = "inner " + nr.case_id(case)
    st, cd, _ = nr.inner_case(case)
    r64, r32 = nr.inner_refs(case)
    got = run_inner(dev, st, cd, Q, Cn, tag, step0=step0, steps=steps, single=single)
    hold_inner(tag, got, r64, r32)
    if single:           # ... and the same with buffers in slot 0: untouched (run_inner), same result bit for bit
        again = run_inner(dev, st, cd, Q, Cn, tag + " slot 0 given", step0=step0, steps=steps, single=single, slot0="sentinel")
        assert all(bits_equal(again[f][1], got[f][1]) for f in got)
    if steps == 0:       # nothing to optimise: w (its diagonal included, as in the reference), the moments and ntm_grad stay; T_out is written
        for k in ((1,) if single else (0, 1)):
            for f, src in (("w", "w"), ("m", "m"), ("v", "v"), ("ntm_grad", "ntm_grad")):
                assert bits_equal(got[f][k], st[src][k]), f"{tag}: steps = 0 changed {f}[{k}]"
            assert torch.equal(r32["w"][k], st["w"][k])
            assert not bool((got["T"][k] == SENTINEL).any())


def test_inner_loop_resumes_bit_for_bit_and_is_deterministic(dev):
    """5 steps from step0 = 0, then 5 from step0 = 5 on what they left == one launch of 10 steps, bit for bit in w, m, v and T_out (the state
    between two launches is exactly what the kernel keeps in LDS between two steps; the leaked gradient is summed in another order and is not
    compared).  Two launches on equal inputs: everything bit for bit."""
    for Q, Cn, kind, pk in ((22, 19, "init", "real"), (40, 20, "trained", "softmax")):
        st, cd = nr.state(Q, Cn, kind), nr.prior(Cn, pk)
        tag = f"resume {Q}x{Cn} {kind}"
        one = run_inner(dev, st, cd, Q, Cn, tag, step0=0, steps=10, single=0)
        two = run_inner(dev, st, cd, Q, Cn, tag, step0=0, steps=10, single=0)
        for f in one:
            assert all(bits_equal(one[f][k], two[f][k]) for k in range(2)), f"{tag}: {f} differs between two equal launches"
        half = run_inner(dev, st, cd, Q, Cn, tag, step0=0, steps=5, single=0)
        rest = run_inner(dev, dict(st, w=half["w"], m=half["m"], v=half["v"]), cd, Q, Cn, tag, step0=5, steps=5, single=0)
        for f in ("w", "m", "v", "T"):
            assert all(bits_equal(one[f][k], rest[f][k]) for k in range(2)), f"{tag}: 5 + 5 steps differ from 10 in {f}"
        wrong = run_inner(dev, dict(st, w=half["w"], m=half["m"], v=half["v"]), cd, Q, Cn, tag, step0=0, steps=5, single=0)
        assert not bits_equal(one["w"][0], wrong["w"][0])                      # (step0 is what makes them equal)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# simt_ntm_post
# ---------------------------------------------------------------------------------------------------------------------------------------------
def launch_post(dev, ntm, w, ntm_grad, cd, hout, Q, Cn, *, lambda_seg, lambdas, gscale, single, lout0=None, slot0="null", keep=None):
    """One simt_ntm_post (keep: the buffers of an earlier call, to call again on them).  -> (dict of Bufs, return code)"""
    ks = (1,) if single else (0, 1)
    if keep is None:
        mk = lambda ts, n: [Buf(dev, ts[k]) if k in ks else (Buf(dev, n=n) if slot0 == "sentinel" else None) for k in range(2)]
        zeros = [torch.zeros(Q, Cn), torch.zeros(Q, Cn)]
        b = {"ntm": mk(ntm, Q * Cn), "w": mk(w, Q * Q), "ntm_grad": mk(zeros if ntm_grad is None else ntm_grad, Q * Cn), "cd": Buf(dev, cd),
             "hout": Buf(dev, hout), "lout": Buf(dev, torch.zeros(16) if lout0 is None else lout0)}
    else:
        b = keep
    npd = L.NtmPostDesc()
    for k in range(2):
        p = lambda x: None if x is None else x.ptr()
        npd.ntm[k], npd.w[k], npd.ntm_grad[k] = p(b["ntm"][k]), p(b["w"][k]), p(b["ntm_grad"][k])
    npd.class_dist, npd.hout, npd.lout, npd.Q, npd.C = b["cd"].ptr(), b["hout"].ptr(), b["lout"].ptr(), Q, Cn
    npd.lambda_seg, (npd.lambda_convex, npd.lambda_volume, npd.lambda_anchor), npd.gscale, npd.single = lambda_seg, lambdas, gscale, int(single)
    rc = L.load().simt_ntm_post(C.byref(npd), ops.stream_ptr())
    torch.cuda.synchronize()
    return b, rc


def run_post(dev, ntm, w, cd, hout_small, Q, Cn, what, kw, slot0="null"):
    """-> (dict(lout, ntm_grad [2], w [2]), the Bufs).  hout is padded with zeros to simt_head_hout_floats(Q, C)."""
    hout = torch.zeros(L.load().simt_head_hout_floats(Q, Cn))
    hout[: hout_small.numel()] = hout_small
    lout0 = torch.zeros(16)
    lout0[12] = kw["lout12"]
    b, rc = launch_post(dev, ntm, w, kw["ntm_grad"], cd, hout, Q, Cn, lambda_seg=kw["lambda_seg"], lambdas=kw["lambdas"], gscale=kw["gscale"],
                        single=kw["single"], lout0=lout0, slot0=slot0)
    L.check(rc)
    _check_all(b, what)
    ks = (1,) if kw["single"] else (0, 1)
    for name in ("cd", "hout"):
        b[name].untouched(f"{what} {name}")
    for k in range(2):
        if b["ntm"][k] is not None:
            b["ntm"][k].untouched(f"{what} ntm[{k}]")
        if k not in ks and b["w"][k] is not None:
            b["w"][k].untouched(f"{what}: single = 1, w[0]"), b["ntm_grad"][k].untouched(f"{what}: single = 1, ntm_grad[0]")
    assert bool((b["lout"].cpu()[13:] == 0).all()), f"{what}: lout[13..15] written"
    return {"lout": b["lout"].cpu(), "ntm_grad": [b["ntm_grad"][k].cpu() if k in ks else None for k in range(2)],
            "w": [b["w"][k].cpu() if k in ks else None for k in range(2)]}, b


def only_diagonal_moved(tag, w_after, w_before):
    for k in range(2):
        if w_after[k] is not None:
            Q = w_after[k].shape[0]
            off = nr.offdiag(Q)
            assert bits_equal(w_after[k][off], w_before[k][off]), f"{tag}: off-diagonal of w[{k}] changed"
            assert bool((w_after[k].diagonal() == -10000.0).all()), f"{tag}: diagonal of w[{k}] is not -1e4"


@pytest.mark.parametrize("case", nr.POST_CASES, ids=nr.case_id)
def test_post_vs_float64(dev, case):
    Q, Cn, kind, ex, lam, single, _ = case
    tag = "post " + nr.case_id(case)
    st, cd, hout, kw = nr.post_case(case)
    r64, r32 = nr.post_refs(case)
    assert not r64["guarded"] and not r32["guarded"]
    got, b = run_post(dev, st["ntm"], st["w"], cd, hout, Q, Cn, tag, kw, slot0="sentinel" if single and Q == 22 else "null")
    nr.scalars_close(got["lout"], r64["lout"], range(12), tag)
    assert float(got["lout"][9]) == 1.0
    assert float(got["lout"][12]) == nr.LOUT12_BEFORE + float(hout[15])
    if single:
        assert float(got["lout"][1]) == 0.0 and float(got["lout"][3]) == 0.0 and float(got["lout"][10]) == 0.0
    for k in range(2):
        if r64["ntm_grad"][k] is not None:
            nr.report(tag, f"ntm_grad[{k}]", nr.bar(got["ntm_grad"][k], r64["ntm_grad"][k], r32["ntm_grad"][k], f"{tag} ntm_grad[{k}]"))
    only_diagonal_moved(tag, got["w"], st["w"])
    # a second call on the same buffers: the count of out-of-range labels accumulates, the other slots are written again
    _, rc = launch_post(dev, None, None, None, None, None, Q, Cn, lambda_seg=kw["lambda_seg"], lambdas=kw["lambdas"], gscale=kw["gscale"],
                        single=kw["single"], keep=b)
    L.check(rc)
    lo2 = b["lout"].cpu()
    assert float(lo2[12]) == nr.LOUT12_BEFORE + 2 * float(hout[15])
    assert bits_equal(lo2[:12], got["lout"][:12])


def test_post_gscale_half_is_bitwise_half(dev):
    """gscale multiplies the gradient once, before the sigmoid's backward, and the total once: a power of two scales every product and sum
    exactly, so from ntm_grad = 0 the outputs at 0.5 are half those at 1 bit for bit."""
    for case in ((22, 19, "trained", "mixed", "train", 0, "real"), (40, 20, "trained", "mixed", "train", 0, "softmax")):
        Q, Cn = case[:2]
        st, cd, hout, kw = nr.post_case(case)
        kw = dict(kw, ntm_grad=None)
        one, _ = run_post(dev, st["ntm"], st["w"], cd, hout, Q, Cn, "gscale 1", dict(kw, gscale=1.0))
        half, _ = run_post(dev, st["ntm"], st["w"], cd, hout, Q, Cn, "gscale 0.5", dict(kw, gscale=0.5))
        for k in range(2):
            assert bool((one["ntm_grad"][k] != 0).any()) and bits_equal(half["ntm_grad"][k], 0.5 * one["ntm_grad"][k])
        assert bits_equal(half["lout"][:1], 0.5 * one["lout"][:1]) and bits_equal(half["lout"][1:12], one["lout"][1:12])


def test_post_pivot_swap_input(dev):
    """class_dist * 8, NTM = randn * 3: the elimination of T^T T swaps rows for both NTMs (tests/test_ntm_ref_cpu.py counts them)."""
    ntm, w, cd, hout, kw, _ = nr.special_post_case("swap")
    r64, r32 = nr.special_post_refs("swap")
    got, _ = run_post(dev, ntm, w, cd, hout, 22, 19, "post swap", kw)
    nr.scalars_close(got["lout"], r64["lout"], range(12), "post swap")
    assert float(got["lout"][9]) == 1.0
    for k in range(2):
        nr.report("post swap", f"ntm_grad[{k}]", nr.bar(got["ntm_grad"][k], r64["ntm_grad"][k], r32["ntm_grad"][k], f"post swap ntm_grad[{k}]"))
    only_diagonal_moved("post swap", got["w"], w)


@pytest.mark.parametrize("name", ["guard_both", "guard_one"])
def test_post_volume_guard(dev, name):
    """det(T1^T T1) underflows to 0 in fp32 (both NTMs / NTM1 only; the guard is on the SUM of the two log-volumes): no volume term in the
    total, none in EITHER gradient, and the NaN / Inf the elimination produced on the way leaks nowhere."""
    ntm, w, cd, hout, kw, _ = nr.special_post_case(name)
    r64, r32 = nr.special_post_refs(name)                      # float64 with the guard forced, fp32 as it decides
    assert r32["guarded"] and r64["guarded"]
    got, _ = run_post(dev, ntm, w, cd, hout, 22, 19, f"post {name}", kw)
    lo = got["lout"]
    assert float(lo[9]) == 0.0 and float(lo[7]) == 0.0
    for i in (10, 11):
        assert bool(torch.isfinite(lo[i])) == bool(torch.isfinite(r32["lout"][i])), f"{name}: lout[{i}] = {float(lo[i])}, fp32 oracle {float(r32['lout'][i])}"
    nr.scalars_close(lo, r64["lout"], [0, 1, 2, 3, 4, 5, 6, 8], f"post {name}")          # lout[0]: the total without the volume term
    if name == "guard_one":
        nr.scalars_close(lo, r64["lout"], [11], f"post {name}")
    for k in range(2):
        assert bool(torch.isfinite(got["ntm_grad"][k]).all()), f"{name}: ntm_grad[{k}] is not finite"
        nr.report(f"post {name}", f"ntm_grad[{k}]", nr.bar(got["ntm_grad"][k], r64["ntm_grad"][k], r32["ntm_grad"][k], f"post {name} ntm_grad[{k}]"))
    only_diagonal_moved(f"post {name}", got["w"], w)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# rejections: SIMT_ERR_INVALID, a message, nothing launched
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _refused(rc, bufs, what):
    assert rc == 1, f"{what}: return code {rc}"                                      # SIMT_ERR_INVALID
    msg = L.load().simt_last_error()
    assert msg and b"ntm.hip" in msg, f"{what}: simt_last_error() = {msg}"
    torch.cuda.synchronize()
    for name, b in bufs.items():
        for x in (b if isinstance(b, list) else [b]):
            if x is not None:
                x.untouched(f"{what}: {name}")


@pytest.mark.parametrize("Q,Cn,null_cd", [(41, 19, False), (40, 21, False), (19, 20, False), (22, 19, True)])
def test_invalid_descriptors_are_refused(dev, Q, Cn, null_cd):
    """Q > 40, C > 20, C > Q, class_dist NULL: both entry points refuse.  (The buffers have the size the descriptor claims.)"""
    g = torch.Generator().manual_seed(3)
    st = {"ntm": [torch.randn(Q, Cn, generator=g) for _ in range(2)], "w": [torch.randn(Q, Q, generator=g) for _ in range(2)],
          "m": [torch.zeros(Q, Q) for _ in range(2)], "v": [torch.zeros(Q, Q) for _ in range(2)],
          "ntm_grad": [torch.randn(Q, Cn, generator=g) for _ in range(2)]}
    cd = torch.softmax(torch.randn(Cn, generator=g), 0)
    what = f"Q = {Q}, C = {Cn}{', class_dist NULL' if null_cd else ''}"
    for single in (0, 1):
        ks = (1,) if single else (0, 1)
        b = {f: [Buf(dev, st[f][k]) if k in ks else None for k in range(2)] for f in ("ntm", "w", "ntm_grad", "m", "v")}
        b["T"], b["cd"] = [Buf(dev, n=Q * Cn) if k in ks else None for k in range(2)], Buf(dev, cd)
        ni = L.NtmInnerDesc()
        for k in ks:
            ni.ntm[k], ni.w[k], ni.ntm_grad[k], ni.w_m[k], ni.w_v[k], ni.T_out[k] = (b[f][k].ptr() for f in ("ntm", "w", "ntm_grad", "m", "v", "T"))
        ni.class_dist, ni.Q, ni.C, ni.steps, ni.step0, ni.single = None if null_cd else b["cd"].ptr(), Q, Cn, 10, 0, single
        ni.lr, ni.beta1, ni.beta2, ni.eps = nr.LR_T, 0.9, 0.999, 1e-8
        _refused(L.load().simt_ntm_inner_loop(C.byref(ni), ops.stream_ptr()), b, f"simt_ntm_inner_loop {what} single {single}")
        b["hout"], b["lout"] = Buf(dev, torch.rand(16 + 4 * Q * Cn + 4 * nr.QMAXH + 4096, generator=g)), Buf(dev, torch.rand(16, generator=g))
        npd = L.NtmPostDesc()
        for k in ks:
            npd.ntm[k], npd.w[k], npd.ntm_grad[k] = b["ntm"][k].ptr(), b["w"][k].ptr(), b["ntm_grad"][k].ptr()
        npd.class_dist, npd.hout, npd.lout, npd.Q, npd.C = None if null_cd else b["cd"].ptr(), b["hout"].ptr(), b["lout"].ptr(), Q, Cn
        npd.lambda_seg, npd.lambda_convex, npd.lambda_volume, npd.lambda_anchor, npd.gscale, npd.single = 0.1, 0.5, 0.1, 0.5, 1.0, single
        _refused(L.load().simt_ntm_post(C.byref(npd), ops.stream_ptr()), b, f"simt_ntm_post {what} single {single}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# simt_sig_ntm / simt_sig_w
# ---------------------------------------------------------------------------------------------------------------------------------------------
SIG_CASES = [(22, 19, "init", "real"), (25, 19, "trained", "real"), (34, 19, "saturated", "real"), (40, 20, "saturated", "zero"),
             (20, 20, "trained", "softmax"), (3, 2, "trained", "softmax")]


@pytest.mark.parametrize("Q,Cn,kind,pk", SIG_CASES)
def test_sig_ntm_forms_vs_float64(dev, Q, Cn, kind, pk):
    tag = f"sig_ntm {Q}-{Cn}-{kind}-{pk}"
    st, cd = nr.state(Q, Cn, kind), nr.prior(Cn, pk)
    ntm = st["ntm"][0]
    dT = torch.randn(Q, Cn, generator=torch.Generator().manual_seed(Q)) * 0.5
    (T64, dN64), (T32, dN32) = nr.ref_pair((tag,), lambda dt: nr.sig_ntm_ref(dt, ntm, cd, Cn, dT))
    for form in ("forward", "backward", "both"):
        b = {"ntm": Buf(dev, ntm), "cd": Buf(dev, cd), "dT": Buf(dev, dT), "T": Buf(dev, n=Q * Cn), "dN": Buf(dev, n=Q * Cn)}
        ops.sig_ntm(b["ntm"].t, b["cd"].t, T_out=None if form == "backward" else b["T"].t.view(Q, Cn), dT=None if form == "forward" else b["dT"].t,
                    dN_out=None if form == "forward" else b["dN"].t.view(Q, Cn))
        torch.cuda.synchronize()
        _check_all(b, f"{tag} {form}")
        for name in ("ntm", "cd", "dT") + (("T",) if form == "backward" else ()) + (("dN",) if form == "forward" else ()):
            b[name].untouched(f"{tag} {form}: {name}")
        if form != "backward":
            nr.report(tag, f"{form} T", nr.bar(b["T"].cpu().view(Q, Cn), T64, T32, f"{tag} {form} T"))
        if form != "forward":
            nr.report(tag, f"{form} dN", nr.bar(b["dN"].cpu().view(Q, Cn), dN64, dN32, f"{tag} {form} dN"))


@pytest.mark.parametrize("Q,Cn,kind,pk", SIG_CASES)
def test_sig_w_forms_vs_float64(dev, Q, Cn, kind, pk):
    tag = f"sig_w {Q}-{kind}"
    w = nr.state(Q, Cn, kind)["w"][1]
    dW = torch.randn(Q, Q, generator=torch.Generator().manual_seed(100 + Q)) * 0.5
    (W64, dw64, _), (W32, dw32, _) = nr.ref_pair((tag,), lambda dt: nr.sig_w_ref(dt, w, dW))
    off = nr.offdiag(Q)
    for form in ("forward", "backward", "both"):
        b = {"w": Buf(dev, w), "dW": Buf(dev, dW), "W": Buf(dev, n=Q * Q), "dw": Buf(dev, n=Q * Q)}
        ops.sig_w(b["w"].t, W_out=None if form == "backward" else b["W"].t.view(Q, Q), dW=None if form == "forward" else b["dW"].t,
                  dweight_out=None if form == "forward" else b["dw"].t.view(Q, Q))
        torch.cuda.synchronize()
        _check_all(b, f"{tag} {form}")
        for name in ("dW",) + (("W",) if form == "backward" else ()) + (("dw",) if form == "forward" else ()):
            b[name].untouched(f"{tag} {form}: {name}")
        only_diagonal_moved(f"{tag} {form}", [b["w"].cpu(), None], [w, None])
        if form != "backward":       # W = softmax - I: the diagonal is exactly -1 (the softmax of -1e4 is 0), the rest under the bar
            got = b["W"].cpu().view(Q, Q)
            assert bool((got.diagonal() == -1.0).all())
            nr.report(tag, f"{form} W", nr.bar(got, W64, W32, f"{tag} {form} W", mask=off))
        if form != "forward":
            got = b["dw"].cpu().view(Q, Q)
            assert bool((got.diagonal() == 0.0).all())
            nr.report(tag, f"{form} dweight", nr.bar(got, dw64, dw32, f"{tag} {form} dweight", mask=off))
