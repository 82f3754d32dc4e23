"""simt_head_loss_entropy / simt_head_grad_entropy on the GPU, launch by launch (csrc/head_loss.hip), against the float64
restatement of tests/_entropy_ref.py under the bars of tests/_head_bar.py as they stand.

  pure     w = 0 exactly, lambda_ent = 1, eta in {2, 0.5}: the term on its own scale (at lambda = 0.005 its gradient hides below the cross-entropy's);
  scaling  at w = 0 doubling lambda_ent doubles hout[14] and every gradient word exactly;
  sum      general weights with a random item map, and w = NULL, at lambda_ent = 0.005, eta = 2; hout[6], hout[15] and conf_out equal the
           weighted / plain launches';
  finite   no non-finite output where a block of the logits is saturated (near one-hot) or uniform;
  refused  refusals leave poisoned hout, gradients and byte maps untouched.

Cases: tests/test_gpu_online_weighted.py's HEADS ("rows" is a compile-time-count descriptor (22, 19): the entropy launches run it on the
run-time-count build with ONE image row per pass-2 block) and "wide" (Q = 27: the <QMAX, 0, 0> builds), two heads and one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _entropy_ref as er
import _head_bar as hb
from _launch_oracle import SENTINEL
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from test_gpu_online_weighted import HEADS as _WHEADS, _bits, _grads, _HID, _normal

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF = torch.bfloat16
HEADS = list(_WHEADS) + [("wide", False, False), ("wide", False, True)]
LAMBDA_SEG = 0.1
_IN = {}


def _inputs(case):
    if case not in _IN:
        _IN[case] = er.inputs(case, CD)
    return _IN[case]


def _head(dev, case, half, single, pred1, pred2, lab, *, w=None, w_item=None, ent=None, gscale=1.0):
    """One pass-1 + pass-2 pair at er.CASES[case]: fp32 AND bf16 gradient outputs from the same launch, conf_out and label_ws, every output
    pre-filled.  ent = (lambda_ent, eta): the entropy launches (w None: the NULL table);  ent None: the weighted launches (w given) or the
    plain ones."""
    B, h, w_, H, W, Q, Cn = er.CASES[case]
    lib = L.load()
    ldp = ops.round_up(Q, 4) + 4
    QP = ops.round_up(Q, 8)
    ld_t = QP + 8

    def low(p):
        t = torch.zeros(B * h * w_, ldp, device=dev)
        t[:, :Q] = p.to(dev).permute(0, 2, 3, 1).reshape(-1, Q)
        return t
    p2 = low(pred2)
    p1 = None if single else low(pred1)
    labd = lab.to(dev)
    part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Cn), device=dev)
    keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
    hout = torch.zeros(lib.simt_head_hout_floats(Q, Cn), device=dev)
    g1 = torch.zeros(2, B, H, w_, QP, device=dev)
    dp = [torch.full((B * h * w_, ldp), 5.0, device=dev) for _ in range(2)]
    dt = [torch.full((B * h * w_, ld_t), SENTINEL, dtype=BF, device=dev) for _ in range(2)]
    conf = torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
    hd = L.HeadDesc()
    hd.pred1, hd.pred2, hd.fixp, hd.label, hd.T1, hd.T2 = (None if single else p1.data_ptr()), p2.data_ptr(), None, labd.data_ptr(), None, None
    hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
    hd.dpred1_f32, hd.dpred2_f32 = (None if single else dp[0].data_ptr()), dp[1].data_ptr()
    hd.dpred1_t, hd.dpred2_t = (None if single else dt[0].data_ptr()), dt[1].data_ptr()
    hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w_, H, W, Cn, Q
    hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = ldp, ldp, QP, ldp, ld_t, L.SIMT_BF16
    hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, LAMBDA_SEG, 0.0, gscale
    hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1, int(single), int(half), 0
    hd.conf_out = conf.data_ptr()
    st = ops.stream_ptr()
    wd = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev)
    item = None if w_item is None else w_item.to(dev).contiguous()
    wp, ip, nw = (None if wd is None else wd.data_ptr()), (None if item is None else item.data_ptr()), (0 if wd is None else wd.numel())
    if ent is not None:
        he = L.HeadEntropy(float(ent[0]), float(ent[1]))
        L.call("simt_head_loss_entropy", C.byref(hd), wp, nw, ip, C.byref(he), st)
        L.call("simt_head_grad_entropy", C.byref(hd), wp, nw, ip, C.byref(he), st)
    elif w is None:
        L.call("simt_head_loss", C.byref(hd), st)
        L.call("simt_head_grad", C.byref(hd), st)
    else:
        L.call("simt_head_loss_weighted", C.byref(hd), wp, ip, st)
        L.call("simt_head_grad_weighted", C.byref(hd), wp, ip, st)
    torch.cuda.synchronize()
    back = lambda g: g.cpu()[:, :Q].reshape(B, h, w_, Q).permute(0, 3, 1, 2)          # noqa: E731
    return dict(hout=hout[:16].cpu(), dp1=dp[0].cpu(), dp2=dp[1].cpu(), dt1=dt[0].cpu(), dt2=dt[1].cpu(), conf=conf.cpu(), back=back, QP=QP, Q=Q,
                desc=hd, keep=(p1, p2, labd, part, keys, hout, g1, dp, dt, conf, wd, item))


def _finite(tag, r, single):
    for n, g in _grads(r, single):
        assert bool(torch.isfinite(g.float()).all()), f"{tag} {n}: {int((~torch.isfinite(g.float())).sum())} non-finite words in the written columns"
    idx = [1, 3, 6, 14, 15] + ([] if single else [0, 2])
    assert bool(torch.isfinite(r["hout"][idx]).all()), (tag, r["hout"].tolist())


def _against(tag, c, got, r64, r32):
    """The restatement's bars on one launch pair: losses, fp32 gradients (er.compare), then the trainer's form of both dtypes (hb.trainer_form)."""
    case, half, single = c
    Q = er.CASES[case][5]
    grads = {"dpred2": got["back"](got["dp2"])}
    if not single:
        grads["dpred1"] = got["back"](got["dp1"])
    er.compare(tag, got["hout"], grads, r64, r32, single)
    for hd_, f32, bf in (("dpred2", got["dp2"], got["dt2"]),) + (() if single else (("dpred1", got["dp1"], got["dt1"]),)):
        hb.trainer_form(tag, hd_, f32, bf, got["back"], Q, got["QP"], r64[hd_], r32[hd_], 1.0)
    _finite(tag, got, single)


@pytest.mark.parametrize("eta", [2.0, 0.5])
@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_entropy_head_pure_term(dev, c, eta):
    """w = 0 exactly and lambda_ent = 1: hout[0] == hout[1] == 0, and the term's losses and gradients on their own scale."""
    case, half, single = c
    B, h, w_, H, W, Q, Cn = er.CASES[case]
    p1, p2, lab, _wt, _item = _inputs(case)
    zero = np.zeros(B, np.float32)
    got = _head(dev, case, half, single, p1, p2, lab, w=zero, ent=(1.0, eta))
    assert float(got["hout"][1]) == 0.0 and (single or float(got["hout"][0]) == 0.0), got["hout"].tolist()
    assert int(got["hout"][15]) == 2
    r64, r32 = hb.ref_pair(("entropy pure", c, eta),
                           lambda dt: er.entropy_ref(None if single else p1, p2, lab, zero, None, LAMBDA_SEG, half, dt, Cn, 1.0, eta))
    _against(f"pure eta {eta} {_HID(c)}", c, got, r64, r32)
    if single:
        assert float(got["hout"][2]) == 0.0


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_entropy_head_scales_exactly_with_lambda(dev, c):
    case, half, single = c
    B = er.CASES[case][0]
    p1, p2, lab, _wt, _item = _inputs(case)
    zero = np.zeros(B, np.float32)
    one = _head(dev, case, half, single, p1, p2, lab, w=zero, ent=(0.5, 2.0))
    two = _head(dev, case, half, single, p1, p2, lab, w=zero, ent=(1.0, 2.0))
    assert float(two["hout"][14]) == 2.0 * float(one["hout"][14]) and _normal(one["hout"][[14]]), (one["hout"].tolist(), two["hout"].tolist())
    for i in ((3,) if single else (2, 3)):
        assert float(two["hout"][i]) == float(one["hout"][i])
    for (n, a), (_n, b) in zip(_grads(two, single), _grads(one, single)):
        assert _normal(b), f"{n}: a compared value is subnormal"
        assert bool((b[:, :one["Q"]] != 0).any())
        assert bool((a.float() == 2.0 * b.float()).all()), f"{n}: {int((a.float() != 2.0 * b.float()).sum())} elements are not twice the half-lambda launch"


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_entropy_head_sum_vs_float64(dev, c):
    """Cross-entropy + 0.005 * entropy: general weights through the random item map, and the NULL table."""
    case, half, single = c
    B, h, w_, H, W, Q, Cn = er.CASES[case]
    p1, p2, lab, wt, item = _inputs(case)
    ent = (0.005, 2.0)
    for name, w, m in (("map", wt, item), ("null", None, None)):
        got = _head(dev, case, half, single, p1, p2, lab, w=w, w_item=m, ent=ent)
        r64, r32 = hb.ref_pair(("entropy sum", c, name),
                               lambda dt: er.entropy_ref(None if single else p1, p2, lab, w, m, LAMBDA_SEG, half, dt, Cn, *ent))
        _against(f"sum {name} {_HID(c)}", c, got, r64, r32)
        base = _head(dev, case, half, single, p1, p2, lab, w=w, w_item=m)          # the weighted / plain launches on the same inputs
        assert float(got["hout"][6]) == float(base["hout"][6]) and float(got["hout"][15]) == float(base["hout"][15]) == 2.0
        assert torch.equal(got["conf"], base["conf"])
        for i in ((1,) if single else (0, 1)):          # the cross-entropy sums are the same arithmetic
            assert abs(float(got["hout"][i]) - float(base["hout"][i])) <= 1e-6 * (1 + abs(float(base["hout"][i])))
        assert not torch.equal(_bits(got["dp2"]), _bits(base["dp2"])), "the term changed no gradient word"
    # a NULL table == a table of ones, bit for bit (the weight is a run-time test, 1.f either way)
    ones = _head(dev, case, half, single, p1, p2, lab, w=np.ones(B, np.float32), ent=ent)
    assert torch.equal(_bits(ones["hout"]), _bits(got["hout"]))
    for (n, a), (_n, b) in zip(_grads(ones, single), _grads(got, single)):
        assert torch.equal(_bits(a), _bits(b)), f"{n}: w = 1 differs from the NULL table"


def test_entropy_head_refusals_write_nothing(dev):
    c = HEADS[0]
    case, half, single = c
    B = er.CASES[case][0]
    p1, p2, lab, wt, item = _inputs(case)
    ok = _head(dev, case, half, single, p1, p2, lab, w=wt, w_item=item, ent=(0.005, 2.0))
    hd = ok["desc"]
    _p1, _p2, _labd, _part, _keys, hout, _g1, dp, dt, conf, wd, itemd = ok["keep"]
    hout.fill_(-3.0)
    conf.fill_(77)
    for t in dp:
        t.fill_(5.0)
    for t in dt:
        t.fill_(SENTINEL)
    st = ops.stream_ptr()
    E = lambda lam, eta: C.byref(L.HeadEntropy(lam, eta))          # noqa: E731
    good = E(0.005, 2.0)
    nan, inf = float("nan"), float("inf")
    bad = [
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), None),                       # no record
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(0.0, 2.0)),                # a zero lambda is the caller's business
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(-1.0, 2.0)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(nan, 2.0)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(inf, 2.0)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(0.005, 0.0)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(0.005, -2.0)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(0.005, nan)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), E(0.005, inf)),
        (C.byref(hd), None, 0, itemd.data_ptr(), good),                                # a map without a table
        (C.byref(hd), None, B, None, good),                                            # entries without a table
        (C.byref(hd), wd.data_ptr(), B - 1, None, good),                               # a table shorter than the batch
        (C.byref(hd), wd.data_ptr(), L.HEAD_WEIGHTS_MAX + 1, None, good),
        (C.byref(hd), wd.data_ptr() + 2, B, None, good),                               # misaligned
        (None, wd.data_ptr(), B, None, good),
    ]
    for name in ("simt_head_loss_entropy", "simt_head_grad_entropy"):
        for args in bad:
            with pytest.raises(L.SimtHipError):
                L.call(name, *args, st)
        hd.mode = 0                                                                    # the SimT loss block has no such term
        try:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(hd), wd.data_ptr(), B, None, good, st)
        finally:
            hd.mode = 1
        keep = hd.pred2
        hd.pred2 = None                                                                # what simt_head_loss refuses
        try:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(hd), wd.data_ptr(), B, None, good, st)
        finally:
            hd.pred2 = keep
    torch.cuda.synchronize()
    assert bool((hout == -3.0).all()) and bool((conf == 77).all())
    assert all(bool((t == 5.0).all()) for t in dp) and all(bool((t == SENTINEL).all()) for t in dt)
    L.call("simt_head_loss_entropy", C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), good, st)          # the descriptor itself is sound
    L.call("simt_head_grad_entropy", C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), good, st)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hout[:16].cpu()), _bits(ok["hout"])) and bool((conf != 77).all())
