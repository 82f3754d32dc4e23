"""simt_head_loss_uncertain / simt_head_grad_uncertain on the GPU, launch pair by launch pair (csrc/head_loss.hip), against the
float64 restatement of tests/_uncertain_ref.py under the bars of tests/_head_bar.py as they stand.

  kl only    w = 0 exactly, lambda_kl = 1: hout[0] == hout[1] == 0, K and the gradients on their own scale;
  ce only    lambda_kl = 0, general weights: the rectified cross-entropy alone;
  sum        lambda_kl = 1, weights through the random item map, and the NULL table; hout[6], hout[15] and conf_out equal the weighted / plain
             launches'; a table of ones equals the NULL table bit for bit;
  identical  pred1 holds pred2's values: D = 0 exactly, the weights 1 exactly, R_k the plain launch's loss;
  scaling    at w = 0 doubling lambda_kl doubles every gradient word exactly;
  finite     no non-finite word where a block of the logits is saturated (D reaches ~264 and exp(-D) underflows to 0);
  refused    refusals leave poisoned hout, gradients and byte maps untouched.

Cases: tests/_uncertain_ref.py's HEADS, two heads each.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _head_bar as hb
import _uncertain_ref as ur
from _launch_oracle import SENTINEL
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF = torch.bfloat16
HEADS, _HID = ur.HEADS, ur.HID
LAMBDA_SEG = 0.1
_IN = {}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _normal(t):
    """No non-zero value of t is subnormal in its own format: fp32 and bf16 share the exponent range."""
    v = t.float().abs()
    v = v[v > 0]
    return v.numel() > 0 and float(v.min()) >= 2.0 ** -126


def _grads(r):
    """The written columns of the gradient outputs (the driver pre-fills the rest)."""
    return [(n, r[n][:, :r["QP"]]) for n in ("dp2", "dt2", "dp1", "dt1")]


def _inputs(case):
    if case not in _IN:
        _IN[case] = ur.inputs(case, CD)
    return _IN[case]


def _head(dev, case, half, pred1, pred2, lab, *, w=None, w_item=None, unc=None, gscale=1.0):
    """One pass-1 + pass-2 pair at ur.CASES[case], two heads: fp32 AND bf16 gradient outputs from the same launch, conf_out, every output
    pre-filled.  unc = lambda_kl: the uncertainty launches (w None: the NULL table);  unc None: the weighted launches (w given) or the plain
    ones."""
    B, h, w_, H, W, Q, Cn = ur.CASES[case]
    lib = L.load()
    ldp = ops.round_up(Q, 4) + 4
    QP = ops.round_up(Q, 8)
    ld_t = QP + 8

    def low(p):
        t = torch.zeros(B * h * w_, ldp, device=dev)
        t[:, :Q] = p.to(dev).permute(0, 2, 3, 1).reshape(-1, Q)
        return t
    p1, p2 = low(pred1), low(pred2)
    labd = lab.to(dev)
    part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Cn), device=dev)
    keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
    hout = torch.zeros(lib.simt_head_hout_floats(Q, Cn), device=dev)
    g1 = torch.zeros(2, B, H, w_, QP, device=dev)
    dp = [torch.full((B * h * w_, ldp), 5.0, device=dev) for _ in range(2)]
    dt = [torch.full((B * h * w_, ld_t), SENTINEL, dtype=BF, device=dev) for _ in range(2)]
    conf = torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
    hd = L.HeadDesc()
    hd.pred1, hd.pred2, hd.fixp, hd.label, hd.T1, hd.T2 = p1.data_ptr(), p2.data_ptr(), None, labd.data_ptr(), None, None
    hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
    hd.dpred1_f32, hd.dpred2_f32 = dp[0].data_ptr(), dp[1].data_ptr()
    hd.dpred1_t, hd.dpred2_t = dt[0].data_ptr(), dt[1].data_ptr()
    hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w_, H, W, Cn, Q
    hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = ldp, ldp, QP, ldp, ld_t, L.SIMT_BF16
    hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, LAMBDA_SEG, 0.0, gscale
    hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1, 0, int(half), 0
    hd.conf_out = conf.data_ptr()
    st = ops.stream_ptr()
    wd = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev)
    item = None if w_item is None else w_item.to(dev).contiguous()
    wp, ip, nw = (None if wd is None else wd.data_ptr()), (None if item is None else item.data_ptr()), (0 if wd is None else wd.numel())
    if unc is not None:
        hu = L.HeadUncertainty(float(unc))
        L.call("simt_head_loss_uncertain", C.byref(hd), wp, nw, ip, C.byref(hu), st)
        L.call("simt_head_grad_uncertain", C.byref(hd), wp, nw, ip, C.byref(hu), st)
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


def _finite(tag, r):
    for n, g in _grads(r):
        assert bool(torch.isfinite(g.float()).all()), f"{tag} {n}: {int((~torch.isfinite(g.float())).sum())} non-finite words in the written columns"
    assert bool(torch.isfinite(r["hout"][[0, 1, 2, 3, 4, 5, 6, 14, 15]]).all()), (tag, r["hout"].tolist())


def _against(tag, c, got, r64, r32):
    """The restatement's bars on one launch pair: losses, fp32 gradients (ur.compare), then the trainer's form of both dtypes (hb.trainer_form),
    and no non-finite word (the inputs carry the saturated block)."""
    Q = ur.CASES[c[0]][5]
    ur.compare(tag, got["hout"], {"dpred2": got["back"](got["dp2"]), "dpred1": got["back"](got["dp1"])}, r64, r32)
    for hd_, f32, bf in (("dpred2", got["dp2"], got["dt2"]), ("dpred1", got["dp1"], got["dt1"])):
        hb.trainer_form(tag, hd_, f32, bf, got["back"], Q, got["QP"], r64[hd_], r32[hd_], 1.0)
    _finite(tag, got)


def _ref(key, c, p1, p2, lab, w, m, lam):
    case, half = c
    Cn = ur.CASES[case][6]
    return hb.ref_pair(("uncertain", key, c), lambda dt: ur.uncertain_ref(p1, p2, lab, w, m, LAMBDA_SEG, half, dt, Cn, lam))


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_uncertain_head_kl_only(dev, c):
    """w = 0 exactly and lambda_kl = 1: hout[0] == hout[1] == 0, and the regulariser's losses and gradients on their own scale."""
    case, half = c
    B = ur.CASES[case][0]
    p1, p2, lab, _wt, _item = _inputs(case)
    zero = np.zeros(B, np.float32)
    got = _head(dev, case, half, p1, p2, lab, w=zero, unc=1.0)
    assert float(got["hout"][0]) == 0.0 and float(got["hout"][1]) == 0.0, got["hout"].tolist()
    assert int(got["hout"][15]) == 2
    r64, r32 = _ref("kl", c, p1, p2, lab, zero, None, 1.0)
    _against(f"kl only {_HID(c)}", c, got, r64, r32)


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_uncertain_head_rectified_ce_only(dev, c):
    """lambda_kl = 0 and general weights through the map: the rectified cross-entropy alone (its gradient still flows through exp(-D))."""
    case, half = c
    p1, p2, lab, wt, item = _inputs(case)
    got = _head(dev, case, half, p1, p2, lab, w=wt, w_item=item, unc=0.0)
    r64, r32 = _ref("ce", c, p1, p2, lab, wt, item, 0.0)
    _against(f"ce only {_HID(c)}", c, got, r64, r32)


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_uncertain_head_sum_vs_float64(dev, c):
    """Rectified cross-entropy + KL at lambda_kl = 1: general weights through the random item map, and the NULL table."""
    case, half = c
    B = ur.CASES[case][0]
    p1, p2, lab, wt, item = _inputs(case)
    for name, w, m in (("map", wt, item), ("null", None, None)):
        got = _head(dev, case, half, p1, p2, lab, w=w, w_item=m, unc=1.0)
        r64, r32 = _ref("sum " + name, c, p1, p2, lab, w, m, 1.0)
        _against(f"sum {name} {_HID(c)}", c, got, r64, r32)
        base = _head(dev, case, half, p1, p2, lab, w=w, w_item=m)          # the weighted / plain launches on the same inputs
        assert float(got["hout"][6]) == float(base["hout"][6]) and float(got["hout"][15]) == float(base["hout"][15]) == 2.0
        assert torch.equal(got["conf"], base["conf"])
        assert not torch.equal(_bits(got["dp2"]), _bits(base["dp2"])), "the flavour changed no gradient word"
    # a NULL table == a table of ones, bit for bit (the weight is a run-time test, 1.f either way)
    ones = _head(dev, case, half, p1, p2, lab, w=np.ones(B, np.float32), unc=1.0)
    assert torch.equal(_bits(ones["hout"]), _bits(got["hout"]))
    for (n, a), (_n, b) in zip(_grads(ones), _grads(got)):
        assert torch.equal(_bits(a), _bits(b)), f"{n}: w = 1 differs from the NULL table"


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_uncertain_head_identical_heads(dev, c):
    """pred1 holds pred2's values (another tensor): D = 0 and exp(-D) = 1 exactly at every pixel, R_k is the plain launch's loss."""
    case, half = c
    _p1, p2, lab, _wt, _item = _inputs(case)
    p1 = p2.clone()
    got = _head(dev, case, half, p1, p2, lab, unc=1.0)
    h = got["hout"]
    assert float(h[2]) == 0.0 and float(h[3]) == 0.0 and float(h[4]) == 1.0 and float(h[5]) == 1.0, h.tolist()
    base = _head(dev, case, half, p1, p2, lab)
    for i in (0, 1):
        assert abs(float(h[i]) - float(base["hout"][i])) <= 1e-6 * abs(float(base["hout"][i])), (i, h.tolist(), base["hout"].tolist())
    r64, r32 = _ref("identical", c, p1, p2, lab, None, None, 1.0)
    _against(f"identical {_HID(c)}", c, got, r64, r32)


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_uncertain_head_scales_exactly_with_lambda(dev, c):
    case, half = c
    B = ur.CASES[case][0]
    p1, p2, lab, _wt, _item = _inputs(case)
    zero = np.zeros(B, np.float32)
    one = _head(dev, case, half, p1, p2, lab, w=zero, unc=0.5)
    two = _head(dev, case, half, p1, p2, lab, w=zero, unc=1.0)
    for i in (2, 3):
        assert float(two["hout"][i]) == float(one["hout"][i]) and float(one["hout"][i]) > 0.0
    assert float(two["hout"][14]) == 2.0 * float(one["hout"][14]) and _normal(one["hout"][[14]]), (one["hout"].tolist(), two["hout"].tolist())
    for (n, a), (_n, b) in zip(_grads(two), _grads(one)):
        assert _normal(b), f"{n}: a compared value is subnormal"
        assert bool((b[:, :one["Q"]] != 0).any())
        assert bool((a.float() == 2.0 * b.float()).all()), f"{n}: {int((a.float() != 2.0 * b.float()).sum())} elements are not twice the half-lambda launch"
    _finite(f"scaling {_HID(c)}", two)


def test_uncertain_head_refusals_write_nothing(dev):
    c = HEADS[0]
    case, half = c
    B = ur.CASES[case][0]
    p1, p2, lab, wt, item = _inputs(case)
    ok = _head(dev, case, half, p1, p2, lab, w=wt, w_item=item, unc=1.0)
    hd = ok["desc"]
    _p1, _p2, _labd, _part, _keys, hout, _g1, dp, dt, conf, wd, itemd = ok["keep"]
    hout.fill_(-3.0)
    conf.fill_(77)
    for t in dp:
        t.fill_(5.0)
    for t in dt:
        t.fill_(SENTINEL)
    st = ops.stream_ptr()
    U = lambda lam: C.byref(L.HeadUncertainty(lam))          # noqa: E731
    good = U(1.0)
    nan, inf = float("nan"), float("inf")
    bad = [
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), None),                       # no record
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), U(-1.0)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), U(nan)),
        (C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), U(inf)),
        (C.byref(hd), None, 0, itemd.data_ptr(), good),                                # a map without a table
        (C.byref(hd), None, B, None, good),                                            # entries without a table
        (C.byref(hd), wd.data_ptr(), B - 1, None, good),                               # a table shorter than the batch
        (C.byref(hd), wd.data_ptr(), L.HEAD_WEIGHTS_MAX + 1, None, good),
        (C.byref(hd), wd.data_ptr() + 2, B, None, good),                               # misaligned
        (None, wd.data_ptr(), B, None, good),
    ]

    def with_field(name, field, value):
        keep = getattr(hd, field)
        setattr(hd, field, value)
        try:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(hd), wd.data_ptr(), B, None, good, st)
        finally:
            setattr(hd, field, keep)
    for name in ("simt_head_loss_uncertain", "simt_head_grad_uncertain"):
        for args in bad:
            with pytest.raises(L.SimtHipError):
                L.call(name, *args, st)
        with_field(name, "mode", 0)                  # the SimT loss block has no such term
        with_field(name, "single", 1)                # one head: no second prediction to compare with
        with_field(name, "pred1", None)
        with_field(name, "pred2", None)              # what simt_head_loss refuses
    torch.cuda.synchronize()
    assert bool((hout == -3.0).all()) and bool((conf == 77).all())
    assert all(bool((t == 5.0).all()) for t in dp) and all(bool((t == SENTINEL).all()) for t in dt)
    L.call("simt_head_loss_uncertain", C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), good, st)          # the descriptor itself is sound
    L.call("simt_head_grad_uncertain", C.byref(hd), wd.data_ptr(), B, itemd.data_ptr(), good, st)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hout[:16].cpu()), _bits(ok["hout"])) and bool((conf != 77).all())
    for t, k in ((dp[0], "dp1"), (dp[1], "dp2"), (dt[0], "dt1"), (dt[1], "dt2")):
        assert torch.equal(_bits(t.cpu()), _bits(ok[k])), k
