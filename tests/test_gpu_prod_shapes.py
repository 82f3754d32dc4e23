"""Parity at the BENCHMARKED configuration (BASELINE.json configs[1]: B=4, 768x768, bf16, K=3): every kernel instantiation
bench.py times is run here on its production shape and dtype, through the C ABI, and `simt_conv_variant` is asserted so
that the test provably hits the timed template instance (conv_igemm2_kernel<256,5,3> / <128,4,2> / <128,5,*> / <256,4,3> /
<64,2,3>, conv_wgrad2 at its production pixel split, the BatchNorm / stem / head kernels at M = 4*97*97 and 4*768*768).

Checkers: torch-CPU fp32 of the same op on the bf16-rounded operands (oracle/ops_ref.py; 1e-2 of max|ref|, the bar of
tests/test_gpu_conv.py), the CPU oracle for the head (1e-4 / 1e-5, fp32 kernel), and for the full-depth network the
float64 bf16-storage model `oracle.simt_oracle.bf16_model_forward` (the reference's forward with a bf16 rounding wherever
the HIP plan stores bf16): what is left is accumulation order and rare 1-ulp rounding flips, so the bounds are ~10x tighter
than bf16's own error.  Reference: model/deeplab_multi.py:57-119,172-192; tools/trainV2_simt.py:351-409.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_bar as hb
from _launch_oracle import tight_bf16 as _tight_bf16
from _launch_oracle import ulp_bf16 as _ulp_bf16
from oracle import ops_ref
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.engine import TrunkPlan, multi_heads

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B4, HW = 4, 97                      # stride-8 feature map of a 768x768 input; M = 37 636
CD = so.load_class_dist()


def _threads():
    import os
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 8)))


def _rel(a, b):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---- the bf16 per-op bar, tied to the STORAGE FORMAT (round 5): tests/_launch_oracle.py tight_bf16 (its comment derives the bound).  Every element
# is compared with the float64 result of the same op on the same bf16 operands (shifted float64 matmuls on the device: test infrastructure, the
# product never calls a vendor GEMM).
def _conv64(x_nhwc, w_oihw, stride, pad, dil):
    """float64 conv of NHWC x (any float dtype, on the device) with OIHW weights -> [B, Ho, Wo, Cout] float64, as k*k shifted matmuls."""
    B, H, W, Cin = x_nhwc.shape
    Cout, _, kh, kw = w_oihw.shape
    Ho, Wo = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    xp = F.pad(x_nhwc.double(), (0, 0, pad, pad, pad, pad))
    wd = w_oihw.double().to(x_nhwc.device)
    out = torch.zeros(B * Ho * Wo, Cout, device=x_nhwc.device, dtype=torch.float64)
    for r in range(kh):
        for c in range(kw):
            xs = xp[:, r * dil:r * dil + (Ho - 1) * stride + 1:stride, c * dil:c * dil + (Wo - 1) * stride + 1:stride, :]
            out += xs.reshape(-1, Cin) @ wd[:, :, r, c].t()
    return out.view(B, Ho, Wo, Cout)


def _variant(d):
    bn_, tm_, nst_ = C.c_int(), C.c_int(), C.c_int()
    gen = L.load().simt_conv_variant(C.byref(d), C.byref(bn_), C.byref(tm_), C.byref(nst_))
    return gen, (bn_.value, tm_.value, nst_.value)


def _bits(keep_nhwc):
    M, Cn = keep_nhwc.shape
    kb = keep_nhwc.reshape(M, Cn // 8, 8).to(torch.int32)
    return (kb << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


STREAM = "stream"          # conv1x1_stream_kernel (persistent, deferred epilogue): short-K / wide-output 1x1 shapes the rows kernel does not take
ROWS = "rows"              # conv1x1_rows_kernel (weights in registers, pixel rows streamed): dense 1x1, Cin <= 256, wide outputs
# (id, B, H, W, Cin, Cout, k, dil, stride, epilogue, expected conv_igemm2_kernel<BN, TM, NST> or STREAM)
CONV_CASES = [
    ("l3.conv2 3x3 d2 + stats", B4, HW, HW, 256, 256, 3, 2, 1, "stats", (256, 5, 3)),
    ("l3.conv2 dgrad 3x3 d2 + bnr2", B4, HW, HW, 256, 256, 3, 2, 1, "bnr2", (256, 5, 3)),
    ("l4.conv2 3x3 d4 + stats", B4, HW, HW, 512, 512, 3, 4, 1, "stats", (256, 5, 3)),
    ("l3.conv3 256->1024 + stats", B4, HW, HW, 256, 1024, 1, 1, 1, "stats", ROWS),
    ("fixed l3.conv3 256->1024 bias+res+relu", B4, HW, HW, 256, 1024, 1, 1, 1, "bias_res_relu", ROWS),
    ("l3.conv1 dgrad 256->1024 + res_bits + bnr3", B4, HW, HW, 256, 1024, 1, 1, 1, "res_bits_bnr3", ROWS),
    ("l3.conv1 1024->256 + stats", B4, HW, HW, 1024, 256, 1, 1, 1, "stats", (256, 5, 3)),
    ("fixed l3.conv1 1024->256 bias+relu", B4, HW, HW, 1024, 256, 1, 1, 1, "bias_relu", (256, 5, 3)),
    ("l3.conv3 dgrad 1024->256 + bnr2", B4, HW, HW, 1024, 256, 1, 1, 1, "bnr2", (256, 5, 3)),
    ("l4.conv1 2048->512", B4, HW, HW, 2048, 512, 1, 1, 1, "stats", (256, 5, 3)),
    ("l4.conv3 512->2048", B4, HW, HW, 512, 2048, 1, 1, 1, "stats", ROWS),
    ("fixed l4.conv3 512->2048 bias+res+relu", B4, HW, HW, 512, 2048, 1, 1, 1, "bias_res_relu", ROWS),
    ("l4.conv1 dgrad 512->2048 + res_bits + bnr3", B4, HW, HW, 512, 2048, 1, 1, 1, "res_bits_bnr3", (128, 5, 2)),      # (160-row tiles since round 6: pick_rows breaks cost ties towards the largest tile)
    ("l4.0.downsample 1024->2048", B4, HW, HW, 1024, 2048, 1, 1, 1, "stats", (256, 5, 3)),          # (8 rounds of 160 rows = 10 rounds of 128: the tie goes to
    ("l4.0.downsample dgrad 2048->1024", B4, HW, HW, 2048, 1024, 1, 1, 1, "plain", (256, 5, 3)),    #  the larger tile since round 6; measured 165 vs 173 us)
    ("l4.0.conv1 1024->512", B4, HW, HW, 1024, 512, 1, 1, 1, "stats", (256, 5, 3)),
    ("l2.conv3 128->512", B4, HW, HW, 128, 512, 1, 1, 1, "stats", ROWS),
    ("fixed l2.conv3 128->512 bias+res+relu", B4, HW, HW, 128, 512, 1, 1, 1, "bias_res_relu", ROWS),
    ("l2.conv1 dgrad 128->512 + res_bits + bnr3", B4, HW, HW, 128, 512, 1, 1, 1, "res_bits_bnr3", ROWS),
    ("l2.0.downsample 256->512 s2", B4, 193, 193, 256, 512, 1, 1, 2, "stats", STREAM),
    ("l2.conv2 3x3 128->128", B4, HW, HW, 128, 128, 3, 1, 1, "stats", (128, 5, 3)),
    ("l2.conv1 512->128", B4, HW, HW, 512, 128, 1, 1, 1, "stats", (128, 5, 3)),
    ("l1.conv3 64->256", B4, 193, 193, 64, 256, 1, 1, 1, "stats", ROWS),
    ("fixed l1.conv3 64->256 bias+res+relu", B4, 193, 193, 64, 256, 1, 1, 1, "bias_res_relu", ROWS),
    ("l1.conv1 dgrad 64->256 + res_bits + bnr3", B4, 193, 193, 64, 256, 1, 1, 1, "res_bits_bnr3", ROWS),
    ("l1.conv2 3x3 64->64", B4, 193, 193, 64, 64, 3, 1, 1, "stats", (64, 2, 3)),
    ("l1.conv1 256->64", B4, 193, 193, 256, 64, 1, 1, 1, "stats", (64, 2, 3)),
    # the rows kernel on ragged pixel counts (M = 442 / 1 330: partial last 128-row tile, fewer tiles than workgroups, zero-page rows)
    ("rows ragged 256->1024 + stats", 2, 13, 17, 256, 1024, 1, 1, 1, "stats", ROWS),
    ("rows ragged 256->1024 bias+res+relu", 2, 13, 17, 256, 1024, 1, 1, 1, "bias_res_relu", ROWS),
    ("rows ragged 256->1024 + res_bits + bnr3", 2, 35, 19, 256, 1024, 1, 1, 1, "res_bits_bnr3", ROWS),
    ("rows ragged 512->2048 + stats", 2, 13, 17, 512, 2048, 1, 1, 1, "stats", ROWS),
    ("rows ragged 128->512 + res_bits + bnr3", 2, 35, 19, 128, 512, 1, 1, 1, "res_bits_bnr3", ROWS),
    ("rows ragged 64->256 bias+res+relu", 2, 35, 19, 64, 256, 1, 1, 1, "bias_res_relu", ROWS),
    ("rows ragged 64->256 + stats", 3, 9, 11, 64, 256, 1, 1, 1, "stats", ROWS),
    ("rows ragged 256->1024 plain", 2, 13, 17, 256, 1024, 1, 1, 1, "plain", ROWS),
    ("rows ragged 256->1024 bias+relu", 2, 13, 17, 256, 1024, 1, 1, 1, "bias_relu", ROWS),
    ("rows ragged 128->512 bias+stats", 2, 35, 19, 128, 512, 1, 1, 1, "bias_stats", ROWS),
    ("rows ragged 256->1024 residual only", 2, 35, 19, 256, 1024, 1, 1, 1, "res_only", ROWS),
    ("rows ragged 512->2048 residual only", 2, 13, 17, 512, 2048, 1, 1, 1, "res_only", ROWS),
    ("rows ragged 64->256 bias+relu", 3, 9, 11, 64, 256, 1, 1, 1, "bias_relu", ROWS),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_production_shapes_bf16(dev, case):
    _id, B, H, W, Cin, Cout, k, dil, stride, epi, want = case
    _threads()
    g = torch.Generator().manual_seed(Cin * 3 + Cout + k * 17 + dil)
    x = torch.randn(B, Cin, H, W, generator=g).to(BF)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (1.0 / (Cin * k * k)) ** 0.5)
    pad = dil * (k // 2)
    ref = ops_ref.conv2d(x.float(), w.to(BF).float(), None, stride=stride, pad=pad, dil=dil)
    Ho, Wo = ref.shape[2:]
    M = B * Ho * Wo
    taps = ops.conv_taps(k, k, dil, pad)
    x_d = x.permute(0, 2, 3, 1).contiguous().to(dev)
    tile = ops.pick_tile_n(Cout, BF)
    npad = ops.round_up(Cout, tile)
    wp = torch.zeros(npad, len(taps) * Cin, device=dev, dtype=BF)
    ops.pack_weight(w.to(dev).contiguous(), wp, Cout=Cout, Cin=Cin, RS=k * k, ldk=len(taps) * Cin, mode=0)
    y_d = torch.full((B, Ho, Wo, Cout), float("nan"), device=dev, dtype=BF)
    kw, stats, bnr = {}, None, None
    if epi == "stats":
        stats = torch.full(((M + 127) // 128, 2, Cout), float("nan"), device=dev)
        kw["stats"] = stats
    if epi in ("bias_relu", "bias_stats"):                 # generic (run-time flag) flavours of the rows kernel
        bias = torch.randn(Cout, generator=g)
        kw.update(bias=bias.to(dev), relu=(epi == "bias_relu"))
        ref_conv = ref
        ref = ref + bias.view(1, -1, 1, 1)
        if epi == "bias_relu":
            ref = torch.relu(ref)
        if epi == "bias_stats":
            stats = torch.full(((M + 127) // 128, 2, Cout), float("nan"), device=dev)
            kw["stats"] = stats
    if epi in ("bias_res_relu", "res_bits_bnr3", "res_only"):
        r = torch.randn(B, Cout, Ho, Wo, generator=g).to(BF)
        kw["res"] = r.permute(0, 2, 3, 1).contiguous().to(dev)
        if epi == "bias_res_relu":
            bias = torch.randn(Cout, generator=g)
            kw.update(bias=bias.to(dev), relu=True)
            ref = torch.relu(ref + bias.view(1, -1, 1, 1) + r.float())
        elif epi == "res_only":
            ref = ref + r.float()
        else:
            keep = torch.rand(B, Cout, Ho, Wo, generator=g) > 0.5
            kw["res_bits"] = _bits(keep.permute(0, 2, 3, 1).reshape(M, Cout)).to(dev)
            ref = ref + r.float() * keep
    if epi in ("bnr2", "res_bits_bnr3"):
        mode = 2 if epi == "bnr2" else 3
        yb = torch.randn(M, Cout, generator=g).to(BF)
        bnr = {"y": yb.to(dev), "mean": (torch.randn(Cout, generator=g) * 0.2).to(dev), "rstd": (torch.rand(Cout, generator=g) + 0.5).to(dev),
               "scale": (torch.rand(Cout, generator=g) + 0.5).to(dev), "shift": (torch.randn(Cout, generator=g) * 0.3).to(dev),
               "bits": torch.randint(0, 256, (M, Cout // 8), generator=g, dtype=torch.uint8).to(dev), "mode": mode,
               "part": torch.full((M // 128 + 2, 3, Cout), float("nan"), device=dev)}
        kw["bnr"] = bnr
    d = ops.make_conv_desc(x_d, wp, y_d, B=B, H=H, W=W, Cin=Cin, Ho=Ho, Wo=Wo, Cout=Cout, taps=taps, stride=stride, Npad=npad,
                           tile_n=tile, **kw)
    gen, var = _variant(d)
    if want == ROWS:
        assert gen == 5, f"{_id}: the benchmark times conv1x1_rows_kernel, this runs generation {gen} <{var}>"
    elif want == STREAM:
        assert gen == 4, f"{_id}: the benchmark times conv1x1_stream_kernel, this runs generation {gen} <{var}>"
    else:
        assert gen == 2 and var == want, f"{_id}: runs conv_igemm2_kernel<{var}>, the benchmark times <{want}>"
    ops.conv_fprop_desc(d)
    torch.cuda.synchronize()
    got = y_d.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    assert _rel(got, ref) < 1e-2, f"{_id}: {_rel(got, ref)}"
    # ---- the storage-format bar: every element within 1 bf16 ulp (+ fp32 accumulation slack) of the float64 result, >= 99.5 % exactly equal
    r64 = _conv64(x_d, w.to(BF), stride, pad, dil)
    inner = None
    if "bias" in kw or "res" in kw or kw.get("relu"):      # two roundings: the parked bf16 conv tile, then the epilogue's result
        inner = r64
        r64 = r64.float().to(BF).double()
    if "bias" in kw:
        r64 = r64 + kw["bias"].double().view(1, 1, 1, -1)
    if "res" in kw:
        rr = kw["res"].double()
        if "res_bits" in kw:
            rr = rr * keep.permute(0, 2, 3, 1).to(dev)
        r64 = r64 + rr
    if kw.get("relu"):
        r64 = torch.relu(r64)
    exact = _tight_bf16(y_d, r64, len(taps) * Cin, _id, inner64=inner)
    print(f"{_id}: {exact:.5f} of the elements equal bf16(float64 result)")
    stored = y_d.double().reshape(M, Cout)
    if stats is not None:                                  # BN batch statistics of the STORED bf16 values, every slot summed
        s = stats.double().sum(0)
        assert torch.isfinite(s).all()
        pre = stored                                       # statistics are taken BEFORE bias / ReLU (of the rounded conv result)
        if epi == "bias_stats":
            pre = ref_conv.permute(0, 2, 3, 1).reshape(M, Cout).to(torch.bfloat16).double().to(stored.device)
        assert _rel(s[0].cpu(), pre.sum(0).cpu()) < 2e-3 and _rel(s[1].cpu(), (pre * pre).sum(0).cpu()) < 2e-3
    if bnr is not None:                                    # fused first pass of the BatchNorm backward (simt_conv_desc.bnr_*)
        nblk = L.load().simt_conv_mtiles(C.byref(d))
        assert 0 < nblk <= bnr["part"].shape[0]
        yy = bnr["y"].double()
        if bnr["mode"] == 2:
            msk = (bnr["y"].float() * bnr["scale"] + bnr["shift"]) > 0
        else:
            msk = ((bnr["bits"].unsqueeze(-1).to(torch.int32) >> torch.arange(8, device=dev, dtype=torch.int32)) & 1).reshape(M, Cout).bool()
        gm = stored * msk
        s1, s2 = gm.sum(0), (gm * ((yy - bnr["mean"].double()) * bnr["rstd"].double())).sum(0)
        part = bnr["part"][:nblk].double().sum(0)
        assert _rel(part[0].cpu(), s1.cpu()) < 2e-3 and _rel(part[1].cpu(), s2.cpu()) < 2e-3


def test_storage_format_bar_is_red_on_a_corrupted_row(dev):
    """The bar above must catch what the 1e-2-of-max bar let through in round 4 (stale dwords in single rows of a conv output): one row of a
    correct 3x3 256 -> 256 output overwritten with its neighbour row's values differs by ~rms on 256 of 9.6 M elements -- 1e-2 of max|ref| can
    miss it when the neighbour is close, the element-wise bar cannot; and a SINGLE element moved by two bf16 ulps passes 1e-2 and fails here."""
    B, H, W, Cin, Cout, k, dil = B4, HW, HW, 256, 256, 3, 2
    g = torch.Generator().manual_seed(99)
    x = torch.randn(B, H, W, Cin, generator=g).to(dev, BF)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (1.0 / (Cin * k * k)) ** 0.5)
    taps = ops.conv_taps(k, k, dil, dil)
    wp = torch.zeros(Cout, len(taps) * Cin, device=dev, dtype=BF)
    ops.pack_weight(w.to(dev).contiguous(), wp, Cout=Cout, Cin=Cin, RS=k * k, ldk=len(taps) * Cin, mode=0)
    y = torch.empty(B, H, W, Cout, device=dev, dtype=BF)
    ops.conv_fprop_desc(ops.make_conv_desc(x, wp, y, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, Npad=Cout, tile_n=256))
    torch.cuda.synchronize()
    r64 = _conv64(x, w.to(BF), 1, dil, dil)
    _tight_bf16(y, r64, len(taps) * Cin, "clean output")                     # green
    two_ulps = y.clone()
    v = two_ulps[2, 40, 17, 100].float()
    two_ulps[2, 40, 17, 100] = (v + 2.5 * float(_ulp_bf16(v.double().abs(), 1e-30)) * (1 if v >= 0 else -1)).to(BF)
    assert _rel(two_ulps.float(), r64) < 1e-2                                # the old bar does not see it
    with pytest.raises(AssertionError, match="off by more than 1 bf16 ulp"):
        _tight_bf16(two_ulps, r64, len(taps) * Cin, "one element moved by two ulps")
    stale = y.clone()
    stale[1, 50, 33, 64:72] = y[1, 50, 31, 64:72]                            # eight channels (one 16-byte store) of one row from the row two pixels back
    with pytest.raises(AssertionError, match="off by more than 1 bf16 ulp"):
        _tight_bf16(stale, r64, len(taps) * Cin, "one stale 16-byte store")


def test_tap_expanded_head_gemm_production(dev):
    """The N = 18*24 = 432 column tap-expanded ASPP GEMM of the main head (Cin 2048, fp32 output) + tap gather-sum at M = 37 636
    against the two dilated convs of torch CPU; instantiation <256, 5, 3> with the fp32 epilogue."""
    B, H, W, Cin, Q, QP = B4, HW, HW, 2048, 22, 24
    _threads()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, Cin, H, W, generator=g).to(BF)
    ws = [torch.randn(c, Cin, 3, 3, generator=g) * 0.01 for c in (19, 19, 3, 3)]
    bias = torch.randn(Q, generator=g)
    wq = [w_.to(BF).float() for w_ in ws]
    xf = x.float()
    y0 = ops_ref.conv2d(xf, wq[0], None, pad=6, dil=6) + ops_ref.conv2d(xf, wq[1], None, pad=12, dil=12)
    y1 = ops_ref.conv2d(xf, wq[2], None, pad=6, dil=6) + ops_ref.conv2d(xf, wq[3], None, pad=12, dil=12)
    ref = torch.cat([y0, y1], 1) + bias.view(1, -1, 1, 1)
    taps = ops.conv_taps(3, 3, 6, 6) + ops.conv_taps(3, 3, 12, 12)
    nt, M = len(taps), B * H * W
    nexp, npe = nt * QP, 512
    x_d = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wexp = torch.zeros(npe, Cin, device=dev, dtype=BF)
    for (w_, row, i) in ((ws[0], 0, 0), (ws[1], 0, 1), (ws[2], 19, 0), (ws[3], 19, 1)):
        ops.pack_weight(w_.to(dev).contiguous(), wexp, Cout=w_.shape[0], Cin=Cin, RS=9, row_off=row, tap_off=9 * i, ldk=Cin, Ck=QP, mode=2)
    P = torch.full((M, nexp), float("nan"), device=dev)
    d = ops.make_conv_desc(x_d, wexp, P, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=nexp, taps=[(0, 0)], Npad=npe, tile_n=256, ldy=nexp,
                           Nstore=nexp)
    gen, var = _variant(d)
    assert gen == 2 and var == (256, 5, 3)
    ops.conv_fprop_desc(d)
    logits = torch.zeros(M, 32, device=dev)
    td = L.TapDesc()
    bias_d = bias.to(dev)
    td.src, td.bias, td.dst = P.data_ptr(), bias_d.data_ptr(), logits.data_ptr()
    td.B, td.H, td.W, td.Q, td.QP, td.lds, td.ldd, td.ntaps = B, H, W, Q, QP, nexp, 32, nt
    ops._fill_taps(td.dy, td.dx, taps)
    L.call("simt_tap_gather_sum", C.byref(td), ops.stream_ptr())
    torch.cuda.synchronize()
    got = logits[:, :Q].cpu().reshape(B, H, W, Q).permute(0, 3, 1, 2)
    assert _rel(got, ref) < 1e-2 and torch.all(logits[:, Q:] == 0)


WGRAD_CASES = [
    # id, Cin, Cd, k, dil
    ("l3.conv2 3x3 256<-256", 256, 256, 3, 2),
    ("l3.conv3 1024<-256", 256, 1024, 1, 1),
    ("l3.conv1 256<-1024", 1024, 256, 1, 1),
    ("l4.conv2 3x3 512<-512", 512, 512, 3, 4),
    ("l4.conv3 2048<-512", 512, 2048, 1, 1),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_production_shapes_bf16(dev, case):
    """conv_wgrad2_kernel at M = 37 636 with the pixel split the plan uses (ops.wgrad_nsplit) + the fixed-order slab reduce."""
    _id, Cin, Cd, k, dil = case
    B, H, W = B4, HW, HW
    _threads()
    g = torch.Generator().manual_seed(Cin + Cd + k)
    x = torch.randn(B, Cin, H, W, generator=g).to(BF)
    dy = torch.randn(B, Cd, H, W, generator=g).to(BF)
    pad = dil * (k // 2)
    ref = torch.nn.grad.conv2d_weight(x.float(), (Cd, Cin, k, k), dy.float(), stride=1, padding=pad, dilation=dil)
    taps = ops.conv_taps(k, k, dil, pad)
    Ktot, M = len(taps) * Cin, B * H * W
    nsplit = ops.wgrad_nsplit(M, Cd, Ktot, BF)
    assert nsplit > 1
    x_d = x.permute(0, 2, 3, 1).contiguous().to(dev)
    dy_d = dy.permute(0, 2, 3, 1).contiguous().to(dev)
    slab = torch.full((nsplit, Cd, Ktot), float("nan"), device=dev)
    wd = ops.make_wgrad_desc(dy_d, x_d, slab, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cd=Cd, taps=taps, nsplit=nsplit)
    ops.conv_wgrad_desc(wd)
    dw = torch.full((Cd, Cin, k, k), float("nan"), device=dev)
    ops.wgrad_reduce(slab, dw, nsplit=nsplit, Cd=Cd, Ktot=Ktot, Cin=Cin, co_off=0, tap_off=0, Cout=Cd, RS=k * k)
    torch.cuda.synchronize()
    assert torch.isfinite(dw).all()
    assert _rel(dw.cpu(), ref) < 1e-2, f"{_id} split {nsplit}: {_rel(dw.cpu(), ref)}"
    # element-wise against float64 (shifted float64 matmuls on the device): an fp32 result of a sum of M products of bf16 values, split in
    # nsplit fp32 slabs -> |got - ref| <= 16 sqrt(M) 2^-24 rms(ref) + 2^-22 |ref| for EVERY element (the 1e-2-of-max bar above is ~1000x looser)
    xp = F.pad(x_d.double(), (0, 0, pad, pad, pad, pad))
    dyf = dy_d.double().reshape(M, Cd)
    r64 = torch.empty(Cd, Cin, k, k, device=dev, dtype=torch.float64)
    for r_ in range(k):
        for c_ in range(k):
            xs = xp[:, r_ * dil:r_ * dil + H, c_ * dil:c_ * dil + W, :].reshape(M, Cin)
            r64[:, :, r_, c_] = dyf.t() @ xs
    rms = r64.pow(2).mean().sqrt().item()
    tol = 16.0 * (M ** 0.5) * 2.0 ** -24 * rms + 2.0 ** -22 * r64.abs()
    worst = ((dw.double() - r64).abs() / tol).max().item()
    assert worst <= 1.0, f"{_id}: an element of the weight gradient is {worst:.1f} x its fp32 accumulation bound away from float64"
    # bitwise reproducible (fixed-order slab sum): a second launch gives the same bits
    dw2 = torch.empty_like(dw)
    ops.conv_wgrad_desc(wd)
    ops.wgrad_reduce(slab, dw2, nsplit=nsplit, Cd=Cd, Ktot=Ktot, Cin=Cin, co_off=0, tap_off=0, Cout=Cd, RS=k * k)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize("Cn,mode", [(256, "plain"), (1024, "residual"), (2048, "downsample")])
def test_bn_production_size_bf16(dev, Cn, mode):
    """simt_bn_finalize / apply(_bits) / bwd at M = 4*97*97 (295 statistic slots), bf16: same checker as tests/test_gpu_bn_pool.py."""
    from test_gpu_bn_pool import test_bn_train_forward_backward
    _threads()
    test_bn_train_forward_backward(dev, BF, Cn, B4, HW, HW, mode)


@pytest.mark.parametrize("Cn,with_res", [(256, False), (1024, True)], ids=["bn2_256", "bn3_1024_residual_bits"])
def test_bn_passes_storage_format_bar(dev, Cn, with_res):
    """The element-wise BatchNorm passes at M = 37 636 held to the storage format: forward z = bf16(relu(y * scale + shift [+ x])), backward
    dy = bf16(scale * (g - c1 - xhat * c2)) with the coefficients the kernel itself derived, both against float64 of the same expression on
    the same bf16 operands (one rounding: K = 1), >= 99.9 % of the elements exactly equal; the ReLU bit mask equals z > 0 bit for bit."""
    M = B4 * HW * HW
    g = torch.Generator().manual_seed(Cn)
    y = (torch.randn(M, Cn, generator=g) * 1.7 + 0.3).to(dev, BF)
    scale, shift = (torch.rand(Cn, generator=g) + 0.5).to(dev), (torch.randn(Cn, generator=g) * 0.3).to(dev)
    res = torch.randn(M, Cn, generator=g).to(dev, BF) if with_res else None
    z = torch.empty(M, Cn, device=dev, dtype=BF)
    bits = torch.empty(M, Cn // 8, device=dev, dtype=torch.uint8) if with_res else None
    ops.bn_apply(y, scale, shift, z, M=M, Cn=Cn, relu=True, res=res, bits=bits)
    torch.cuda.synchronize()
    r64 = y.double() * scale.double() + shift.double()
    if with_res:
        r64 = r64 + res.double()
    exact = _tight_bf16(z, torch.relu(r64), 1, f"bn_apply C={Cn}", exact_min=0.999)
    print(f"bn_apply C={Cn}: {exact:.6f} exactly equal")
    if with_res:
        assert torch.equal(bits, _bits((z > 0).cpu()).to(dev))
    # backward apply (mask from the bits / from y * scale + shift), coefficients from the kernel's own reduce + finalize
    dz = (torch.randn(M, Cn, generator=g) * 1e-3).to(dev, BF)
    mean, rstd = (torch.randn(Cn, generator=g) * 0.2).to(dev), (torch.rand(Cn, generator=g) + 0.5).to(dev)
    part = torch.empty(ops.bn_bwd_nblk(M, Cn), 3, Cn, device=dev)
    coef = torch.empty(3, Cn, device=dev)
    dy = torch.empty(M, Cn, device=dev, dtype=BF)
    d = ops.make_bn_bwd_desc(dz=dz, y=y, mean=mean, rstd=rstd, scale=scale, shift=shift, part=part, coef=coef, dy=dy, M=M, Cn=Cn,
                             mask_mode=3 if with_res else 2, z=bits)
    ops.bn_bwd_desc(d)
    torch.cuda.synchronize()
    if with_res:
        msk = ((bits.unsqueeze(-1).to(torch.int32) >> torch.arange(8, device=dev, dtype=torch.int32)) & 1).reshape(M, Cn).bool()
    else:
        msk = (y.float() * scale + shift) > 0
    gm = dz.double() * msk
    xhat = (y.double() - mean.double()) * rstd.double()
    c64 = torch.stack([gm.sum(0), (gm * xhat).sum(0)]) / M
    assert _rel(coef[:2].double(), c64) < 1e-5                                # fp32 partials, double finalize
    d64 = scale.double() * (gm - coef[0].double() - xhat * coef[1].double())
    exact = _tight_bf16(dy, d64, 4, f"bn_bwd_apply C={Cn}", exact_min=0.999)
    print(f"bn_bwd_apply C={Cn}: {exact:.6f} exactly equal")


def test_stem_production_size_bf16(dev):
    """Stem at 4 x 768 x 768 (M0 = 589 824): im2col -> <64,2,3> GEMM + statistics -> finalize -> BN+ReLU+ceil max-pool, and the pool's
    backward scatter, against torch CPU on the bf16-rounded image / weights (model/deeplab_multi.py:127-133,172-176)."""
    B, H, W = B4, 768, 768
    _threads()
    g = torch.Generator().manual_seed(3)
    img, _ = so.synthetic_batch(B, H, W, CD.numpy(), seed=7)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.01
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    H0 = W0 = 384
    Hp = Wp = 193
    M0 = B * H0 * W0
    A = torch.zeros(M0, 192, device=dev, dtype=BF)
    ops.im2col_stem(img.to(dev).contiguous(), A, B=B, Cin=3, H=H, W=W, Ho=H0, Wo=W0, KH=7, KW=7, stride=2, pad=3, ldk=192)
    wp = torch.zeros(64, 192, device=dev, dtype=BF)
    ops.pack_weight(w.to(dev).contiguous(), wp, Cout=64, Cin=147, RS=1, ldk=192)
    y0 = torch.empty(M0, 64, device=dev, dtype=BF)
    stats = torch.full(((M0 + 127) // 128, 2, 64), float("nan"), device=dev)
    d = ops.make_conv_desc(A, wp, y0, B=1, H=1, W=M0, Cin=192, Ho=1, Wo=M0, Cout=64, taps=[(0, 0)], stats=stats)
    gen, var = _variant(d)
    assert gen == 2 and var == (64, 2, 3)
    ops.conv_fprop_desc(d)
    outs = [torch.zeros(64, device=dev) for _ in range(4)]
    rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    ops.bn_finalize(stats, stats.shape[0], 64, M0, gamma.to(dev), beta.to(dev), rm, rv, 0.1, 1e-5, *outs)
    pool = torch.empty(B * Hp * Wp, 64, device=dev, dtype=BF)
    pidx = torch.empty(B * Hp * Wp, 64, device=dev, dtype=torch.uint8)
    ops.bn_relu_maxpool(y0, outs[2], outs[3], pool, pidx, B=B, H=H0, W=W0, Cn=64, Hp=Hp, Wp=Wp)
    torch.cuda.synchronize()
    yr = F.conv2d(img.to(BF).float(), w.to(BF).float(), stride=2, padding=3)
    assert _rel(y0.float().cpu().view(B, H0, W0, 64).permute(0, 3, 1, 2), yr) < 1e-2
    ys = y0.float().cpu().view(B, H0, W0, 64).permute(0, 3, 1, 2)          # BN of the STORED conv output, like the device
    pr = F.max_pool2d(F.relu(F.batch_norm(ys, None, None, gamma, beta, training=True, eps=1e-5)), 3, 2, 1, ceil_mode=True)
    assert _rel(pool.float().cpu().view(B, Hp, Wp, 64).permute(0, 3, 1, 2), pr) < 1e-2
    dp = torch.randn(B * Hp * Wp, 64, generator=g).to(dev, BF)
    da = torch.empty(M0, 64, device=dev, dtype=BF)
    ops.maxpool_bwd(dp, pidx, da, B=B, H=H0, W=W0, Cn=64, Hp=Hp, Wp=Wp)
    torch.cuda.synchronize()
    # adjoint identity of the scatter: <da, 1> == <dp, 1> per channel, and every gradient lands on a window maximum
    assert _rel(da.double().sum(0).cpu(), dp.double().sum(0).cpu()) < 2e-2


@pytest.mark.parametrize("geom", [(B4, 768, 768), (2, 65, 97), (1, 512, 1024)], ids=["b4_768", "ragged_65x97", "b1_512x1024"])
def test_direct_stem_both_networks_one_launch_bf16(dev, geom):
    """Round 6 (VERDICT r5 #1c): csrc/stem7.hip -- the 7x7 stride-2 stem convolved DIRECTLY from the fp32 NCHW image (no im2col matrix), the
    trainable net (BatchNorm statistics) and the frozen net (folded scale, bias + ReLU) in ONE launch (model/deeplab_multi.py:127,172-173;
    tools/trainV2_simt.py:351-353,370).  Every output element against the float64 convolution of the same bf16-rounded image / weights at the
    storage-format bar (1 bf16 ulp + fp32 accumulation slack, >= 99.5 % exactly the rounded float64 result); the per-tile statistics against the
    float64 sums of the STORED values; a ragged size exercises the tile-edge masks."""
    B, H, W = geom
    H0, W0 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    M0 = B * H0 * W0
    g = torch.Generator().manual_seed(H + W)
    img = (torch.rand(B, 3, H, W, generator=g) * 255.0 - 115.0).to(dev)                    # BGR - mean range
    w = [(torch.randn(64, 3, 7, 7, generator=g) * 0.01).to(dev) for _ in range(2)]
    cscale = (torch.rand(64, generator=g) + 0.5).to(dev)
    bias = (torch.randn(64, generator=g) * 0.5).to(dev)
    lib = L.load()
    wp = [torch.empty(64 * 7 * 32, device=dev, dtype=BF) for _ in range(2)]
    assert lib.simt_stem7_pack(w[0].data_ptr(), None, wp[0].data_ptr(), ops.stream_ptr()) == 0
    assert lib.simt_stem7_pack(w[1].data_ptr(), cscale.data_ptr(), wp[1].data_ptr(), ops.stream_ptr()) == 0
    tiles = lib.simt_stem7_tiles(B, H0, W0)
    y = [torch.full((M0, 64), float("nan"), device=dev, dtype=BF) for _ in range(2)]
    stats = torch.full((tiles, 2, 64), float("nan"), device=dev)
    d = L.StemDesc()
    d.x, d.B, d.H, d.W, d.Ho, d.Wo, d.nsets = img.data_ptr(), B, H, W, H0, W0, 2
    d.w[0], d.y[0], d.stats[0] = wp[0].data_ptr(), y[0].data_ptr(), stats.data_ptr()
    d.w[1], d.y[1], d.bias[1], d.relu[1] = wp[1].data_ptr(), y[1].data_ptr(), bias.data_ptr(), 1
    L.call("simt_stem7_fwd", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    x_nhwc = img.to(BF).permute(0, 2, 3, 1).contiguous()
    # the packed operands, read back: [64][7][32] with k' = s * 3 + c -> OIHW (what the kernel multiplies, scale folded and rounded)
    def unpack(t):
        return t.view(64, 7, 32)[:, :, :21].reshape(64, 7, 7, 3).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(unpack(wp[0]), w[0].to(BF)) and bool((wp[0].view(64, 7, 32)[:, :, 21:] == 0).all())
    r0 = _conv64(x_nhwc, unpack(wp[0]).float().cpu(), 2, 3, 1).view(M0, 64)
    e0 = _tight_bf16(y[0], r0, 147, "direct stem, trainable set")
    r1 = torch.relu(_conv64(x_nhwc, unpack(wp[1]).float().cpu(), 2, 3, 1).view(M0, 64) + bias.double())
    e1 = _tight_bf16(y[1], r1, 147, "direct stem, frozen set (bias + ReLU, ONE rounding)")
    s_ref = torch.stack([y[0].double().sum(0), (y[0].double() ** 2).sum(0)])
    s_got = stats.double().sum(0)
    assert torch.isfinite(stats).all()
    assert ((s_got - s_ref).abs() / (s_ref[1].sqrt() * M0 ** 0.5).clamp_min(1e-30)).max().item() < 1e-6
    print(f"direct stem {geom}: {tiles} tiles, exactly-rounded fraction {e0:.5f} / {e1:.5f}")
    # one weight set alone (an evaluation plan): the same values
    y1 = torch.full((M0, 64), float("nan"), device=dev, dtype=BF)
    d1 = L.StemDesc()
    d1.x, d1.B, d1.H, d1.W, d1.Ho, d1.Wo, d1.nsets = img.data_ptr(), B, H, W, H0, W0, 1
    d1.w[0], d1.y[0], d1.bias[0], d1.relu[0] = wp[1].data_ptr(), y1.data_ptr(), bias.data_ptr(), 1
    L.call("simt_stem7_fwd", C.byref(d1), ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(y1, y[1])


@pytest.mark.parametrize("geom", [(B4, 768, 768), (2, 65, 97), (1, 512, 1024), (1, 33, 41)], ids=["b4_768", "ragged_65x97", "b1_512x1024", "one_tile_row"])
def test_direct_stem_weight_gradient_vs_float64(dev, geom):
    """simt_stem7_wgrad: conv1's weight gradient straight from the fp32 NCHW image (loss.backward() through model/deeplab_multi.py:172,
    tools/trainV2_simt.py:428) against torch's float64 conv2d_weight of the same bf16-rounded image and bf16 gradient rows: fp32 accumulation
    (products of two bf16 values are exact in fp32), so the bar is fp32 summation error over B * Ho * Wo terms, not bf16; two calls agree bit
    for bit (fixed-order reduction of the workgroups' partials); ragged sizes exercise the zero rows of partial tiles."""
    B, H, W = geom
    H0, W0 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    M0 = B * H0 * W0
    g = torch.Generator().manual_seed(H * 3 + W)
    img = (torch.rand(B, 3, H, W, generator=g) * 255.0 - 115.0).to(dev)
    dy = (torch.randn(M0, 64, generator=g) * 1e-3).to(dev, BF)
    lib = L.load()
    nwg = lib.simt_stem7_wgrad_workgroups(B, H0, W0)
    assert nwg == min(256, lib.simt_stem7_tiles(B, H0, W0))
    part = torch.full((nwg, 64 * 7 * 32), float("nan"), device=dev)
    out = []
    for _ in range(2):
        dw = torch.full((64, 3, 7, 7), float("nan"), device=dev)
        L.call("simt_stem7_wgrad", img.data_ptr(), dy.data_ptr(), part.data_ptr(), dw.data_ptr(), B, H, W, H0, W0, ops.stream_ptr())
        torch.cuda.synchronize()
        out.append(dw)
    assert torch.equal(out[0], out[1])
    xr = img.to(BF).double().cpu()
    dyr = dy.double().cpu().view(B, H0, W0, 64).permute(0, 3, 1, 2).contiguous()
    ref = torch.nn.grad.conv2d_weight(xr, (64, 3, 7, 7), dyr, stride=2, padding=3)
    # scale of one output: sqrt(M0) * |x| * |dy|; fp32 accumulation in tiles of 256 pixels then <= 256 partials
    scale = (xr.pow(2).mean().sqrt() * dyr.pow(2).mean().sqrt()).item() * M0 ** 0.5
    err = (out[0].double().cpu() - ref).abs().max().item()
    print(f"direct stem wgrad {geom}: {nwg} workgroups, max err {err:.3e} (scale {scale:.3e})")
    assert err < 2e-5 * scale


def test_direct_stem_plan_matches_the_im2col_plan(dev, monkeypatch):
    """The production plans with the direct stem (default) against SIMT_DIRECT_STEM=0 (im2col + GEMM): a different summation order in the stem
    (filter rows of 21 + 11 zero columns vs the OIHW flattening), so the comparison is at the storage format: the stem outputs within 1 bf16 ulp,
    the frozen network's logits (well conditioned, BatchNorm folded) within 1e-2 of max|logit| of each other; the trainable plan's stem feeds
    BOTH nets from its first launch; the weight gradient of conv1 (im2col built in the backward) equals the im2col plan's to rounding."""
    from simt_amd import model_spec as ms
    from simt_amd.step import Hyper, SimTTrainer
    lay = (1, 1, 2, 1)
    st = ms.trained_like_init(ms.state_shapes(19, 3, True, layers=lay), seed=5)
    fst = ms.trained_like_init(ms.state_shapes(19, 0, False, layers=lay), seed=5)
    cd = ms.load_class_dist("bapa")
    img, lab = ms.synthetic_batch(2, 129, 193, cd, seed=4, device=dev)
    res = []
    for direct, dwg in (("1", "1"), ("0", "1"), ("1", "0")):
        monkeypatch.setenv("SIMT_DIRECT_STEM", direct)
        monkeypatch.setenv("SIMT_DIRECT_STEM_WGRAD", dwg)
        tr = SimTTrainer(st, fst, ms.ntm_init(19, 3, 1), ms.ntm_init(19, 3, 2), Hyper(open_classes=3), cd, 2, 129, 193, dtype=BF, device=dev, layers=lay)
        assert tr.plan.direct_stem == (direct == "1") and tr.fixed.direct_stem == (direct == "1")
        tag0 = tr.plan.fwd_list.items[0].tag
        assert tag0 == ("simt_stem7_fwd" if direct == "1" else "simt_im2col_stem")
        assert not any(it.tag in ("simt_stem7_fwd", "simt_im2col_stem") for it in tr.fixed.fwd_list.items)
        if direct == "1":
            assert tr.plan.stem_desc.nsets == 2
            # no im2col matrix anywhere in the step when the weight gradient is direct too
            tags = [it.tag for it in tr.plan.bwd_list.items]
            assert ("simt_stem7_wgrad" in tags) == (dwg == "1") and ("simt_im2col_stem" in tags) == (dwg == "0")
        tr.step(img, lab, 0)
        torch.cuda.synchronize()
        res.append(dict(y=tr.plan.saved["stem.y"].clone(), fy=tr.fixed.saved["stem.y"].clone(), fx2=tr.fixed.out["x2"].clone(),
                        gw=tr.plan.grads["conv1.weight"].clone(), l=tr.lout[:9].clone()))
        del tr
        torch.cuda.empty_cache()
    a, b, c = res
    # same forward, same dy0 (bitwise): the direct weight gradient against the im2col + GEMM one differs by fp32 summation order only
    assert torch.equal(a["y"], c["y"]) and torch.equal(a["l"], c["l"])
    assert _rel(a["gw"], c["gw"]) < 1e-5
    for k in ("y", "fy"):
        da, db = a[k].double(), b[k].double()
        ulp = _ulp_bf16(db, db.pow(2).mean().sqrt().item() * 2.0 ** -6)
        assert ((da - db).abs() <= 2 * ulp).all(), k           # each side is within one ulp of the float64 result
        assert (a[k] == b[k]).double().mean().item() > 0.8, k      # (the frozen set rounds ONCE here, twice in the GEMM path: 0.88 measured)
    assert _rel(a["fx2"].float(), b["fx2"].float()) < 1e-2
    assert torch.isfinite(a["l"]).all() and torch.isfinite(a["gw"]).all() and a["gw"].abs().max().item() > 0
    assert _rel(a["gw"], b["gw"]) < 0.25       # (the gradient passes back through the whole train-mode toy net: same order of magnitude is the claim)


HEAD_D = {"K": 3, "lam": np.array([0.5, 0.1, 0.5]), "lr_T": 6e-3, "th": np.array([0.8, 0.2]), "lambda_seg": 0.1, "lambda_place": 0.1}


def _prod_head_inputs():
    """4 x 768 x 768 labels over 97 x 97 logits, K = 3: seed 5 (logits) / 11 (labels)."""
    return hb.cached("prod inputs", lambda: hb.head_inputs((B4, HW, HW, 768, 768), 3, CD, block=16))


def _prod_head_refs():
    """(float64, fp32) CPU oracle on _prod_head_inputs (tests/_head_bar.py two_head_ref), computed once for every test of this module."""
    _threads()
    return hb.ref_pair("prod refs", lambda dt: hb.two_head_ref(*_prod_head_inputs(), HEAD_D, CD, dt))


def test_head_production_size_vs_oracle(dev):
    """head_pass1 / head_pass2 / yreduce + ntm kernels at 4 x 768 x 768 (P = 2 359 296 pixels, 9 216 blocks) from 97 x 97 logits,
    against the CPU oracle: losses 1e-4, gradients 1e-5, confidence-label count exact (trainV2_simt.py:351-409).

    On top of that (tests/_head_bar.py): both heads' gradients and both NTM gradients element by element on their own scale against the float64
    oracle, the per-pixel confidence labels equal to the fp32 oracle's, and the trainers' route (label_ws: the gradient pass reads the two
    byte maps of the loss pass back) bit for bit the same outputs."""
    from test_gpu_head_ntm import close, run_head
    _threads()
    K, Cn = 3, 19
    Q = Cn + K
    p1, p2, f2, lab, ntm = _prod_head_inputs()
    d = HEAD_D
    r = run_head(dev, d, p1, p2, f2, lab, ntm)
    r64, r32 = _prod_head_refs()
    out = r32["out"]                 # (the fp32 oracle run this test has always compared with)
    for idx, key in [(0, "total"), (1, "loss_p1"), (2, "loss_p2"), (3, "loss_y1"), (4, "loss_y2"), (5, "place"), (6, "convex"),
                     (7, "volume"), (8, "anchor")]:
        close(r["lout"][idx], out[key].detach(), 1e-4, key)
    assert int(r["hout"][6]) == int((out["conf"] != 255).sum())
    close(r["dpred1"], r32["dpred1"], 1e-5, "dpred1")
    close(r["dpred2"], r32["dpred2"], 1e-5, "dpred2")
    close(r["ntm_grad"][0], r32["ntm_grad1"], 2e-5, "ntm grad")
    nflip = int((r["conf"] != out["conf"].long().view_as(r["conf"])).sum())
    print(f"[head-bar] v2 4x768x768: {nflip} confidence labels differ from the fp32 oracle's; the references differ on "
          f"{int((r64['out']['conf'] != out['conf']).sum())} (conf) / {int((r64['out']['conf0'] != out['conf0']).sum())} (conf0)", flush=True)
    assert nflip == 0, f"{nflip} confidence labels differ"
    for k, got in (("dpred1", r["dpred1"]), ("dpred2", r["dpred2"]), ("ntm_grad1", r["ntm_grad"][0]), ("ntm_grad2", r["ntm_grad"][1])):
        hb.report("v2 4x768x768", k, hb.grad_bar(got, r64[k], r32[k], f"v2 4x768x768 {k}"))
    r2 = run_head(dev, d, p1, p2, f2, lab, ntm, label_ws=True)
    for k in ("lout", "dp1_raw", "dp2_raw", "conf"):                  # (compared as bit patterns)
        a, b = (x.view(torch.int32) if x.dtype == torch.float32 else x for x in (r[k], r2[k]))
        assert torch.equal(a, b), f"{k}: the label_ws route differs at {(a != b).nonzero()[:4].tolist()}"
    for k in ("ntm_grad", "w", "T", "ntm_after"):
        assert all(torch.equal(a, b) for a, b in zip(r[k], r2[k])), f"{k}: the label_ws route differs"


def _v2_head_plan_geometry(dev, warmup):
    """(h, w, pitch of the logits, pitch of the bf16 gradient) of the two heads of the plan SimTTrainer (warmup: WarmupTrainer) builds at the
    benchmarked B = 4, 768 x 768, bf16 (simt_amd/step.py: hd.ldp = plan.ldp["x1"], hd.ld_t = plan.dlogits["x1"].shape[1])."""
    def make():
        K = 0 if warmup else 3
        st = so.recipe_state(so.state_shapes(19, K, not warmup), seed=1234)
        plan = TrunkPlan({k: v.clone().to(dev) for k, v in st.items()}, B4, 768, 768, multi_heads(19, K, not warmup), dtype=BF, train=True)
        hd = plan.heads[1]
        geo = (hd.h, hd.w, plan.ldp["x1"], plan.dlogits["x1"].shape[1])
        assert (plan.heads[0].h, plan.heads[0].w, plan.ldp["x2"], plan.dlogits["x2"].shape[1]) == geo and plan.dlogits["x1"].dtype == BF
        del plan
        torch.cuda.empty_cache()
        return geo
    return hb.cached(("v2 plan geometry", warmup), make)


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_head_production_form_v2_simt(dev, gscale):
    """simt_head_loss / simt_head_grad as SimTTrainer launches them at the benchmarked size (simt_amd/step.py:124-141): bf16 dpred*_t with the
    plan's pitch, the plan's logits pitch, gscale = 1 / iter_size, conf_out + label_ws -- and dpred*_f32 from the SAME launch, so that the
    bf16 store is held bit for bit against the fp32 one.  The bars of tests/_head_bar.py against the float64 oracle; pad columns; the fp32
    output at gscale = 0.5 bit for bit half the one at gscale = 1 (gscale enters once, in the factors gscale * lambda / N of head_pass2: a
    power of two is exact); lout[0] = total * gscale."""
    from test_gpu_head_ntm import close, run_head
    h, w, ldp, ld_t = _v2_head_plan_geometry(dev, False)
    p1, p2, f2, lab, ntm = _prod_head_inputs()
    assert (h, w) == tuple(p1.shape[2:]) and ld_t > ops.round_up(22, 8)
    r64, r32 = _prod_head_refs()
    run = lambda gs: run_head(dev, HEAD_D, p1, p2, f2, lab, ntm, label_ws=True, grad_dtype=BF, ld_t=ld_t, gscale=gs, ldp=ldp)
    base = hb.cached(("gpu v2 simt", 1.0), lambda: run(1.0))
    r = base if gscale == 1.0 else run(gscale)
    tag = "v2 simt 4x768x768"
    assert torch.equal(r["conf"], r32["out"]["conf"].long().view_as(r["conf"]))
    for k, f32_raw, dt_raw in (("dpred1", r["dp1_raw"], r["dt1"]), ("dpred2", r["dp2_raw"], r["dt2"])):
        hb.trainer_form(tag, k, f32_raw, dt_raw, r["back"], 22, 24, r64[k], r32[k], gscale)
    close(r["lout"][0], r64["out"]["total"] * gscale, 1e-4, "lout[0] = total * gscale")
    if gscale == 0.5:
        for k in ("dp1_raw", "dp2_raw"):
            hb.half_is_bitwise(tag, k, r[k], base[k])


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_head_production_form_v2_warmup(dev, gscale):
    """The warm-up stage's launch of the same kernels (mode = 1, simt_amd/step.py:447-457: C = Q = 19, both heads against the labels, the
    auxiliary one weighted lambda_seg) in WarmupTrainer's form at B = 4, 768 x 768: as test_head_production_form_v2_simt; the references are
    float64 / fp32 autograd of oracle.simt_oracle.warmup_losses' cross entropies."""
    from test_gpu_warmup_single import _run_head
    h, w, ldp, ld_t = _v2_head_plan_geometry(dev, True)
    g = torch.Generator().manual_seed(23)
    pa, pb = torch.randn(B4, 19, h, w, generator=g) * 3, torch.randn(B4, 19, h, w, generator=g) * 3
    _, lab = so.synthetic_batch(B4, 768, 768, CD.numpy(), seed=13)
    lam = 0.1
    _threads()
    r64, r32 = hb.ref_pair("v2 warmup refs", lambda dt: hb.warmup_ref(pa, pb, lab, lam, False, dt))
    run = lambda gs: _run_head(dev, pb.to(dev), lab.to(dev), False, single=False, pred1=pa.to(dev), lambda_seg=lam, grad_dtype=BF, ld_t=ld_t,
                               gscale=gs, ldp=ldp, byte_maps=True, full=True)
    base = hb.cached(("gpu v2 warmup", 1.0), lambda: run(1.0))
    r = base if gscale == 1.0 else run(gscale)
    tag = "v2 warm-up 4x768x768"
    assert torch.equal(r["conf"], lab)               # (mode 1: the confidence label is the label itself)
    for k, f32_raw, dt_raw in (("dpred1", r["dp1_raw"], r["dt1"]), ("dpred2", r["dp2_raw"], r["dt2"])):
        hb.trainer_form(tag, k, f32_raw, dt_raw, r["back"], 19, 24, r64[k], r32[k], gscale)
    tot = float(r64["total"])
    assert abs(float(r["hout"][14]) - tot) <= 1e-4 * abs(tot), (float(r["hout"][14]), tot)
    if gscale == 0.5:
        for k in ("dp1_raw", "dp2_raw"):                           # (the columns the kernel writes: this driver pre-fills the fp32 buffers)
            hb.half_is_bitwise(tag, k, r[k][:, :24], base[k][:, :24])


# ---------------------------------------------------------------------------------------------------------------------
# full-depth ResNet-101 in bf16 against the float64 bf16-storage model
# ---------------------------------------------------------------------------------------------------------------------
def _nchw(t, Cn):
    return t[..., :Cn].permute(0, 3, 1, 2).double().cpu()


def _feat(t, B, h, w):
    """[B*h*w, C] device buffer -> float64 NCHW on the host."""
    return t.view(B, h, w, -1).permute(0, 3, 1, 2).double().cpu()


def test_full_depth_r101_bf16_forward_b4_768(dev):
    """BASELINE configs[1] exactly (B=4, 768x768, bf16, 33 bottlenecks): the production plans against the float64 bf16-storage model.
      * frozen (BN-folded) forward, END TO END: well conditioned, 1e-2 of max|logit| (measured 4-7e-3: 1-ulp bf16 rounding flips of
        fp32- vs float64-accumulated sums through 101 layers), arg-max differs on < 0.2 % of the positions;
      * train-mode forward, EVERY BLOCK fed with the GPU's own block input (the conditioning argument of tests/test_gpu_trunk.py: an
        untrained 101-layer net with batch-statistic BN is a chaotic map -- a 1-ulp bf16 flip moves the END-TO-END logits by tens of
        per cent in ANY implementation, two float64 runs with different thread counts included -- so end-to-end agreement is not a
        meaningful bar in bf16; per block it is): a1, a2, z within 2e-2 of max|ref|, the heads' logits from the GPU's own features 1e-2."""
    K, B, H, W = 3, B4, 768, 768
    _threads()
    st = so.recipe_state(so.state_shapes(19, K, True), seed=1234, head_scale=8.0)
    img, _ = so.synthetic_batch(B, H, W, CD.numpy(), seed=1234)
    p = {k: v.clone().to(dev) for k, v in st.items()}
    ev = TrunkPlan(p, B, H, W, multi_heads(19, K, True), dtype=BF, train=False)
    tags = {it.tag for it in ev.fwd_list.items}
    assert any(t.startswith("conv_igemm2_kernel<256, 5, 3,") for t in tags) and "conv1x1_rows_kernel" in tags
    out = ev.forward(img.to(dev))
    torch.cuda.synchronize()
    e1, e2 = _nchw(out["x1"], 22), _nchw(out["x2"], 22)
    del ev
    with torch.no_grad():
        m1, m2 = so.bf16_model_forward(st, img, False, True)
    r1, r2 = _rel(e1, m1), _rel(e2, m2)
    print(f"eval bf16 vs storage model: x1 {r1:.2e} x2 {r2:.2e}")
    assert r1 < 1e-2 and r2 < 1e-2
    # arg-max of the logits, margin-aware: the logits agree to r2 * max|logit| (asserted above), so two labels may only differ where the
    # model's own top-2 gap is below twice that error; elsewhere the label maps are identical.  Flip rate reported.
    t2 = m2.topk(2, dim=1).values
    gap = (t2[:, 0] - t2[:, 1])
    flips = e2.argmax(1) != m2.argmax(1)
    bound = 2.0 * max(r2, 1e-3) * m2.abs().max().item()
    print(f"eval arg-max: {int(flips.sum())} of {flips.numel()} positions differ ({flips.float().mean().item():.2e}); "
          f"{int((gap < bound).sum())} positions with a top-2 gap below {bound:.3f}")
    assert not bool((flips & (gap >= bound)).any()), "arg-max differs where the top-2 logit gap exceeds the measured logit error"
    assert flips.float().mean().item() < 2e-3
    tr = TrunkPlan(p, B, H, W, multi_heads(19, K, True), dtype=BF, train=True)
    tags = {it.tag for it in tr.fwd_list.items}
    assert any(t.startswith("conv_igemm2_kernel<256, 5, 3,") for t in tags) and "conv1x1_stream_kernel" in tags
    out = tr.forward(img.to(dev))
    torch.cuda.synchronize()
    worst = 0.0
    with torch.no_grad():
        for rec in tr.block_io:
            x = _feat(rec["x"], B, rec["Hi"], rec["Wi"])
            a1, a2, z = so.bf16_block_forward(st, rec["name"], x, rec["stride"], rec["dil"], rec["down"], True)
            for key, ref in (("a1", a1), ("a2", a2), ("z", z)):
                e = _rel(_feat(rec[key], B, rec["Ho"], rec["Wo"]), ref)
                worst = max(worst, e)
                assert e < 2e-2, f"{rec['name']} {key}: {e:.2e}"
        for hd in tr.heads:
            f = _feat(hd.feat, B, hd.h, hd.w)
            ref = torch.cat([so.bf16_aspp(st, pref, f) for pref, _c in hd.groups], 1)
            e = _rel(_nchw(out[hd.name], 22), ref)
            assert e < 1e-2, f"head {hd.name}: {e:.2e}"
    print(f"train-mode bf16, 33 blocks at B=4 768x768: worst block-level error {worst:.2e}")


def _bwd_setup(dev, B, fuse, monkeypatch, seed=99, pair=True):
    monkeypatch.setenv("SIMT_BN_FUSE", "1" if fuse else "0")
    # pair=False: every Bottleneck's weight gradients in its OWN launch range (a per-block replay needs them there); the product plan
    # groups two consecutive Bottlenecks into one launch, issued in the second one's range
    monkeypatch.setenv("SIMT_WGRAD_PAIR", "1" if pair else "0")
    K, H, W = 3, 768, 768
    st = so.recipe_state(so.state_shapes(19, K, True), seed=1234, head_scale=8.0)
    img, _ = so.synthetic_batch(B, H, W, CD.numpy(), seed=seed)
    p = {k: v.clone().to(dev) for k, v in st.items()}
    tr = TrunkPlan(p, B, H, W, multi_heads(19, K, True), dtype=BF, train=True)
    tr.forward(img.to(dev))
    return st, tr


def test_full_depth_r101_bf16_backward_blocks_b1_768(dev, monkeypatch):
    """Full-depth bf16 BACKWARD, block by block (dgrad <256,*,3> / <128,4,2>, grouped conv_wgrad2 / conv_wgrad3 + slab reduce, BatchNorm backward with bit masks)
    at 1 x 768 x 768: every Bottleneck's backward launches are replayed on a seeded dz and compared with autograd through the float64
    bf16-storage model of that block evaluated on the GPU's own block input (roundings passed straight through; the backward's own bf16
    storage of dY is not modelled): input gradient and all 3-4 weight gradients cos > 0.999 and relative L2 < 3e-2.  The fused
    BatchNorm-backward reduce is switched off here (its partial sums come from the PREVIOUS block's launches, which a per-block replay
    does not run); test_full_depth_bf16_backward_fused_equals_unfused_b4 covers it in situ."""
    from simt_amd.engine import LaunchList
    _threads()
    B = 1
    st, tr = _bwd_setup(dev, B, False, monkeypatch, pair=False)
    g = torch.Generator().manual_seed(8)
    worst_cos, worst_l2 = 1.0, 0.0
    for rec in tr.block_io:
        name = rec["name"]
        x = _feat(rec["x"], B, rec["Hi"], rec["Wi"]).requires_grad_(True)
        sd = {k: (v.double().requires_grad_(True) if ("conv" in k or "downsample.0" in k) else v) for k, v in st.items() if k.startswith(name + ".")}
        _, _, z = so.bf16_block_forward(sd, name, x, rec["stride"], rec["dil"], rec["down"], True)
        dz = (torch.randn(z.shape, generator=g) / z.shape[1] ** 0.5).to(BF).double()
        z.backward(dz)
        start, end, dzb, dxb = tr.bwd_marks[name]
        dzb.copy_(dz.permute(0, 2, 3, 1).reshape(dzb.shape).to(dev, BF))
        sub = LaunchList()
        sub.items = tr.bwd_list.items[start:end]
        sub.run()
        torch.cuda.synchronize()
        pairs = [(f"{name} dx", _feat(dxb, B, rec["Hi"], rec["Wi"]), x.grad)]
        pairs += [(k, tr.grads[k].double().cpu(), v.grad) for k, v in sd.items() if v.dtype == torch.float64 and v.requires_grad]
        for what, got, ref in pairs:
            c = F.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
            l2 = ((got - ref).norm() / ref.norm()).item()
            worst_cos, worst_l2 = min(worst_cos, c), max(worst_l2, l2)
            assert c > 0.999 and l2 < 3e-2, f"{what}: cos {c:.5f} rel-L2 {l2:.2e}"
    print(f"bf16 block-level backward, 33 blocks: worst cos {worst_cos:.5f}, worst rel-L2 {worst_l2:.2e}")


def _dcopy(ptr, n, dtype, dev):
    """Device pointer -> fresh tensor (hipMemcpy device-to-device through torch's own runtime)."""
    import ctypes
    t = torch.empty(n, dtype=dtype, device=dev)
    hip = ctypes.CDLL("libamdhip64.so")
    rc = hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(n * t.element_size()), 3)
    assert rc == 0
    return t


def test_full_depth_bf16_backward_fused_bn_reduce_in_situ_b4(dev, monkeypatch):
    """The production backward (B=4, 768x768, bf16) with the BatchNorm-backward reduce FUSED into the dgrad epilogues (default;
    simt_conv_desc.bnr_*), checked IN SITU: the backward is replayed launch by launch, and at each of the ~94 simt_bn_bwd launches
    that consume partial sums written by a conv epilogue the same launch is repeated with its own reduce pass over the same dz / y /
    masks: S1, S2 agree to 1e-5 of max|S| and dy to 1e-4 relative L2 (measured 1e-7 / 5e-6: summation order only).
    A whole-network fused-vs-unfused comparison is NOT a meaningful bar: those 5e-6 flip single bf16 roundings of the stored dY
    tensors, and 100 layers of batch-statistic BatchNorm backward amplify them to percents (measured up to 2.5e-2 relative L2 on single
    tensors) -- the same conditioning argument as for the forward."""
    monkeypatch.setenv("SIMT_SINGLE_STREAM", "1")
    # (round 4: layer 3's 46 dgrads run their whole BatchNorm backward inside the launch by default -- tests/test_gpu_bn_fused.py holds that
    # form BIT-identical to this one; switched off here so that all ~94 reduce hand-overs are the separate simt_bn_bwd launches this test replays)
    monkeypatch.setenv("SIMT_BN_GRID", "0")
    import simt_amd.engine as eng
    eng._SIDE_STREAMS.clear()
    st, tr = _bwd_setup(dev, B4, True, monkeypatch, seed=1234)
    g = torch.Generator().manual_seed(8)
    h, w = tr.heads[0].h, tr.heads[0].w
    for nm in ("x1", "x2"):
        up = (torch.randn(B4, 22, h, w, generator=g) / (h * w)).to(BF)
        dl = tr.dlogits[nm]
        dl.zero_()
        dl[:, :22] = up.permute(0, 2, 3, 1).reshape(-1, 22).to(dev)
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    seen, worst_dy, worst_s = 0, 0.0, 0.0
    for it in tr.bwd_list.items:
        if it.fn is None:
            continue
        assert it.fn(*it.args, stream) == 0
        if it.tag != "simt_bn_bwd" or it.keep.reduce_done_nblk == 0:
            continue
        d = it.keep
        M, Cn, nf = d.M, d.C, d.reduce_done_nblk
        torch.cuda.synchronize()
        dy_f = _dcopy(d.dy, M * Cn, BF, dev)
        s_f = _dcopy(d.part, nf * 3 * Cn, torch.float32, dev).view(nf, 3, Cn).double().sum(0)
        d.reduce_done_nblk = 0
        assert it.fn(*it.args, stream) == 0
        torch.cuda.synchronize()
        d.reduce_done_nblk = nf
        dy_u = _dcopy(d.dy, M * Cn, BF, dev)
        nb = lib.simt_bn_bwd_nblk(M, Cn)
        s_u = _dcopy(d.part, nb * 3 * Cn, torch.float32, dev).view(nb, 3, Cn).double().sum(0)
        l2 = ((dy_f.double() - dy_u.double()).norm() / dy_u.double().norm()).item()
        es = max(((s_f[k] - s_u[k]).abs().max() / s_u[k].abs().max()).item() for k in (0, 1))
        worst_dy, worst_s, seen = max(worst_dy, l2), max(worst_s, es), seen + 1
        assert l2 < 1e-4 and es < 1e-5, f"bn_bwd M={M} C={Cn} mask_mode={d.mask_mode}: dy rel-L2 {l2:.2e}, S rel {es:.2e}"
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")           # continue the chain on the production (fused) result
        hip.hipMemcpy(ctypes.c_void_p(d.dy), ctypes.c_void_p(dy_f.data_ptr()), ctypes.c_size_t(M * Cn * 2), 3)
    print(f"fused BN-backward reduce in situ: {seen} launches, worst dy rel-L2 {worst_dy:.2e}, worst S rel {worst_s:.2e}")
    assert seen > 60
    eng._SIDE_STREAMS.clear()


def test_full_depth_bf16_backward_is_bitwise_reproducible_b4(dev, monkeypatch):
    """Two fresh plans, same inputs, the production two-stream schedule at B=4 768x768 bf16: all 120 gradient tensors BIT-IDENTICAL
    (fixed-order reductions, no float atomics, stream hand-offs by events)."""
    g = torch.Generator().manual_seed(8)
    res, ups = [], None
    for _ in range(2):
        st, tr = _bwd_setup(dev, B4, True, monkeypatch, seed=1234)
        h, w = tr.heads[0].h, tr.heads[0].w
        if ups is None:
            ups = [(torch.randn(B4, 22, h, w, generator=g) / (h * w)).to(BF) for _ in range(2)]
        for nm, up in zip(("x1", "x2"), ups):
            dl = tr.dlogits[nm]
            dl.zero_()
            dl[:, :22] = up.permute(0, 2, 3, 1).reshape(-1, 22).to(dev)
        grads = tr.backward()
        torch.cuda.synchronize()
        res.append({k: v.clone() for k, v in grads.items()})
        del tr
        torch.cuda.empty_cache()
    diff = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
    assert not diff, f"{len(diff)} gradient tensors differ between two runs of the same backward: {diff[:5]}"
    assert all(torch.isfinite(v).all() for v in res[0].values())


# ---------------------------------------------------------------------------------------------------------------------
# round 6: the CU budget of a tile list (simt_conv_desc.cu_budget; data-parallel plans leave CUs to the collective's kernels)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 256, 3, 2), (1024, 256, 1, 1), (512, 512, 3, 4)], ids=["3x3_d2_256", "1x1_1024_256", "3x3_d4_512"])
def test_cu_budget_changes_the_tile_list_not_the_results(dev, shape):
    """The wide convs at M = 37 636 under CU budgets 256 (0), 248, 236, 200, 120: the plan is what pick_rows' cost model gives for that many
    CUs -- 236 tiles of 160 rows for every budget >= 236 (ONE round of full 160-row MFMA tiles: the default), 295 tiles of 128 rows in two
    rounds at 200, 236 tiles in two rounds at 120.  Every output element is bit-identical across budgets (an element's K reduction does not
    depend on the tile it sits in); the BatchNorm partial sums are one slot per TILE, so their grouping -- hence the last bit of their fp32
    rounding -- changes with the rows per tile: the per-channel totals agree to 1e-6."""
    Cin, Cout, k, dil = shape
    B, H, W = B4, HW, HW
    M = B * H * W
    g = torch.Generator().manual_seed(Cin + k)
    x = torch.randn(B, H, W, Cin, generator=g).to(dev, BF)
    taps = ops.conv_taps(k, k, dil, dil * (k // 2))
    wp = (torch.randn(Cout, len(taps) * Cin, generator=g) * 0.02).to(dev, BF)
    outs = {}
    for budget, tiles in ((0, 236), (248, 236), (236, 236), (200, 295), (120, 236)):
        y = torch.full((M, Cout), float("nan"), device=dev, dtype=BF)
        part = torch.zeros((M + 127) // 128, 2, Cout, device=dev)
        d = ops.make_conv_desc(x, wp, y, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, Npad=Cout, tile_n=256, stats=part)
        d.cu_budget = budget
        bn, tm, nst = C.c_int(), C.c_int(), C.c_int()
        assert L.load().simt_conv_variant(C.byref(d), C.byref(bn), C.byref(tm), C.byref(nst)) == 2 and (bn.value, nst.value) == (256, 3)
        assert tm.value == (4 if tiles == 295 else 5)
        assert L.load().simt_conv_mtiles(C.byref(d)) == tiles, f"budget {budget}: {L.load().simt_conv_mtiles(C.byref(d))} pixel tiles"
        ops.conv_fprop_desc(d)
        torch.cuda.synchronize()
        outs[budget] = (y, part.double().sum(0))
    y0, s0 = outs[0]
    assert torch.isfinite(y0.float()).all()
    for budget in (248, 236, 200, 120):
        y, s = outs[budget]
        assert torch.equal(y, y0), f"budget {budget}: output differs from the full-chip plan"
        rss = s0[1].sqrt().clamp_min(1e-30)
        assert ((s[0] - s0[0]).abs() / (rss * M ** 0.5)).max().item() < 1e-6 and ((s[1] - s0[1]).abs() / s0[1]).max().item() < 1e-6


def test_data_parallel_plan_carries_the_cu_budget(dev, monkeypatch):
    """A plan built for a trainer with a process group plans its conv tile lists for 256 - NCCL_MAX_NCHANNELS CUs (16 assumed when unset);
    SIMT_CU_BUDGET wins; a single-GPU plan keeps the whole device.  At M = 37 636 every budget down to 236 gives the default plan (236 tiles of
    160 rows: it already leaves 20 CUs free); a budget of 200 changes the tile list -- same forward output bit for bit (frozen / eval plan)."""
    st = so.recipe_state(so.state_shapes(19, 3, True, layers=(1, 1, 2, 1)), seed=1, head_scale=8.0)
    p = lambda: {k: v.clone().to(dev) for k, v in st.items()}
    kw = dict(dtype=BF, train=False, layers=(1, 1, 2, 1))
    monkeypatch.delenv("SIMT_CU_BUDGET", raising=False)
    monkeypatch.delenv("NCCL_MAX_NCHANNELS", raising=False)
    solo = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), **kw)
    dp = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), data_parallel=True, **kw)
    monkeypatch.setenv("NCCL_MAX_NCHANNELS", "8")
    dp8 = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), data_parallel=True, **kw)
    monkeypatch.setenv("SIMT_CU_BUDGET", "200")
    dpx = TrunkPlan(p(), B4, 768, 768, multi_heads(19, 3, True), data_parallel=True, **kw)
    assert (solo.cu_budget, dp.cu_budget, dp8.cu_budget, dpx.cu_budget) == (0, 240, 248, 200)

    def wide_tiles(plan):
        return {L.load().simt_conv_mtiles(C.byref(it.keep)) for it in plan.fwd_list.items
                if it.tag and it.tag.startswith("conv_igemm2_kernel<256, ") and "N256" in (it.shape or "")}
    assert wide_tiles(solo) == {236} and wide_tiles(dp) == {236} and wide_tiles(dp8) == {236} and wide_tiles(dpx) == {295}
    img, _ = so.synthetic_batch(B4, 768, 768, CD.numpy(), seed=3)
    o = [pl.forward(img.to(dev))["x2"].clone() for pl in (solo, dp, dp8, dpx)]
    torch.cuda.synchronize()
    assert all(torch.equal(o[0], t) for t in o[1:])
