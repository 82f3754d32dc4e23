"""The float64 launch oracle's fp32-storage forms (tests/_launch_oracle.py), shown sound WITHOUT a GPU.

For each handler form the fp32 plans reach, the operands are CPU tensors behind a `Mem`, the launch is a descriptor / argument tuple exactly
as a plan records it, and a plain torch CPU float32 evaluation of the same operation stands in for the kernel.  The check must pass (the
reference alone stays inside every bar before a kernel meets it; the worst error / bound is printed), and the perturbations of
tests/test_gpu_plan_launches_small.py's red tests must fail: one element moved by 4 x its own bound (read from the bound tensor of the check),
two output columns swapped, one border row zeroed, one statistics slot scaled by 1 + 1e-3 (where the launch has statistics).

Also: the storage-format bars themselves (tight_f32_ratio: the 2^-22 |ref| final rounding in place of a bf16 ulp, ambiguous ReLU signs
accepted either way; tight_bf16_ratio: outputs below 2048 elements held per element only, the 0.995 cap untouched above)."""

import pytest
import torch
import torch.nn.functional as F

import _launch_oracle as lo
from _plan_replay import _perturb
from simt_amd import _lib as L
from simt_amd import ops

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


class It:
    """A recorded launch as engine._Launch holds it (the handlers read keep / args / tag / shape only)."""

    def __init__(self, args=(), keep=None, tag="cpu", shape=None):
        self.fn, self.args, self.keep, self.tag, self.shape = None, args, keep, tag, shape


@pytest.fixture()
def host_desc(monkeypatch):
    """Let ops.make_*_desc take CPU tensors: the descriptors are only read back by the oracle here, never launched."""
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _move(t, idx, bound, k=4.0):
    v = t[idx].double()
    t[idx] = (v + k * bound * (1 if v >= 0 else -1)).to(t.dtype)


def _swap01(t):
    t.copy_(t[..., [1, 0] + list(range(2, t.shape[-1]))])


def _green_then_red(chk, got, what, make_cases):
    recs = chk.check(got)
    for (tag, shape, r) in recs:
        print(f"{what}: {r:6.3f}  {tag}  {shape}")
        assert r <= 1.0
    cases = make_cases()
    caught = _perturb(chk, got, what, cases)
    print(f"{what}: caught {caught}")
    assert caught == [c[0] for c in cases], f"{what}: the checker missed {sorted(set(c[0] for c in cases) - set(caught))}"
    chk.finish()


# ---- convolution ------------------------------------------------------------------------------------------------------------------------------
def _conv_setup(B, H, W, Cin, Cout, dil, seed, *, stats=False, bias=False, res=False, relu=False):
    g = _gen(seed)
    taps = ops.conv_taps(3, 3, dil, dil)
    M, K = B * H * W, 9 * Cin
    npad = ops.round_up(Cout, ops.pick_tile_n(Cout, F32))
    t = {"x": torch.randn(B, H, W, Cin, generator=g), "w": torch.zeros(npad, K), "y": torch.zeros(M, Cout)}
    t["w"][:Cout] = torch.randn(Cout, K, generator=g) * (2.0 / K) ** 0.5
    if stats:
        t["stats"] = torch.zeros(-(-M // 128), 2, Cout)
    if bias:
        t["bias"] = torch.randn(Cout, generator=g) * 0.1
    if res:
        t["res"] = torch.randn(M, Cout, generator=g)
    d = ops.make_conv_desc(t["x"], t["w"], t["y"], B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cout=Cout, taps=taps, bias=t.get("bias"),
                           res=t.get("res"), stats=t.get("stats"), relu=relu, Npad=npad)
    return t, d, M


def _conv_cpu(t, d, M, Cout):
    """float32 CPU evaluation: gathered operand rows x W^T (sgemm), epilogue in fp32, statistics as fp32 sums over 128-row blocks."""
    rows = torch.arange(M)
    v = lo.conv_gather(t["x"], d, rows).float() @ t["w"][:Cout].t()
    out = {}
    if "stats" in t:
        pad = torch.zeros(-(-M // 128) * 128 - M, Cout)
        blk = torch.cat([v, pad]).view(-1, 128, Cout)
        out["stats"] = torch.stack([blk.sum(1), (blk * blk).sum(1)], 1)
    if "bias" in t:
        v = v + t["bias"]
    if "res" in t:
        v = v + t["res"]
    if d.relu:
        v = torch.relu(v)
    out["y"] = v
    return out


@pytest.mark.parametrize("form", ["dilated 3x3 + statistics", "bias + residual + ReLU"])
def test_conv_fp32_storage(host_desc, form):
    """prepare_conv with fp32 in / out: the training conv that feeds a BatchNorm (statistics slots of the raw result; the dilation is larger
    than the 5-row map, so every off-centre tap row reads outside the image) and the frozen plan's folded-BatchNorm epilogue."""
    stats = form.endswith("statistics")
    B, H, W, Cin, Cout = 2, 5, 25, 32, 64                                    # M = 250: two 128-row statistics slots, the second ragged
    t, d, M = _conv_setup(B, H, W, Cin, Cout, 6 if stats else 2, 11, stats=stats, bias=not stats, res=not stats, relu=not stats)
    chk = lo.prepare_conv(It(keep=d, tag="conv_igemm_kernel<f32, f32, 64>"), lo.Mem(list(t.values())))
    assert bool(torch.isnan(t["y"]).all()), "outputs must be poisoned before the launch"
    got = _conv_cpu(t, d, M, Cout)
    t["y"].copy_(got["y"])

    def cases():
        tol = chk.bounds["y"]
        col = int(got["y"][0].abs().argmax())
        cs = [("4 x its bound", lambda g: _move(g["y"], (0, col), tol[0, col])),
              ("columns swapped", lambda g: _swap01(g["y"])),
              ("border row zeroed", lambda g: g["y"][10].zero_())]
        if stats:
            cs.append(("stats slot 1e-3", lambda g: g["stats"][1].mul_(1.0 + 1e-3)))
        return cs
    _green_then_red(chk, got, f"conv fp32 ({form})", cases)


def test_wgrad_fp32_storage(host_desc):
    """prepare_wgrad_descs with fp32 operands: the slab's split sum against float64 dY^T x (ungrouped launch, 3 pixel splits)."""
    g = _gen(12)
    B, H, W, Cin, Cd, ns = 3, 13, 17, 32, 64, 3
    taps = ops.conv_taps(3, 3, 4, 4)
    M, Kt = B * H * W, 9 * Cin
    x, dy, slab = torch.randn(B, H, W, Cin, generator=g), torch.randn(M, Cd, generator=g) / M, torch.zeros(ns, Cd, Kt)
    d = ops.make_wgrad_desc(dy, x, slab, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, Cd=Cd, taps=taps, nsplit=ns)
    chk = lo.prepare_wgrad_descs(It(keep=d, tag="conv_wgrad<f32>", shape=f"M{M} Cd{Cd} K{Kt}"), [d], lo.Mem([x, dy, slab]))
    dd = lo._wgrad_views(d, lo.Mem([x, dy, slab]))[3]
    X = lo.conv_gather(x, dd, torch.arange(M)).float()
    per = -(-M // ns)
    got = {"slab0": torch.stack([dy[i * per:(i + 1) * per].t() @ X[i * per:(i + 1) * per] for i in range(ns)])}

    def cases():
        tol = chk.bounds["slab0"]
        flat = int(got["slab0"].sum(0).abs().argmax())
        co, kk = flat // Kt, flat % Kt
        return [("4 x its bound", lambda g_: _move(g_["slab0"], (0, co, kk), tol[co, kk])),
                ("columns swapped", lambda g_: _swap01(g_["slab0"])),
                ("edge-tap row zeroed", lambda g_: g_["slab0"][:, 0, :Cin].zero_())]
    _green_then_red(chk, got, "wgrad fp32", cases)


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [False, True])
def test_bn_apply_fp32_storage(bits):
    """simt_bn_apply / simt_bn_apply_bits on fp32 storage: z = relu(y * scale + shift + residual), the bit mask from the stored z."""
    g = _gen(13)
    M, Cn = 99, 64
    y, res, z = torch.randn(M, Cn, generator=g), torch.randn(M, Cn, generator=g), torch.zeros(M, Cn)
    sc, sh = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.1
    zb = torch.zeros(M, Cn // 8, dtype=torch.uint8)
    args = (y.data_ptr(), sc.data_ptr(), sh.data_ptr(), res.data_ptr(), None, None, None, z.data_ptr()) + ((zb.data_ptr(),) if bits else ()) \
        + (M, Cn, 1, L.SIMT_F32)
    chk = lo.prepare_bn_apply(It(args=args, tag="simt_bn_apply"), lo.Mem([y, res, z, sc, sh, zb]), bits)
    zz = torch.relu(y * sc + sh + res)
    got = {"z": zz}
    if bits:
        got["bits"] = ((zz > 0).view(M, Cn // 8, 8).int() << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)

    def cases():
        tol = chk.bounds["z"]
        col = int(zz[0].argmax())
        return [("4 x its bound", lambda g_: _move(g_["z"], (0, col), tol[0, col])),
                ("columns swapped", lambda g_: _swap01(g_["z"])),
                ("border row zeroed", lambda g_: g_["z"][10].zero_())]
    _green_then_red(chk, got, f"bn_apply fp32{' bits' if bits else ''}", cases)


def test_bn_bwd_fp32_storage(host_desc):
    """simt_bn_bwd on fp32 storage, mask mode 2 (ReLU sign from y * scale + shift), the stand-alone reduce: slot sums, coefficients, dy."""
    g = _gen(14)
    M, Cn = 663, 64
    nblk = L.load().simt_bn_bwd_nblk(M, Cn)
    y, dz = torch.randn(M, Cn, generator=g) * 2 + 0.3, torch.randn(M, Cn, generator=g) / M
    mean, var = y.mean(0), y.var(0, unbiased=False)
    rstd = 1.0 / (var + 1e-5).sqrt()
    gamma, beta = torch.rand(Cn, generator=g) * 0.6 + 0.7, torch.randn(Cn, generator=g) * 0.1
    scale = gamma * rstd
    shift = beta - mean * scale
    part, coef, dy = torch.zeros(nblk, 3, Cn), torch.zeros(3, Cn), torch.zeros(M, Cn)
    d = ops.make_bn_bwd_desc(dz=dz, y=y, mean=mean, rstd=rstd, scale=scale, shift=shift, part=part, coef=coef, dy=dy, M=M, Cn=Cn, mask_mode=2)
    chk = lo.prepare_bn_bwd(It(keep=d, tag="simt_bn_bwd"), lo.Mem([y, dz, mean, rstd, scale, shift, part, coef, dy]))
    # float32 stand-in: blocks of ceil(M / nblk) rows
    gm = dz * ((y * scale + shift) > 0)
    xh = (y - mean) * rstd
    R = -(-M // nblk)
    P = torch.zeros(nblk, 3, Cn)
    for k in range(nblk):
        P[k, 0], P[k, 1] = gm[k * R:(k + 1) * R].sum(0), (gm * xh)[k * R:(k + 1) * R].sum(0)
    S = P.double().sum(0)
    cf = torch.zeros(3, Cn)
    cf[:2] = (S[:2] / M).float()
    got = {"part": P, "coef": cf, "dy": scale * (gm - cf[0] - xh * cf[1])}

    def cases():
        tol, ctol = chk.bounds["dy"], chk.bounds["coef"]
        col = int(got["dy"][0].abs().argmax())
        cc = int(cf[1].abs().argmax())
        return [("dy: 4 x its bound", lambda g_: _move(g_["dy"], (0, col), tol[0, col])),
                ("coef: 4 x its bound", lambda g_: _move(g_["coef"], (1, cc), ctol[1, cc])),
                ("dy: columns swapped", lambda g_: _swap01(g_["dy"])),
                ("dy: border row zeroed", lambda g_: g_["dy"][10].zero_()),
                ("statistics slot 1e-3", lambda g_: g_["part"][0].mul_(1.0 + 1e-3))]
    _green_then_red(chk, got, "bn_bwd fp32", cases)


def test_bn_relu_maxpool_fp32_storage():
    """The stem's BatchNorm + ReLU + 3x3 / stride-2 max-pool on fp32 storage (ragged on both axes: 33 x 41 -> 17 x 21)."""
    g = _gen(15)
    B, H, W, Cn, Hp, Wp = 1, 33, 41, 64, 17, 21
    y = torch.randn(B, H, W, Cn, generator=g)
    sc, sh = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.1
    p, idx = torch.zeros(B, Hp, Wp, Cn), torch.zeros(B, Hp, Wp, Cn, dtype=torch.uint8)
    args = (y.data_ptr(), sc.data_ptr(), sh.data_ptr(), p.data_ptr(), idx.data_ptr(), B, H, W, Cn, Hp, Wp, L.SIMT_F32)
    chk = lo.prepare_bn_relu_maxpool(It(args=args, tag="simt_bn_relu_maxpool"), lo.Mem([y, sc, sh, p, idx]))
    a = torch.relu(y * sc + sh).permute(0, 3, 1, 2)
    ap = F.pad(a, (1, 1, 1, 1), value=float("-inf"))
    win = F.unfold(ap, 3, stride=2).view(B, Cn, 9, -1)                       # tap k = r * 3 + s, windows in scan order
    assert win.shape[-1] == Hp * Wp
    mx = win.max(2).values
    first = torch.where(win == mx.unsqueeze(2), torch.arange(9).view(1, 1, 9, 1), torch.tensor(9)).min(2).values      # the FIRST maximum
    got = {"p": mx.view(B, Cn, Hp, Wp).permute(0, 2, 3, 1).contiguous(), "idx": first.view(B, Cn, Hp, Wp).permute(0, 2, 3, 1).to(torch.uint8).contiguous()}

    def cases():
        j = int(got["p"][0, 0, 0].argmax())
        v = got["p"][0, 0, 0, j].double()
        tol = 2.0 ** -22 * v.abs() + 16.0 * 2 ** 0.5 * lo.U * got["p"].double().pow(2).mean().sqrt()
        return [("4 x its bound", lambda g_: _move(g_["p"], (0, 0, 0, j), tol)),
                ("columns swapped", lambda g_: _swap01(g_["p"])),
                ("border row zeroed", lambda g_: g_["p"][0, 0].zero_())]
    _green_then_red(chk, got, "bn_relu_maxpool fp32", cases)


def test_pack_folded_scale_fp32_storage():
    """simt_pack_weight into an fp32 operand with a folded BatchNorm scale (frozen fp32 plans): fp32(w * scale), one rounding."""
    g = _gen(16)
    Cout, Cin, RS = 64, 32, 9
    w, cs = torch.randn(Cout, Cin, RS, generator=g) * 0.05, torch.rand(Cout, generator=g) + 0.5
    dst = torch.zeros(128, RS * Cin)
    mem = lo.Mem([w, cs, dst])
    job = (w.data_ptr(), dst.data_ptr(), cs.data_ptr(), RS * Cin, Cout, Cin, RS, 0, 0, 0, 0, L.SIMT_F32)
    chk = lo.prepare_pack(It(tag="simt_pack_weight"), mem, [job], lambda ptr, dt: dst.numel())
    out = torch.zeros(128, RS * Cin)
    out[:Cout] = (w * cs.view(Cout, 1, 1)).permute(0, 2, 1).reshape(Cout, RS * Cin)
    got = {"d0": out.view(-1)}

    def cases():
        tol = chk.bounds["d0"]                                              # over the scaled elements, in destination order
        e = int(out.view(-1)[:Cout * RS * Cin].abs().argmax())
        return [("4 x its bound", lambda g_: _move(g_["d0"], (e,), tol[e])),
                ("columns swapped", lambda g_: g_["d0"].copy_(out[:, [1, 0] + list(range(2, RS * Cin))].reshape(-1))),
                ("border row zeroed", lambda g_: g_["d0"][:RS * Cin].zero_()),
                ("padding written", lambda g_: g_["d0"][-1:].fill_(1.0))]
    _green_then_red(chk, got, "pack fp32 (folded scale)", cases)


# ---- the storage-format bars ------------------------------------------------------------------------------------------------------------------
def test_tight_f32_is_the_bf16_derivation_with_the_fp32_rounding():
    g = _gen(17)
    ref = torch.randn(64, 64, generator=g, dtype=F64)
    K = 9
    rms = ref.pow(2).mean().sqrt().item()
    keep = {}
    _e, r = lo.tight_f32_ratio(ref.float(), ref, K, "rounded reference", keep=(keep, "t"))
    assert r <= 2.0 ** -24 / 2.0 ** -22 + 1e-9                                # one fp32 rounding is at most a quarter of the final-rounding term
    assert torch.equal(keep["t"], 2.0 ** -22 * ref.abs() + 16.0 * K ** 0.5 * 2.0 ** -24 * rms)
    bad = ref.float().clone()
    _move(bad, (3, 5), keep["t"][3, 5], k=1.5)
    with pytest.raises(AssertionError):
        lo.tight_f32_ratio(bad, ref, K, "moved by 1.5 bounds")
    # an ambiguous ReLU sign: either reference is accepted, nothing else
    alt = torch.full_like(ref, float("nan"))
    alt[3, 5] = 0.0
    flipped = ref.float().clone()
    flipped[3, 5] = 0.0
    lo.tight_f32_ratio(flipped, ref, K, "alt", alt64=alt)
    with pytest.raises(AssertionError):
        lo.tight_f32_ratio(flipped, ref, K, "no alt")
    # dispatch by storage dtype
    assert lo.tight_ratio(ref.float(), ref, K, "f32")[1] == r
    assert lo.tight_ratio(ref.float().to(BF), ref, K, "bf16")[0] == 1.0


def test_exact_share_cap_applies_from_2048_elements():
    """bf16: every element within one ulp but only ~90 % exactly rounded.  2048 elements and more: refused at the unchanged 0.995 cap; fewer:
    held to the per-element bound only."""
    g = _gen(18)
    for n, refused in ((4096, True), (2048, True), (2047, False), (99, False)):
        ref = torch.rand(n, generator=g, dtype=F64) * 0.9 + 1.0                    # one binade: ulp 2^-7 throughout
        got = ref.float().to(BF)
        off = torch.arange(n) % 10 == 0
        # every tenth element: the bf16 neighbour on the OTHER side of the reference (at most one ulp away: inside the bound, not exact)
        side = torch.where(got[off].double() > ref[off], -1.0, 1.0)
        got[off] = (got[off].double() + side * lo.ulp_bf16(ref[off], 1e-30)).to(BF)
        if refused:
            with pytest.raises(AssertionError, match="of the elements equal the float64 result rounded to bf16"):
                lo.tight_bf16_ratio(got, ref, 1, f"n={n}")
        else:
            e, r = lo.tight_bf16_ratio(got, ref, 1, f"n={n}")
            assert e < 0.995 and r <= 1.0
        got[0] = (got[0].double() + 3 * lo.ulp_bf16(ref[:1], 1e-30)[0]).to(BF)     # the per-element bound holds at every size
        with pytest.raises(AssertionError, match="off by more than"):
            lo.tight_bf16_ratio(got, ref, 1, f"n={n}")
