"""The gradient bar of tests/_head_bar.py proves itself on the CPU: it accepts the fp32 oracle against the float64 oracle, and rejects
gradients that are wrong in the ways the old comparator `close(got, ref, 1e-5)` (max|a - b| <= 1e-5 * (1 + max|ref|)) lets through.

Geometries: `up8_two_chunks` and `rows6` of tests/test_gpu_head_ntm.py HEAD_GEOMS, and B = 1 of the production size (97 x 97 logits ->
768 x 768 labels, K = 3; the inputs of test_head_production_size_vs_oracle with one image instead of four).

Mutants, each built from the float64 oracle's own gradient (so that nothing but the mutation separates them from the reference):
  (a) the auxiliary head's gradient scaled by 0.8 (a lambda_seg off by 20 %);
  (b) one image row's contribution removed: the oracle run again with that row's noisy labels set to 255 and its confidence labels masked;
  (c) one loss term, lambda_place * unknown, dropped from the main head;
  (d) one element of the bf16 form moved by two bf16 ulps;
  (e) the gradient of one low-res column replaced by its neighbour's.
For (a)-(c) the OLD bar is also asked, at the production-like size.  The losses are means over the pixels, so every gradient shrinks like
1 / B: the old bar, absolute at this size, is asked at B = 1 as computed and at the benchmarked B = 4 scale (the B = 1 gradients divided by
four; max|dpred1| = 1.50e-04 / 4 here, 4.75e-05 measured at B = 4).  What it lets through at the B = 4 scale, and what it does not:
  (a) accepted (0.2 * max|dpred1| = 7.5e-06 < 1e-5); rejected at B = 1 (3.0e-05);
  (b) accepted on the auxiliary head (error 5.0e-06), REJECTED on the main head (4.2e-05; 2.0e-05 / 1.7e-04 at B = 1);
  (c) accepted when the term is dropped from the auxiliary head (rejected at B = 1), REJECTED when it is dropped from the main head (3.3e-05).
So the old bar does see the main head's (b) and (c) at this size; it is blind to all three on the auxiliary head, whose gradient carries
lambda_seg = 0.1.  The new bar rejects every one of them at every size.
"""
import pytest
import torch

import _head_bar as hb
from oracle import simt_oracle as so

CD = so.load_class_dist()
BF = torch.bfloat16
K = 3
GEOMS = {"up8_two_chunks": ((2, 13, 37, 97, 289), 8), "rows6": ((4, 97, 3, 768, 16), 8), "prod_b1": ((1, 97, 97, 768, 768), 16)}
D = dict(hb.DEFAULT_D, K=K)


def _row(geom):
    return geom[3] // 2 + 1          # an image row in the middle (of the second row group at rows6)


def _refs(name):
    geom, block = GEOMS[name]
    inp = hb.head_inputs(geom, K, CD, block)

    def make():
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        r64, r32 = hb.two_head_ref(*inp, D, CD, torch.float64), hb.two_head_ref(*inp, D, CD, torch.float32)
        # (c): total - lambda_place * unknown of the main head
        noterm = hb.two_head_ref(*inp, D, CD, torch.float64, total_of=lambda out, hp: out["total"] - hp.lambda_place * out["unknown2"])
        noterm1 = hb.two_head_ref(*inp, D, CD, torch.float64,
                                  total_of=lambda out, hp: out["total"] - hp.lambda_seg * hp.lambda_place * out["unknown1"])
        noterm["dpred1_aux"] = noterm1["dpred1"]
        assert torch.equal(noterm1["dpred2"], r64["dpred2"])
        # (b): the same oracle with one image row's labels ignored and its confidence labels masked out
        y = _row(geom)
        lab = inp[3].clone()
        lab[:, y, :] = 255
        orig = so.confidence_labels

        def masked(fixed_lr2, size, hp):
            conf0, flat = orig(fixed_lr2, size, hp)
            conf0 = conf0.clone()
            conf0[:, y, :] = 255
            return conf0, flat
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(so, "confidence_labels", masked)
            norow = hb.two_head_ref(inp[0], inp[1], inp[2], lab, inp[4], D, CD, torch.float64)
        return r64, r32, noterm, norow
    return hb.cached(("cpu", name), make)


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("name", list(GEOMS))
def test_bar_accepts_the_fp32_oracle(name):
    r64, r32, _t, _r = _refs(name)
    assert torch.equal(r64["out"]["conf"], r32["out"]["conf"])
    for k in ("dpred1", "dpred2", "ntm_grad1", "ntm_grad2"):
        res = hb.grad_bar(r32[k], r64[k], r32[k], f"{name} {k}")
        hb.report(name, k, res)
        assert res["outliers"] == 0 and res["worst"] <= 1.0
        assert res["excluded"] <= hb.CAP * res["n"]
    for gscale in (1.0, 0.5):
        for k in ("dpred1", "dpred2"):
            g32 = (r32[k] * gscale).float()
            res = hb.bf16_bar(g32.to(BF), r64[k], r32[k], f"{name} {k} bf16", gscale, got_f32=g32)
            hb.report(name, f"{k} gscale {gscale}", res)
            assert res["exact"] == res["exact_ref"]
            hb.bf16_bar(g32.to(BF), r64[k], r32[k], f"{name} {k} bf16 alone", gscale)          # (without the fp32 companion)


def _at_b4(fn):
    """fn(scale) at the B = 1 scale and at the benchmarked B = 4 scale (module docstring)."""
    return fn(1.0), fn(0.25)


@pytest.mark.parametrize("name", list(GEOMS))
def test_bar_rejects_a_scaled_auxiliary_head(name):
    r64, r32, _t, _r = _refs(name)
    ref, f32 = r64["dpred1"], r32["dpred1"]
    for c in (1.0, 0.25):
        _rejected(lambda: hb.grad_bar(ref * c * 0.8, ref * c, f32 * c, "(a)"))
        _rejected(lambda: hb.grad_bar(ref * c * 1.2, ref * c, f32 * c, "(a) +20 %"))
    if name == "prod_b1":
        assert _at_b4(lambda c: hb.old_close_ok(ref * c * 0.8, ref * c, 1e-5)) == (False, True)


@pytest.mark.parametrize("name", list(GEOMS))
def test_bar_rejects_a_dropped_image_row(name):
    r64, r32, _t, norow = _refs(name)
    for k in ("dpred1", "dpred2"):
        assert not torch.equal(norow[k], r64[k])
        for c in (1.0, 0.25):
            _rejected(lambda: hb.grad_bar(norow[k] * c, r64[k] * c, r32[k] * c, f"(b) {k}"))
    if name == "prod_b1":
        # the old bar: blind on the auxiliary head at the B = 4 scale; it does reject the main head's (module docstring)
        assert _at_b4(lambda c: hb.old_close_ok(norow["dpred1"] * c, r64["dpred1"] * c, 1e-5)) == (False, True)
        assert _at_b4(lambda c: hb.old_close_ok(norow["dpred2"] * c, r64["dpred2"] * c, 1e-5)) == (False, False)


@pytest.mark.parametrize("name", list(GEOMS))
def test_bar_rejects_a_dropped_loss_term(name):
    r64, r32, noterm, _r = _refs(name)
    assert torch.equal(noterm["dpred1"], r64["dpred1"])          # the main head's term belongs to the main head alone
    for c in (1.0, 0.25):
        _rejected(lambda: hb.grad_bar(noterm["dpred2"] * c, r64["dpred2"] * c, r32["dpred2"] * c, "(c) main head"))
        _rejected(lambda: hb.grad_bar(noterm["dpred1_aux"] * c, r64["dpred1"] * c, r32["dpred1"] * c, "(c) auxiliary head"))
    if name == "prod_b1":
        # the old bar: blind to the auxiliary head's missing term at the B = 4 scale; it does reject the main head's (module docstring)
        assert _at_b4(lambda c: hb.old_close_ok(noterm["dpred1_aux"] * c, r64["dpred1"] * c, 1e-5)) == (False, True)
        assert _at_b4(lambda c: hb.old_close_ok(noterm["dpred2"] * c, r64["dpred2"] * c, 1e-5)) == (False, False)


@pytest.mark.parametrize("name", list(GEOMS))
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_bf16_bar_rejects_two_ulps_on_one_element(name, gscale):
    r64, r32, _t, _r = _refs(name)
    for k in ("dpred1", "dpred2"):
        g32 = (r32[k] * gscale).float()
        gb = g32.to(BF)
        mant = gb.view(torch.int16) & 0x7F
        # a held element of ordinary size, its bf16 mantissa away from a binade edge (two steps down from 2^k are ONE ulp of 2^k)
        ok = ~hb.measure(r64[k], r32[k])["excl"] & (r64[k].abs() > r64[k].pow(2).mean().sqrt()) & (mant >= 16) & (mant < 112)
        pos = tuple(ok.nonzero()[ok.nonzero().shape[0] // 2].tolist())
        for step in (2, -2):
            mut = gb.clone()
            mut[pos] = (mut[pos].view(torch.int16) + step).view(BF)           # two neighbours up / down in bf16
            _rejected(lambda: hb.bf16_bar(mut, r64[k], r32[k], f"(d) {k}", gscale, got_f32=g32))
            _rejected(lambda: hb.bf16_bar(mut, r64[k], r32[k], f"(d) {k}, bf16 alone", gscale))


@pytest.mark.parametrize("name", list(GEOMS))
def test_bar_rejects_a_shifted_low_res_column(name):
    r64, r32, _t, _r = _refs(name)
    w = GEOMS[name][0][2]
    for k in ("dpred1", "dpred2"):
        for x in (0, w // 2, w - 2):
            mut = r64[k].clone()
            mut[..., x] = r64[k][..., x + 1]
            _rejected(lambda: hb.grad_bar(mut, r64[k], r32[k], f"(e) {k} column {x}"))
            _rejected(lambda: hb.bf16_bar(mut.float().to(BF), r64[k], r32[k], f"(e) {k} column {x} bf16"))


def test_bar_holds_nan_and_the_cap():
    r64, r32, _t, _r = _refs("up8_two_chunks")
    g = r32["dpred2"].clone()
    g[0, 0, 0, 0] = float("nan")
    _rejected(lambda: hb.grad_bar(g, r64["dpred2"], r32["dpred2"], "NaN"))
    # a handful of small decision flips passes, one element more than the cap does not
    ref = r64["dpred2"]
    n = ref.numel()
    nflip = int(hb.CAP * n)
    s = ref.abs() + ref.pow(2).mean().sqrt()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    g = r32["dpred2"].double().clone().reshape(-1)
    bump = (1e-3 * s).reshape(-1).clamp_max(0.5 * hb.OLD_TOL)
    g[idx[:nflip]] += bump[idx[:nflip]]
    res = hb.grad_bar(g.view_as(ref), ref, r32["dpred2"], "flips at the cap")
    assert res["outliers"] == nflip
    g[idx[nflip]] += bump[idx[nflip]]
    _rejected(lambda: hb.grad_bar(g.view_as(ref), ref, r32["dpred2"], "one flip over the cap"))
    # ... and an excused element that misses the old absolute bar is not excused
    g = r32["dpred2"].double().clone()
    g[0, 0, 0, 0] += 3 * hb.OLD_TOL
    _rejected(lambda: hb.grad_bar(g, ref, r32["dpred2"], "a large outlier"))
