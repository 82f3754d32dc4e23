"""The ImageNet feature distance on the GPU (simt_feat_dist_mask / simt_feat_dist / simt_feat_dist_finalize in csrc/feat_dist.hip,
TrunkPlan(feat_grad_seed=True), the keywords feat_dist* of WarmupTrainer, --feat-dist of trainV1_warmup).  The yardsticks are the restatement
and the float64 oracle of tests/_feat_dist_ref.py and the trainers without the keyword, never the code under test:

  (a) the mask launch, bit for bit against the restatement, with equal N;
  (b) the distance launch and the finalize against the restatement in float64 under derived bars, the exact properties, the refusals;
  (c) the plan: a seeded plan with the seed switched off equals a plan without the keyword bit for bit, a zero seed changes no value, a
      plan without the keyword has no new launch or buffer, a head-less eval plan builds;
  (d) the trainer against the float64 oracle;
  (e) the trainers bit for bit: lambda = 0, the target pass under online_source, iter_size 2, a one-rank RCCL group, resume, refusals;
  (f) the tool."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _feat_dist_ref as fr
import test_gpu_online_labels as OL
import test_gpu_resume as R
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from simt_amd.engine import TrunkPlan, multi_heads
from simt_amd.step import Hyper, WarmupTrainer
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
CD = so.load_class_dist()
THINGS = fr.DEFAULT_CLASSES
PORT = 29613


def _word(classes):
    return sum(1 << c for c in classes)


# ---- (a) the mask launch ---------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(2, 65, 129, 9, 17), (2, 64, 64, 8, 8), (1, 65, 97, 3, 5), (1, 9, 17, 9, 17), (1, 8, 16, 4, 4), (3, 40, 24, 40, 3)]
MASK_CLASSES = (0, 6, 13, 18, 63)


def _first_count_at(ratio, n):
    """The smallest pixel count the contract keeps in a window of n pixels."""
    bar = np.float32(ratio) * np.float32(n)
    return next(k for k in range(n + 1) if np.float32(k) >= bar)


def _labels(B, H, W, h, w, ratio, seed):
    """Blocks of the size of a window, of classes inside and outside the set, 255, 19 ... 254 and negative values; bands of 255; item 0
    carries a window exactly at the ratio and one a pixel under it (6 of 8 and 48 of 64 at 0.75 where the windows have 8 and 64 pixels)."""
    g = np.random.default_rng(seed)
    values = np.array([0, 0, 6, 6, 13, 13, 18, 63, 63, 1, 2, 255, 19, 64, 254, 100, -1, -255], dtype=np.int64)
    rows, cols = fr.windows(H, h), fr.windows(W, w)
    lab = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        for (r0, r1) in rows:
            for (c0, c1) in cols:
                lab[b, r0:r1, c0:c1] = values[g.integers(0, len(values))]
    noise = g.random((B, H, W)) < 0.1
    lab[noise] = values[g.integers(0, len(values), int(noise.sum()))]
    lab[:, H // 2] = 255
    lab[:, :, W // 3] = 255
    planted = []
    cells = [(i, j) for i in range(h) for j in range(w)]
    for k, (i, j) in enumerate(cells[:: max(1, len(cells) // 6)][:6]):
        (r0, r1), (c0, c1) = rows[i], cols[j]
        n = (r1 - r0) * (c1 - c0)
        need = _first_count_at(ratio, n)
        count = need if k % 2 == 0 else need - 1
        win = np.full(n, 1 if k % 3 else 255, dtype=np.int64)
        win[g.permutation(n)[:count]] = MASK_CLASSES[k % len(MASK_CLASSES)]
        lab[0, r0:r1, c0:c1] = win.reshape(r1 - r0, c1 - c0)
        planted.append((i * w + j, count >= need and count > 0, count, n))
    return lab, planted


def _mask_launch(dev, lab, h, w, classes, ratio):
    B, H, W = lab.shape
    n = L.load().simt_feat_dist_mask_parts(B, h, w)
    assert n == -(-B * h * w // 32)
    mask = torch.full((B * h * w + 16,), 0xEE, dtype=torch.uint8, device=dev)
    part = torch.full((n + 4,), -7, dtype=torch.int32, device=dev)
    labd = torch.from_numpy(lab).to(dev)
    d = L.FeatDistMaskDesc()
    d.label, d.mask, d.part, d.classes = labd.data_ptr(), mask.data_ptr(), part.data_ptr(), _word(classes)
    d.B, d.H, d.W, d.h, d.w, d.min_ratio = B, H, W, h, w, ratio
    L.call("simt_feat_dist_mask", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((mask[B * h * w:] == 0xEE).all()) and bool((part[n:] == -7).all()), "guard words written"
    assert torch.equal(labd.cpu(), torch.from_numpy(lab)), "the labels were written"
    return mask[:B * h * w].cpu().numpy(), part[:n].cpu().numpy()


@pytest.mark.parametrize("ratio", [0.75, 1.0, 0.51])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "B{}-{}x{}-{}x{}".format(*g))
def test_mask_equals_the_restatement(dev, geo, ratio):
    B, H, W, h, w = geo
    lab, planted = _labels(B, H, W, h, w, ratio, seed=H + 7 * w)
    want, N = fr.mask_ref(lab, h, w, MASK_CLASSES, ratio)
    for cell, kept, count, n in planted:
        assert want[cell] == (1 if kept else 0), (cell, count, n)
    if ratio == 0.75 and (H // h, W // w) in ((8, 8), (2, 4)):
        assert any((count, n) in ((48, 64), (6, 8)) and kept for _c, kept, count, n in planted)
        assert any((count, n) in ((47, 64), (5, 8)) and not kept for _c, kept, count, n in planted)
    got, part = _mask_launch(dev, lab, h, w, MASK_CLASSES, ratio)
    assert (got == want).all(), f"{int((got != want).sum())} of {want.size} cells differ"
    assert int(part.sum()) == N and 0 < N < want.size
    assert (part == np.add.reduceat(want.astype(np.int64), np.arange(0, want.size, 32))).all()
    # the default set: the classes 0 and 63 no longer count
    want2, N2 = fr.mask_ref(lab, h, w, THINGS, ratio)
    got2, part2 = _mask_launch(dev, lab, h, w, THINGS, ratio)
    assert (got2 == want2).all() and int(part2.sum()) == N2 and N2 < N


def test_mask_of_labels_without_a_thing_class(dev):
    B, H, W, h, w = GEOMETRIES[0]
    for fill in (255, -1, 64, 1):
        lab = np.full((B, H, W), fill, dtype=np.int64)
        got, part = _mask_launch(dev, lab, h, w, THINGS, 0.75)
        assert not got.any() and not part.any()
    lab = np.full((B, H, W), 13, dtype=np.int64)
    lab[1] = 255                                         # an all-ignore item beside a full one
    got, part = _mask_launch(dev, lab, h, w, THINGS, 1.0)
    assert got[:h * w].all() and not got[h * w:].any() and int(part.sum()) == h * w


def test_mask_refusals_write_nothing(dev):
    B, H, W, h, w = 2, 16, 24, 4, 6
    lab = torch.zeros(B * H * W + 1, dtype=torch.int64, device=dev)
    mask = torch.full((B * h * w,), 0xEE, dtype=torch.uint8, device=dev)
    part = torch.full((4,), -7, dtype=torch.int32, device=dev)

    def desc(**kw):
        d = L.FeatDistMaskDesc()
        d.label, d.mask, d.part, d.classes = lab.data_ptr(), mask.data_ptr(), part.data_ptr(), _word(THINGS)
        d.B, d.H, d.W, d.h, d.w, d.min_ratio = B, H, W, h, w, 0.75
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [desc(label=None), desc(mask=None), desc(part=None), desc(h=H + 1), desc(w=W + 1), desc(min_ratio=0.5), desc(min_ratio=1.5),
           desc(min_ratio=float("nan")), desc(min_ratio=-1.0), desc(B=0), desc(h=0), desc(w=0), desc(H=0), desc(label=lab.data_ptr() + 4),
           desc(part=part.data_ptr() + 2)]
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_feat_dist_mask", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_feat_dist_mask", None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((mask == 0xEE).all()) and bool((part == -7).all())
    assert L.load().simt_feat_dist_mask_parts(0, 4, 4) == 0 and L.load().simt_feat_dist_parts(0) == 0
    L.call("simt_feat_dist_mask", C.byref(desc()), ops.stream_ptr())          # the descriptor itself is sound
    torch.cuda.synchronize()
    assert bool((mask == 0).all()) and part[:2].tolist() == [0, 0] and part[2:].tolist() == [-7, -7]


# ---- (b) distance, seed, scalars -------------------------------------------------------------------------------------------------------------------
# (M, C): 2 * 9 * 17 rows and 2 * 34 * 34 (about 2 * 97 * 97 / 8) at C = 256 and 2048; C = 264: a last chunk of 8 elements on one lane only;
# M = 4133: more rows than the launch has waves (4 * 1024), a wave loops; C = 4104: beyond 2048, the path that reads the row twice
SIZES = [(306, 256), (306, 2048), (2312, 256), (2312, 2048), (306, 264), (4133, 256), (64, 4104)]
LAM = 0.005


def _features(M, Cn, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    fs = (torch.randn(M, Cn, generator=g) * 1.5).to(dtype)
    fi = (fs.float() + torch.randn(M, Cn, generator=g) * 0.7).to(dtype)
    mask = (torch.rand(M, generator=g) < 0.4).to(torch.uint8)
    mask[:6] = torch.tensor([1, 0, 1, 0, 1, 1], dtype=torch.uint8)
    fi[2] = fs[2]                                        # a kept row at distance 0
    for t in (fs, fi):                                   # rows that are not kept are never read
        t[1] = float("nan")
        t[3] = float("inf")
    fs[3, ::2] = float("-inf")
    return fs, fi, mask


class _Launch:
    """The buffers and the descriptor of the two launches over given features; run() -> (seed, d, part, out) on the host."""

    def __init__(self, dev, fs, fi, mask, lam=LAM, gscale=1.0, split=3):
        self.dev, self.M, self.Cn, self.dtype = dev, fs.shape[0], fs.shape[1], fs.dtype
        self.fs, self.fi, self.mask = fs.to(dev).contiguous(), fi.to(dev).contiguous(), mask.to(dev)
        N = int(mask.sum())
        kp = [N - N // 2, 0, N // 2][:split]
        self.kept = torch.tensor(kp if split == 3 else [N], dtype=torch.int32, device=dev)
        self.nparts = L.load().simt_feat_dist_parts(self.M)
        assert self.nparts == min(-(-self.M // 4), 1024)
        self.seed = torch.empty(self.M * self.Cn + 16, dtype=fs.dtype, device=dev)
        self.d = torch.empty(self.M + 4, device=dev)
        self.part = torch.empty(self.nparts + 4, device=dev)
        self.out = torch.empty(3 + 4, device=dev)
        self.desc = self.make(lam, gscale)

    def make(self, lam, gscale, **kw):
        d = L.FeatDistDesc()
        d.fs, d.fi, d.mask, d.kept_part = self.fs.data_ptr(), self.fi.data_ptr(), self.mask.data_ptr(), self.kept.data_ptr()
        d.seed, d.d, d.part, d.out = self.seed.data_ptr(), self.d.data_ptr(), self.part.data_ptr(), self.out.data_ptr()
        d.lam, d.M, d.C, d.ld, d.dtype, d.n_kept_part = lam, self.M, self.Cn, self.Cn, ops.dt_code(self.dtype), self.kept.numel()
        d.lam_g = lam * gscale
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def poison(self):
        _bits(self.seed).fill_(_nan_bits(self.dtype))
        self.d.fill_(-3.0)
        self.part.fill_(-3.0)
        self.out.fill_(-3.0)

    def run(self, desc=None, finalize=True):
        self.poison()
        d = desc or self.desc
        L.call("simt_feat_dist", C.byref(d), ops.stream_ptr())
        if finalize:
            L.call("simt_feat_dist_finalize", C.byref(d), ops.stream_ptr())
        torch.cuda.synchronize()
        n = self.M * self.Cn
        assert bool((_bits(self.seed[n:]) == _nan_bits(self.dtype)).all())
        assert bool((self.d[self.M:] == -3).all()) and bool((self.part[self.nparts:] == -3).all()) and bool((self.out[3:] == -3).all()), "guards"
        return self.seed[:n].view(self.M, self.Cn).cpu(), self.d[:self.M].cpu(), self.part[:self.nparts].cpu(), self.out[:3].cpu()


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _nan_bits(dtype):
    """A NaN pattern no launch produces: the poison of the output buffers."""
    return 0x7FC1 if dtype == BF else 0x7FC00001


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "M{}-C{}".format(*s))
def test_distance_and_seed_vs_float64(dev, size, dtype):
    M, Cn = size
    fs, fi, mask = _features(M, Cn, dtype, seed=M + Cn)
    ref = fr.dist_ref(fs.double().numpy(), fi.double().numpy(), mask.numpy(), LAM, 1.0)
    assert 0 < ref["N"] < M
    run = _Launch(dev, fs, fi, mask)
    seed, d, part, out = run.run()
    print(f"[feat_dist] M {M} C {Cn} {dtype}: N {ref['N']} out {out.tolist()} float64 {ref['out'].tolist()}")
    fr.check_d(d.double().numpy(), ref, mask.numpy(), Cn)
    fr.check_seed(seed.double().numpy(), ref, mask.numpy(), Cn, dtype == BF)
    fr.check_scalars(out.double().numpy(), ref, M, Cn)
    assert float(d[2]) == 0.0 and not bool(_bits(seed[2]).any()), "a kept row with fs == fi"
    for m in (1, 3):
        assert float(d[m]) == 0.0 and not bool(_bits(seed[m]).any()), "a row that is not kept, NaN / Inf in both maps"
    assert not bool(_bits(seed[mask == 0]).any()), "a row that is not kept is not +0"
    assert abs(float(part.double().sum()) - ref["S"]) <= (Cn + 5 + -(-M // 4)) * fr.EPS24 * ref["S"]
    # a second launch repeats the first bit for bit
    seed2, d2, part2, out2 = run.run()
    assert torch.equal(_bits(seed), _bits(seed2)) and torch.equal(d.view(torch.int32), d2.view(torch.int32))
    assert torch.equal(part.view(torch.int32), part2.view(torch.int32)) and torch.equal(out.view(torch.int32), out2.view(torch.int32))
    # N is the SUM of the mask launch's partials, however they are split
    one = _Launch(dev, fs, fi, mask, split=1)
    seed1, d1, _p, out1 = one.run()
    assert torch.equal(_bits(seed), _bits(seed1)) and torch.equal(out.view(torch.int32), out1.view(torch.int32))
    # doubling lambda, halving gscale: exactly the power of two
    twice, _d, _p, out_t = run.run(run.make(2 * LAM, 1.0))
    assert torch.equal(twice.float(), 2 * seed.float()) and float(out_t[0]) == 2 * float(out[0]) and float(out_t[1]) == float(out[1])
    half, _d, _p, out_h = run.run(run.make(LAM, 0.5))
    assert torch.equal(half.float(), 0.5 * seed.float()) and torch.equal(out_h.view(torch.int32), out.view(torch.int32))
    assert bool((seed.float() != 0).any())


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_no_kept_cell(dev, dtype):
    M, Cn = SIZES[0]
    fs, fi, mask = _features(M, Cn, dtype, seed=5)
    run = _Launch(dev, fs, fi, torch.zeros_like(mask))
    seed, d, part, out = run.run()
    assert out.tolist() == [0.0, 0.0, 0.0] and not bool(_bits(seed).any()) and not bool(d.any()) and not bool(part.any())


def test_distance_refusals_write_nothing(dev):
    M, Cn = 64, 256
    fs, fi, mask = _features(M, Cn, BF, seed=9)
    run = _Launch(dev, fs, fi, mask)
    run.poison()
    before = [t.clone() for t in (run.seed, run.d, run.part, run.out)]
    m = run.make
    bad = [m(LAM, 1.0, **{k: None}) for k in ("fs", "fi", "mask", "kept_part", "seed", "d", "part", "out")]
    bad += [m(LAM, 1.0, C=Cn - 4), m(LAM, 1.0, C=0), m(LAM, 1.0, ld=Cn + 8), m(LAM, 1.0, dtype=2), m(LAM, 1.0, dtype=-1), m(LAM, 1.0, M=0),
            m(LAM, 1.0, n_kept_part=0), m(LAM, 1.0, fs=run.fs.data_ptr() + 8), m(LAM, 1.0, fi=run.fi.data_ptr() + 2),
            m(LAM, 1.0, seed=run.seed.data_ptr() + 8), m(LAM, 1.0, d=run.d.data_ptr() + 2), m(float("nan"), 1.0)]
    for name in ("simt_feat_dist", "simt_feat_dist_finalize"):
        for d in bad:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(d), ops.stream_ptr())
        with pytest.raises(L.SimtHipError):
            L.call(name, None, ops.stream_ptr())
    torch.cuda.synchronize()
    for t, b in zip((run.seed, run.d, run.part, run.out), before):
        assert torch.equal(_bits(t), _bits(b))


# ---- (c) the plan ----------------------------------------------------------------------------------------------------------------------------------
SIZE = OL.SIZE          # (2, 65, 129)
SMALL = R.SMALL         # (1, 1, 2, 1): layer 4 is one block with a downsample branch
DEEP4 = (1, 1, 1, 2)    # layer 4 ends in an identity block: the head's launch also makes the first pass of bn3's backward


def _plan(dev, dtype, layers, **kw):
    st = so.recipe_state(so.state_shapes(19, 0, False, layers=layers), seed=41, head_scale=8.0)
    params = {k: v.detach().to(dev, torch.long if v.dtype == torch.long else F32).clone() for k, v in st.items()}
    return TrunkPlan(params, *SIZE, multi_heads(19, 0, False), dtype=dtype, train=True, layers=layers, **kw)


def _backward(plan, x, dl):
    plan.forward(x)
    for k, t in dl.items():
        plan.dlogits[k].copy_(t)
    plan.backward()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in plan.grads.items()}


@pytest.mark.parametrize("layers", [SMALL, DEEP4], ids=["small", "identity-last"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_seeded_plan(dev, dtype, layers):
    B, H, W = SIZE
    plain, seeded, default = _plan(dev, dtype, layers), _plan(dev, dtype, layers, feat_grad_seed=True), _plan(dev, dtype, layers, feat_grad_seed=False)
    # without the keyword: the plan it was -- no new launch, tag or buffer
    for name in ("fwd_list", "bwd_list", "pack_list"):
        assert [it.tag for it in getattr(default, name).items] == [it.tag for it in getattr(plain, name).items]
        assert len(getattr(seeded, name).items) == len(getattr(plain, name).items), "the seed needs no launch of its own"
    assert default.bytes_allocated() == plain.bytes_allocated() and plain.feat_seed is None and plain.feat_seed_desc is None
    with pytest.raises(ValueError, match="feat_grad_seed"):
        plain.use_feat_seed(True)
    Mo, c4 = seeded.block_io[-1]["z"].shape
    assert seeded.feat_seed.shape == (Mo, c4) and seeded.feat_seed.dtype == dtype and c4 == 2048 and not bool(seeded.feat_seed.any())
    assert seeded.bytes_allocated() == plain.bytes_allocated() + Mo * c4 * seeded.esz
    assert seeded.feat_seed_desc.res == seeded.feat_seed.data_ptr()
    x, _lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=17, block=8)
    x = x.to(dev)
    g = torch.Generator().manual_seed(3)
    dl = {k: (torch.randn(t.shape, generator=g) * 1e-3).to(dev).to(t.dtype) for k, t in plain.dlogits.items()}
    for k, t in dl.items():
        t[:, 19:] = 0          # the K padding of the head's gradient stays zero
    want = _backward(plain, x, dl)
    seeded.use_feat_seed(False)
    assert seeded.feat_seed_desc.res is None
    got = _backward(seeded, x, dl)
    bad = [k for k in want if not torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))]
    assert not bad, f"seed off: {len(bad)} of {len(want)} gradients differ: {bad[:6]}"
    seeded.use_feat_seed(True)          # a zero seed: equal as values
    for k, p in plain.p.items():        # (the train-mode forward moved the running statistics: both plans start the second pass alike)
        seeded.p[k].copy_(p)
    want2 = _backward(plain, x, dl)
    got2 = _backward(seeded, x, dl)
    bad = [k for k in want2 if not torch.equal(got2[k], want2[k])]
    assert not bad, f"zero seed: {len(bad)} of {len(want2)} gradients differ: {bad[:6]}"
    # a seed arrives: trunk gradients move, the heads' do not (theirs come from the logits alone)
    seeded.feat_seed.copy_((torch.randn(Mo, c4, generator=g) * 1e-4).to(dev))
    for k, p in plain.p.items():
        seeded.p[k].copy_(p)
    want3 = _backward(plain, x, dl)
    got3 = _backward(seeded, x, dl)
    heads = [k for k in want3 if k.startswith(("layer5", "layer6"))]
    assert heads and all(torch.equal(got3[k], want3[k]) for k in heads)
    moved = [k for k in want3 if k not in heads and not torch.equal(got3[k], want3[k])]
    assert len(moved) == len(want3) - len(heads), "the seed did not reach every trunk gradient"
    assert all(bool(torch.isfinite(v).all()) for v in got3.values())


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_eval_plan_without_heads(dev, dtype):
    B, H, W = SIZE
    st = so.recipe_state(so.state_shapes(19, 0, False, layers=SMALL), seed=43, head_scale=8.0)
    params = {k: v.detach().to(dev, torch.long if v.dtype == torch.long else F32).clone() for k, v in st.items()}
    trunk_only = {k: v for k, v in params.items() if not k.startswith(("layer5", "layer6"))}
    bare = TrunkPlan(trunk_only, B, H, W, [], dtype=dtype, train=False, layers=SMALL)
    full = TrunkPlan(params, B, H, W, multi_heads(19, 0, False), dtype=dtype, train=False, layers=SMALL)
    assert bare.out == {} and len(bare.fwd_list.items) < len(full.fwd_list.items)
    x, _lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=19, block=8)
    for k in range(2):          # rebuilt by every forward
        bare.forward((x * (k + 1)).to(dev))
        full.forward((x * (k + 1)).to(dev))
        torch.cuda.synchronize()
        z, zf = bare.block_io[-1]["z"], full.block_io[-1]["z"]
        assert z.shape == (B * bare.feat_hw[0] * bare.feat_hw[1], 2048) and z.dtype == dtype and torch.equal(z, zf) and bool(z.any())
    with pytest.raises(ValueError, match="feat_grad_seed needs a train plan"):
        TrunkPlan(trunk_only, B, H, W, [], dtype=dtype, train=False, layers=SMALL, feat_grad_seed=True)


# ---- (d) the trainer against the float64 oracle ---------------------------------------------------------------------------------------------------
ORACLE_LAYERS = (1, 1, 2, 1)
ORACLE_KEYS = ("conv1.weight", "layer1.0.conv2.weight", "layer3.1.conv3.weight", "layer6.conv2d_list.1.weight", "layer5.conv2d_list.0.bias")
# lambda = 1: on the CPU, with the two oracles, the float64 step WITHOUT the term misses the bar of the step with it on all five tensors (by 6x on
# conv1.weight, 2x on layer3.1.conv3.weight), so a trainer whose gradient did not arrive could not pass; at DAFormer's 0.005 it would
ORACLE_LAM = 1.0


def _oracle_states():
    st = so.recipe_state(so.state_shapes(19, 0, False, layers=ORACLE_LAYERS), seed=77, head_scale=8.0)
    im = so.recipe_state(so.state_shapes(19, 0, False, layers=ORACLE_LAYERS), seed=78, head_scale=8.0)
    return st, {k: v for k, v in im.items() if not k.startswith(("layer5", "layer6"))}


def test_trainer_vs_float64_oracle(dev):
    st, im = _oracle_states()
    B, H, W = 2, 97, 97
    data = [so.synthetic_batch(B, H, W, CD.numpy(), seed=500 + j, block=16) for j in range(2)]
    hp = dict(open_classes=0, lr=2.5e-4)
    tr = WarmupTrainer(st, Hyper(**hp), B, H, W, dtype=F32, device=dev, layers=ORACLE_LAYERS, feat_dist=ORACLE_LAM, feat_dist_state=im)
    o64 = fr.OracleFeatDistTrainer(st, so.Hyper(**hp), im, ORACLE_LAM, layers=ORACLE_LAYERS, dtype=torch.float64)
    o32 = fr.OracleFeatDistTrainer(st, so.Hyper(**hp), im, ORACLE_LAM, layers=ORACLE_LAYERS)
    plain = so.OracleWarmupTrainer(st, so.Hyper(**hp), layers=ORACLE_LAYERS, dtype=torch.float64)
    for it, (x, lab) in enumerate(data):
        tr.step(x.to(dev), lab.to(dev), it)
        want = o64.step(x, lab, it)
        o32.step(x, lab, it)
        plain.step(x, lab, it)
        l = tr.losses()
        print(f"[feat_dist] step {it}: {l}; float64 total {float(want['total'])!r} feat_dist {float(want['feat_dist'])!r} cells {want['cells']}")
        assert l["feat_dist_cells"] == want["cells"] and 0 < want["cells"] < B * tr.h * tr.w
        assert abs(l["feat_dist"] - float(want["feat_dist"])) < 1e-4 * abs(float(want["feat_dist"])), (l, want)
        assert abs(l["total"] - float(want["total"])) < 1e-4 * abs(float(want["total"])), (l, want)
    missed = []
    for k in ORACLE_KEYS:
        v, p64 = tr.params[k].detach().cpu().double(), o64.st[k].detach()
        e_ref = (o32.st[k].detach().double() - p64).abs().max().item()
        err = (v - p64).abs().max().item()
        e_plain = (plain.st[k].detach() - p64).abs().max().item()
        print(f"[feat_dist] {k}: error {err:.3e}, fp32 oracle {e_ref:.3e}, the step without the term {e_plain:.3e}")
        assert err < 3 * e_ref + 5e-6, (k, err, e_ref)
        if e_plain >= 3 * e_ref + 5e-6:
            missed.append(k)
    assert set(missed) >= set(ORACLE_KEYS[:3]), f"the step without the term passes the bar on {set(ORACLE_KEYS[:3]) - set(missed)}: the case shows nothing"


def test_iter_size_2_matches_the_oracle(dev):
    st, im = _oracle_states()
    B, H, W = 2, 97, 97
    mb = [so.synthetic_batch(B, H, W, CD.numpy(), seed=520 + j, block=16) for j in range(2)]
    hp = dict(open_classes=0, lr=2.5e-4, iter_size=2)
    tr = WarmupTrainer(st, Hyper(**hp), B, H, W, dtype=F32, device=dev, layers=ORACLE_LAYERS, feat_dist=ORACLE_LAM, feat_dist_state=im)
    o64 = fr.OracleFeatDistTrainer(st, so.Hyper(**hp), im, ORACLE_LAM, layers=ORACLE_LAYERS, dtype=torch.float64)
    o32 = fr.OracleFeatDistTrainer(st, so.Hyper(**hp), im, ORACLE_LAM, layers=ORACLE_LAYERS)
    tr.step([m[0].to(dev) for m in mb], [m[1].to(dev) for m in mb], 0)
    want = o64.step([m[0] for m in mb], [m[1] for m in mb], 0)
    o32.step([m[0] for m in mb], [m[1] for m in mb], 0)
    l = tr.losses()
    assert tr.fd_desc.lam_g == 0.5 and l["feat_dist_cells"] == want["cells"] > 0
    assert abs(l["feat_dist"] - float(want["feat_dist"])) < 1e-4 * abs(float(want["feat_dist"])), (l, want)
    assert abs(l["total"] - float(want["total"])) < 1e-4 * abs(float(want["total"])), (l, want)
    for k in ORACLE_KEYS:
        v, p64 = tr.params[k].detach().cpu().double(), o64.st[k].detach()
        e_ref = (o32.st[k].detach().double() - p64).abs().max().item()
        assert (v - p64).abs().max().item() < 3 * e_ref + 5e-6, (k, e_ref)


# ---- (e) the trainers, bit for bit ----------------------------------------------------------------------------------------------------------------
def _imnet(seed=9):
    st, _arch = OL._start("v2", seed)
    return {k: v for k, v in st.items() if not k.startswith(("layer5", "layer6"))}


def _labelled(dev, n, its=1, seed=800):
    B, H, W = SIZE
    out = []
    for i in range(n):
        mb = [so.synthetic_batch(B, H, W, CD.numpy(), seed=seed + 10 * i + j, block=16) for j in range(its)]
        out.append([(x.to(dev), lab.to(dev)) for x, lab in mb])
    return out


def _steps(tr, data, start=0):
    outs = []
    for mb in data[start:]:
        one = len(mb) == 1
        tr.step(mb[0][0] if one else [m[0] for m in mb], mb[0][1] if one else [m[1] for m in mb])
        torch.cuda.synchronize()
        outs.append((R.scalars(tr), tr.fd_out.clone().view(torch.int32) if getattr(tr, "feat_dist", None) is not None else None))
    return outs


def _same_state(a, b, what):
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ: {bad[:6]}"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_lambda_zero_is_the_trainer_without_the_keyword(dev, dtype):
    data = _labelled(dev, 3)
    plain = OL._trainer("v2", dev, dtype)
    assert plain.feat_dist is None and not hasattr(plain, "imnet") and plain.plan.feat_seed is None
    want = _steps(plain, data)
    tr = OL._trainer("v2", dev, dtype, feat_dist=0.0, feat_dist_state=_imnet())
    got = _steps(tr, data)
    l = tr.losses()
    assert l["feat_dist"] == 0.0 and l["feat_dist_cells"] > 0 and "feat_dist" not in plain.losses()
    assert all(torch.equal(a[0], b[0]) for a, b in zip(got, want)), "the head's scalars differ"
    bad = [k for k in plain.params if not torch.equal(plain.params[k], tr.params[k])]
    assert not bad, f"{len(bad)} of {len(plain.params)} parameters differ: {bad[:6]}"
    assert set(tr.state_dict()) == set(plain.state_dict()) and set(tr.mom) == set(plain.mom)
    if tr.ema is None:
        assert not any(k in tr.imnet_params and v.data_ptr() == tr.imnet_params[k].data_ptr() for k, v in tr.params.items())


def test_the_term_moves_the_trajectory(dev):
    data = _labelled(dev, 2)
    a, b = OL._trainer("v2", dev, BF), OL._trainer("v2", dev, BF, feat_dist=0.5, feat_dist_state=_imnet())
    _steps(a, data)
    _steps(b, data)
    assert b.losses()["feat_dist"] > 0
    heads = ("layer5", "layer6")
    assert any(not torch.equal(a.params[k], b.params[k]) for k in a.params if k.endswith("conv1.weight") and not k.startswith(heads))


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "plain"])
def test_target_pass_under_online_source_is_the_parents(dev, mix, monkeypatch):
    """Step 0: the labels, the input and the head's scalars of the TARGET pass equal the keyword-less online_source trainer's; the three
    launches run once, in the source pass, and the target pass's backward runs with the seed off."""
    B, H, W = SIZE
    views = OL._views(dev, 1)
    strong, weak = views[0][0]
    sx, sl = _labelled(dev, 1, seed=4000)[0][0]
    kw = dict(online_labels=0.0, online_source=True)
    if mix:
        kw.update(online_mix=0.5, online_mix_seed=11)
    outs = []
    for extra in ({}, dict(feat_dist=0.5, feat_dist_state=_imnet())):
        tr = OL._trainer("v2", dev, BF, **kw, **extra)
        calls = []
        real = L.call
        monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        tr.step(strong, None, teacher_image=weak, source_image=sx, source_label=sl)
        torch.cuda.synchronize()
        monkeypatch.setattr(L, "call", real)
        outs.append((tr.label.clone(), tr.plan.x_in.clone(), R.scalars(tr), tr.source_hout.clone(), calls, tr))
    (lab0, x0, s0, k0, calls0, _t0), (lab1, x1, s1, k1, calls1, tr1) = outs
    assert torch.equal(lab0, lab1) and torch.equal(x0.view(torch.int32), x1.view(torch.int32)) and torch.equal(s0, s1) and torch.equal(k0, k1)
    new = ("simt_feat_dist_mask", "simt_feat_dist", "simt_feat_dist_finalize")
    assert not set(calls0) & set(new) and [calls1.count(n) for n in new] == [1, 1, 1]
    assert calls1.index("simt_feat_dist_finalize") < min(i for i, n in enumerate(calls1) if n.startswith("simt_online_label")), "not in the source pass"
    assert tr1.plan.feat_seed_desc.res is None, "the target pass ran with the seed on"
    l = tr1.losses()
    assert l["feat_dist"] > 0 and 0 < l["feat_dist_cells"] < B * tr1.h * tr1.w and "source_seg2" in l


def test_one_rank_rccl_group(dev):
    data = _labelled(dev, 2)
    kw = dict(feat_dist=0.5, feat_dist_state=_imnet())
    alone = OL._trainer("v2", dev, BF, **kw)
    a = _steps(alone, data)
    with one_rank_group(dev, PORT) as pg:
        tr = OL._trainer("v2", dev, BF, pg, **kw)
        b = _steps(tr, data)
        state = OL._state(tr)
        del tr
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    _same_state(state, OL._state(alone), "one-rank RCCL group")


def test_resume_and_the_train_state_refusals(dev, tmp_path):
    data = _labelled(dev, 6)
    im = _imnet()
    kw = dict(feat_dist=0.5, feat_dist_state=im)
    whole = OL._trainer("v2", dev, BF, **kw)
    w = _steps(whole, data)
    first = OL._trainer("v2", dev, BF, **kw)
    h = _steps(first, data[:3])
    ts0 = first.training_state()
    hy = ts0["hyper"]
    assert hy["feat_dist"] == 0.5 and hy["feat_dist_classes"] == list(THINGS) and hy["feat_dist_min_ratio"] == 0.75
    assert hy["feat_dist_sha256"] == tsf.state_sha256(first.imnet_params) and "feat_dist_out" in ts0["accumulators"]
    assert not any(k.startswith("imnet") for k in ts0) and set(ts0["model"]) == set(whole.state_dict())
    path = str(tmp_path / "run.state")
    tsf.save(path, ts0, None, {"world": 1})
    ts, _k, _l = tsf.load(path)
    rest = OL._trainer("v2", dev, BF, seed=1, **kw)          # (other start weights: they are replaced)
    rest.load_training_state(ts)
    assert rest.it_done == 3 and torch.equal(rest.fd_out, first.fd_out) and rest.losses()["feat_dist"] == first.losses()["feat_dist"]
    r = _steps(rest, data, start=3)
    for (a0, a1), (b0, b1) in zip(h + r, w):
        assert torch.equal(a0, b0) and torch.equal(a1, b1)
    _same_state(OL._state(rest), OL._state(whole), "resumed after step 3")
    # refusals: the flag dropped, added, changed; another ImageNet file
    plain = OL._trainer("v2", dev, BF)
    assert "feat_dist" not in plain.training_state()["hyper"] and "feat_dist_out" not in plain.training_state()["accumulators"]
    with pytest.raises(ValueError, match=r"feat_dist \(state: 0\.5, this trainer: None\)"):
        plain.load_training_state(ts)
    with pytest.raises(ValueError, match=r"feat_dist \(state: None, this trainer: 0\.5\)"):
        rest.load_training_state(plain.training_state())
    for other, field in ((dict(kw, feat_dist=0.25), r"feat_dist \(state: 0\.5, this trainer: 0\.25\)"),
                         (dict(kw, feat_dist_classes=[11, 12]), r"feat_dist_classes \(state: \[6, 7, .*this trainer: \[11, 12\]\)"),
                         (dict(kw, feat_dist_min_ratio=0.9), r"feat_dist_min_ratio \(state: 0\.75, this trainer: 0\.9\)"),
                         (dict(kw, feat_dist_state=_imnet(10)), r"feat_dist_sha256 \(state: ")):
        tr = OL._trainer("v2", dev, BF, **other)
        with pytest.raises(ValueError, match=field):
            tr.load_training_state(ts)
        del tr


def test_trainer_refusals(dev):
    im = _imnet()
    with pytest.raises(ValueError, match="^feat_dist with online_labels needs online_source"):
        OL._trainer("v2", dev, BF, online_labels=0.5, feat_dist=0.005, feat_dist_state=im)
    with pytest.raises(ValueError, match="^feat_dist_state is required"):
        OL._trainer("v2", dev, BF, feat_dist=0.005)
    for model in ("v3", "vgg"):
        with pytest.raises(ValueError, match="^feat_dist: the ImageNet feature distance is built for DeepLab-v2"):
            OL._trainer(model, dev, BF, feat_dist=0.005, feat_dist_state=im)


# ---- (f) the tool ----------------------------------------------------------------------------------------------------------------------------------
def _data_sets(root):
    """A four-image GTA5-shaped source set (images/, labels/ with GTA5 ids; thing classes in large blocks) and a four-image target set listed
    by image alone; frames of 160 x 96, so the loaders resize."""
    from PIL import Image
    g = np.random.default_rng(3)
    ids = np.array([7, 8, 11, 24, 24, 26, 26, 26, 33, 32, 1, 255], dtype=np.uint8)          # road, sidewalk, building, person, car, bicycle, ...
    for sub in ("source/images", "source/labels", "target/leftImg8bit"):
        os.makedirs(root / sub)
    names = [f"{n:05d}.png" for n in range(4)]
    for name in names:
        blocks = ids[g.integers(0, len(ids), (3, 4))]
        Image.fromarray(np.kron(blocks, np.ones((32, 40), dtype=np.uint8))).save(root / "source/labels" / name)
        colour = (blocks[..., None].astype(np.int64) * np.array([37, 91, 53]) % 256).astype(np.uint8)
        noise = g.integers(0, 40, (96, 160, 3), dtype=np.uint8)
        Image.fromarray(np.kron(colour, np.ones((32, 40, 1), dtype=np.uint8)) // 2 + noise).save(root / "source/images" / name)
        Image.fromarray(g.integers(0, 256, (6, 8, 3), dtype=np.uint8).repeat(16, 0).repeat(20, 1) // 2 + noise).save(root / "target/leftImg8bit" / name)
    open(root / "source.txt", "w").write("".join(n + "\n" for n in names))
    open(root / "target.txt", "w").write("".join("leftImg8bit/" + n + "\n" for n in names))
    return ["--data-dir", str(root / "source"), "--data-list", str(root / "source.txt"), "--data-dir-target", str(root / "target"),
            "--data-list-target", str(root / "target.txt")]


def _loss_lines(out):
    return [re.sub(r"\s*\([0-9.]+ img/s\)", "", ln) for ln in out.splitlines() if ln.startswith("iter = ")]


def test_tool_trains_with_the_flag_and_resumes(dev, tmp_path, capsys, monkeypatch):
    """trainV1_warmup --online-labels 0 --online-source --feat-dist --feat-dist-from <a file in DeeplabMulti's keys> on generated files,
    B = 2, 129,65: ` fd = ` in every loss line, no nan; 2 + 2 == 4 through --train-state in the loss lines and the final snapshot, which
    loads strict=True; without the flag none of the new symbols is launched and the loss lines are those of --feat-dist 0 without its
    ` fd = ` part; a resume with the flag dropped or beside another file is refused."""
    from simt_amd import model_spec as ms
    from simt_amd.model.deeplab_multi import DeeplabMulti
    from simt_amd.tools import trainV1_warmup as tool
    sets = _data_sets(tmp_path)
    weights = str(tmp_path / "imagenet.pth")
    torch.save(ms.reference_init(ms.state_shapes(19, 0, False), seed=5), weights)          # DeeplabMulti's keys, heads included
    common = ["--learning-rate", "2.5e-4", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--save-pred-every", "100",
              "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2", "--random-mirror", "--online-labels", "0",
              "--online-source"] + sets
    flag = ["--feat-dist", "0.5", "--feat-dist-from", weights]
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    new = ("simt_feat_dist_mask", "simt_feat_dist", "simt_feat_dist_finalize")

    def run(tag, stop, *more):
        del calls[:]
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_4.pth")

    out_a, snap_a = run("a", 4, *flag)
    lines = _loss_lines(out_a)
    assert len(lines) == 4 and not re.search(r"= nan", out_a), out_a
    assert all(re.search(r" src = \d+\.\d{3} fd = \d+\.\d{4} \(\d+\)  lr = ", ln) for ln in lines), lines
    assert any(int(re.search(r" fd = \S+ \((\d+)\)", ln).group(1)) > 0 for ln in lines), "no line reports a kept cell"
    assert [calls.count(n) for n in new] == [4, 4, 4]
    assert out_a.count("feature distance: lambda 0.5 over the layer-4 cells one of the classes 6 7 11 12 13 14 15 16 17 18 fills to 0.75") == 1
    assert "DeeplabMulti layout" in out_a and weights in out_a
    DeeplabMulti(19, 0, False).load_state_dict(torch.load(snap_a), strict=True)
    state = str(tmp_path / "run.state")
    out_b1, _ = run("b", 2, *flag, "--train-state", state)
    assert _loss_lines(out_b1) == lines[:2]
    out_b2, snap_b = run("b", 4, *flag, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_b2), out_b2
    assert _loss_lines(out_b2) == lines[2:], (out_a, out_b2)
    sa, sb = torch.load(snap_a), torch.load(snap_b)
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(SystemExit, match="feat_dist"):          # dropped
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "6", "--train-state", state])
    other = str(tmp_path / "other.pth")
    torch.save(ms.reference_init(ms.state_shapes(19, 0, False), seed=6), other)
    with pytest.raises(SystemExit, match="feat_dist_sha256"):
        tool.main(common + ["--feat-dist", "0.5", "--feat-dist-from", other, "--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "6",
                            "--train-state", state])
    capsys.readouterr()
    # without the flag: no new launch, no ` fd = `; the loss lines of lambda = 0 without their ` fd = ` part
    out_o, _ = run("o", 4)
    assert not set(calls) & set(new) and " fd = " not in out_o and "feature distance" not in out_o
    out_z, _ = run("z", 4, "--feat-dist", "0", "--feat-dist-from", weights)
    assert [re.sub(r" fd = \S+ \(\d+\)", "", ln) for ln in _loss_lines(out_z)] == _loss_lines(out_o)
