"""The prototype contrastive term on the GPU, launch by launch (simt_cell_labels / simt_proto_contrast_prep / simt_proto_contrast /
simt_proto_contrast_finalize in csrc/proto_contrast.hip).  The yardstick is the restatement of tests/_proto_contrast_ref.py, never the code under
test:

  (a) the cell labels, bit for bit against the restatement and, through the class-set identity, equal to simt_feat_dist_mask;
  (b) d, the scalars and the seed against float64 under the bar 4 * err32 + 2^-22 * max|value| (+ half a bf16 unit for a bf16 seed), with
      gpu_err / err32 printed per case; the seen set, N and the normalised prototypes of the prep launch;
  (c) the contract's words: no seen class, one seen class, an unseen class holding cells, every cell 255, a zero-norm row, a NaN row, a zero
      prototype, rows that are never read; NaN-filled outputs overwritten, guard bands, bit-for-bit repeats, lambda doubled; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import _feat_dist_ref as fr
import _proto_contrast_ref as pr
import test_gpu_feat_dist as FD
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import proto_contrast as PC

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GUARD = 16


# ---- (a) the cell labels ---------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(1, 7, 5, 7, 5), (2, 65, 129, 9, 17), (1, 33, 33, 5, 5), (3, 16, 16, 1, 1)]


def _cell_launch(dev, lab, h, w, Cn, ratio, n):
    B, H, W = lab.shape
    parts = L.load().simt_cell_labels_parts(B, h, w)
    assert parts == -(-B * h * w // 32)
    out = torch.full((B * h * w + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    part = torch.full((parts + 4,), -7, dtype=torch.int32, device=dev)
    labd = torch.from_numpy(lab).to(dev)
    nd = None if n is None else torch.from_numpy(np.asarray(n, dtype=np.int32)).to(dev)
    d = PC.fill_cell_labels(labd, out, part, nd, B, H, W, h, w, Cn, ratio)
    L.call("simt_cell_labels", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out[B * h * w:] == 0xEE).all()) and bool((part[parts:] == -7).all()), "guard words written"
    assert torch.equal(labd.cpu(), torch.from_numpy(lab)), "the labels were written"
    return out[:B * h * w].cpu().numpy(), part[:parts].cpu().numpy()


@pytest.mark.parametrize("Cn", [2, 19, 64])
@pytest.mark.parametrize("ratio", [0.75, 1.0, 0.51])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "B{}-{}x{}-{}x{}".format(*g))
def test_cell_labels_equal_the_restatement_and_the_mask(dev, geo, ratio, Cn):
    B, H, W, h, w = geo
    lab, planted = FD._labels(B, H, W, h, w, ratio, seed=H + 7 * w)          # classes 0, 6, 13, 18, 63, values 255, -1, 19, 64 ..., windows on the boundary
    assert {255, -1, 19, 64} <= set(np.unique(lab).tolist()) or B * h * w < 40
    rng = np.random.default_rng(Cn)
    mixed = (rng.random(Cn) < 0.5).astype(np.int32) * 3
    mixed[0] = 1
    for n in (None, np.zeros(Cn, dtype=np.int32), mixed):
        want, seen_cells = pr.cell_labels_ref(lab, h, w, Cn, ratio, n)
        got, part = _cell_launch(dev, lab, h, w, Cn, ratio, n)
        assert (got == want).all(), f"{int((got != want).sum())} of {want.size} cells differ"
        ok = (want < Cn) & ((np.ones(Cn, dtype=bool) if n is None else n > 0)[np.minimum(want, Cn - 1)])
        assert int(part.sum()) == seen_cells == int(ok.sum())
        assert (part == np.add.reduceat(ok.astype(np.int64), np.arange(0, want.size, 32))).all()
    for i, (cell, kept, count, n_pix) in enumerate(planted):          # the planted windows sit exactly on / one below the boundary
        cls = FD.MASK_CLASSES[i % len(FD.MASK_CLASSES)]
        if cls < Cn:
            assert (want[cell] == cls) == bool(kept), (cell, count, n_pix)
    # the class-set identity with 7.22's mask, on the device and in the restatement
    classes = tuple(c for c in FD.MASK_CLASSES if c < Cn)
    mask, mpart = FD._mask_launch(dev, lab, h, w, classes, ratio)
    mine = ((got < Cn) & np.isin(got, classes)).astype(np.uint8)
    assert (mine == mask).all() and (mine == fr.mask_ref(lab, h, w, classes, ratio)[0]).all() and int(mpart.sum()) == int(mine.sum())


def test_cell_label_refusals_write_nothing(dev):
    B, H, W, h, w = 2, 16, 24, 4, 6
    lab = torch.zeros(B * H * W + 1, dtype=torch.int64, device=dev)
    out = torch.full((B * h * w,), 0xEE, dtype=torch.uint8, device=dev)
    part = torch.full((4,), -7, dtype=torch.int32, device=dev)
    n = torch.ones(20, dtype=torch.int32, device=dev)

    def desc(**kw):
        d = PC.fill_cell_labels(lab, out, part, n, B, H, W, h, w, 19, 0.75)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [desc(label=None), desc(lab=None), desc(part=None), desc(h=H + 1), desc(w=W + 1), desc(min_ratio=0.5), desc(min_ratio=1.5),
           desc(min_ratio=float("nan")), desc(min_ratio=-1.0), desc(B=0), desc(h=0), desc(w=0), desc(H=0), desc(C=1), desc(C=65),
           desc(label=lab.data_ptr() + 4), desc(part=part.data_ptr() + 2), desc(n=n.data_ptr() + 2)]
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_cell_labels", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_cell_labels", None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == 0xEE).all()) and bool((part == -7).all())
    assert L.load().simt_cell_labels_parts(0, 4, 4) == 0 and L.load().simt_cell_labels_parts(1 << 16, 1 << 8, 1 << 8) == 0
    L.call("simt_cell_labels", C.byref(desc()), ops.stream_ptr())          # the descriptor itself is sound
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and part[:2].tolist() == [32, 16] and part[2:].tolist() == [-7, -7]


# ---- (b) the contrast ------------------------------------------------------------------------------------------------------------------------------
class _Launch:
    """The buffers and the descriptor of prep / contrast / finalize over a case of the restatement; run() -> the outputs on the host.  Every output
    starts as NaN (hdr: -7) and carries a guard band behind it."""

    def __init__(self, dev, k):
        self.k, self.dev = k, dev
        self.M, self.D, self.Cn = k["M"], k["D"], k["C"]
        self.dtype = BF if k["bf16"] else F32
        self.fs = torch.from_numpy(np.ascontiguousarray(k["F"])).to(dev, self.dtype).contiguous()
        self.lab = torch.from_numpy(np.ascontiguousarray(k["lab"])).to(dev)
        self.eta = torch.from_numpy(np.ascontiguousarray(k["eta"])).to(dev)
        self.n = torch.from_numpy(np.ascontiguousarray(k["n"]).astype(np.int32)).to(dev)
        lib = L.load()
        self.nparts, self.words = lib.simt_proto_contrast_parts(self.M), lib.simt_proto_contrast_phat_floats(self.Cn, self.D)
        assert self.nparts == min(-(-self.M // 32), 4096) and self.words == (32 if self.Cn <= 32 else 64) * self.D
        self.fresh()

    def fresh(self):
        dev, nan = self.dev, float("nan")
        self.phat = torch.full((self.words + GUARD,), nan, device=dev)
        self.hdr = torch.full((4 + GUARD,), -7, dtype=torch.int32, device=dev)
        self.seed = torch.full((self.M * self.D + GUARD,), nan, dtype=self.dtype, device=dev)
        self.d = torch.full((self.M + GUARD,), nan, device=dev)
        self.part = torch.full((self.nparts + GUARD,), nan, device=dev)
        self.out = torch.full((3 + GUARD,), nan, device=dev)

    def desc(self, lam=None, **kw):
        k = self.k
        d = PC.fill_contrast(self.fs, self.lab, self.eta, self.n, self.phat, self.hdr, self.seed, self.d, self.part, self.out, self.M, self.D,
                             self.Cn, self.dtype, k["lam"] if lam is None else lam, k["temp"], k["gscale"])
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t.float()).all()) for t in (self.phat, self.seed, self.d, self.part, self.out)) and bool((self.hdr == -7).all())

    def run(self, lam=None):
        d, st = self.desc(lam), ops.stream_ptr()
        for name in ("simt_proto_contrast_prep", "simt_proto_contrast", "simt_proto_contrast_finalize"):
            L.call(name, C.byref(d), st)
        torch.cuda.synchronize()
        for t, used in ((self.phat, self.words), (self.seed, self.M * self.D), (self.d, self.M), (self.part, self.nparts), (self.out, 3)):
            assert bool(torch.isnan(t[used:].float()).all()), "guard words written"
        assert bool((self.hdr[4:] == -7).all()), "guard words written"
        hdr = self.hdr[:4].cpu().numpy().view(np.uint32)
        return dict(seed=self.seed[:self.M * self.D].view(self.M, self.D).float().cpu().numpy(), d=self.d[:self.M].cpu().numpy(),
                    part=self.part[:self.nparts].cpu().numpy(), out=self.out[:3].cpu().numpy(), phat=self.phat[:self.words].view(-1, self.D).cpu().numpy(),
                    seen=int(hdr[0]) | (int(hdr[1]) << 32), N=int(hdr[2]), nseen=int(hdr[3]),
                    bits=[t.clone() for t in (self.seed, self.d, self.part, self.out, self.phat, self.hdr)])


def _check_prep(got, k, r64):
    """The seen set, N and the normalised prototypes: seen rows within 4 float32 units of eta / |eta|, every other row +0."""
    seen = r64["seen"]
    assert got["seen"] == sum(1 << int(c) for c in np.nonzero(seen)[0]) and got["N"] == r64["N"] and got["nseen"] == int(seen.sum())
    want = np.zeros_like(got["phat"], dtype=np.float64)
    if seen.any():
        e = k["eta"][seen].astype(np.float64)
        want[:len(seen)][seen] = e / np.sqrt((e * e).sum(axis=1))[:, None]
    rest = np.ones(len(want), dtype=bool)
    rest[:len(seen)] = ~seen
    z = got["phat"][rest]
    assert (z == 0).all() and not np.signbit(z).any(), "a row of phat that must be +0 is not"
    err = np.abs(got["phat"][~rest] - want[~rest])
    assert (err <= (k["D"] + 4) * 2.0 ** -24 * np.abs(want[~rest]) + 1e-45).all(), "phat beyond (D + 4) * 2^-24"


@pytest.mark.parametrize("name", list(pr.CASES))
def test_contrast_against_float64(dev, name):
    k = pr.case(name)
    r64, r32 = pr.refs(k, dt=np.float64), pr.refs(k, dt=np.float32)
    assert r64["N"] > 0 and (k["M"] < 40 or r64["N"] < k["M"])
    if len(k["n"]) > 2 and k["M"] > 4:
        assert ((k["lab"] < k["C"]) & ~r64["valid"]).any(), "no cell labelled with an unseen class"
    la = _Launch(dev, k)
    got = la.run()
    _check_prep(got, k, r64)
    pr.check_contrast(got, k, report=name, r64=r64, r32=r32)
    # the partials: tile by tile, at most 32 losses each
    tiles = np.add.reduceat(r64["d"], np.arange(0, k["M"], pr.TILE))
    assert len(tiles) == len(got["part"]) and np.allclose(got["part"], tiles, rtol=1e-4, atol=1e-6)
    # a second launch into fresh NaN-filled buffers: bit for bit
    first = got["bits"]
    la.fresh()
    again = la.run()
    for a, b in zip(first, again["bits"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two launches differ"


def test_lambda_doubled_doubles_the_term_exactly(dev):
    k = pr.case("f32_243_1024_19")
    la = _Launch(dev, k)
    one = la.run()
    la.fresh()
    two = la.run(lam=2 * k["lam"])
    assert two["out"][0] == 2 * one["out"][0] and two["out"][1] == one["out"][1] and two["out"][2] == one["out"][2]
    assert np.array_equal(two["seed"], 2 * one["seed"]) and np.array_equal(two["d"], one["d"]) and np.abs(one["seed"]).max() > 0
    la.fresh()
    zero = la.run(lam=0.0)
    assert zero["out"][0] == 0 and zero["out"][1] == one["out"][1] and not zero["seed"].any() and np.array_equal(zero["d"], one["d"])


# ---- (c) the contract's words ----------------------------------------------------------------------------------------------------------------------
def _variant(name, **kw):
    k = dict(pr.case(name))
    for q in ("F", "lab", "eta", "n"):
        k[q] = k[q].copy()
    k.update(kw)
    return k


def _all_zero(got, M):
    for q in ("seed", "d", "part", "out"):
        v = got[q]
        assert (v == 0).all() and not np.signbit(v).any(), f"{q} is not +0 everywhere"
    assert got["N"] == 0 and got["seen"] == 0


@pytest.mark.parametrize("name", ["bf16_70_2048_19", "f32_162_64_64"])
def test_no_valid_cell_is_all_zero(dev, name):
    base = pr.case(name)
    Cn = base["C"]
    none_seen = _variant(name, n=np.zeros(Cn, dtype=np.int32), eta=np.full_like(base["eta"], np.nan))
    one = np.zeros(Cn, dtype=np.int32)
    one[int(np.nonzero(base["n"] > 0)[0][0])] = 5
    one_seen = _variant(name, n=one)
    ignored = _variant(name, lab=np.full_like(base["lab"], 255))
    for k in (none_seen, one_seen, ignored):
        got = _Launch(dev, k).run()
        if k is ignored:
            assert got["N"] == 0 and got["nseen"] >= 2
            got["seen"] = 0
        else:
            assert got["nseen"] == (0 if k is none_seen else 1)
        _all_zero(got, k["M"])


def test_degenerate_rows_and_prototypes(dev):
    """A zero-norm row and a NaN row (valid: loss 0, a +0 row, counted in N), a zero prototype with n > 0 (unseen: its cells are not valid), and
    NaN / Inf in every row that is not valid (never read)."""
    k = _variant("f32_243_1024_19")
    seen = np.nonzero(k["n"] > 0)[0]
    dead = int(seen[1])
    k["eta"][dead] = 0.0
    live = np.nonzero((k["lab"] < k["C"]) & np.isin(k["lab"], seen) & (k["lab"] != dead))[0]
    k["F"][live[0]] = 0.0
    k["F"][live[1]] = np.nan
    k["F"][live[2], 5] = np.inf
    assert (k["lab"] == dead).any()
    r64 = pr.refs(k)
    assert not r64["seen"][dead] and r64["degenerate"].sum() == 3 and r64["valid"][live[:3]].all()
    invalid = np.nonzero(~r64["valid"])[0]
    k["F"][invalid[0::2]] = np.nan
    k["F"][invalid[1::2]] = np.inf
    r64, r32 = pr.refs(k), pr.refs(k, dt=np.float32)
    got = _Launch(dev, k).run()
    _check_prep(got, k, r64)
    pr.check_contrast(got, k, report="degenerate", r64=r64, r32=r32)
    assert got["N"] == r64["N"] == int(r64["valid"].sum())


def test_refusals_write_nothing(dev):
    k = pr.case("f32_40_24_19")
    la = _Launch(dev, k)
    nan, inf = float("nan"), float("inf")
    bad = [dict(fs=None), dict(lab=None), dict(eta=None), dict(n=None), dict(phat=None), dict(hdr=None), dict(seed=None), dict(d=None),
           dict(part=None), dict(out=None), dict(D=12), dict(D=0), dict(D=4104), dict(C=1), dict(C=65), dict(dtype=7), dict(temp=0.0),
           dict(temp=-1.0), dict(temp=inf), dict(temp=nan), dict(lam=nan), dict(lam_g=nan), dict(M=0), dict(M=1 << 31),
           dict(fs=la.fs.data_ptr() + 4), dict(seed=la.seed.data_ptr() + 8), dict(eta=la.eta.data_ptr() + 4), dict(phat=la.phat.data_ptr() + 4),
           dict(n=la.n.data_ptr() + 2), dict(hdr=la.hdr.data_ptr() + 2), dict(d=la.d.data_ptr() + 2), dict(part=la.part.data_ptr() + 2),
           dict(out=la.out.data_ptr() + 2)]
    for name in ("simt_proto_contrast_prep", "simt_proto_contrast", "simt_proto_contrast_finalize"):
        for kw in bad:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(la.desc(**kw)), ops.stream_ptr())
        with pytest.raises(L.SimtHipError):
            L.call(name, None, ops.stream_ptr())
    assert la.untouched()
    lib = L.load()
    assert lib.simt_proto_contrast_parts(0) == 0 and lib.simt_proto_contrast_parts(1 << 31) == 0
    assert lib.simt_proto_contrast_phat_floats(1, 64) == 0 and lib.simt_proto_contrast_phat_floats(19, 12) == 0 and lib.simt_proto_contrast_phat_floats(65, 64) == 0
    pr.check_contrast(la.run(), k)          # the descriptor itself is sound
