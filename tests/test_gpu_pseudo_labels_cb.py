"""GPU tests of the class-balanced pseudo labels (csrc/label_sweep.hip simt_pseudo_conf_u8 / simt_pseudo_conf2_u8, make_pseudo_labels
--class-balanced).  Every comparison is exact (integers or bytes): the histogram against NumPy where the resample is the identity, the
histogram and the labels against the existing confidence-mode kernels (whose (arg, conf) the new kernels share) where it interpolates,
and the exported files against compositions of single-threshold confidence-mode runs."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from test_gpu_pseudo_labels import _write_frames

pytestmark = pytest.mark.gpu
BINS = L.CONF_BINS
GUARD = 0x5A5A5A5A5A5A5A5A
EDGES = (0, 1, 128, 205, 230, 255)


def _below(t):
    """The strict threshold of the confidence mode equivalent to conf >= t (t a float32 >= 0): nextafter(t, -inf); -1 for t = 0."""
    t = np.float32(t)
    return -1.0 if t == 0 else float(np.nextafter(t, np.float32(-np.inf)))


class Conf:
    """One family of kernels over one device input: .stats / .labels (optionally both in one launch) call the new entry point, .old the existing
    confidence-mode kernel (mode 1) at one strict threshold."""

    def __init__(self, dev, geo, B, H, W, C, two):
        self.dev, self.geo, self.B, self.H, self.W, self.C, self.two = dev, geo, B, H, W, C, two
        self.P = B * H * W

    def _call(self, thr, out, counts, hist):
        thr = None if thr is None else np.ascontiguousarray(thr, dtype=np.float32)
        L.call("simt_pseudo_conf2_u8" if self.two else "simt_pseudo_conf_u8", *self.geo, self.B, self.H, self.W, self.C,
               thr.ctypes.data if thr is not None else None, ops._p(out), ops._p(counts), ops._p(hist), ops.stream_ptr())

    def hist_buf(self, C=None):
        return torch.full(((C or self.C) * BINS + 16,), GUARD, device=self.dev, dtype=torch.int64)

    def stats(self, calls=1):
        buf = self.hist_buf()
        buf[:self.C * BINS] = 0
        for _ in range(calls):
            self._call(None, None, None, buf)
        assert torch.all(buf[self.C * BINS:].cpu() == GUARD), "the kernel wrote past the end of the histogram"
        return buf[:self.C * BINS].view(self.C, BINS).cpu().numpy()

    def labels(self, thr, with_hist=False):
        buf = torch.full((self.P + 64,), 77, device=self.dev, dtype=torch.uint8)       # 64 guard bytes behind the map
        counts = torch.zeros(self.C + 1, device=self.dev, dtype=torch.int64)
        hbuf = None
        if with_hist:
            hbuf = self.hist_buf()
            hbuf[:self.C * BINS] = 0
        self._call(thr, buf, counts, hbuf)
        assert torch.all(buf[self.P:].cpu() == 77), "the kernel wrote past the end of the label map"
        res = (buf[:self.P].view(self.B, self.H, self.W).cpu().numpy(), counts.cpu().numpy())
        if with_hist:
            assert torch.all(hbuf[self.C * BINS:].cpu() == GUARD)
            res += (hbuf[:self.C * BINS].view(self.C, BINS).cpu().numpy(),)
        return res

    def old(self, threshold):
        out = torch.zeros(self.B, self.H, self.W, device=self.dev, dtype=torch.uint8)
        counts = torch.zeros(self.C + 1, device=self.dev, dtype=torch.int64)
        if self.two:
            L.call("simt_pseudo_label2_u8", *self.geo, None, 0, 0, 0, 0, 0, self.B, self.H, self.W, self.C, 1, threshold, ops._p(out),
                   ops._p(counts), ops.stream_ptr())
        else:
            L.call("simt_pseudo_label_u8", *self.geo, None, 0, 0, 0, self.B, self.H, self.W, self.C, 1, threshold, ops._p(out),
                   ops._p(counts), ops.stream_ptr())
        return out.cpu().numpy(), counts.cpu().numpy()


# ---- 1. the histogram against NumPy where the resample is the identity -----------------------------------------------------------------
def _identity_input(B, H, W, C, ld, seed):
    """"Probabilities" [B, H, W, ld] in [0, 1): rows forced to all zeros, to a maximum on a bin edge k/256 and to 1.0 (the top-bin clamp),
    and a region (the first half) where 60 % of the pixels are class 0 at exactly 1.0 -- the crowded bin.  Channels >= C hold 1e3 (never
    read)."""
    rng = np.random.default_rng(seed)
    P = B * H * W
    x = np.full((P, ld), 1e3, np.float32)
    x[:, :C] = rng.random((P, C), dtype=np.float32) * rng.random((P, 1), dtype=np.float32)     # maxima spread over all the bins
    kind = rng.integers(0, 12, P)
    cls = rng.integers(0, C, P)
    for j, v in enumerate((0.0, 1 / 256, 128 / 256, 205 / 256, 255 / 256, 1.0)):
        rows = np.nonzero(kind == j)[0]
        x[rows, :C] = 0 if v == 0 else x[rows, :C] * np.float32(v * 0.5)        # below v ...
        if v:
            x[rows, cls[rows]] = np.float32(v)                                  # ... but for one entry exactly on the edge
    hot = np.nonzero(rng.random(P // 2) < 0.6)[0]
    x[hot, 0] = 1.0
    x[hot, 1:C] = np.minimum(x[hot, 1:C], np.float32(0.99))
    return x.reshape(B, H, W, ld)


@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (1, 3, 5), (1, 600, 900)])
def test_histogram_equals_numpy_at_identity_geometry(dev, B, H, W):
    """h == H, w == W: the align-corners weights are exactly (1, 0), so conf is exactly the maximum of the supplied row.  3 922 pixels
    (no multiple of 4 or 64, 4 blocks); 15 (less than one wave); 540 000 (above the grid cap: the grid-stride loop runs)."""
    C, ld = 19, 22
    x = _identity_input(B, H, W, C, ld, seed=H + W)
    rows = x.reshape(-1, ld)[:, :C]
    arg = rows.argmax(1)                                                        # first index on ties
    bins = np.minimum(BINS - 1, np.floor(rows.max(1) * np.float32(BINS)).astype(np.int64))
    exp = np.bincount(arg * BINS + bins, minlength=C * BINS).reshape(C, BINS)
    if rows.shape[0] > 1000:
        assert exp[0, BINS - 1] > 0.25 * rows.shape[0] and exp[:, 0].sum() > 0 and exp[:, 128].sum() > 0 and (exp > 0).sum() > 800
    xd = torch.from_numpy(x).to(dev)
    k = Conf(dev, (ops._p(xd), H, W, ld), B, H, W, C, two=False)
    got = k.stats()
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bins differ"
    assert np.array_equal(k.stats(calls=2), 2 * exp)                            # the histogram accumulates across calls


# ---- 2 - 5. against the existing confidence-mode kernels where the resample interpolates ---------------------------------------------
def _ramp_logits(B, h, w, ld, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, h, w, ld), 1e3)
    x[..., :C] = torch.randn(B, h, w, C, generator=g) * 2.5
    x[..., 3] += torch.linspace(-2, 12, w).view(1, 1, w)                       # confident on one side, uncertain on the other
    return x


@pytest.fixture(scope="module", params=["one", "two-vec4", "two-scalar"])
def fam(request):
    """The kernels of one family over one input, with the statistics launch and the existing kernel's runs at the bin edges, shared by
    the tests below.  one: simt_pseudo_conf_u8 on softmax_rows of 33 x 33 logits -> 130 x 130.  two-*: simt_pseudo_conf2_u8 on 17 x 33
    logits, in-model size 65 x 129, labels 72 x 144, with ld % 4 == 0 and a 16-byte aligned base (float4 gathers) or ld = 22 (scalar)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    C = 19
    if request.param == "one":
        ld, h, H = 22, 33, 130
        src = _ramp_logits(1, h, h, ld, C, 11).to(dev)
        prob = torch.zeros_like(src)
        ops.softmax_rows(src, ld, prob, ld, h * h, C)
        k = Conf(dev, (ops._p(prob), h, h, ld), 1, H, H, C, two=False)
        k.keep = prob
    else:
        ld = 24 if request.param == "two-vec4" else 22
        lg = _ramp_logits(2, 17, 33, ld, C, 12).reshape(-1, ld).to(dev)
        assert lg.data_ptr() % 16 == 0
        k = Conf(dev, (ops._p(lg), 17, 33, ld, 65, 129), 2, 72, 144, C, two=True)
        k.keep = lg
    k.hist = k.stats()
    k.edge = {b: k.old(_below(b / BINS)) for b in EDGES}
    return k


def test_histogram_tail_sums_equal_confidence_mode_counts(fam):
    C = fam.C
    assert fam.hist.sum() == fam.P
    kept = fam.edge[205][1][:C].sum() / fam.P
    assert 0.05 < kept < 0.95 and (fam.hist.sum(1) > 0).sum() >= 10, "both sides of the threshold and many classes must occur"
    for b in EDGES:
        lab, counts = fam.edge[b]
        assert np.array_equal(fam.hist[:, b:].sum(1), counts[:C]), f"bin {b}"
    assert fam.edge[0][1][C] == 0


def test_uniform_thresholds_equal_confidence_mode_labels(fam):
    for b in EDGES:
        lab, counts = fam.labels(np.full(fam.C, b / BINS, np.float32))
        ref, ref_counts = fam.edge[b]
        assert np.array_equal(lab, ref), f"bin {b}: {int((lab != ref).sum())} labels differ"
        assert np.array_equal(counts, ref_counts)


def _per_class(fam):
    C = fam.C
    thr = np.array([((37 * c) % 256) / 256 for c in range(C)], np.float32)
    arg = fam.edge[0][0]
    assert arg.max() < C
    exp = np.full_like(arg, 255)
    for c in range(C):
        kept = fam.old(_below(thr[c]))[0] != 255
        m = (arg == c) & kept
        exp[m] = c
    return thr, exp


def test_per_class_thresholds(fam):
    thr, exp = _per_class(fam)
    lab, counts = fam.labels(thr)
    assert np.array_equal(lab, exp), f"{int((lab != exp).sum())} labels differ"
    assert 0.05 < (lab == 255).mean() < 0.95
    assert np.array_equal(counts, np.bincount(lab.reshape(-1), minlength=256)[[*range(fam.C), 255]])


def test_combined_launch_equals_the_two(fam):
    thr, exp = _per_class(fam)
    lab, counts, hist = fam.labels(thr, with_hist=True)
    lab1, counts1 = fam.labels(thr)
    assert np.array_equal(lab, lab1) and np.array_equal(lab, exp) and np.array_equal(counts, counts1)
    assert np.array_equal(hist, fam.hist)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True])
def test_refusals_write_nothing(dev, two):
    C, ld, h, w, H, W = 65, 68, 5, 7, 9, 11
    src = torch.rand(1, h, w, ld, device=dev)
    geo = (ops._p(src), h, w, ld) + ((20, 28) if two else ())
    k = Conf(dev, geo, 1, H, W, 19, two)
    out = torch.full((k.P + 64,), 77, device=dev, dtype=torch.uint8)
    counts = torch.full((C + 1,), GUARD, device=dev, dtype=torch.int64)
    hist = k.hist_buf(C)
    thr = np.zeros(C, np.float32)
    with pytest.raises(L.SimtHipError):                                         # both outputs NULL
        k._call(thr, None, counts, None)
    with pytest.raises(L.SimtHipError):                                         # labels without thresholds
        k._call(None, out, counts, None)
    with pytest.raises(L.SimtHipError):                                         # labels without counts
        k._call(thr, out, None, None)
    k.C = 65
    with pytest.raises(L.SimtHipError):                                         # 65 x 256 counters do not fit the workgroup's LDS
        k._call(None, None, None, hist)
    with pytest.raises(L.SimtHipError):
        k._call(thr, out, counts, hist)
    torch.cuda.synchronize()
    assert torch.all(out.cpu() == 77) and torch.all(counts.cpu() == GUARD) and torch.all(hist.cpu() == GUARD)
    k.C = 64                                                                    # the largest class count the histogram takes
    hist[:64 * BINS] = 0
    counts[:] = 0
    k._call(thr, out, counts, hist)
    got = hist[:64 * BINS].cpu().numpy()
    assert got.sum() == k.P and counts.cpu().numpy()[:65].sum() == k.P and torch.all(hist[64 * BINS:].cpu() == GUARD)
    assert torch.all(out[k.P:].cpu() == 77)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
def _state(arch):
    """The reduced-depth recipe states of the export tests; v3 / vgg: the classifier scaled so that the oracle's logits have a standard
    deviation of 3 (neither saturated nor flat)."""
    if arch == "multi":
        layers = (1, 1, 2, 1)
        return so.recipe_state(so.state_shapes(19, 3, True, layers=layers), seed=31, head_scale=8.0), 3, layers
    img = torch.randn(1, 3, 48, 96, generator=torch.Generator().manual_seed(5)) * 50
    if arch == "v3":
        from test_gpu_pseudo_labels_single import _v3_state
        st, layers, head = _v3_state(0, 41), (1, 1, 1), ("conv.", "conv_1.")
        with torch.no_grad():
            o = so.v3_forward(st, img, layers, openset=False, train=False)
    else:
        from test_gpu_single import VGG_SMALL, _vgg_state
        st, layers, head = _vgg_state(19, VGG_SMALL, 8), VGG_SMALL, ("classifier.",)
        with torch.no_grad():
            o = so.vgg_forward(st, img, layers)
    f = 3.0 / float(o[:, :19].std())
    return {k: (v * f if k.startswith(head) else v) for k, v in st.items()}, 0, layers


def _pngs(root, out_name, names):
    from PIL import Image
    return [np.asarray(Image.open(os.path.join(root, out_name, os.path.basename(n)))) for n in names]


@pytest.mark.parametrize("arch", ["multi", "v3", "vgg"])
def test_export_end_to_end(dev, tmp_path, arch):
    from PIL import Image

    from simt_amd.data.pipeline import InputPrep
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    from simt_amd.tools import compute_ClassDistribution as ccd
    from simt_amd.tools import make_pseudo_labels as mpl
    C = 19
    st, K, layers = _state(arch)
    root = str(tmp_path)
    names, kit = _write_frames(root, 3, (96, 192), 1)
    scales, label_hw = ((48, 96), (64, 128)), (72, 144)
    kw = dict(num_classes=C, open_classes=K, arch=arch, scales=scales, label_hw=label_hw, device=dev, layers=layers)
    lst = os.path.join(root, "lists", "pseudo_cb.lst")
    os.makedirs(os.path.dirname(lst))
    data_list = os.path.join(root, "train.txt")
    counts = mpl.export(st, root, data_list, "pseudo_cb", lst, workers=2, mode="class_balanced", portion=0.5, cap=1.0, verbose=False, **kw)
    rec = json.load(open(os.path.join(root, "lists", "pseudo_cb_thresholds.json")))
    assert (rec["num_classes"], rec["bins"], rec["portion"], rec["cap"], rec["data_list"]) == (C, BINS, 0.5, 1.0, data_list)
    hist = np.array([e["hist"] for e in rec["classes"]], np.int64)
    thr = np.array([e["threshold"] for e in rec["classes"]], np.float32)
    assert hist.sum() == 3 * 72 * 144 and (hist.sum(1) > 0).sum() >= 3
    assert np.array_equal(thr, mpl.class_thresholds(hist, 0.5, 1.0))
    # the per-class composition of single-threshold confidence-mode runs
    ref_lab = mpl.PseudoLabeller(st, mode="confidence", threshold=-1.0, **kw)
    prep = None
    pngs = _pngs(root, "pseudo_cb", names)
    for name, png in zip(names, pngs):
        rgb = np.asarray(Image.open(os.path.join(root, "train", name)).convert("RGB"))
        prep = prep or InputPrep(1, rgb.shape[:2], (scales[0][1], scales[0][0]), dev, with_label=False)
        x = torch.empty(1, 3, *scales[0], device=dev)
        prep.run(torch.from_numpy(rgb[None].copy()).to(dev), x)
        ref_lab.threshold = -1.0
        arg = ref_lab.label(x)[0].cpu().numpy()
        exp = np.full_like(arg, 255)
        for c in np.unique(arg):
            ref_lab.threshold = _below(thr[c])
            kept = ref_lab.label(x)[0].cpu().numpy() != 255
            exp[(arg == c) & kept] = c
        assert png.dtype == np.uint8 and png.shape == label_hw
        assert np.array_equal(png, exp), f"{name}: {int((png != exp).sum())} labels differ from the composition"
    kept = np.bincount(np.concatenate([p.reshape(-1) for p in pngs]), minlength=256)
    for c, e in enumerate(rec["classes"]):
        b = int(round(float(thr[c]) * BINS))
        assert kept[c] == hist[c, b:].sum() == counts[c] == e["kept"] and e["pixels"] == hist[c].sum()
        assert kept[c] >= e["pixels"] - int(np.round(e["pixels"] * 0.5)), "never fewer than asked"
    assert counts[C] == kept[255] and counts.sum() == hist.sum()
    assert open(lst).read().splitlines() == [f"train/{n}\tpseudo_cb/{os.path.basename(n)}" for n in names]
    ds = cityscapesPseudo(root, lst)
    for i in range(len(ds)):
        _, lab, _ = ds.decode(i)
        assert lab.shape == label_hw
    ref_npy = os.path.join(root, "ref.npy")
    ccd.main(["--pred-dir", os.path.join(root, "pseudo_cb"), "--devkit-dir", kit, "--out", ref_npy, "--device", str(dev)])
    mine = np.load(os.path.join(root, "lists", "ClassDist_pseudo_cb.npy"))
    assert mine.dtype == np.float64 and np.array_equal(mine, np.load(ref_npy))
    for d in (os.path.join(root, "pseudo_cb"), os.path.join(root, "lists")):
        assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
    # a lower cap keeps a superset of the pixels
    mpl.export(st, root, data_list, "pseudo_cap", os.path.join(root, "lists", "pseudo_cap.lst"), workers=2, mode="class_balanced",
               portion=0.5, cap=0.5, verbose=False, **kw)
    more = 0
    for p, q in zip(pngs, _pngs(root, "pseudo_cap", names)):
        assert np.array_equal(q[p != 255], p[p != 255])
        more += int(((q != 255) & (p == 255)).sum())
    assert more > 0 or thr.max() <= 0.5
    # the labeller refuses to label before thresholds are set
    with pytest.raises(RuntimeError):
        mpl.PseudoLabeller(st, mode="class_balanced", **kw).label(torch.empty(1, 3, *scales[0], device=dev))


def test_command_line_and_thresholds_from(dev, tmp_path):
    from simt_amd.tools import make_pseudo_labels as mpl
    from simt_amd.tools.trainV2_simt import single_model_state
    root = str(tmp_path)
    names, kit = _write_frames(root, 3, (96, 192), 3)
    ckpt = os.path.join(root, "ckpt.pth")
    torch.save(single_model_state("DeepLabVGG", 19, seed=8), ckpt)
    common = ["--restore-from", ckpt, "--arch", "vgg", "--data-dir", root, "--data-list", os.path.join(root, "train.txt"),
              "--input-size", "96,48", "--label-size", "144,72", "--num-workers", "2"]
    mpl.main([*common, "--class-balanced", "0.5", "--out-name", "pseudo_a", "--list-out", os.path.join(root, "pseudo_a.lst")])
    rec = json.load(open(os.path.join(root, "pseudo_a_thresholds.json")))
    assert rec["portion"] == 0.5 and rec["cap"] == 0.9 and rec["thresholds_from"] is None
    mpl.main([*common, "--thresholds-from", os.path.join(root, "pseudo_a_thresholds.json"), "--out-name", "pseudo_b",
              "--list-out", os.path.join(root, "pseudo_b.lst")])
    for n in names:
        a = open(os.path.join(root, "pseudo_a", os.path.basename(n)), "rb").read()
        assert a == open(os.path.join(root, "pseudo_b", os.path.basename(n)), "rb").read()
    labs = np.concatenate([p.reshape(-1) for p in _pngs(root, "pseudo_a", names)])
    assert (labs == 255).sum() <= 0.5 * labs.size + 19                         # at least half of every class is kept (up to rounding)
    rec_b = json.load(open(os.path.join(root, "pseudo_b_thresholds.json")))
    assert rec_b["thresholds_from"] == os.path.join(root, "pseudo_a_thresholds.json")
    assert [e["threshold"] for e in rec_b["classes"]] == [e["threshold"] for e in rec["classes"]]
    assert [e["kept"] for e in rec_b["classes"]] == [e["kept"] for e in rec["classes"]]
    assert np.array_equal(np.load(os.path.join(root, "ClassDist_pseudo_a.npy")), np.load(os.path.join(root, "ClassDist_pseudo_b.npy")))
