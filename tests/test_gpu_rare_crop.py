"""Rare-class crops on the device (csrc/rare_crop.hip, simt_amd/data/rare_class.py, GpuLoader, --rare-class-sampling).

The yardstick is tests/_rare_crop_ref.py -- Pillow's NEAREST resize of the whole label, a numpy window, the documented draws -- and every
comparison is EXACT: the counts and the pick against the restatement, the crop bit for bit against simt_scale_crop launched at the
restatement's windows, the loader against the composition of restated draws, restated picks and _scale_crop_ref.item, the cached loader
against the uncached one, a resumed loader / tool against the uninterrupted one.  Source frames 96 x 160, crops (72, 40) and (73, 41)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _rare_crop_ref as rref
import _scale_crop_ref as ref
from simt_amd import _lib as L
from simt_amd.data import rare_class as rc
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import GpuLoader, InputPrep
from test_gpu_scale_crop import CROP, HS, KERNEL_CHOICES, LOADER_CHOICES, WS, _assert_same_batches, _collect, _loss_lines, _same_snapshot, _stream

pytestmark = pytest.mark.gpu

RESIZED = ref.Resized()
NEAREST = {}
NEW = ["simt_rare_crop_counts", "simt_rare_crop_pick", "simt_scale_crop_win"]
BAR = 150                 # min_count of the kernel tests: a window of 72 x 40 holds 2880 pixels


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------
def _kernel_frames():
    """B = 5 label frames made of rectangles, and the class counted in each: present (a rectangle in one corner), absent, covering the whole
    frame, 255 in `cls`, and present in a frame that also holds 255 pixels."""
    g = np.random.default_rng(21)
    rgb = g.integers(0, 256, (5, HS, WS, 3), dtype=np.uint8)
    base = np.zeros((HS, WS), np.uint8)
    base[:, WS // 2:] = 1
    base[HS // 2:, :WS // 3] = 2
    lab = np.stack([base] * 5)
    lab[0, 60:, 100:] = 3                   # item 0: class 3 in the bottom right corner
    lab[2] = 4                              # item 2: class 4 everywhere
    lab[4, :30, :50] = 6                    # item 4: class 6 in the top left corner, 255 pixels across the middle
    lab[4, 40:56, :] = 255
    return rgb, lab, [3, 7, 4, 255, 6]


def _candidates(K, crop, seed, shift):
    """Candidate (b, k): choice (b + k) % 5 -- K = 1 sees every choice once, K >= 5 every choice in every item -- at the low extreme, the
    high extreme or the middle of its range on each axis: drawn by `seed`, rotated by `shift`, so the three shifts put every candidate at
    all three on both axes."""
    g = np.random.default_rng(seed)
    w, h = crop
    wx, wy = g.integers(0, 3, (5, K)), g.integers(0, 3, (5, K))
    pick = [[(b + k) % 5 for k in range(K)] for b in range(5)]
    ox, oy = [], []
    for b in range(5):
        rx, ry = [], []
        for k in range(K):
            c = KERNEL_CHOICES[pick[b][k]]
            (xl, xh), (yl, yh) = ref.origin_range(ref.scaled(w, c), w), ref.origin_range(ref.scaled(h, c), h)
            rx.append((xl, xh, (xl + xh) // 2)[(wx[b, k] + shift) % 3])
            ry.append((yl, yh, (yl + yh) // 2)[(wy[b, k] + shift) % 3])
        ox.append(rx)
        oy.append(ry)
    return pick, ox, oy


def _launch(prep, dev, rgb, lab, mirror, cand, cls, bar, crop):
    """counts, pick and crop of one batch -> (counts [B][K], win [B][4], x, lab_out) as numpy."""
    w, h = crop
    B, K = len(cls), len(cand[0][0])
    rgb_d, lab_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(lab).to(dev)
    x = torch.full((B, 3, h, w), float("nan"), device=dev)
    lo = torch.full((B, h, w), -1, dtype=torch.int64, device=dev)
    parts = torch.full((B, K, L.RARE_CROP_PARTS), -7, dtype=torch.int32, device=dev)
    win = torch.full((B, 4), -7, dtype=torch.int32, device=dev)
    prep.rare_crop_batch([rgb_d[b].data_ptr() for b in range(B)], [lab_d[b].data_ptr() for b in range(B)], (mirror,) + tuple(cand), cls, bar, x,
                         lo, parts, win, _stream(dev))
    torch.cuda.synchronize()
    return parts.cpu().numpy().astype(np.int64).sum(axis=2), win.cpu().numpy(), x.cpu().numpy(), lo.cpu().numpy()


def _scale_crop(prep, dev, rgb, lab, mirror, windows, crop):
    """simt_scale_crop at the windows [(choice, ox, oy)] -> (x, lab_out) as numpy."""
    w, h = crop
    B = len(windows)
    rgb_d, lab_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(lab).to(dev)
    x = torch.full((B, 3, h, w), float("nan"), device=dev)
    lo = torch.full((B, h, w), -1, dtype=torch.int64, device=dev)
    prep.scale_crop_batch([rgb_d[b].data_ptr() for b in range(B)], [lab_d[b].data_ptr() for b in range(B)],
                          (mirror, [wd[0] for wd in windows], [wd[1] for wd in windows], [wd[2] for wd in windows]), x, lo, _stream(dev))
    torch.cuda.synchronize()
    return x.cpu().numpy(), lo.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


SEED = 0                  # of _candidates, checked on the CPU with the restatement alone: the conditions asserted in the test hold for every K, shift, crop


# ---- 1. counts, pick, crop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [CROP, (73, 41)], ids=["vec", "novec"])
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_counts_pick_and_crop_equal_the_restatement(dev, K, shift, crop):
    """B = 5, K candidates per item over the five choices (scaled sizes 36 x 20 ... 180 x 100 at crop (72, 40): padding on all four sides,
    the pure window, an upsample past the source), origins at the extremes and the middle of their ranges.  Counts and win equal the
    restatement exactly; x and lab_out equal simt_scale_crop at the restatement's windows bit for bit, mirror flags mixed."""
    pytest.importorskip("PIL.Image")
    rgb, lab, cls = _kernel_frames()
    cand = _candidates(K, crop, SEED, shift)
    want, ks, win_r = rref.windows(NEAREST, [("k", b) for b in range(5)], lab, crop, KERNEL_CHOICES, cand, cls, BAR)
    # the conditions, from the restatement alone
    assert all(n == 0 for n in want[1]) and ks[1] == K - 1, "item 1 (absent class): no candidate passes, the last one is taken"
    assert want[2][0] > BAR and ks[2] == 0, "item 2 (the class covers the frame): candidate 0 passes"
    assert ks[3] == 0 and all(n == 0 for n in want[3]), "item 3 (class 255): candidate 0, nothing counted"
    if K >= 3:
        assert any(0 < ks[b] < K - 1 for b in (0, 4)), "an item whose k* is neither 0 nor K - 1"
        assert len(set(want[0])) > 1 and len(set(want[4])) > 1, "the candidates' counts differ"
    mirror = [False, True, False, True, True]
    prep = InputPrep(5, (HS, WS), crop, dev, mean=ref.IMG_MEAN, scale_crop=KERNEL_CHOICES)
    counts, win, x, lo = _launch(prep, dev, rgb, lab, mirror, cand, cls, BAR, crop)
    assert counts.tolist() == want, (counts.tolist(), want)
    assert win.tolist() == win_r, (win.tolist(), win_r)
    xs, ls = _scale_crop(prep, dev, rgb, lab, mirror, win_r, crop)
    assert _same_bits(x, xs) and np.array_equal(lo, ls)
    for b in range(5):                                   # and the count IS (lab_out == c).sum() of that launch
        assert cls[b] == 255 or int((ls[b] == cls[b]).sum()) == win_r[b][3]
    b = 0                                                # one item against Pillow itself (the rest is simt_scale_crop's own test)
    xr, lr = ref.item(RESIZED, ("k", b), rgb[b], lab[b], crop, KERNEL_CHOICES[win_r[b][0]], win_r[b][1], win_r[b][2], mirror[b])
    assert np.array_equal(x[b], xr) and np.array_equal(lo[b], lr)


def test_pick_bar_is_strict_and_zero_counts_never_pass(dev):
    """min_count = 0 with a zero count: not accepted (K - 1 is taken).  A count of exactly min_count + 1: accepted."""
    pytest.importorskip("PIL.Image")
    rgb, lab, _cls = _kernel_frames()
    rgb, lab, cls = rgb[:2], lab[[1, 0]], [7, 3]          # item 0: class 7 is absent; item 1: class 3 in the bottom right corner
    i15 = KERNEL_CHOICES.index("1.5")                     # scaled 108 x 60: origins 0 .. 36, 0 .. 20
    cand = ([[i15] * 3] * 2, [[0, 36, 18]] * 2, [[0, 20, 10]] * 2)
    want, _ks, _win = rref.windows(NEAREST, [("p", 0), ("p", 1)], lab, CROP, KERNEL_CHOICES, cand, cls, 0)
    assert want[0] == [0, 0, 0] and 0 <= want[1][0] < want[1][2] < want[1][1], want
    prep = InputPrep(2, (HS, WS), CROP, dev, mean=ref.IMG_MEAN, scale_crop=KERNEL_CHOICES)
    for bar, k1 in ((0, 0 if want[1][0] > 0 else 1), (want[1][1] - 1, 1), (want[1][1], 2), (want[1][2] - 1, 1)):
        _c, ks, win_r = rref.windows(NEAREST, [("p", 0), ("p", 1)], lab, CROP, KERNEL_CHOICES, cand, cls, bar)
        assert ks == [2, k1], (bar, ks)
        counts, win, _x, _lo = _launch(prep, dev, rgb, lab, [False, True], cand, cls, bar, CROP)
        assert counts.tolist() == want and win.tolist() == win_r, (bar, win.tolist(), win_r)
        assert win[0].tolist() == [i15, 18, 10, 0]


@pytest.mark.parametrize("crop", [CROP, (73, 41)], ids=["vec", "novec"])
def test_one_candidate_and_no_class_equal_scale_crop_on_candidate_0(dev, crop):
    pytest.importorskip("PIL.Image")
    rgb, lab, cls = _kernel_frames()
    mirror = [True, False, False, True, False]
    prep = InputPrep(5, (HS, WS), crop, dev, mean=ref.IMG_MEAN, scale_crop=KERNEL_CHOICES)
    for K, classes in ((1, cls), (3, [255] * 5)):
        cand = _candidates(K, crop, 5, 1)
        counts, win, x, lo = _launch(prep, dev, rgb, lab, mirror, cand, classes, BAR, crop)
        first = [(cand[0][b][0], cand[1][b][0], cand[2][b][0]) for b in range(5)]
        assert [tuple(r[:3]) for r in win.tolist()] == first
        if K == 3:
            assert not counts.any() and not win[:, 3].any()
        xs, ls = _scale_crop(prep, dev, rgb, lab, mirror, first, crop)
        assert _same_bits(x, xs) and np.array_equal(lo, ls)


def _descs(prep, dev, rgb, lab, mirror, cand, cls, bar, crop, sentinel=True):
    w, h = crop
    B, K = len(cls), len(cand[0][0])
    t = {"rgb": torch.from_numpy(rgb).to(dev), "lab": torch.from_numpy(lab).to(dev),
         "x": torch.full((B, 3, h, w), float("nan"), device=dev), "lo": torch.full((B, h, w), -1, dtype=torch.int64, device=dev),
         "parts": torch.full((B, K, L.RARE_CROP_PARTS), -7, dtype=torch.int32, device=dev),
         "win": torch.full((B, 4), -7, dtype=torch.int32, device=dev)}
    (d,) = prep.rare_crop_descs([t["rgb"][b].data_ptr() for b in range(B)], [t["lab"][b].data_ptr() for b in range(B)], (mirror,) + tuple(cand),
                                cls, bar, t["x"], t["lo"], t["parts"], t["win"])
    return d, t


@pytest.mark.parametrize("crop", [CROP, (73, 41)], ids=["vec", "novec"])
def test_the_crop_clamps_whatever_win_holds(dev, crop):
    """`win` overwritten with out-of-range words: the launch reads no table out of range -- the choice is clamped to n_choices - 1, the
    origin to its choice's range -- and the output is simt_scale_crop's at the clamped window.  The clamp is the contract."""
    pytest.importorskip("PIL.Image")
    rgb, lab, cls = _kernel_frames()
    w, h = crop
    mirror = [False, True, True, False, True]
    prep = InputPrep(5, (HS, WS), crop, dev, mean=ref.IMG_MEAN, scale_crop=KERNEL_CHOICES)
    d, t = _descs(prep, dev, rgb, lab, mirror, _candidates(2, crop, 1, 0), cls, BAR, crop)
    big = 2 ** 31 - 1
    words = [[200, 10 ** 6, -10 ** 6, 0], [-1, -big - 1, big, 5], [len(KERNEL_CHOICES), big, -big - 1, -3], [0, 5, -5, 1], [2, -1000, 1000, 9]]
    t["win"].copy_(torch.tensor(words, dtype=torch.int32))
    L.call("simt_scale_crop_win", C.byref(d), _stream(dev))
    torch.cuda.synchronize()
    clamped = []
    for c, ox, oy, _n in words:
        c = len(KERNEL_CHOICES) - 1 if (c < 0 or c >= len(KERNEL_CHOICES)) else c
        (xl, xh), (yl, yh) = ref.origin_range(ref.scaled(w, KERNEL_CHOICES[c]), w), ref.origin_range(ref.scaled(h, KERNEL_CHOICES[c]), h)
        clamped.append((c, min(max(ox, xl), xh), min(max(oy, yl), yh)))
    if crop == CROP:                                       # "0.5": 36 x 20 inside 72 x 40, origins -36 .. 0 and -20 .. 0
        assert clamped[3] == (0, 0, -5) and clamped[0] == (4, 108, 0) and clamped[1] == (4, 0, 60)
    xs, ls = _scale_crop(prep, dev, rgb, lab, mirror, clamped, crop)
    assert _same_bits(t["x"].cpu().numpy(), xs) and np.array_equal(t["lo"].cpu().numpy(), ls)
    assert t["win"].cpu().tolist() == words                # the launch only reads it


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _break(name):
    """-> a function that makes a valid descriptor invalid in one way."""
    i10 = KERNEL_CHOICES.index("1.0")
    i15 = KERNEL_CHOICES.index("1.5")

    def cand(d, field, v, c=None):
        if c is not None:
            d.cand_choice[1][1] = c
        getattr(d, field)[1][1] = v
    return {
        "K = 0": lambda d: setattr(d, "K", 0),
        "K = 17": lambda d: setattr(d, "K", L.RARE_CROP_CANDS + 1),
        "a candidate choice past the choices": lambda d: cand(d, "cand_choice", len(KERNEL_CHOICES)),
        "ox above its range": lambda d: cand(d, "cand_ox", 37, i15),
        "ox below its range": lambda d: cand(d, "cand_ox", -1, i15),
        "oy above its range": lambda d: cand(d, "cand_oy", 1, i10),
        "oy below its range": lambda d: cand(d, "cand_oy", -21, KERNEL_CHOICES.index("0.5")),
        "min_count < 0": lambda d: setattr(d, "min_count", -1),
        "parts NULL": lambda d: setattr(d, "parts", None),
        "parts misaligned": lambda d: setattr(d, "parts", d.parts + 2),
        "win NULL": lambda d: setattr(d, "win", None),
        "win misaligned": lambda d: setattr(d, "win", d.win + 4),
        "a label pointer NULL": lambda d: d.lab.__setitem__(2, None),
        "an image pointer NULL": lambda d: d.img.__setitem__(0, None),
        "B = 0": lambda d: setattr(d, "B", 0),
        "B = 17": lambda d: setattr(d, "B", L.RARE_CROP_MAX + 1),
        "no choices": lambda d: setattr(d, "n_choices", 0),
        "x NULL": lambda d: setattr(d, "x", None),
        "tables too short": lambda d: setattr(d, "n_tables", d.n_tables - 1),
        "max_rows 0": lambda d: setattr(d, "max_rows", 0),
    }[name]


REFUSALS = ["K = 0", "K = 17", "a candidate choice past the choices", "ox above its range", "ox below its range", "oy above its range",
            "oy below its range", "min_count < 0", "parts NULL", "parts misaligned", "win NULL", "win misaligned", "a label pointer NULL",
            "an image pointer NULL", "B = 0", "B = 17", "no choices", "x NULL", "tables too short", "max_rows 0"]


def test_refusals_leave_every_buffer_untouched(dev):
    """Each refusal, on each of the three launches: an error, and parts, win, x and lab_out keep their sentinel fills."""
    rgb, lab, cls = _kernel_frames()
    prep = InputPrep(5, (HS, WS), CROP, dev, mean=ref.IMG_MEAN, scale_crop=KERNEL_CHOICES)
    cand = _candidates(3, CROP, 0, 0)
    d, t = _descs(prep, dev, rgb, lab, [False] * 5, cand, cls, BAR, CROP)
    before = {k: t[k].clone() for k in ("x", "lo", "parts", "win")}
    for name in REFUSALS:
        bad = L.RareCropDesc()
        C.memmove(C.byref(bad), C.byref(d), C.sizeof(d))          # the good descriptor, pointing at the watched buffers
        _break(name)(bad)
        for fn in NEW:
            with pytest.raises(L.SimtHipError):
                L.call(fn, C.byref(bad), _stream(dev))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert _same_bits(t[k].cpu().numpy(), v.cpu().numpy()), k
    for fn in NEW:                                                 # and the descriptor they were made from is accepted
        L.call(fn, C.byref(d), _stream(dev))
    torch.cuda.synchronize()
    assert not torch.isnan(t["x"]).any() and (t["win"][:, 0] >= 0).all()


# ---- 3. loader -------------------------------------------------------------------------------------------------------------------------------------------
GTA5_ID = {0: 7, 1: 8, 2: 11, 13: 26, 18: 33}          # train id -> GTA5 id of the classes the frames hold
MIN_PIXELS, RATIO, K_LOADER, T_LOADER = 400, "0.5", 4, 0.5


def _write_frames(root, n=9):
    """n frames of 96 x 160 under images/ and labels/ (GTA5 ids): road / building halves everywhere; a rectangle of a rarer class in a corner
    that moves with the frame -- wall in frames 1, 4, 7, car in 2, 5, bicycle in 8 alone --, an unmapped id and 255 pixels.
    -> (rgb, train-id labels, counts [n, 19])."""
    from PIL import Image
    g = np.random.default_rng(4)
    os.makedirs(root / "images")
    os.makedirs(root / "labels")
    rgb = g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)
    lab = np.zeros((n, HS, WS), np.uint8)
    lab[:, :, WS // 2:] = 1
    corners = [(slice(0, 30), slice(0, 40)), (slice(0, 30), slice(120, 160)), (slice(66, 96), slice(0, 40)), (slice(66, 96), slice(120, 160))]
    for i in range(n):
        c = 2 if i in (1, 4, 7) else 13 if i in (2, 5) else 18 if i == 8 else None
        if c is not None:
            lab[(i,) + corners[i % 4]] = c
        lab[i, 45:50, 10:30] = 255
    ids = np.full(256, 255, np.uint8)
    for t, gid in GTA5_ID.items():
        ids[t] = gid
    for i in range(n):
        raw = ids[lab[i]]
        raw[50:52, 10:30] = 1                    # an unmapped GTA5 id: ignore
        lab[i, 50:52, 10:30] = 255
        Image.fromarray(rgb[i]).save(root / "images" / f"f{i}.png")
        Image.fromarray(raw).save(root / "labels" / f"f{i}.png")
    open(root / "train.txt", "w").write("".join(f"f{i}.png\n" for i in range(n)))
    counts = np.stack([np.bincount(lab[i][lab[i] < 19], minlength=19) for i in range(n)]).astype(np.int64)
    return rgb, lab, counts


def _dataset(root, counts, choices=LOADER_CHOICES, rare=True, mirror=True):
    from simt_amd.dataset.gta5_dataset import GTA5DataSet
    r = rc.RareClass(counts, T=T_LOADER, min_pixels=MIN_PIXELS, min_crop_ratio=RATIO, K=K_LOADER) if rare else None
    return GTA5DataSet(str(root), str(root / "train.txt"), crop_size=CROP, mean=ref.IMG_MEAN, mirror=mirror, scale_crop=choices, rare_class=r)


def _restated_batches(n_batches, rgb, lab, counts, seed, rank, mirror=True):
    """The batches the loader must make: restated sampler draws, restated candidate draws, restated picks, _scale_crop_ref.item."""
    probs, lists = rref.class_probs(counts, T_LOADER, MIN_PIXELS), rref.items_with_class(counts, MIN_PIXELS)
    bar = rref.min_count(MIN_PIXELS, RATIO)
    gs, gl = rref.generator(seed, rank), np.random.default_rng(seed + 7919 * rank)
    out = []
    for _ in range(n_batches):
        cls, idx = rref.draw_batch(gs, 2, probs, lists)
        fl, pick, ox, oy = rref.cand_draws(gl, 2, K_LOADER, LOADER_CHOICES, CROP, mirror)
        _c, ks, win = rref.windows(NEAREST, [("l", i) for i in idx], [lab[i] for i in idx], CROP, LOADER_CHOICES, (pick, ox, oy), cls, bar)
        items = [ref.item(RESIZED, ("l", i), rgb[i], lab[i], CROP, LOADER_CHOICES[win[b][0]], win[b][1], win[b][2], fl[b]) for b, i in enumerate(idx)]
        out.append({"cls": cls, "idx": idx, "ks": ks, "win": win, "x": np.stack([it[0] for it in items]), "lab": np.stack([it[1] for it in items])})
    return out


def _assert_equals_restatement(got, want):
    assert len(got) == len(want) > 0
    for k, ((x, lo, _sizes, names), wb) in enumerate(zip(got, want)):
        assert names == [f"f{i}.png" for i in wb["idx"]], (k, names, wb["idx"])
        assert np.array_equal(x.cpu().numpy(), wb["x"]), (k, wb)
        assert np.array_equal(lo.cpu().numpy(), wb["lab"]), (k, wb)


def test_loader_equals_the_restated_composition_cached_equals_uncached_and_ranks_differ(dev, tmp_path):
    """Nine frames, B = 2, K = 4, two "epochs" (2 x 2 batches per rank of a world of 2): every batch is the composition of the restated
    draws and picks; the cached loader yields the same batches and counts a repeated item as a hit; the two ranks draw different batches."""
    pytest.importorskip("PIL.Image")
    rgb, lab, counts = _write_frames(tmp_path)
    seen = []
    for rank in (0, 1):
        kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2, rank=rank, world=2)
        loader = GpuLoader(_dataset(tmp_path, counts), 2, **kw)
        unc = _collect(loader)
        want = _restated_batches(4, rgb, lab, counts, 3, rank)
        _assert_equals_restatement(unc, want)
        assert loader.last_windows().cpu().tolist() == want[-1]["win"]
        seen.append(want)
        cache = DatasetCache((WS, HS), slab_slots=3, device=dev)
        got = _collect(GpuLoader(_dataset(tmp_path, counts), 2, cache=cache, **kw))
        _assert_same_batches(unc, got)
        dealt = {i for wb in want for i in wb["idx"]}
        assert cache.hits + cache.misses == 8 and cache.misses == len(dealt) == len(cache)
    assert [wb["idx"] for wb in seen[0]] != [wb["idx"] for wb in seen[1]], "the two ranks drew the same batches"
    both = [wb for r in seen for wb in r]
    classes = {c for wb in both for c in wb["cls"]}
    assert classes <= {0, 1, 2, 13, 18} and classes & {2, 13, 18}, classes            # classes with a qualifying frame only; a rare one is drawn
    for wb in both:
        assert all(counts[i, c] >= MIN_PIXELS for i, c in zip(wb["idx"], wb["cls"]))
    assert any(0 < k < K_LOADER - 1 for wb in both for k in wb["ks"]), "the seed exercises a pick that is neither the first nor the last"


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_loader_start_batch_yields_the_tail(dev, tmp_path, cached):
    """Nine frames, B = 2 (4 batches per epoch), 3 epochs: from inside epoch 0, from an epoch boundary and from inside epoch 1; nothing
    skipped is decoded."""
    pytest.importorskip("PIL.Image")
    rgb, lab, counts = _write_frames(tmp_path)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=5, epochs=3)
    full = _collect(GpuLoader(_dataset(tmp_path, counts), 2, **kw))
    assert len(full) == 12
    _assert_equals_restatement(full, _restated_batches(12, rgb, lab, counts, 5, 0))
    for n in (1, 4, 6):
        cache = DatasetCache((WS, HS), slab_slots=4, device=dev) if cached else None
        ds = _dataset(tmp_path, counts)
        decoded, real = [], ds.decode
        ds.decode = lambda i: (decoded.append(ds.files[i]["name"]), real(i))[1]
        tail = _collect(GpuLoader(ds, 2, cache=cache, start_batch=n, **kw))
        _assert_same_batches(full[n:], tail)
        assert set(decoded) <= {name for (_x, _l, _s, names) in tail for name in names}


def test_loader_without_scale_crop_samples_and_is_the_plain_loader_for_those_items(dev, tmp_path, monkeypatch):
    """scale_crop=None: the items are the restated draws, the batches InputPrep.run of those frames with the mirror draws the loader always
    made, and none of the new launches runs.  rare_class=None: no sampler state, none of the new launches, the parent's order."""
    pytest.importorskip("PIL.Image")
    rgb, lab, counts = _write_frames(tmp_path)
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    got = _collect(GpuLoader(_dataset(tmp_path, counts, choices=None), 2, shuffle=True, num_workers=2, device=dev, seed=4, epochs=2))
    assert len(got) == 8 and not set(calls) & set(NEW) and "simt_scale_crop" not in calls
    probs, lists = rref.class_probs(counts, T_LOADER, MIN_PIXELS), rref.items_with_class(counts, MIN_PIXELS)
    gs, rng = rref.generator(4, 0), np.random.default_rng(4)
    prep = InputPrep(2, (HS, WS), CROP, dev, mean=ref.IMG_MEAN)
    for x, lo, _s, names in got:
        _cls, ids = rref.draw_batch(gs, 2, probs, lists)
        assert names == [f"f{i}.png" for i in ids]
        flags = (rng.integers(0, 2, 2) == 0).tolist()
        xr = torch.empty(2, 3, CROP[1], CROP[0], device=dev)
        lr = torch.empty(2, CROP[1], CROP[0], dtype=torch.int64, device=dev)
        prep.run(torch.from_numpy(rgb[ids]).to(dev), xr, torch.from_numpy(lab[ids]).to(dev), lr, mirror=flags)
        torch.cuda.synchronize()
        assert torch.equal(x, xr) and torch.equal(lo, lr)
    # rare_class=None
    del calls[:]
    loader = GpuLoader(_dataset(tmp_path, counts, rare=False), 2, shuffle=True, num_workers=2, device=dev, seed=4, epochs=1)
    off = _collect(loader)
    assert loader.rare_class is None and loader._rcs_rng is None and loader.last_windows() is None
    assert not set(calls) & set(NEW) and calls.count("simt_scale_crop") == len(off) == 4
    order = torch.randperm(9, generator=torch.Generator().manual_seed(4)).tolist()
    assert [n for (_x, _l, _s, names) in off for n in names] == [f"f{i}.png" for i in order[:8]]
    del calls[:]
    on = _collect(GpuLoader(_dataset(tmp_path, counts), 2, shuffle=True, num_workers=2, device=dev, seed=4, epochs=1))
    assert [calls.count(n) for n in NEW] == [len(on)] * 3 and "simt_scale_crop" not in calls


# ---- 4. tool ---------------------------------------------------------------------------------------------------------------------------------------------
def _tool_sets(root):
    """The loader test's nine source frames with their statistics file (written by the statistics tool), and a four-image target set."""
    from PIL import Image
    from simt_amd.tools import compute_class_stats
    os.makedirs(root / "source")
    _write_frames(root / "source")
    compute_class_stats.main(["--data-dir", str(root / "source"), "--data-list", str(root / "source" / "train.txt"), "--out", str(root / "stats.json"),
                              "--num-workers", "2"])
    os.makedirs(root / "target" / "leftImg8bit")
    g = np.random.default_rng(8)
    for n in range(4):
        Image.fromarray(g.integers(0, 256, (6, 8, 3), dtype=np.uint8).repeat(16, 0).repeat(20, 1)).save(root / "target" / "leftImg8bit" / f"{n}.png")
    open(root / "target.txt", "w").write("".join(f"leftImg8bit/{n}.png\n" for n in range(4)))
    return (["--data-dir", str(root / "source"), "--data-list", str(root / "source" / "train.txt"), "--data-dir-target", str(root / "target"),
             "--data-list-target", str(root / "target.txt")],
            ["--rcs-stats", str(root / "stats.json"), "--rcs-min-pixels", str(MIN_PIXELS), "--rcs-crops", str(K_LOADER)])


def test_tool_resume_equals_one_run_and_a_changed_temperature_is_refused(dev, tmp_path, capsys):
    """trainV1_warmup --online-labels 0 --online-source --rare-class-sampling --scale-crop --train-state on the nine frames, B = 2, 129,65:
    3 steps + resume + 3 steps == 6 steps in the loss lines (` rcs = ` among them) and in every tensor of the final snapshot; one start-up line;
    a resume with another T is refused, the field named; without --scale-crop there is no ` rcs = `."""
    pytest.importorskip("PIL.Image")
    from simt_amd.tools import trainV1_warmup as tool
    sets, rcs = _tool_sets(tmp_path)
    capsys.readouterr()
    common = ["--learning-rate", "2.5e-4", "--model", "DeepLab", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
              "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2", "--random-mirror",
              "--online-labels", "0", "--online-source"] + sets
    crop = ["--scale-crop", "0.5", "1.0", "1.5"]

    def run(tag, stop, *more):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    on = ["--rare-class-sampling", "0.5"] + rcs
    out_a, snap_a = run("a", 6, *on, *crop)
    lines = _loss_lines(out_a)
    assert len(lines) == 6 and not re.search(r"= nan", out_a), out_a
    shares = [re.search(r" src = \d+\.\d{3} rcs = (\d\.\d{3})  lr = ", ln) for ln in lines]
    assert all(shares) and {m.group(1) for m in shares} <= {"0.000", "0.500", "1.000"}, lines
    assert out_a.count("rare-class sampling: T = 0.5, a frame holds a class with >= 400 pixels; P(class) = [") == 1
    assert re.search(r"frames per class = \[9, 9, 3, 0, .*, 2, 0, 0, 0, 0, 1\]; with --scale-crop the first of 4 windows with more than 200 pixels", out_a)
    out_b1, _ = run("b", 3, *on, *crop, "--train-state", state)
    assert _loss_lines(out_b1) == lines[:3]
    out_b2, snap_b = run("b", 6, *on, *crop, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert _loss_lines(out_b2) == lines[3:], (out_a, out_b2)
    _same_snapshot(snap_a, snap_b)
    with pytest.raises(SystemExit, match="rare_class_sampling"):          # another temperature
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state, "--rare-class-sampling", "0.25"] +
                  rcs + crop)
    with pytest.raises(SystemExit, match="rare_class_sampling"):          # dropped
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state] + crop)
    capsys.readouterr()
    out_c, _ = run("c", 2, *on)                  # no --scale-crop: the sampler alone, no window to choose
    assert len(_loss_lines(out_c)) == 2 and " rcs = " not in out_c and "rare-class sampling: T = 0.5" in out_c
    out_d, _ = run("d", 2, *crop)                                           # flag off: no line, no field
    assert len(_loss_lines(out_d)) == 2 and " rcs = " not in out_d and "rare-class sampling" not in out_d
