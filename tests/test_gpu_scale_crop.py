"""Random scale + crop on the device (csrc/scale_crop.hip, simt_amd/data/scale_crop.py, GpuLoader, --scale-crop).

The yardstick is Pillow itself plus numpy (tests/_scale_crop_ref.py) and every comparison is BITWISE: the kernel and the loader against
`Image.resize` of the whole frame -> window with pad 0 / 255 -> [:, :, ::-1] - mean -> the mirror rule; the cached loader against the
uncached one; a resumed loader / tool against the uninterrupted one.  Source frames 96 x 160, crop (72, 40): partial 16 x 64 tiles on both axes."""
import os
import re

import numpy as np
import pytest
import torch

import _scale_crop_ref as ref
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import GpuLoader, InputPrep

pytestmark = pytest.mark.gpu

HS, WS = 96, 160
CROP = (72, 40)
KERNEL_CHOICES = ("0.5", "1.0", "1.5", "2.0", "2.5")
LOADER_CHOICES = ("0.5", "1.0", "1.5")
RESIZED = ref.Resized()


def _frames(n, seed=11):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)
    lab = rng.integers(0, 20, (n, HS, WS), dtype=np.uint8)
    return rgb, lab


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 1. kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [CROP, (73, 41)], ids=["vec", "novec"])
@pytest.mark.parametrize("where", ["low", "high", "middle"])
def test_scale_crop_kernel_equals_pillow_composition(dev, where, crop):
    """B = 5, one item per choice: scaled sizes 36 x 20 ... 180 x 100 at crop (72, 40) -- padding on all four sides, the pure window,
    ksize 21 / 19 down to 5, an upsample past the source size; mirror flags mixed; the origins at the low extreme, the high extreme and
    the middle of their ranges.  (73, 41): the stores that are not 16 bytes wide."""
    pytest.importorskip("PIL.Image")
    w, h = crop
    B = len(KERNEL_CHOICES)
    rgb, lab = _frames(B)
    if crop == CROP:
        assert [(ref.scaled(w, c), ref.scaled(h, c)) for c in KERNEL_CHOICES] == [(36, 20), (72, 40), (108, 60), (144, 80), (180, 100)]
    mirror = [False, True, False, True, True]
    pick = list(range(B))
    ox, oy = [], []
    for c in KERNEL_CHOICES:
        (xl, xh), (yl, yh) = ref.origin_range(ref.scaled(w, c), w), ref.origin_range(ref.scaled(h, c), h)
        ox.append({"low": xl, "high": xh, "middle": (xl + xh) // 2}[where])
        oy.append({"low": yl, "high": yh, "middle": (yl + yh) // 2}[where])
    prep = InputPrep(B, (HS, WS), crop, dev, mean=ref.IMG_MEAN, scale_crop=KERNEL_CHOICES)
    rgb_d, lab_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(lab).to(dev)
    x = torch.full((B, 3, h, w), float("nan"), device=dev)
    lo = torch.full((B, h, w), -1, dtype=torch.int64, device=dev)
    prep.scale_crop_batch([rgb_d[b].data_ptr() for b in range(B)], [lab_d[b].data_ptr() for b in range(B)], (mirror, pick, ox, oy), x, lo,
                          _stream(dev))
    torch.cuda.synchronize()
    x, lo = x.cpu().numpy(), lo.cpu().numpy()
    for b in range(B):
        xr, lr = ref.item(RESIZED, ("k", b), rgb[b], lab[b], crop, KERNEL_CHOICES[b], ox[b], oy[b], mirror[b])
        bad = np.argwhere(x[b] != xr)
        assert bad.size == 0, f"item {b} (s = {KERNEL_CHOICES[b]}, origin {ox[b]}, {oy[b]}): {len(bad)} image values differ, first at {bad[0]}"
        bad = np.argwhere(lo[b] != lr)
        assert bad.size == 0, f"item {b} (s = {KERNEL_CHOICES[b]}, origin {ox[b]}, {oy[b]}): {len(bad)} labels differ, first at {bad[0]}"
    # images only: lab_out NULL
    prep2 = InputPrep(B, (HS, WS), crop, dev, mean=ref.IMG_MEAN, with_label=False, scale_crop=KERNEL_CHOICES)
    x2 = torch.full((B, 3, h, w), float("nan"), device=dev)
    prep2.scale_crop_batch([rgb_d[b].data_ptr() for b in range(B)], [None] * B, (mirror, pick, ox, oy), x2, None, _stream(dev))
    torch.cuda.synchronize()
    assert np.array_equal(x2.cpu().numpy(), x)


def test_scale_crop_refuses_what_the_descriptor_or_the_lds_cannot_hold(dev):
    """A choice index past the choices, and a geometry whose tile needs more LDS than the kernel has: errors, not launches.  The loader's
    InputPrep refuses the geometry when it is built, naming it."""
    import ctypes as C

    from simt_amd import _lib as L
    prep = InputPrep(1, (HS, WS), CROP, dev, mean=ref.IMG_MEAN, scale_crop=("1.0",))
    rgb_d = torch.zeros(HS, WS, 3, dtype=torch.uint8, device=dev)
    lab_d = torch.zeros(HS, WS, dtype=torch.uint8, device=dev)
    x = torch.empty(1, 3, CROP[1], CROP[0], device=dev)
    lo = torch.empty(1, CROP[1], CROP[0], dtype=torch.int64, device=dev)
    with pytest.raises(L.SimtHipError):
        prep.scale_crop_batch([rgb_d.data_ptr()], [lab_d.data_ptr()], ([False], [1], [0], [0]), x, lo, _stream(dev))
    d = L.ScaleCropDesc()
    d.B = L.SCALE_CROP_MAX + 1
    with pytest.raises(L.SimtHipError):
        L.call("simt_scale_crop", C.byref(d), _stream(dev))
    with pytest.raises(ValueError, match=r"4096 x 4096.*LDS"):          # 4096 rows -> 16: a tile reads 4096 source rows
        InputPrep(1, (4096, 4096), (32, 32), dev, scale_crop=("0.5",))


# ---- 2. loader -----------------------------------------------------------------------------------------------------------------------------
def _write_files(tmp_path, n):
    from PIL import Image
    rgb, lab = _frames(n, seed=2)
    (tmp_path / "img").mkdir()
    (tmp_path / "lab").mkdir()
    for i in range(n):
        Image.fromarray(rgb[i]).save(tmp_path / "img" / f"f{i}.png")
        Image.fromarray(lab[i]).save(tmp_path / "lab" / f"f{i}.png")
    (tmp_path / "list.lst").write_text("".join(f"img/f{i}.png lab/f{i}.png\n" for i in range(n)))
    return str(tmp_path), str(tmp_path / "list.lst"), rgb, lab


def _dataset(root, lst, mirror=True, choices=LOADER_CHOICES):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    return cityscapesPseudo(root, lst, crop_size=CROP, mean=ref.IMG_MEAN, mirror=mirror, scale_crop=choices)


def _collect(loader):
    out = []
    for images, labels, sizes, names in loader:
        out.append((images.clone(), labels.clone(), np.array(sizes), list(names)))
    torch.cuda.synchronize()
    return out


def _assert_same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for k, ((xa, la, sa, na), (xb, lb, sb, nb)) in enumerate(zip(a, b)):
        assert na == nb, (k, na, nb)
        assert np.array_equal(sa, sb), k
        assert torch.equal(xa, xb), f"batch {k}: images differ"
        assert torch.equal(la, lb), f"batch {k}: labels differ"


def _assert_equals_pillow(got, rgb, lab, seed, rank, mirror=True):
    """Every batch of `got` against the composition driven by the loader's generator: default_rng(seed + 7919 * rank)."""
    rng = np.random.default_rng(seed + 7919 * rank)
    all_draws = []
    for k, (x, lo, _sizes, names) in enumerate(got):
        fl, pick, ox, oy = ref.draws(rng, len(names), LOADER_CHOICES, CROP, mirror)
        all_draws.append((fl, pick, ox, oy))
        for b, name in enumerate(names):
            i = int(name[1:])
            xr, lr = ref.item(RESIZED, ("l", i), rgb[i], lab[i], CROP, LOADER_CHOICES[pick[b]], ox[b], oy[b], fl[b])
            assert np.array_equal(x[b].cpu().numpy(), xr), (k, b, name, pick[b], ox[b], oy[b], fl[b])
            assert np.array_equal(lo[b].cpu().numpy(), lr), (k, b, name, pick[b], ox[b], oy[b], fl[b])
    return all_draws


class _Counting:
    def __init__(self, ds):
        self.ds, self.calls, self.real = ds, [], ds.decode
        ds.decode = self

    def __call__(self, index):
        self.calls.append(self.ds.cache_key(index))
        return self.real(index)


def test_loader_equals_pillow_composition_cached_equals_uncached_and_ranks_draw_independently(dev, tmp_path):
    """7 items, B = 2, shuffle + mirror, 2 epochs, two data-parallel ranks.  Uncached = the Pillow composition driven by the same
    generator; cached = uncached, each item decoded once, the cache holding the original frames; the two ranks' draws differ."""
    pytest.importorskip("PIL.Image")
    root, lst, rgb, lab = _write_files(tmp_path, 7)
    seen = []
    for rank in (0, 1):
        kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2, rank=rank, world=2)
        unc = _collect(GpuLoader(_dataset(root, lst), 2, **kw))
        assert len(unc) == 2 * ((4, 3)[rank] // 2)
        seen.append(_assert_equals_pillow(unc, rgb, lab, 3, rank))
        ds = _dataset(root, lst)
        cnt = _Counting(ds)
        cache = DatasetCache((WS, HS), slab_slots=3, device=dev)
        got = _collect(GpuLoader(ds, 2, cache=cache, **kw))
        _assert_same_batches(unc, got)
        dealt = {n for (_x, _l, _s, names) in unc for n in names}
        assert len(cnt.calls) == len(set(cnt.calls)) == len(dealt) == len(cache)
        assert cache.hits + cache.misses == 2 * len(unc) and cache.misses == len(dealt)
    assert seen[0][0] != seen[1][0], "the two ranks made the same draws"
    picks = {p for r in seen for (_f, pk, _x, _y) in r for p in pk}
    assert picks == {0, 1, 2}, picks                                    # the seed exercises every choice


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_loader_start_batch_yields_the_tail(dev, tmp_path, cached):
    """7 items, B = 2 (3 batches per epoch), 3 epochs: from inside epoch 0, from an epoch boundary and from inside epoch 1."""
    pytest.importorskip("PIL.Image")
    root, lst, _rgb, _lab = _write_files(tmp_path, 7)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=5, epochs=3)
    full = _collect(GpuLoader(_dataset(root, lst), 2, **kw))
    assert len(full) == 9
    for n in (1, 3, 4):
        cache = DatasetCache((WS, HS), slab_slots=4, device=dev) if cached else None
        _assert_same_batches(full[n:], _collect(GpuLoader(_dataset(root, lst), 2, cache=cache, start_batch=n, **kw)))


def test_loader_without_the_flag_is_the_parent_loader(dev, tmp_path):
    """scale_crop=None: the batches are InputPrep.run of the same frames with the mirror draws the loader always made."""
    pytest.importorskip("PIL.Image")
    root, lst, rgb, lab = _write_files(tmp_path, 5)
    got = _collect(GpuLoader(_dataset(root, lst, choices=None), 2, shuffle=True, num_workers=2, device=dev, seed=4, epochs=2))
    assert len(got) == 4
    rng = np.random.default_rng(4)
    prep = InputPrep(2, (HS, WS), CROP, dev, mean=ref.IMG_MEAN)
    for x, lo, _s, names in got:
        flags = (rng.integers(0, 2, 2) == 0).tolist()
        ids = [int(n[1:]) for n in names]
        xr = torch.empty(2, 3, CROP[1], CROP[0], device=dev)
        lr = torch.empty(2, CROP[1], CROP[0], dtype=torch.int64, device=dev)
        prep.run(torch.from_numpy(rgb[ids]).to(dev), xr, torch.from_numpy(lab[ids]).to(dev), lr, mirror=flags)
        torch.cuda.synchronize()
        assert torch.equal(x, xr) and torch.equal(lo, lr)


def test_loader_names_the_frame_of_another_size(dev, tmp_path):
    from PIL import Image
    root, lst, _rgb, _lab = _write_files(tmp_path, 4)
    Image.fromarray(np.zeros((HS, WS + 2, 3), np.uint8)).save(tmp_path / "img" / "f1.png")
    with pytest.raises(ValueError, match=r"f1\.png.*162 x 96"):
        _collect(GpuLoader(_dataset(root, lst), 2, shuffle=False, num_workers=2, device=dev, seed=1, epochs=1))


# ---- 3. tools ------------------------------------------------------------------------------------------------------------------------------
def _tool_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    for d in ("train_img", "train_lab"):
        (tmp_path / d).mkdir(parents=True)
    lines = []
    for i in range(4):
        Image.fromarray(rng.integers(0, 256, (96, 192, 3), dtype=np.uint8)).save(tmp_path / "train_img" / f"t{i}.png")
        lab = rng.integers(0, 19, (96, 192), dtype=np.uint8)
        lab[rng.random(lab.shape) < 0.1] = 255
        Image.fromarray(lab).save(tmp_path / "train_lab" / f"t{i}.png")
        lines.append(f"train_img/t{i}.png train_lab/t{i}.png")
    (tmp_path / "pseudo.lst").write_text("\n".join(lines) + "\n")


def _loss_lines(out):
    return [re.sub(r"\s*\([0-9.]+ img/s\)", "", ln) for ln in out.splitlines() if ln.startswith("iter = ")]


def _same_snapshot(a, b):
    sa, sb = torch.load(a), torch.load(b)
    assert set(sa) == set(sb) and len(sa) > 0
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


def test_tool_scale_crop_resume_equals_one_run_and_cache_equals_off(dev, tmp_path, capsys):
    """trainV2_simt --model DeepLab --scale-crop 0.5 1.5 --random-mirror on 4 PNG pairs, B = 2, at 129 x 65: 3 steps + resume + 3 steps
    equals 6 steps in the loss lines and the final snapshot (the resumed loader skips three batches' draws), and `--cache-dataset device`
    (original frames in the cache) equals `off`."""
    pytest.importorskip("PIL.Image")
    from simt_amd.tools import trainV2_simt as tool
    _tool_files(tmp_path / "data")
    common = ["--model", "DeepLab", "--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3", "--input-size-target", "129,65",
              "--batch-size", "2", "--num-steps", "50", "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "",
              "--num-workers", "2", "--data-dir-target", str(tmp_path / "data"), "--data-list-target", str(tmp_path / "data" / "pseudo.lst"),
              "--random-mirror", "--scale-crop", "0.5", "1.5"]

    def run(tag, stop, *flags):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(flags))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6)
    assert len(_loss_lines(out_a)) == 6 and "dataset cache:" not in out_a
    out_b1, _ = run("b", 3, "--train-state", state)
    assert _loss_lines(out_b1) == _loss_lines(out_a)[:3]
    out_b2, snap_b = run("b", 6, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert _loss_lines(out_b2) == _loss_lines(out_a)[3:], (out_a, out_b2)
    _same_snapshot(snap_a, snap_b)
    out_c, snap_c = run("c", 6, "--cache-dataset", "device")
    assert _loss_lines(out_c) == _loss_lines(out_a), (out_a, out_c)
    _same_snapshot(snap_a, snap_c)
    lines = re.findall(r"dataset cache: rank 0 epoch (\d+): (\d+) hits, (\d+) misses, ([0-9.]+) GB of ([0-9.]+) GB", out_c)
    assert [(int(e), int(h), int(m)) for (e, h, m, _g, _b) in lines[:3]] == [(0, 0, 4), (1, 4, 0), (2, 4, 0)], out_c
    # a resume with other choices is refused, the field named
    with pytest.raises(SystemExit, match="scale_crop"):
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state, "--scale-crop", "0.5", "1.0"])
    capsys.readouterr()
