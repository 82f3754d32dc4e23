"""The device-resident dataset cache (simt_amd/data/cache.py, csrc/dataset_cache.hip, GpuLoader(cache=...), --cache-dataset device).

Every comparison is between two paths over the same bytes and therefore BITWISE (torch.equal / np.array_equal): the gather kernel against
simt_image_to_input + simt_label_nearest, the cached loader against the uncached one (order, content, sizes, names, decode counts),
and the tools with `--cache-dataset device` against `off` (loss lines and final snapshot)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import pil_resize as pr
from simt_amd import _lib as L
from simt_amd.data.cache import DatasetCache, slot_bytes
from simt_amd.data.pipeline import GpuLoader, InputPrep

pytestmark = pytest.mark.gpu


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 8])
@pytest.mark.parametrize("hw", [(512, 1024), (768, 768), (512, 512), (321, 321)])
def test_cache_gather_equals_image_to_input_and_label_nearest(dev, hw, B):
    """Slots that are non-contiguous, out of order, in different slabs and repeated within a batch; mixed per-item mirror flags.  The
    reference path runs on the same resized frames: simt_image_to_input (rgb_order = flag) and simt_label_nearest with identity tables
    (flip_x = flag), item by item."""
    h, w = hw
    g = torch.Generator().manual_seed(h * 7 + w + B)
    cache = DatasetCache((w, h), slab_slots=3, device=dev)            # 3 slots per slab: 7 slots span 3 slabs
    nslot = 7
    frames = torch.randint(0, 256, (nslot, h, w, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, 256, (nslot, h, w), dtype=torch.uint8, generator=g).to(dev)
    for k in range(nslot):
        s = cache.reserve(("f%d" % k, "l%d" % k))
        cache.img_view(s).copy_(frames[k].reshape(-1))
        cache.lab_view(s).copy_(labels[k].reshape(-1))
    assert len(cache.slabs) == 3
    pick = [5, 0, 6, 0, 3, 2, 6, 1][:B]                               # out of order, across slabs, 0 and 6 repeated
    mirror = [bool((k * 5 + B) % 3 == 0) for k in range(B)]
    if B > 1:
        assert any(mirror) and not all(mirror)
    prep = InputPrep(B, (h, w), (w, h), dev, mean=pr.IMG_MEAN)
    x = torch.full((B, 3, h, w), float("nan"), device=dev)
    lo = torch.full((B, h, w), -1, dtype=torch.int64, device=dev)
    prep.gather([cache.img_ptr(s) for s in pick], [cache.lab_ptr(s) for s in pick], mirror, x, lo, _stream(dev))
    xr = torch.full((B, 3, h, w), float("nan"), device=dev)
    lr = torch.full((B, h, w), -1, dtype=torch.int64, device=dev)
    ident_y = torch.arange(h, dtype=torch.int32, device=dev)
    ident_x = torch.arange(w, dtype=torch.int32, device=dev)
    m = prep.mean
    for b, s in enumerate(pick):
        f = 1 if mirror[b] else 0
        L.call("simt_image_to_input", frames[s].data_ptr(), xr[b].data_ptr(), 1, h, w, m[0], m[1], m[2], f, _stream(dev))
        L.call("simt_label_nearest", labels[s].data_ptr(), lr[b].data_ptr(), 1, h, w, h, w, ident_y.data_ptr(), ident_x.data_ptr(), f,
               _stream(dev))
    torch.cuda.synchronize()
    assert torch.equal(x, xr), "image planes differ from simt_image_to_input"
    assert torch.equal(lo, lr), "labels differ from simt_label_nearest"
    # images only: no label slab, lab_out NULL
    x2 = torch.full((B, 3, h, w), float("nan"), device=dev)
    prep.gather([cache.img_ptr(s) for s in pick], [None] * B, mirror, x2, None, _stream(dev))
    torch.cuda.synchronize()
    assert torch.equal(x2, xr)


@pytest.mark.parametrize("geom", [((1024, 2048), (512, 1024)), ((1024, 2048), (768, 768)), ((96, 192), (321, 321)), ((40, 24), (12, 20))])
def test_label_nearest_u8_equals_label_nearest_cast(dev, geom):
    (H, W), (h, w) = geom
    N = 3
    g = torch.Generator().manual_seed(H + w)
    src = torch.randint(0, 256, (N, H, W), dtype=torch.uint8, generator=g).to(dev)
    prep = InputPrep(N, (H, W), (w, h), dev, mean=pr.IMG_MEAN)
    ref = torch.full((N, h, w), -1, dtype=torch.int64, device=dev)
    got = torch.full((N, h, w), 77, dtype=torch.uint8, device=dev)
    L.call("simt_label_nearest", src.data_ptr(), ref.data_ptr(), N, H, W, h, w, prep.ytab.data_ptr(), prep.xtab.data_ptr(), 0, _stream(dev))
    L.call("simt_label_nearest_u8", src.data_ptr(), got.data_ptr(), N, H, W, h, w, prep.ytab.data_ptr(), prep.xtab.data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    assert torch.equal(got, ref.to(torch.uint8))


def test_cache_gather_refuses_more_items_than_the_descriptor_holds(dev):
    d = L.GatherDesc()
    d.B, d.h, d.w = L.GATHER_MAX + 1, 4, 4
    d.x = torch.empty(16, device=dev).data_ptr()
    with pytest.raises(L.SimtHipError):
        L.call("simt_cache_gather", C.byref(d), _stream(dev))


# ---- 2.-6. loader ------------------------------------------------------------------------------------------------------------------------
def _write_files(tmp_path, Image, n, hw=(64, 128), repeat_list=1):
    rng = np.random.default_rng(2)
    (tmp_path / "img").mkdir()
    (tmp_path / "lab").mkdir()
    lines = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(tmp_path / "img" / f"f{i}.png")
        lab = rng.integers(0, 19, hw, dtype=np.uint8)
        lab[rng.random(hw) < 0.1] = 255
        Image.fromarray(lab).save(tmp_path / "lab" / f"f{i}.png")
        lines.append(f"img/f{i}.png lab/f{i}.png")
    (tmp_path / "list.lst").write_text("\n".join(lines * repeat_list) + "\n")
    return str(tmp_path), str(tmp_path / "list.lst")


class _Counting:
    """ds.decode wrapped in a counter (the loader calls it from worker threads: list.append is atomic)."""

    def __init__(self, ds):
        self.ds, self.calls, self.real = ds, [], ds.decode
        ds.decode = self

    def __call__(self, index):
        self.calls.append(self.ds.cache_key(index))
        return self.real(index)


def _dataset(root, lst, crop=(48, 24), mirror=True, **kw):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    return cityscapesPseudo(root, lst, crop_size=crop, mean=pr.IMG_MEAN, mirror=mirror, **kw)


def _collect(loader):
    """Every batch of the loader, cloned while it is valid (the loader's consumer protocol: batch k is valid until call k + hold)."""
    out = []
    for images, labels, sizes, names in loader:
        out.append((images.clone(), None if labels is None else labels.clone(), np.array(sizes), list(names)))
    torch.cuda.synchronize()
    return out


def _assert_same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for k, ((xa, la, sa, na), (xb, lb, sb, nb)) in enumerate(zip(a, b)):
        assert na == nb, (k, na, nb)
        assert np.array_equal(sa, sb), k
        assert torch.equal(xa, xb), f"batch {k}: images differ"
        assert (la is None and lb is None) or torch.equal(la, lb), f"batch {k}: labels differ"


def _dealt(ds, B, seed, epochs, rank=0, world=1):
    """The keys the loader deals, epoch by epoch, incomplete last batch dropped (GpuLoader._order restated)."""
    out = []
    for e in range(epochs):
        idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(seed + e)).tolist()[rank::world]
        out.append([ds.cache_key(i) for i in idx[:len(idx) // B * B]])
    return out


@pytest.mark.parametrize("budget_items", [None, 4])
def test_cached_loader_equals_uncached_and_decodes_each_item_once(dev, tmp_path, budget_items):
    """11 items, B = 2 (each epoch drops one), shuffle + mirror, 3 epochs.  Uncached: 3 x the dealt items are decoded.  Cached: each item
    once, the first time it is dealt -- an item that fell into epoch one's dropped batch is decoded when it first appears.  With a budget
    of 4 of the 11 items: equal batches still; decodes = first sightings + every later sighting of an item that got no slot."""
    Image = pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, Image, 11)
    ds0, ds1 = _dataset(root, lst), _dataset(root, lst)
    c0, c1 = _Counting(ds0), _Counting(ds1)
    ref = _collect(GpuLoader(ds0, 2, shuffle=True, num_workers=2, device=dev, seed=3, epochs=3))
    budget = None if budget_items is None else budget_items * slot_bytes((48, 24))
    cache = DatasetCache((48, 24), budget_bytes=budget, slab_slots=3, device=dev)
    log = []
    got = _collect(GpuLoader(ds1, 2, shuffle=True, num_workers=2, device=dev, seed=3, epochs=3, cache=cache,
                             on_epoch=lambda *a: log.append(a)))
    assert len(ref) == 15
    _assert_same_batches(ref, got)
    dealt = _dealt(ds0, 2, 3, 3)
    assert sorted(c0.calls) == sorted(k for ep in dealt for k in ep) and len(c0.calls) == 30
    flat = [k for ep in dealt for k in ep]
    first = list(dict.fromkeys(flat))
    assert len(first) == 11                                       # 3 epochs of 10 out of 11: every item appears
    assert any(k not in dealt[0] for k in first)                  # ... one of them not in epoch one
    if budget_items is None:
        assert sorted(c1.calls) == sorted(first)
        assert len(cache) == 11 and len(cache.slabs) == 4 and not cache.closed
        seen, expect_log = set(), []
        for e, ep in enumerate(dealt):                            # per epoch: misses = keys never dealt before
            new = set(ep) - seen
            expect_log.append((e, len(ep) - len(new), len(new)))
            seen |= new
        assert [(e, h, m) for (e, h, m, _b) in log] == expect_log and expect_log[0] == (0, 0, 10)
    else:
        kept = set(first[:4])                                     # slots go to the first 4 items sighted; nothing is evicted
        assert set(cache.table) == kept and cache.closed and cache.bytes == 4 * slot_bytes((48, 24))
        expect = [k for j, k in enumerate(flat) if k not in kept or flat.index(k) == j]
        assert sorted(c1.calls) == sorted(expect) and len(expect) == 4 + sum(1 for k in flat if k not in kept)
    assert log[-1][3] == cache.bytes and cache.hits + cache.misses == 30 and cache.misses == len(c1.calls)


def test_cached_loader_gradient_accumulation_hold(dev, tmp_path):
    """hold = 2 (--iter-size 2): the loop pulls two micro-batches before it enqueues the step that reads them; both stay valid while
    ~20 ms of GPU work enqueued after the pulls runs first (the pattern of test_prefetcher_gradient_accumulation_hold)."""
    Image = pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, Image, 9)
    ref = _collect(GpuLoader(_dataset(root, lst), 2, shuffle=True, num_workers=2, device=dev, seed=5, epochs=4))
    cache = DatasetCache((48, 24), slab_slots=4, device=dev)
    it = iter(GpuLoader(_dataset(root, lst), 2, shuffle=True, num_workers=2, device=dev, seed=5, epochs=4, hold=2, cache=cache))
    busy = torch.zeros(64 << 20, device=dev)
    got = []
    for _step in range(len(ref) // 2):
        mb = [next(it) for _ in range(2)]
        for _ in range(40):
            busy.add_(1.0)
        for images, labels, sizes, names in mb:
            got.append((images.clone(), labels.clone(), np.array(sizes), list(names)))
    torch.cuda.synchronize()
    assert len(ref) == 16 and len(got) == 16
    _assert_same_batches(ref, got)


def test_cached_loader_data_parallel_ranks(dev, tmp_path):
    """world = 2: each rank caches what it is dealt and equals its uncached twin."""
    Image = pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, Image, 11)
    for rank in (0, 1):
        kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=3, rank=rank, world=2)
        ref = _collect(GpuLoader(_dataset(root, lst), 2, **kw))
        ds = _dataset(root, lst)
        cnt = _Counting(ds)
        cache = DatasetCache((48, 24), slab_slots=4, device=dev)
        got = _collect(GpuLoader(ds, 2, cache=cache, **kw))
        _assert_same_batches(ref, got)
        flat = [k for ep in _dealt(ds, 2, 3, 3, rank, 2) for k in ep]
        assert sorted(cnt.calls) == sorted(set(flat)) and len(cache) == len(set(flat))


def test_cache_keys_are_file_paths_max_iters_repeats_share_slots(dev, tmp_path):
    """max_iters repeats the list (the reference's "infinite" loader): 5 files listed for max_iters = 17 are 20 entries, 5 slots."""
    Image = pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, Image, 5)
    ds = _dataset(root, lst, max_iters=17)
    assert len(ds) == 20
    cnt = _Counting(ds)
    cache = DatasetCache((48, 24), slab_slots=2, device=dev)
    ref = _collect(GpuLoader(_dataset(root, lst, max_iters=17), 4, shuffle=True, num_workers=2, device=dev, seed=1, epochs=2))
    got = _collect(GpuLoader(ds, 4, shuffle=True, num_workers=2, device=dev, seed=1, epochs=2, cache=cache))
    _assert_same_batches(ref, got)
    assert len(cache) == 5 and len(cache.slabs) == 3 and len(cnt.calls) == 5 and len(set(cnt.calls)) == 5


def test_cached_loader_images_only_dataset(dev, tmp_path):
    """cityscapesDataSet (no labels) goes through the same cache with no label slab."""
    Image = pytest.importorskip("PIL.Image")
    from simt_amd.dataset.cityscapes_dataset import cityscapesDataSet
    root, _ = _write_files(tmp_path, Image, 5)
    os.rename(os.path.join(root, "img"), os.path.join(root, "val"))
    lst = os.path.join(root, "val.txt")
    open(lst, "w").write("".join(f"f{i}.png\n" for i in range(5)))
    mk = lambda: cityscapesDataSet(root, lst, crop_size=(48, 24), mean=pr.IMG_MEAN, set="val")
    ref = _collect(GpuLoader(mk(), 2, shuffle=True, num_workers=2, device=dev, seed=1, epochs=3))
    ds = mk()
    cnt = _Counting(ds)
    cache = DatasetCache((48, 24), with_label=False, slab_slots=2, device=dev)
    got = _collect(GpuLoader(ds, 2, shuffle=True, num_workers=2, device=dev, seed=1, epochs=3, cache=cache))
    _assert_same_batches(ref, got)
    assert all(lab is None for (_x, lab, _s, _n) in got) and all(s[1] is None for s in cache.slabs)
    assert len(cnt.calls) == len(set(cnt.calls)) == len(cache) == 5
    assert cache.bytes == sum(s[2] for s in cache.slabs) * slot_bytes((48, 24), with_label=False)


# ---- 7. Cityscapes geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("crop", [(1024, 512), (768, 768)])
def test_cityscapes_geometry_second_epoch_equals_first_and_restatement(dev, tmp_path, crop, mirror):
    """Two 1024 x 2048 frame pairs (the frames of test_cityscapes_geometry_batch_and_mirror_quirk) through the cached loader for two
    epochs: epoch two (all hits) equals epoch one (all misses) and both equal oracle.pil_resize.cityscapes_pseudo_item.  With
    `mirror` the loader draws a flag per item: the draws are restated here from the loader's seed."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (2, 1024, 2048, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:1024, 0:2048]
    rgb[0, :, :, 1] = ((xx // 9 + yy // 5) % 2 * 255).astype(np.uint8)
    lab = rng.integers(0, 19, (2, 1024, 2048), dtype=np.uint8)
    lab[rng.random(lab.shape) < 0.1] = 255
    (tmp_path / "img").mkdir()
    (tmp_path / "lab").mkdir()
    for i in range(2):
        Image.fromarray(rgb[i]).save(tmp_path / "img" / f"f{i}.png", compress_level=1)
        Image.fromarray(lab[i]).save(tmp_path / "lab" / f"f{i}.png", compress_level=1)
    lst = tmp_path / "list.lst"
    lst.write_text("img/f0.png lab/f0.png\nimg/f1.png lab/f1.png\n")
    ds = _dataset(str(tmp_path), str(lst), crop=crop, mirror=mirror)
    cnt = _Counting(ds)
    seed = 2 if mirror else 0
    cache = DatasetCache(crop, device=dev)
    got = _collect(GpuLoader(ds, 2, shuffle=False, num_workers=2, device=dev, seed=seed, epochs=2, cache=cache))
    assert len(got) == 2 and len(cnt.calls) == 2 and (cache.hits, cache.misses) == (2, 2)
    draws = np.random.default_rng(seed)
    flags = [(draws.integers(0, 2, 2) == 0).tolist() for _ in range(2)] if mirror else [[False, False]] * 2
    if mirror:
        assert {f for ep in flags for f in ep} == {False, True}            # the seed exercises both branches
    for (x, lo, _s, names), fl in zip(got, flags):
        assert names == ["f0", "f1"]
        for b in range(2):
            img, lb = pr.cityscapes_pseudo_item(rgb[b], lab[b], crop[0], crop[1], mirror_flip=-1 if fl[b] else 1)
            assert np.array_equal(x[b].cpu().numpy(), img), (b, fl)
            assert np.array_equal(lo[b].cpu().numpy().astype(np.float32), lb), (b, fl)
    for b in range(2):                                                     # epoch two (hits) = epoch one (misses) wherever the flag is the same
        if flags[0][b] == flags[1][b]:
            assert torch.equal(got[0][0][b], got[1][0][b]) and torch.equal(got[0][1][b], got[1][1][b])
    assert any(flags[0][b] == flags[1][b] for b in range(2))


# ---- 8. tools ----------------------------------------------------------------------------------------------------------------------------
def _tool_files(tmp_path, Image):
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
    """The `iter = ...` lines without the wall-clock rate the warm-up tool appends."""
    return [re.sub(r"\s*\([0-9.]+ img/s\)", "", ln) for ln in out.splitlines() if ln.startswith("iter = ")]


@pytest.mark.parametrize("which", ["warmup-DeepLabVGG", "simt-DeepLabv3"])
def test_tools_cache_dataset_device_equals_off(dev, tmp_path, capsys, which):
    """4 files, B = 2, 6 steps = 3 epochs, the full model on files of a tiny geometry, --random-mirror: `--cache-dataset device` against
    `off`: the loss line of every step and every tensor of the final snapshot are equal, and the log has one hit / miss line per
    epoch.  `off` runs twice first: the comparison only means something if the step itself is reproducible from run to run (it is, for both
    tools: the two `off` runs are held to the same bitwise equality)."""
    Image = pytest.importorskip("PIL.Image")
    if which.startswith("warmup"):
        from simt_amd.tools import trainV1_warmup as tool
        extra = ["--model", "DeepLabVGG", "--learning-rate", "2.5e-4"]
    else:
        from simt_amd.tools import trainV2_simt as tool
        extra = ["--model", "DeepLabv3", "--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3"]
    _tool_files(tmp_path, Image)

    def run(tag, *flags):
        snap = str(tmp_path / tag)
        tool.main(extra + ["--data-dir-target", str(tmp_path), "--data-list-target", str(tmp_path / "pseudo.lst"),
                           "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--num-steps-stop", "6",
                           "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--snapshot-dir", snap,
                           "--num-workers", "2", "--random-mirror"] + list(flags))
        out = capsys.readouterr().out
        return out, torch.load(os.path.join(snap, "GTA5_6.pth"))

    def same(a, b):
        assert _loss_lines(a[0]) == _loss_lines(b[0]) and len(_loss_lines(a[0])) == 6, (a[0], b[0])
        assert set(a[1]) == set(b[1])
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), k

    off1, off2 = run("off1"), run("off2", "--cache-dataset", "off")
    same(off1, off2)
    assert "dataset cache:" not in off1[0] + off2[0]
    on = run("on", "--cache-dataset", "device")
    same(off1, on)
    lines = re.findall(r"dataset cache: rank 0 epoch (\d+): (\d+) hits, (\d+) misses, ([0-9.]+) GB", on[0])
    assert [(int(e), int(h), int(m)) for (e, h, m, _g) in lines[:3]] == [(0, 0, 4), (1, 4, 0), (2, 4, 0)], on[0]
    # a budget too small for one item: nothing is cached, the run is the same
    none = run("none", "--cache-dataset", "device", "--cache-gb", "0.00001")
    same(off1, none)
    assert re.search(r"epoch 1: 0 hits, 4 misses, 0.000 GB", none[0])
