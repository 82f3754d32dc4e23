"""--mask-patches on the GPU: simt_patch_mask against the numpy restatement of its contract (tests/_patch_mask_ref.py) bit for
bit, in place and out of place; its refusals; the loader with the flag on against the restatement applied to the flag-off loader's batches;
both training tools resumed through --train-state."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _patch_mask_ref as ref
from simt_amd import _lib as L
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import IMG_MEAN, GpuLoader, InputPrep
from test_patch_mask_cpu import MASKS, SHAPES, mask_words, special_bits

pytestmark = pytest.mark.gpu

GUARD = 64                      # bytes on both sides of the output
PATTERN = 0x5A


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(shape):
    """The input words and, per mask, (row words, expected words) of one shape: computed once, shared by both placements, never changed."""
    if shape not in _CASES:
        B, h, w, P = shape
        x = special_bits(B, h, w)
        x.setflags(write=False)
        per_mask = {}
        for kind in MASKS:
            words = mask_words(kind, B, h, w, P)
            want = ref.out_of_place(x, words, P)
            want.setflags(write=False)
            per_mask[kind] = (words, want)
        _CASES[shape] = (x, per_mask)
    return _CASES[shape]


def _guarded(B, h, w, dev):
    n = B * 3 * h * w
    buf = torch.full((GUARD + 4 * n + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + 4 * n].view(torch.float32).view(B, 3, h, w)


def _differences(got, want):
    bad = np.argwhere(got != want)
    return "" if bad.size == 0 else (f"{len(bad)} of {want.size} words differ, first at {tuple(bad[0])}: "
                                     f"{got[tuple(bad[0])]:#010x} != {want[tuple(bad[0])]:#010x}")


@pytest.mark.parametrize("place", ["out_of_place", "in_place"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement_bit_for_bit(dev, shape, place):
    """Every mask of MASKS on one shape, through InputPrep.patch_mask_batch (one launch per 16 items).  The expected words hold for both
    placements: in place the kept words must keep their bits, which is what equality with the restatement says."""
    B, h, w, P = shape
    x, per_mask = _case(shape)
    prep = InputPrep(B, (h, w), (w, h), dev, patch_mask=(P, 0.7))
    n = B * 3 * h * w
    x_host = torch.from_numpy(x.view(np.int32).copy())
    for kind in MASKS:
        words, want = per_mask[kind]
        if place == "out_of_place":
            x_d = x_host.to(dev).view(torch.float32)
            buf, x_out = _guarded(B, h, w, dev)
            prep.patch_mask_batch(x_d, words, x_out, _stream(dev))
            torch.cuda.synchronize()
            assert np.array_equal(x_d.view(torch.int32).cpu().numpy().view(np.uint32), x), f"{kind}: the input was written"
        else:
            buf, x_out = _guarded(B, h, w, dev)
            x_out.view(torch.int32).copy_(x_host)
            prep.patch_mask_batch(x_out, words, x_out, _stream(dev))
            torch.cuda.synchronize()
        got = x_out.view(torch.int32).cpu().numpy().view(np.uint32)
        assert _differences(got, want) == "", f"mask {kind!r}, {place}"
        g = buf.cpu().numpy()
        assert (g[:GUARD] == PATTERN).all() and (g[GUARD + 4 * n:] == PATTERN).all(), f"mask {kind!r}: a guard band was written"


def test_in_place_stores_only_blanked_words(dev):
    """In place nothing is copied: a second launch over the result with an all-kept mask, and one with the same mask, change no word."""
    shape = SHAPES[0]
    B, h, w, P = shape
    x, per_mask = _case(shape)
    words, want = per_mask["random"]
    prep = InputPrep(B, (h, w), (w, h), dev, patch_mask=(P, 0.7))
    x_d = torch.from_numpy(x.view(np.int32).copy()).to(dev).view(torch.float32)
    for wd in (words, per_mask["kept"][0], words):
        prep.patch_mask_batch(x_d, wd, x_d, _stream(dev))
    torch.cuda.synchronize()
    assert _differences(x_d.view(torch.int32).cpu().numpy().view(np.uint32), want) == ""


def test_refusals_return_the_error_without_launching(dev):
    B, h, w, P = 2, 8, 8, 4
    n = B * 3 * h * w
    x = torch.zeros(n + 64, device=dev)
    x_out = torch.full((n + 64,), 7.0, device=dev)
    rows = np.full((L.PATCH_MASK_MAX, L.PATCH_MASK_GRID), 0xFFFFFFFF, dtype=np.uint32)

    def desc():
        d = L.PatchMaskDesc()
        d.x, d.x_out, d.B, d.h, d.w, d.patch = x.data_ptr(), x_out.data_ptr(), B, h, w, P
        C.memmove(d.rows, rows.ctypes.data, rows.nbytes)
        return d

    def no_input(d):
        d.x = None

    def no_output(d):
        d.x_out = None

    def no_items(d):
        d.B = 0

    def negative_items(d):
        d.B = -1

    def too_many_items(d):
        d.B = L.PATCH_MASK_MAX + 1

    def no_patch(d):
        d.patch = 0

    def negative_patch(d):
        d.patch = -4

    def too_many_patch_rows(d):
        d.h, d.w, d.patch = 33, 1, 1

    def too_many_patch_columns(d):
        d.h, d.w, d.patch = 1, 33, 1

    def too_many_pixels(d):
        d.h, d.w, d.patch = 65536, 32768, 4096          # 16 x 8 patches, h * w = 2^31

    def misaligned_input(d):
        d.x = x.data_ptr() + 4

    def misaligned_output(d):
        d.x_out = x_out.data_ptr() + 4

    def output_overlaps_behind(d):
        d.x_out = x.data_ptr() + 16

    def output_overlaps_in_front(d):
        d.x, d.x_out = x.data_ptr() + 4 * n - 16, x.data_ptr()

    changes = (no_input, no_output, no_items, negative_items, too_many_items, no_patch, negative_patch, too_many_patch_rows,
               too_many_patch_columns, too_many_pixels, misaligned_input, misaligned_output, output_overlaps_behind, output_overlaps_in_front)
    for change in changes:
        d = desc()
        change(d)
        with pytest.raises(L.SimtHipError, match=r"code 1\b"):
            L.call("simt_patch_mask", C.byref(d), _stream(dev))
    with pytest.raises(L.SimtHipError, match=r"code 1\b"):                  # a NULL descriptor
        L.call("simt_patch_mask", None, _stream(dev))
    torch.cuda.synchronize()
    assert (x_out == 7.0).all() and (x == 0).all()                         # nothing ran
    x.fill_(3.0)
    L.call("simt_patch_mask", C.byref(desc()), _stream(dev))               # the descriptor itself is sound: everything blanked
    torch.cuda.synchronize()
    assert (x_out[:n].view(torch.int32) == 0).all() and (x_out[n:] == 7.0).all() and (x == 3.0).all()


# ---- 2. the loader ------------------------------------------------------------------------------------------------------------------------------
HS, WS = 96, 160
CROP = (72, 40)
N_CLASSES = 19
CHOICES = ("0.5", "1.0", "1.5")
MASK = (8, 0.7)                 # 9 x 5 patches of the crop; 72 % 4 == 0 and 8 % 4 == 0: the 16-byte flavour
GRID_HW = (5, 9)


def _write_files(tmp_path, n):
    from PIL import Image
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)
    (tmp_path / "img").mkdir()
    (tmp_path / "lab").mkdir()
    for i in range(n):
        blocks = rng.integers(0, N_CLASSES, (HS // 16, WS // 16)).astype(np.uint8)
        blocks[rng.random(blocks.shape) < 0.15] = 255
        lab = np.kron(blocks, np.ones((16, 16), np.uint8))
        Image.fromarray(rgb[i]).save(tmp_path / "img" / f"f{i}.png")
        Image.fromarray(lab).save(tmp_path / "lab" / f"f{i}.png")
    (tmp_path / "list.lst").write_text("".join(f"img/f{i}.png lab/f{i}.png\n" for i in range(n)))
    return str(tmp_path), str(tmp_path / "list.lst")


def _dataset(root, lst, mask, choices=None, mix=None, photo=None, tv=False, crop=CROP):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    return cityscapesPseudo(root, lst, crop_size=crop, mean=IMG_MEAN, mirror=True, scale_crop=choices, class_mix=mix, photometric=photo,
                            teacher_view=tv, patch_mask=mask)


def _collect(loader):
    out = []
    for batch in loader:
        out.append(tuple(t.clone() if torch.is_tensor(t) else t for t in batch))
    torch.cuda.synchronize()
    return out


def _same_image(a, b, what):
    diff = (a.view(torch.int32) != b.view(torch.int32)).sum(dim=(1, 2, 3)).tolist()
    assert not any(diff), f"{what}: image words that differ per item: {diff}"


def _assert_same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for k, (p, q) in enumerate(zip(a, b)):
        assert list(p[3]) == list(q[3]) and np.array_equal(np.array(p[2]), np.array(q[2])), (k, p[3], q[3])
        _same_image(p[0], q[0], f"batch {k}")
        assert (p[1] is None and q[1] is None) or torch.equal(p[1], q[1]), f"batch {k}: labels differ"


def _masked_by_the_restatement(off, seed, rank, mask=MASK, grid=GRID_HW, skip=0):
    """The flag-off loader's batches with their images masked by the restatement, with the draws of generator(seed, rank); labels as they were."""
    rng = ref.generator(seed, rank)
    out, blanked, total = [], 0, 0
    for k, b in enumerate(off):
        words = ref.draws(rng, len(b[3]), grid[0], grid[1], mask[1])
        if k < skip:
            continue
        xb = b[0].view(torch.int32).cpu().numpy().view(np.uint32)
        xo = ref.out_of_place(xb, words, mask[0])
        blanked += int(ref.mask_pixels(words, xb.shape[2], xb.shape[3], mask[0]).sum())
        total += xb.shape[0] * xb.shape[2] * xb.shape[3]
        out.append((torch.from_numpy(xo.view(np.int32)).view(torch.float32).to(b[0].device),) + tuple(b[1:]))
    assert 0.4 < blanked / total < 0.95
    return out


@pytest.mark.parametrize("mode", ["plain", "scale-crop", "class-mix+photometric", "odd-crop"])
def test_loader_equals_restatement_on_flag_off_batches_and_cached_equals_uncached(dev, tmp_path, mode):
    """8 items, B = 2, shuffle + mirror, 2 epochs: the masked loader = the restatement applied to the images of the loader without the flag
    (not one of its other draws moves); the labels are the flag-off labels; with a DatasetCache the same.  odd-crop: 71 x 39, the dword flavour."""
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    choices = CHOICES if mode == "scale-crop" else None
    mix, photo = ((N_CLASSES, 0.7), (0.5, 0.7)) if mode == "class-mix+photometric" else (None, None)
    crop = (71, 39) if mode == "odd-crop" else CROP
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2)
    off = _collect(GpuLoader(_dataset(root, lst, None, choices, mix, photo, crop=crop), 2, **kw))
    assert len(off) == 8
    want = _masked_by_the_restatement(off, 3, 0)
    _assert_same_batches(want, _collect(GpuLoader(_dataset(root, lst, MASK, choices, mix, photo, crop=crop), 2, **kw)))
    cache = DatasetCache((WS, HS) if choices is not None else crop, slab_slots=3, device=dev)
    _assert_same_batches(want, _collect(GpuLoader(_dataset(root, lst, MASK, choices, mix, photo, crop=crop), 2, cache=cache, **kw)))
    assert cache.misses == 8 and cache.hits == 8


def test_loader_teacher_view(dev, tmp_path, monkeypatch):
    """teacher_view with the mask alone: the weak view is the flag-off batch, the strong view its masked copy (out of place, into a buffer of
    its own), no item map.  With class-mix too: weak view and item map are those of the run without the mask, the strong view is that
    run's, masked in place.  The flag-off loader makes no mask buffer and no launch of the kernel."""
    pytest.importorskip("PIL.Image")
    from simt_amd.data import pipeline
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2)
    made, calls = [], []

    class Spy(pipeline.DevicePrefetcher):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    real_call = L.call
    monkeypatch.setattr(pipeline, "DevicePrefetcher", Spy)
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    off = _collect(GpuLoader(_dataset(root, lst, None), 2, **kw))
    pf = made.pop()
    assert len(off) == 8 and "simt_patch_mask" not in calls and pf.mask_fn is None and not any("xk" in s for s in pf.slots)
    got = _collect(GpuLoader(_dataset(root, lst, MASK, tv=True), 2, **kw))
    pf = made.pop()
    assert all(len(b) == 6 and b[5] is None for b in got) and all("xk" in s for s in pf.slots) and calls.count("simt_patch_mask") >= 8
    _assert_same_batches(off, [(b[4], b[1], b[2], b[3]) for b in got])                        # the weak view: whole
    _assert_same_batches(_masked_by_the_restatement(off, 3, 0), [b[:4] for b in got])         # the strong view: its masked copy
    mix = (N_CLASSES, 0.7)
    base = _collect(GpuLoader(_dataset(root, lst, None, mix=mix, tv=True), 2, **kw))
    made.pop()
    got = _collect(GpuLoader(_dataset(root, lst, MASK, mix=mix, tv=True), 2, **kw))
    pf = made.pop()
    assert not any("xk" in s for s in pf.slots)                                               # in place in xm: x stays the weak view
    _assert_same_batches(_masked_by_the_restatement([b[:4] for b in base], 3, 0), [b[:4] for b in got])
    for k, (b, o) in enumerate(zip(got, base)):
        _same_image(b[4], o[4], f"weak view of batch {k}")
        assert torch.equal(b[5], o[5]), f"item map of batch {k}"
    _assert_same_batches(off, [(b[4], o[1], b[2], b[3]) for b, o in zip(got, off)])
    # ranks draw other masks, each its documented ones
    for rank in (0, 1):
        kr = dict(kw, rank=rank, world=2)
        off_r = _collect(GpuLoader(_dataset(root, lst, None), 2, **kr))
        _assert_same_batches(_masked_by_the_restatement(off_r, 3, rank), _collect(GpuLoader(_dataset(root, lst, MASK), 2, **kr)))
    assert not np.array_equal(ref.draws(ref.generator(3, 0), 2, 5, 9, 0.7), ref.draws(ref.generator(3, 1), 2, 5, 9, 0.7))


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_loader_start_batch_yields_the_tail(dev, tmp_path, cached):
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=5, epochs=2)
    mix, photo = (N_CLASSES, 0.6), (0.5, 0.7)
    full = _collect(GpuLoader(_dataset(root, lst, MASK, None, mix, photo), 2, **kw))
    assert len(full) == 8
    cache = DatasetCache(CROP, slab_slots=4, device=dev) if cached else None
    _assert_same_batches(full[3:], _collect(GpuLoader(_dataset(root, lst, MASK, None, mix, photo), 2, cache=cache, start_batch=3, **kw)))
    alone = _collect(GpuLoader(_dataset(root, lst, MASK), 2, **kw))
    _assert_same_batches(alone[5:], _collect(GpuLoader(_dataset(root, lst, MASK), 2, start_batch=5, **kw)))


def test_hold_2_keeps_both_held_batches_valid(dev, tmp_path):
    """The slot life-time rule of DevicePrefetcher with the mask's own buffer (teacher_view, mask alone) and with the in-place mask: the
    tensors of call k are still the batch's when call k + 1 has been made (hold = 2), without a copy in between."""
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2)
    for tv in (True, False):
        want = _collect(GpuLoader(_dataset(root, lst, MASK, tv=tv), 2, **kw))
        it = iter(GpuLoader(_dataset(root, lst, MASK, tv=tv), 2, hold=2, **kw))
        for k in range(0, 8, 2):
            held = [next(it), next(it)]
            torch.cuda.synchronize()
            for j, b in enumerate(held):
                _same_image(b[0], want[k + j][0], f"held batch {k + j}")
                assert torch.equal(b[1], want[k + j][1])
                if tv:
                    _same_image(b[4], want[k + j][4], f"weak view of held batch {k + j}")
        assert next(it, None) is None


# ---- 3. the tools -------------------------------------------------------------------------------------------------------------------------------
def _tool_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    for d in ("train_img", "train_lab"):
        (tmp_path / d).mkdir(parents=True)
    lines = []
    for i in range(4):
        Image.fromarray(rng.integers(0, 256, (96, 192, 3), dtype=np.uint8)).save(tmp_path / "train_img" / f"t{i}.png")
        blocks = rng.integers(0, 19, (6, 12)).astype(np.uint8)
        blocks[rng.random(blocks.shape) < 0.1] = 255
        Image.fromarray(np.kron(blocks, np.ones((16, 16), np.uint8))).save(tmp_path / "train_lab" / f"t{i}.png")
        lines.append(f"train_img/t{i}.png train_lab/t{i}.png")
    (tmp_path / "pseudo.lst").write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("which", ["simt", "warmup"])
def test_tool_resume_equals_one_run_and_the_flag_off_run_is_untouched(dev, tmp_path, capsys, monkeypatch, which):
    """trainV2_simt --mask-patches --weak-teacher / trainV1_warmup --mask-patches on 4 PNG pairs, B = 2, at 129 x 65 (the geometry of
    tests/test_gpu_resume.py), 16-pixel patches: 3 steps + stop + resume + 3 steps equals 6 steps in the loss lines and in every tensor of the
    final snapshot; the flag changes the run; a run without it launches no mask kernel and repeats itself bit for bit (the loader under the
    mask is the loader as it was); a resume with the flag dropped or changed is refused."""
    pytest.importorskip("PIL.Image")
    from test_gpu_resume import _loss_lines, _same_snapshot, _tool
    tool, extra = _tool(which)
    _tool_files(tmp_path / "data")
    common = extra + ["--model", "DeepLab", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--save-pred-every", "100",
                      "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2", "--data-dir-target", str(tmp_path / "data"),
                      "--data-list-target", str(tmp_path / "data" / "pseudo.lst"), "--random-mirror"]
    flags = ["--mask-patches", "--mask-patch-size", "16"] + (["--weak-teacher"] if which == "simt" else [])
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run(tag, stop, *more):
        del calls[:]
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6, *flags)
    assert len(_loss_lines(out_a)) == 6 and not re.search(r"loss_seg\w* = nan", out_a), out_a
    assert calls.count("simt_patch_mask") >= 6
    if which == "simt":
        assert "weak-view teacher: the frozen model sees the batch before --mask-patches" in out_a and "both models" not in out_a
    else:
        assert "patch mask: 16 x 16 patches blanked with probability 0.7" in out_a
    out_b1, _ = run("b", 3, *flags, "--train-state", state)
    assert _loss_lines(out_b1) == _loss_lines(out_a)[:3]
    out_b2, snap_b = run("b", 6, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert _loss_lines(out_b2) == _loss_lines(out_a)[3:], (out_a, out_b2)
    _same_snapshot(snap_a, snap_b)
    out_o, snap_o = run("o", 6)                                   # no augmentation flag: the tool as it was
    assert "simt_patch_mask" not in calls and "patch mask" not in out_o and len(_loss_lines(out_o)) == 6
    out_p, snap_p = run("p", 6)
    assert _loss_lines(out_p) == _loss_lines(out_o)
    _same_snapshot(snap_o, snap_p)
    sa, so = torch.load(snap_a), torch.load(snap_o)
    assert set(sa) == set(so) and any(not torch.equal(sa[k], so[k]) for k in sa)          # the flag makes another run
    weak = flags[3:]                                              # (--weak-teacher needs an augmentation: the mask is swapped for the mix)
    dropped = ["--class-mix", "--weak-teacher"] if weak else []
    for other in (dropped, ["--mask-patches", "0.5", "--mask-patch-size", "16"] + weak, ["--mask-patches", "--mask-patch-size", "8"] + weak):
        with pytest.raises(SystemExit, match="patch_mask"):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state])
    capsys.readouterr()
    if which == "simt":                                           # without --weak-teacher one start-up line says who sees the mask
        out_m, _ = run("m", 1, "--mask-patches", "--mask-patch-size", "16")
        assert "without --weak-teacher both models see the masked image" in out_m
