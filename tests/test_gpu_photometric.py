"""Colour jitter + Gaussian blur on the device (csrc/photometric.hip, simt_amd/data/photometric.py, GpuLoader, --colour-jitter,
--gaussian-blur).

The yardstick is tests/_photometric_ref.py, a numpy restatement of the arithmetic contract (include/simt_hip.h), and every comparison is
BITWISE, images viewed as int32 words: the kernels against the restatement; the loader against the restatement applied to the flag-off
loader's batches; cached against uncached; a resumed loader / tool against the uninterrupted one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _photometric_ref as ref
from simt_amd import _lib as L
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import IMG_MEAN, GpuLoader, InputPrep

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(3, 40, 64),       # full tiles (16 x 64), 16-byte stores
          (3, 37, 41),       # odd: partial tiles in both directions, the dword-store path, h*w % 4 == 1 (the grey mean's tail lane)
          (2, 6, 6),         # the smallest frame: the reflection reaches the far edge
          (2, 70, 132),      # several tiles each way, halos crossing tile edges
          (4, 21, 72)]       # all four flag combinations within one batch; a partial tile row, two tile columns
# (fb, fc, fs, theta, sigma): the factors at both ends (S = 0.5) and at 1, theta in {-0.5, 0, 0.5}, sigma in {0.15, 0.6, 1.15}
PARAMS = [(0.5, 0.5, 0.5, -0.5, 0.15), (1.5, 1.5, 1.5, 0.5, 1.15), (1.0, 1.0, 1.0, 0.0, 0.6), (1.5, 0.5, 1.0, 0.5, 0.6),
          (0.5, 1.5, 1.5, 0.0, 1.15), (1.0, 0.5, 0.5, -0.5, 0.6), (0.83, 1.21, 1.37, 0.11, 0.9)]
COMBOS = [(1, 1), (1, 0), (0, 1), (0, 0)]      # (jitter, blur)
GUARD = 64                                      # bytes on both sides of the output
PATTERN = 0x5A


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _frames(B, h, w, seed=6):
    """uint8 colours minus the mean (what every loader path produces), a zero border as scale-crop leaves one around a smaller frame,
    and values of -300 and +400: every clamp has work to do."""
    rng = np.random.default_rng([seed, B, h, w])
    x = rng.integers(0, 256, (B, 3, h, w)).astype(F) - np.array(IMG_MEAN, F)[None, :, None, None]
    smooth = np.linspace(0, 255, w, dtype=F)[None, :] * np.ones((h, 1), F)          # item 0: a ramp, so that the blur's reach shows
    x[0] = smooth[None] - np.array(IMG_MEAN, F)[:, None, None]
    x[:, :, 0, :] = 0
    x[:, :, :, -1] = 0
    x[:, :, h // 2, w // 2] = -300
    x[:, :, h // 2, w // 2 - 1] = 400
    x[:, 1, h - 1, 0] = 400
    return x


def _draws(B, rnd):
    """Item i of round `rnd`: parameters PARAMS[(i + rnd) % 7], flags COMBOS[(i + rnd) % 4] -- neighbours in a batch differ in both."""
    p = [PARAMS[(i + rnd) % len(PARAMS)] for i in range(B)]
    c = [COMBOS[(i + rnd) % 4] for i in range(B)]
    d = {k: np.array([q[n] for q in p], np.float64) for n, k in enumerate(("fb", "fc", "fs", "theta", "sigma"))}
    d["jit"], d["blur"] = np.array([q[0] for q in c], bool), np.array([q[1] for q in c], bool)
    return d


def _special(x, d):
    """The copy path's items get what arithmetic would not keep: -0.0 and NaNs with payloads."""
    bits = x.view(np.int32).copy()
    for i in range(len(bits)):
        if not d["jit"][i] and not d["blur"][i]:
            flat = bits[i].reshape(-1)
            flat[0], flat[1], flat[-1], flat[flat.size // 2] = np.int32(-2 ** 31), np.int32(0x7FC12345), np.int32(0x7FA00001), np.int32(-2 ** 31)
    return bits


def _expected(bits, d):
    """-> (output words, S per item | None)."""
    out, sums = np.empty_like(bits), []
    for i in range(len(bits)):
        p = ref.params(d["fb"][i], d["fc"][i], d["fs"][i], d["theta"][i], d["sigma"][i])
        o, S, _m = ref.item(bits[i].view(F), IMG_MEAN, bool(d["jit"][i]), bool(d["blur"][i]), *p)
        out[i] = o.view(np.int32)
        sums.append(S)
    return out, sums


_EXPECTED = {}


def _case(shape, rnd):
    """Inputs and the restatement's answer for (shape, round): computed once, shared, never written to."""
    if (shape, rnd) not in _EXPECTED:
        B, h, w = shape
        d = _draws(B, rnd)
        bits = _special(_frames(B, h, w), d)
        want, sums = _expected(bits, d)
        for a in (bits, want):
            a.setflags(write=False)
        _EXPECTED[(shape, rnd)] = (d, bits, want, sums)
    return _EXPECTED[(shape, rnd)]


def test_cases_are_neither_no_ops_nor_trivial():
    """On the restatement alone, before any GPU call: every flagged item changes, the blur reaches across tile edges and the frame's edges,
    clamps are hit at both ends, and the copy items hold their special words."""
    seen = set()
    for shape in SHAPES:
        for rnd in range(4):
            d, bits, want, sums = _case(shape, rnd)
            for i in range(shape[0]):
                combo = (int(d["jit"][i]), int(d["blur"][i]))
                seen.add(combo)
                if combo == (0, 0):
                    assert np.array_equal(want[i], bits[i]) and (bits[i] == np.int32(0x7FC12345)).any() and sums[i] is None
                    continue
                if combo[0]:
                    assert sums[i] is not None and sums[i] > 0
                colour = want[i].view(F) + np.array(IMG_MEAN, F)[:, None, None]
                assert (colour > -1e-3).all() and (colour < 255 + 1e-3).all() and np.isfinite(colour).all()
                identity = (combo == (0, 1) and d["sigma"][i] == 0.15) or (combo == (1, 0) and tuple(d[k][i] for k in ("fb", "fc", "fs", "theta")) == (1, 1, 1, 0))
                if not identity:                                  # (those two only normalise and go back: rounding at the most)
                    assert (want[i] != bits[i]).mean() > 0.2, (shape, rnd, i)
    assert seen == set(COMBOS)
    for rnd in range(4):                                      # the batch of four holds all four combinations at once, in every round
        d = _case(SHAPES[4], rnd)[0]
        assert {(int(a), int(b)) for a, b in zip(d["jit"], d["blur"])} == set(COMBOS)


@pytest.mark.parametrize("rnd", range(4))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_restatement_bit_for_bit(dev, shape, rnd):
    B, h, w = shape
    d, bits, want, sums = _case(shape, rnd)
    prep = InputPrep(B, (h, w), (w, h), dev, photometric=(0.5, 1.0))
    n = B * 3 * h * w
    x_d = torch.from_numpy(bits.copy()).to(dev).view(torch.float32)
    buf = torch.full((GUARD + 4 * n + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    x_out = buf[GUARD:GUARD + 4 * n].view(torch.float32).view(B, 3, h, w)
    prep.grey_part.fill_(-1)                                              # all ones: a word that is only added to would not come out right
    words = []
    for _ in range(2):                                                    # twice over the same buffers: nothing accumulates
        prep.photometric_batch(x_d, d, x_out, _stream(dev))
        torch.cuda.synchronize()
        words.append(prep.grey_part.cpu().numpy().view(np.uint64).reshape(B, L.PHOTOMETRIC_PARTS).copy())
        got = x_out.view(torch.int32).cpu().numpy()
        for i in range(B):
            bad = np.argwhere(got[i] != want[i])
            assert bad.size == 0, (f"item {i} (jit {d['jit'][i]}, blur {d['blur'][i]}): {len(bad)} of {want[i].size} words differ, first at "
                                   f"{bad[0]}: {got[i][tuple(bad[0])]:#x} != {want[i][tuple(bad[0])]:#x}")
    assert np.array_equal(words[0], words[1])
    for i in range(B):
        S = int(words[0][i].astype(object).sum())
        if d["jit"][i]:
            assert S == sums[i], (i, S, sums[i])                          # the partial sums are exact
            # (m itself never leaves the kernel: given S, the device's float64 product and its rounding are held only through the
            # bitwise output of the jittered items with omfc != 0; this line says that the host formula of m is the restatement's)
            assert F(np.float64(S) * (1.0 / (65536.0 * h * w))) == ref.grey_mean(sums[i], h, w)
        else:
            assert not words[0][i].any()                                  # written (they were all ones), with zeros
    if h * w <= 4 * 256:                                                  # one workgroup holds every quad: the others wrote a zero, not nothing
        assert not words[0][:, 1:].any()
    assert np.array_equal(x_d.view(torch.int32).cpu().numpy(), bits)      # the input is untouched
    g = buf.cpu().numpy()
    assert (g[:GUARD] == PATTERN).all() and (g[GUARD + 4 * n:] == PATTERN).all(), "a guard band was written"


def test_a_batch_of_33_is_split_into_launches_and_equals_the_restatement(dev):
    B, h, w = 33, 9, 12
    rng = ref.generator(5, 0)
    d = ref.draws(rng, B, 0.5, 0.5)
    assert {(int(a), int(b)) for a, b in zip(d["jit"], d["blur"])} == set(COMBOS)
    assert (int(d["jit"][32]), int(d["blur"][32])) != (0, 0), "the item of the second launch does something"
    bits = _frames(B, h, w).view(np.int32)
    want = ref.batch(bits, IMG_MEAN, d)
    prep = InputPrep(B, (h, w), (w, h), dev, photometric=(0.5, 0.5))
    x_d = torch.from_numpy(bits.copy()).to(dev).view(torch.float32)
    x_out = torch.full((B, 3, h, w), 7.0, device=dev)
    prep.photometric_batch(x_d, d, x_out, _stream(dev))
    torch.cuda.synchronize()
    got = x_out.view(torch.int32).cpu().numpy()
    assert [i for i in range(B) if not np.array_equal(got[i], want[i])] == []


def test_refusals_return_the_error_without_launching(dev):
    B, h, w = 2, 8, 8
    x = torch.zeros(B * 3 * h * w + 4, device=dev)
    x_out = torch.full((B * 3 * h * w + 4,), 7.0, device=dev)
    part = torch.full((33 * L.PHOTOMETRIC_PARTS + 1,), 7, dtype=torch.int64, device=dev)

    def desc():
        d = L.PhotometricDesc()
        d.x, d.x_out, d.part = x.data_ptr(), x_out.data_ptr(), part.data_ptr()
        d.inv, d.B, d.h, d.w = 1.0 / (65536.0 * h * w), B, h, w
        d.mean[0], d.mean[1], d.mean[2] = IMG_MEAN
        for i in range(B):
            d.jit[i], d.blur[i], d.fb[i], d.fc[i], d.omfc[i] = 1, 1, 1.0, 1.0, 0.0
            d.A[i][0] = d.A[i][4] = d.A[i][8] = 1.0
            d.wk[i][0] = 1.0
        return d

    def too_many_items(d):
        d.B = 33

    def no_items(d):
        d.B = 0

    def frame_too_low(d):
        d.h = 5

    def frame_too_narrow(d):
        d.w = 5

    def no_input(d):
        d.x = None

    def no_output(d):
        d.x_out = None

    def no_partials(d):
        d.part = None

    def misaligned_output(d):
        d.x_out = x_out.data_ptr() + 4

    def misaligned_input(d):
        d.x = x.data_ptr() + 4

    def misaligned_partials(d):
        d.part = part.data_ptr() + 4

    def in_place(d):
        d.x_out = x.data_ptr()

    for change in (too_many_items, no_items, frame_too_low, frame_too_narrow, no_input, no_output, no_partials, misaligned_output,
                   misaligned_input, misaligned_partials, in_place):
        for fn in ("simt_grey_mean_parts", "simt_photometric"):
            d = desc()
            change(d)
            with pytest.raises(L.SimtHipError):
                L.call(fn, C.byref(d), _stream(dev))
    torch.cuda.synchronize()
    assert (x_out == 7.0).all() and (part == 7).all() and (x == 0).all()               # nothing ran
    L.call("simt_grey_mean_parts", C.byref(desc()), _stream(dev))                      # the descriptor itself is sound
    L.call("simt_photometric", C.byref(desc()), _stream(dev))
    torch.cuda.synchronize()
    assert (x_out[:B * 3 * h * w].abs() < 1e-4).all() and (x_out[B * 3 * h * w:] == 7.0).all()      # identity parameters: colour = mean comes back
    assert (part[:B * L.PHOTOMETRIC_PARTS] != 7).all() and (part[B * L.PHOTOMETRIC_PARTS:] == 7).all()


# ---- loader --------------------------------------------------------------------------------------------------------------------------------
HS, WS = 96, 160
CROP = (72, 40)
N_CLASSES = 19
CHOICES = ("0.5", "1.0", "1.5")
SETTINGS = (0.5, 0.7)


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


def _dataset(root, lst, photo, choices=None, mix=None):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    return cityscapesPseudo(root, lst, crop_size=CROP, mean=IMG_MEAN, mirror=True, scale_crop=choices, class_mix=mix, photometric=photo)


def _collect(loader):
    out = []
    for images, labels, sizes, names in loader:
        out.append((images.clone(), None if labels is None else labels.clone(), np.array(sizes), list(names)))
    torch.cuda.synchronize()
    return out


def _assert_same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for k, ((xa, la, sa, na), (xb, lb, sb, nb)) in enumerate(zip(a, b)):
        assert na == nb and np.array_equal(sa, sb), (k, na, nb)
        diff = (xa.view(torch.int32) != xb.view(torch.int32)).sum(dim=(1, 2, 3)).tolist()
        assert not any(diff), f"batch {k}: image words that differ per item: {diff}"
        assert (la is None and lb is None) or torch.equal(la, lb), f"batch {k}: labels differ"


def _by_the_restatement(off, seed, rank, settings, skip=0):
    """The flag-off loader's batches, jittered and blurred by the restatement with the draws of generator(seed, rank)."""
    rng = ref.generator(seed, rank)
    out, changed = [], 0
    for k, (x, lab, sizes, names) in enumerate(off):
        d = ref.draws(rng, len(names), *settings)
        if k < skip:
            continue
        xb = x.view(torch.int32).cpu().numpy()
        xo = ref.batch(xb, IMG_MEAN, d)
        changed += int((xo != xb).sum())
        out.append((torch.from_numpy(xo).view(torch.float32).to(x.device), lab, sizes, names))
    assert changed > 0
    return out


@pytest.mark.parametrize("mode", ["plain", "scale-crop", "class-mix"])
def test_loader_equals_restatement_on_flag_off_batches_and_cached_equals_uncached(dev, tmp_path, mode):
    """8 items, B = 2, shuffle + mirror, 2 epochs: the photometric loader = the restatement applied to the batches of the loader without
    the two flags (its mirror / scale-crop / class-mix draws do not move; labels are handed out as they were); with a DatasetCache the same."""
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    choices = CHOICES if mode == "scale-crop" else None
    mix = (N_CLASSES, 0.7) if mode == "class-mix" else None
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2)
    off = _collect(GpuLoader(_dataset(root, lst, None, choices, mix), 2, **kw))
    assert len(off) == 8
    if mix is not None:                # the batch underneath IS mixed: not the plain loader's
        plain = _collect(GpuLoader(_dataset(root, lst, None), 2, **kw))
        assert any(not torch.equal(a[1], b[1]) for a, b in zip(off, plain))
    for settings in (SETTINGS, (0.2, None), (None, 1.0)):
        want = _by_the_restatement(off, 3, 0, settings)
        _assert_same_batches(want, _collect(GpuLoader(_dataset(root, lst, settings, choices, mix), 2, **kw)))
    cache = DatasetCache((WS, HS) if choices is not None else CROP, slab_slots=3, device=dev)
    _assert_same_batches(want, _collect(GpuLoader(_dataset(root, lst, (None, 1.0), choices, mix), 2, cache=cache, **kw)))
    assert cache.misses == 8 and cache.hits == 8


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_loader_start_batch_yields_the_tail(dev, tmp_path, cached):
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=5, epochs=2)
    mix = (N_CLASSES, 0.6)
    full = _collect(GpuLoader(_dataset(root, lst, SETTINGS, None, mix), 2, **kw))
    assert len(full) == 8
    cache = DatasetCache(CROP, slab_slots=4, device=dev) if cached else None
    _assert_same_batches(full[3:], _collect(GpuLoader(_dataset(root, lst, SETTINGS, None, mix), 2, cache=cache, start_batch=3, **kw)))


def test_ranks_draw_differently_and_the_flag_off_loader_has_no_photometric_buffers(dev, tmp_path, monkeypatch):
    pytest.importorskip("PIL.Image")
    from simt_amd.data import pipeline
    root, lst = _write_files(tmp_path, 8)
    for rank in (0, 1):
        kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2, rank=rank, world=2)
        off = _collect(GpuLoader(_dataset(root, lst, None), 2, **kw))
        assert len(off) == 4
        _assert_same_batches(_by_the_restatement(off, 3, rank, SETTINGS), _collect(GpuLoader(_dataset(root, lst, SETTINGS), 2, **kw)))
    a, b = ref.draws(ref.generator(3, 0), 2, *SETTINGS), ref.draws(ref.generator(3, 1), 2, *SETTINGS)
    assert not np.array_equal(a["fb"], b["fb"])
    # flags off: no partial words, no third image buffer, no launch of the new kernels; flags on: all three
    made, calls = [], []

    class Spy(pipeline.DevicePrefetcher):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    real_call = L.call
    monkeypatch.setattr(pipeline, "DevicePrefetcher", Spy)
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    for photo, has in ((None, False), (SETTINGS, True)):
        del calls[:]
        loader = GpuLoader(_dataset(root, lst, photo), 2, shuffle=True, num_workers=2, device=dev, seed=3, epochs=1)
        got = _collect(loader)
        pf = made.pop()
        assert len(got) == 4 and not made
        assert (loader._prep.grey_part is not None) == has and (loader._prep.ph is not None) == has
        assert all(("xp" in s) == has for s in pf.slots) and len(pf.slots) == 2
        assert (calls.count("simt_grey_mean_parts"), calls.count("simt_photometric")) == ((4, 4) if has else (0, 0))


def test_loader_works_without_labels(dev, tmp_path):
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 4)

    def unlabelled(photo):
        ds = _dataset(root, lst, photo)
        real = ds.decode
        ds.decode = lambda i: (real(i)[0], None, real(i)[2])
        return ds
    kw = dict(shuffle=False, num_workers=1, device=dev, seed=1, epochs=1)
    off = _collect(GpuLoader(unlabelled(None), 2, **kw))
    assert len(off) == 2 and off[0][1] is None
    _assert_same_batches(_by_the_restatement(off, 1, 0, SETTINGS), _collect(GpuLoader(unlabelled(SETTINGS), 2, **kw)))


# ---- tools ---------------------------------------------------------------------------------------------------------------------------------
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


def _loss_lines(out):
    return [re.sub(r"\s*\([0-9.]+ img/s\)", "", ln) for ln in out.splitlines() if ln.startswith("iter = ")]


def _same_snapshot(a, b):
    sa, sb = torch.load(a), torch.load(b)
    assert set(sa) == set(sb) and len(sa) > 0
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


def _common(tmp_path):
    return ["--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--save-pred-every", "100", "--print-every", "1",
            "--from-scratch", "--restore-from", "", "--num-workers", "2", "--data-dir-target", str(tmp_path / "data"),
            "--data-list-target", str(tmp_path / "data" / "pseudo.lst"), "--random-mirror"]


@pytest.mark.parametrize("which", ["simt", "warmup"])
def test_tool_resume_equals_one_run_and_cache_equals_off(dev, tmp_path, capsys, which):
    """Both tools with --class-mix --colour-jitter 0.5 --gaussian-blur 0.8 on 4 PNG pairs, B = 2, at 129 x 65: 3 steps + resume + 3 steps
    equals 6 steps in the loss lines and in every tensor of the final snapshot (the resumed loader skips three batches' draws),
    `--cache-dataset device` equals `off`, the flags change the run, and a resume with a flag dropped is refused with the key named."""
    pytest.importorskip("PIL.Image")
    if which == "simt":
        from simt_amd.tools import trainV2_simt as tool
        common = ["--model", "DeepLab", "--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3"] + _common(tmp_path)
    else:
        from simt_amd.tools import trainV1_warmup as tool
        common = ["--model", "DeepLabVGG", "--learning-rate", "2.5e-4"] + _common(tmp_path)
    _tool_files(tmp_path / "data")
    flags = ["--class-mix", "--colour-jitter", "0.5", "--gaussian-blur", "0.8"]

    def run(tag, stop, *more):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6, *flags)
    assert len(_loss_lines(out_a)) == 6 and not re.search(r"loss_seg\w* = nan", out_a), out_a
    out_b1, _ = run("b", 3, *flags, "--train-state", state)
    assert _loss_lines(out_b1) == _loss_lines(out_a)[:3]
    out_b2, snap_b = run("b", 6, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert _loss_lines(out_b2) == _loss_lines(out_a)[3:], (out_a, out_b2)
    _same_snapshot(snap_a, snap_b)
    out_c, snap_c = run("c", 6, *flags, "--cache-dataset", "device")
    assert _loss_lines(out_c) == _loss_lines(out_a), (out_a, out_c)
    _same_snapshot(snap_a, snap_c)
    _out_d, snap_d = run("d", 6, "--class-mix")                 # without the two flags it is another run: other weights come out
    sa, sd = torch.load(snap_a), torch.load(snap_d)
    assert set(sa) == set(sd) and any(not torch.equal(sa[k], sd[k]) for k in sa)
    for kept in (["--class-mix"], ["--class-mix", "--colour-jitter", "0.5"]):          # a flag dropped
        with pytest.raises(SystemExit, match="photometric"):
            tool.main(common + kept + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state])
    capsys.readouterr()
