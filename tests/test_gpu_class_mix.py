"""ClassMix on the device (csrc/class_mix.hip, simt_amd/data/class_mix.py, GpuLoader, --class-mix).

The yardstick is tests/_class_mix_ref.py, a numpy restatement of the contract (sets, `sorted`, boolean masks), and every comparison is
BITWISE: the mix is a selection, so image values are compared as int32 bit patterns (-0.0 and NaN payloads included); the loader against the
restatement applied to the flag-off loader's batches; cached against uncached; a resumed loader / tool against the uninterrupted one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as ref
from simt_amd import _lib as L
from simt_amd.data.cache import DatasetCache
from simt_amd.data.pipeline import IMG_MEAN, GpuLoader, InputPrep

pytestmark = pytest.mark.gpu

SHAPES = [(3, 40, 64, 19),      # 16-byte path; odd B: the partner cycle wraps
          (3, 37, 41, 19),      # h*w % 4 == 1: the tail lane, item bases that are not 16-byte aligned
          (2, 8, 8, 32),        # bit 31 of the presence word; one workgroup of the 64 parts has pixels, 63 have none
          (2, 40, 64, 1)]
MAIN = SHAPES[0]
KINDS = ("blocky", "special_a", "special_b")
GUARD = 64                      # bytes on both sides of each output
PATTERN = 0x5A


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _blocky(rng, h, w, C):
    """8 x 8 blocks of one class (most quads uniform; mixed quads at the single pixels and, where a row is no multiple of 4, at block
    edges), some blocks 255, some single pixels 255, one C + 1."""
    bh, bw = -(-h // 8), -(-w // 8)
    blocks = rng.integers(0, C, (bh, bw)).astype(np.int64)
    blocks[rng.random((bh, bw)) < 0.15] = 255
    lab = np.kron(blocks, np.ones((8, 8), np.int64))[:h, :w].copy()
    lab[rng.random((h, w)) < 0.03] = 255
    lab[int(rng.integers(0, h)), int(rng.integers(0, w))] = C + 1
    return lab


def _labels(kind, B, h, w, C, seed=5):
    rng = np.random.default_rng([seed, B, h, w, C])
    lab = np.stack([_blocky(rng, h, w, C) for _ in range(B)])
    if kind == "special_a":
        lab[0] = 255                                     # nothing to paste from this partner
        lab[1] = C // 2                                  # exactly one class: n = 1, k = 1, the whole item is pasted
    elif kind == "special_b":
        only = np.where(lab[0] % 2 == 0, C - 1, 255)     # the only valid class is C - 1 (bit 31 at C = 32)
        only[0, 0], only[0, 1] = C - 1, 255
        lab[0] = only
    return lab


def _images(B, h, w, seed=6):
    rng = np.random.default_rng([seed, B, h, w])
    x = rng.standard_normal((B, 3, h, w)).astype(np.float32)
    bits = x.view(np.int32)
    flat = bits.reshape(-1)
    flat[rng.integers(0, flat.size, max(4, flat.size // 50))] = np.int32(-2 ** 31)           # -0.0
    flat[rng.integers(0, flat.size, max(4, flat.size // 50))] = np.int32(0x7FC12345)         # a quiet NaN with a payload
    flat[rng.integers(0, flat.size, max(4, flat.size // 50))] = np.int32(0x7FA00001)         # a signalling one
    flat[0], flat[-1] = np.int32(-2 ** 31), np.int32(0x7FC12345)
    return bits


def _draws(mode, B, C, seed=7):
    rng = np.random.default_rng([seed, B, C])
    rank = rng.permuted(np.tile(np.arange(C, dtype=np.uint8), (B, 1)), axis=1)
    apply = {"on": np.ones(B, bool), "off": np.zeros(B, bool), "mixed": np.arange(B) % 2 == 0}[mode]
    return apply, rank


def _bits_of(classes):
    word = 0
    for c in classes:
        word += 2 ** c
    return word


def test_main_case_is_neither_a_no_op_nor_a_full_copy():
    """On the restatement alone, before any GPU call: in the main case every applied item whose partner shows n >= 2 classes has at least
    one pasted and at least one kept pixel, the quads are of all three kinds, and the special items do what they are there for."""
    B, h, w, Cn = MAIN
    lab = _labels("blocky", B, h, w, Cn)
    apply, rank = _draws("on", B, Cn)
    m = ref.paste_masks(lab, apply, rank, Cn)
    for i in range(B):
        assert len(ref.present(lab[(i + 1) % B], Cn)) >= 2
        assert m[i].any() and not m[i].all(), i
    quads = m.reshape(B, -1, 4).sum(axis=2)
    assert (quads == 0).any() and (quads == 4).any() and ((quads > 0) & (quads < 4)).any()
    assert (lab == 255).any() and (lab == Cn + 1).any()
    sa = _labels("special_a", B, h, w, Cn)
    ma = ref.paste_masks(sa, apply, rank, Cn)
    assert not ma[B - 1].any() and ma[0].all() and ref.present(sa[0], Cn) == set() and ref.present(sa[1], Cn) == {Cn // 2}
    sb = _labels("special_b", *SHAPES[2])
    assert ref.present(sb[0], 32) == {31} and (sb[0] == 255).any()


@pytest.mark.parametrize("mode", ["on", "off", "mixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_restatement_bit_for_bit(dev, shape, mode):
    B, h, w, Cn = shape
    prep = InputPrep(B, (h, w), (w, h), dev, class_mix=(Cn, 1.0))
    n_x, n_l = B * 3 * h * w, B * h * w
    for kind in KINDS:
        lab, xb = _labels(kind, B, h, w, Cn), _images(B, h, w)
        apply, rank = _draws(mode, B, Cn)
        want_x, want_l = ref.mix(xb, lab, apply, rank, Cn)
        x_d = torch.from_numpy(xb).to(dev).view(torch.float32)
        lab_d = torch.from_numpy(lab).to(dev)
        buf_x = torch.full((GUARD + 4 * n_x + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
        buf_l = torch.full((GUARD + 8 * n_l + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
        x_out = buf_x[GUARD:GUARD + 4 * n_x].view(torch.float32).view(B, 3, h, w)
        lab_out = buf_l[GUARD:GUARD + 8 * n_l].view(torch.int64).view(B, h, w)
        prep.part.fill_(-1)                                               # 0xFFFFFFFF: a word that is only ORed into stays all ones
        words = []
        for _ in range(2):                                                # twice over the same buffers: nothing accumulates
            prep.class_mix_batch(x_d, lab_d, (apply, rank), x_out, lab_out, _stream(dev))
            torch.cuda.synchronize()
            words.append(prep.part.cpu().numpy().view(np.uint32).reshape(B, L.CLASS_MIX_PARTS).copy())
            got_x, got_l = x_out.view(torch.int32).cpu().numpy(), lab_out.cpu().numpy()
            bad = np.argwhere(got_l != want_l)
            assert bad.size == 0, f"{kind}: {len(bad)} labels differ, first at {bad[0]}"
            bad = np.argwhere(got_x != want_x)
            assert bad.size == 0, f"{kind}: {len(bad)} image words differ, first at {bad[0]}"
        assert np.array_equal(words[0], words[1])
        for b in range(B):
            assert int(np.bitwise_or.reduce(words[0][b])) == _bits_of(ref.present(lab[b], Cn)), (kind, b)
        if h * w <= 4 * 256:                                              # one workgroup holds every quad: the others wrote a zero, not nothing
            assert not words[0][:, 1:].any()
        assert np.array_equal(x_d.view(torch.int32).cpu().numpy(), xb) and np.array_equal(lab_d.cpu().numpy(), lab)      # inputs untouched
        for buf, n in ((buf_x, 4 * n_x), (buf_l, 8 * n_l)):
            g = buf.cpu().numpy()
            assert (g[:GUARD] == PATTERN).all() and (g[GUARD + n:] == PATTERN).all(), f"{kind}: a guard band was written"


def test_refusals_return_the_error_without_launching(dev):
    B, h, w, Cn = 2, 8, 8, 19
    x = torch.zeros(B, 3, h, w, device=dev)
    lab = torch.zeros(B, h, w, dtype=torch.int64, device=dev)
    x_out = torch.full((B * 3 * h * w + 4,), 7.0, device=dev)
    lab_out = torch.full((B, h, w), 7, dtype=torch.int64, device=dev)
    part = torch.full((33 * L.CLASS_MIX_PARTS,), 7, dtype=torch.int32, device=dev)

    def desc():
        d = L.ClassMixDesc()
        d.x, d.lab, d.x_out, d.lab_out, d.part = x.data_ptr(), lab.data_ptr(), x_out.data_ptr(), lab_out.data_ptr(), part.data_ptr()
        d.B, d.h, d.w, d.n_classes = B, h, w, Cn
        for i in range(B):
            d.partner[i], d.apply[i] = (i + 1) % B, 1
            for c in range(Cn):
                d.rank[i][c] = c
        return d

    def too_many_items(d):
        d.B = 33

    def too_many_classes(d):
        d.n_classes = 33

    def rank_past_the_classes(d):
        d.rank[1][3] = Cn

    def misaligned_output(d):
        d.x_out = x_out.data_ptr() + 4

    def partner_past_the_batch(d):
        d.partner[0] = B

    def in_place(d):
        d.x_out = x.data_ptr()

    for change in (too_many_items, too_many_classes, rank_past_the_classes, misaligned_output, partner_past_the_batch, in_place):
        d = desc()
        change(d)
        with pytest.raises(L.SimtHipError):
            L.call("simt_class_mix", C.byref(d), _stream(dev))
    for args in ((lab.data_ptr(), 33, h * w, Cn, part.data_ptr()), (lab.data_ptr(), B, h * w, 33, part.data_ptr()),
                 (lab.data_ptr(), B, h * w, 0, part.data_ptr()), (lab.data_ptr() + 8, B, h * w, Cn, part.data_ptr()),
                 (lab.data_ptr(), B, 2 ** 31, Cn, part.data_ptr()), (None, B, h * w, Cn, part.data_ptr())):
        with pytest.raises(L.SimtHipError):
            L.call("simt_label_presence", *args, _stream(dev))
    torch.cuda.synchronize()
    assert (x_out == 7.0).all() and (lab_out == 7).all() and (part == 7).all()          # nothing ran
    L.call("simt_label_presence", lab.data_ptr(), B, h * w, Cn, part.data_ptr(), _stream(dev))      # the descriptor itself is sound
    L.call("simt_class_mix", C.byref(desc()), _stream(dev))
    torch.cuda.synchronize()
    assert (x_out[:B * 3 * h * w] == 0).all() and (lab_out == 0).all()
    with pytest.raises(ValueError, match="batch of 33"):                                # the host refuses a larger batch: it is not split
        InputPrep(33, (h, w), (w, h), dev, class_mix=(Cn, 1.0))
    with pytest.raises(ValueError, match="needs labels"):
        InputPrep(2, (h, w), (w, h), dev, with_label=False, class_mix=(Cn, 1.0))


# ---- loader --------------------------------------------------------------------------------------------------------------------------------
HS, WS = 96, 160
CROP = (72, 40)
N_CLASSES = 19
CHOICES = ("0.5", "1.0", "1.5")


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


def _dataset(root, lst, mix, choices=None):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    return cityscapesPseudo(root, lst, crop_size=CROP, mean=IMG_MEAN, mirror=True, scale_crop=choices, class_mix=mix)


def _collect(loader):
    out = []
    for images, labels, sizes, names in loader:
        out.append((images.clone(), labels.clone(), np.array(sizes), list(names)))
    torch.cuda.synchronize()
    return out


def _assert_same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for k, ((xa, la, sa, na), (xb, lb, sb, nb)) in enumerate(zip(a, b)):
        assert na == nb and np.array_equal(sa, sb), (k, na, nb)
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), f"batch {k}: images differ"
        assert torch.equal(la, lb), f"batch {k}: labels differ"


def _mixed_by_the_restatement(off, seed, rank, prob):
    """The flag-off loader's batches, mixed by the restatement with the draws of generator(seed, rank)."""
    rng = ref.generator(seed, rank)
    out, pasted = [], 0
    for x, lab, sizes, names in off:
        apply, rk = ref.draws(rng, len(names), N_CLASSES, prob)
        xb, lb = x.view(torch.int32).cpu().numpy(), lab.cpu().numpy()
        pasted += int(ref.paste_masks(lb, apply, rk, N_CLASSES).sum())
        xo, lo = ref.mix(xb, lb, apply, rk, N_CLASSES)
        out.append((torch.from_numpy(xo).view(torch.float32).to(x.device), torch.from_numpy(lo).to(x.device), sizes, names))
    assert pasted > 0
    return out


@pytest.mark.parametrize("choices", [None, CHOICES], ids=["plain", "scale-crop"])
def test_loader_equals_restatement_on_flag_off_batches_and_cached_equals_uncached(dev, tmp_path, choices):
    """8 items, B = 2, shuffle + mirror, 2 epochs: the class-mix loader = the restatement applied to the batches of the loader without the
    flag (its mirror / scale-crop draws do not move); with a DatasetCache the same."""
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2)
    off = _collect(GpuLoader(_dataset(root, lst, None, choices), 2, **kw))
    assert len(off) == 8
    for prob in (1.0, 0.5):
        want = _mixed_by_the_restatement(off, 3, 0, prob)
        _assert_same_batches(want, _collect(GpuLoader(_dataset(root, lst, (N_CLASSES, prob), choices), 2, **kw)))
    cache = DatasetCache((WS, HS) if choices is not None else CROP, slab_slots=3, device=dev)
    _assert_same_batches(want, _collect(GpuLoader(_dataset(root, lst, (N_CLASSES, 0.5), choices), 2, cache=cache, **kw)))
    assert cache.misses == 8 and cache.hits == 8


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_loader_start_batch_yields_the_tail(dev, tmp_path, cached):
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 8)
    kw = dict(shuffle=True, num_workers=2, device=dev, seed=5, epochs=2)
    full = _collect(GpuLoader(_dataset(root, lst, (N_CLASSES, 0.6)), 2, **kw))
    assert len(full) == 8
    cache = DatasetCache(CROP, slab_slots=4, device=dev) if cached else None
    _assert_same_batches(full[3:], _collect(GpuLoader(_dataset(root, lst, (N_CLASSES, 0.6)), 2, cache=cache, start_batch=3, **kw)))


def test_ranks_draw_differently_and_the_flag_off_loader_has_no_mix_buffers(dev, tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    from simt_amd.data import pipeline
    root, lst = _write_files(tmp_path, 8)
    for rank in (0, 1):
        kw = dict(shuffle=True, num_workers=2, device=dev, seed=3, epochs=2, rank=rank, world=2)
        off = _collect(GpuLoader(_dataset(root, lst, None), 2, **kw))
        assert len(off) == 4
        _assert_same_batches(_mixed_by_the_restatement(off, 3, rank, 1.0), _collect(GpuLoader(_dataset(root, lst, (N_CLASSES, 1.0)), 2, **kw)))
    a, b = ref.draws(ref.generator(3, 0), 2, N_CLASSES, 1.0), ref.draws(ref.generator(3, 1), 2, N_CLASSES, 1.0)
    assert not np.array_equal(a[1], b[1])
    # flag off: no presence words, no second pair of buffers; flag on: both
    made = []

    class Spy(pipeline.DevicePrefetcher):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(pipeline, "DevicePrefetcher", Spy)
    for mix, has in ((None, False), ((N_CLASSES, 1.0), True)):
        loader = GpuLoader(_dataset(root, lst, mix), 2, shuffle=True, num_workers=2, device=dev, seed=3, epochs=1)
        got = _collect(loader)
        pf = made.pop()
        assert (loader._prep.part is not None) == has and (loader._prep.cm is not None) == has and not made
        assert all(("xm" in s) == has and ("labm" in s) == has for s in pf.slots) and len(pf.slots) == 2
        if has:
            continue
        # the flag-off loader is the loader as it was: InputPrep.run of the same frames with the mirror draws it always made
        rng = np.random.default_rng(3)
        prep = InputPrep(2, (HS, WS), CROP, dev, mean=IMG_MEAN)
        for x, lo, _s, names in got:
            flags = (rng.integers(0, 2, 2) == 0).tolist()
            rgb = np.stack([np.array(Image.open(os.path.join(root, "img", n + ".png"))) for n in names])
            lab = np.stack([np.array(Image.open(os.path.join(root, "lab", n + ".png"))) for n in names])
            xr = torch.empty(2, 3, CROP[1], CROP[0], device=dev)
            lr = torch.empty(2, CROP[1], CROP[0], dtype=torch.int64, device=dev)
            prep.run(torch.from_numpy(rgb).to(dev), xr, torch.from_numpy(lab).to(dev), lr, mirror=flags)
            torch.cuda.synchronize()
            assert torch.equal(x, xr) and torch.equal(lo, lr)
    with pytest.raises(ValueError, match="batch of 1"):
        GpuLoader(_dataset(root, lst, (N_CLASSES, 1.0)), 1, device=dev)


def test_loader_refuses_a_dataset_without_labels(dev, tmp_path):
    pytest.importorskip("PIL.Image")
    root, lst = _write_files(tmp_path, 4)
    ds = _dataset(root, lst, (N_CLASSES, 1.0))
    real = ds.decode
    ds.decode = lambda i: (real(i)[0], None, real(i)[2])
    with pytest.raises(ValueError, match="no labels"):
        iter(GpuLoader(ds, 2, shuffle=False, num_workers=1, device=dev, seed=1, epochs=1))


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


def test_tool_class_mix_resume_equals_one_run_and_cache_equals_off(dev, tmp_path, capsys):
    """trainV2_simt --model DeepLab --class-mix on 4 PNG pairs, B = 2, at 129 x 65: 3 steps + resume + 3 steps equals 6 steps in the loss
    lines and the final snapshot (the resumed loader skips three batches' mix draws), `--cache-dataset device` equals `off`, and a resume with the flag dropped is refused with the field named."""
    pytest.importorskip("PIL.Image")
    from simt_amd.tools import trainV2_simt as tool
    _tool_files(tmp_path / "data")
    common = ["--model", "DeepLab", "--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3"] + _common(tmp_path)

    def run(tag, stop, *flags):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(flags))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_6.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 6, "--class-mix")
    assert len(_loss_lines(out_a)) == 6
    out_b1, _ = run("b", 3, "--class-mix", "--train-state", state)
    assert _loss_lines(out_b1) == _loss_lines(out_a)[:3]
    out_b2, snap_b = run("b", 6, "--class-mix", "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert _loss_lines(out_b2) == _loss_lines(out_a)[3:], (out_a, out_b2)
    _same_snapshot(snap_a, snap_b)
    out_c, snap_c = run("c", 6, "--class-mix", "--cache-dataset", "device")
    assert _loss_lines(out_c) == _loss_lines(out_a), (out_a, out_c)
    _same_snapshot(snap_a, snap_c)
    with pytest.raises(SystemExit, match="class_mix"):          # the flag dropped
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state])
    capsys.readouterr()


def test_warmup_tool_runs_with_class_mix(dev, tmp_path, capsys):
    pytest.importorskip("PIL.Image")
    from simt_amd.tools import trainV1_warmup as tool
    _tool_files(tmp_path / "data")
    tool.main(["--model", "DeepLabVGG", "--learning-rate", "2.5e-4", "--snapshot-dir", str(tmp_path / "w"), "--num-steps-stop", "2",
               "--class-mix", "0.5"] + _common(tmp_path))
    out = capsys.readouterr().out
    assert len(_loss_lines(out)) == 2 and all("nan" not in ln for ln in _loss_lines(out)), out
