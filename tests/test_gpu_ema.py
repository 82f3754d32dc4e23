"""The weight EMA on the GPU (simt_amd/ema.py, csrc/ema.hip).  Reference: the numpy restatement of the arithmetic contract,
tests/_ema_ref.py -- every comparison is bitwise (int32 words), the kernel is never compared with itself.

  1. the kernel: every path (16-byte, dword, tail, copy), planted special values, guard bands, the skip word, the refusals;
  2. pure observer: a trainer with ema_decay computes, bit for bit, what it computes without;
  3. the shadow equals the restatement applied on the host to the masters read after every step -- which fails if the launch sees weights
     from before the SGD launch or running statistics from before the forward -- and equals it without the per-step synchronisation too;
  4. resume, the fused-BatchNorm error word, both training tools.
"""
import contextlib
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

import _ema_ref as ref
import test_gpu_resume as R
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import train_state as tsf
from test_gpu_resume import CASES, batches, full_state, make, scalars
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
D = 0.9
CHUNK = 65536
SIZES = [1, 3, 4, 5, 255, 256, 257, 1028, 2048, 2052, 65535, 65536, 65537, 2 * 65536 + 4]          # (1028, 2052: 257 and 513 quads, the pair loop's edges)
GUARD = 16                   # floats: 64 bytes on either side of every e
SENTINEL = 0x5EADBEEF
OMDS = [1.0, 0.5, 2.0 ** -10, float(np.float32(1 - 0.999))]


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------------
class _Table:
    """Segments for one launch: SIZES aligned, then the data of the last size twice more -- w a view 4 bytes into its allocation (e aligned), and
    e 4 bytes behind its guard band (w aligned): both take the dword path and must give the bits of the aligned segment."""

    def __init__(self, dev, seed=0):
        rng = np.random.default_rng(seed)
        self.host = [ref.planted(n, rng) for n in SIZES]
        self.host += [self.host[-1], self.host[-1]]
        self.w_off = [0] * len(SIZES) + [1, 0]
        self.e_off = [GUARD] * len(SIZES) + [GUARD, GUARD + 1]
        self.wbuf, self.ebuf, self.w, self.e = [], [], [], []
        for (w, e), wo, eo in zip(self.host, self.w_off, self.e_off):
            n = w.size
            wb = torch.zeros(n + wo + 3, dtype=torch.float32, device=dev)
            eb = torch.full((n + eo + GUARD + 3,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
            wb[wo:wo + n].view(torch.int32).copy_(torch.from_numpy(ref.words(w).view(np.int32)))
            eb[eo:eo + n].view(torch.int32).copy_(torch.from_numpy(ref.words(e).view(np.int32)))
            self.wbuf.append(wb), self.ebuf.append(eb), self.w.append(wb[wo:wo + n]), self.e.append(eb[eo:eo + n])
        assert all(t.data_ptr() % 16 == 0 for t in self.w[:len(SIZES)] + self.e[:len(SIZES)])
        assert self.w[-2].data_ptr() % 16 == 4 and self.w[-2].data_ptr() - self.wbuf[-2].data_ptr() == 4 and self.e[-1].data_ptr() % 16 == 4
        recs = np.array([(w.data_ptr(), e.data_ptr(), w.numel()) for w, e in zip(self.w, self.e)], dtype=[("w", "<u8"), ("e", "<u8"), ("n", "<i8")])
        chunks = [(si, ci) for si, (w, _e) in enumerate(self.host) for ci in range((w.size + CHUNK - 1) // CHUNK)]
        self.segs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=dev)
        self.skip = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        self.w_before = [b.clone() for b in self.wbuf]

    def desc(self, omd, skip=False):
        d = L.EmaDesc()
        d.segs, d.chunks, d.nchunks, d.chunk, d.omd = self.segs.data_ptr(), self.chunks.data_ptr(), self.chunks.shape[0], CHUNK, omd
        if skip:
            d.skip_if = self.skip.data_ptr()
        return d

    def launch(self, d):
        rc = L.load().simt_ema_multi(C.byref(d), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def e_words(self):
        return [e.view(torch.int32).cpu().numpy().view(np.uint32) for e in self.e]

    def assert_untouched_around(self):
        for i, (wb, w0, eb, eo) in enumerate(zip(self.wbuf, self.w_before, self.ebuf, self.e_off)):
            assert torch.equal(wb.view(torch.int32), w0.view(torch.int32)), f"segment {i}: w was written"
            words, n = eb.view(torch.int32), self.host[i][0].size
            assert bool((words[:eo] == SENTINEL).all()) and bool((words[eo + n:] == SENTINEL).all()), f"segment {i}: a guard band of e was written"


def _assert_words(got, want, copy, what):
    if copy:
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} words differ on the copy path"
        return
    nan_g, nan_w = np.isnan(got.view(np.float32)), np.isnan(want.view(np.float32))
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN positions differ"
    bad = (got != want) & ~nan_w
    assert not bad.any(), (f"{what}: {int(bad.sum())} words differ, first at {int(np.argmax(bad))}: "
                           f"{got[np.argmax(bad)]:#010x} vs {want[np.argmax(bad)]:#010x}")


@pytest.mark.parametrize("omd", OMDS, ids=["copy", "half", "2^-10", "1-0.999"])
def test_kernel_equals_the_restatement_bit_for_bit(dev, omd):
    tb = _Table(dev)
    d = tb.desc(omd)
    once = [ref.update(e, w, np.float32(omd)) for (w, e) in tb.host]
    twice = [ref.update(e1, w, np.float32(omd)) for (w, _e), e1 in zip(tb.host, once)]
    for run, want in ((1, once), (2, twice)):
        assert tb.launch(d) == 0
        got = tb.e_words()
        for i, (g, x) in enumerate(zip(got, want)):
            _assert_words(g, ref.words(x), omd == 1.0, f"launch {run}, segment {i} ({g.size} elements, w+{tb.w_off[i]}, e+{tb.e_off[i] - GUARD})")
        k = len(SIZES) - 1
        assert np.array_equal(got[k], got[k + 1]) and np.array_equal(got[k], got[k + 2]), "the dword path differs from the 16-byte path"
        tb.assert_untouched_around()
    if omd != 1.0:        # the planted values are what the test says they are: something moved, NaNs and infinities are there
        e0 = ref.words(tb.host[-1][1])
        assert (tb.e_words()[len(SIZES) - 1] != e0).mean() > 0.5 and np.isnan(once[-1]).sum() >= 3 and np.isinf(once[-1]).sum() >= 2


def test_kernel_skip_word_and_refusals_leave_everything_untouched(dev):
    tb = _Table(dev, seed=1)
    before = tb.e_words()

    def untouched(what):
        assert all(np.array_equal(a, b) for a, b in zip(before, tb.e_words())), f"{what}: e was written"
        tb.assert_untouched_around()

    tb.skip.fill_(1)
    for omd in (1.0, 0.5):
        assert tb.launch(tb.desc(omd, skip=True)) == 0
        untouched(f"skip word set, omd {omd}")
    tb.skip.zero_()
    for omd in (0.0, -0.5, 1.5, float("nan"), float("inf"), -0.0):
        assert tb.launch(tb.desc(omd)) != 0, f"omd {omd} was accepted"
        untouched(f"omd {omd}")
    for field, value in (("segs", None), ("chunks", None), ("nchunks", 0), ("nchunks", -1), ("chunk", 0), ("chunk", -4)):
        d = tb.desc(0.5)
        setattr(d, field, value)
        assert tb.launch(d) != 0, f"{field} = {value} was accepted"
        untouched(f"{field} = {value}")
    assert L.load().simt_ema_multi(None, None) != 0
    # and the word cleared again: the launch updates
    assert tb.launch(tb.desc(0.5, skip=True)) == 0
    assert not np.array_equal(before[-1], tb.e_words()[-1])


# ---- trainers -------------------------------------------------------------------------------------------------------------------------------------
TRAINERS = ("SimTTrainer", "WarmupTrainer", "SimTSingleTrainer", "WarmupSingleTrainer")
RUN_CASES = ["SimTTrainer", "SimTTrainer-late_sgd", "SimTTrainer-iter_size2", "WarmupTrainer", "SimTSingleTrainer-v3", "WarmupSingleTrainer-vgg"]
LONG_CASE = "SimTTrainer"            # 12 steps: D = 0.9 leaves the running-mean phase at update 9


@contextlib.contextmanager
def ema_on(decay):
    """tests/test_gpu_resume.make builds the four trainers by name: give every one of them `ema_decay=decay` for the duration."""
    saved = {n: getattr(R, n) for n in TRAINERS}
    try:
        if decay is not None:
            for n, cls in saved.items():
                setattr(R, n, functools.partial(cls, ema_decay=decay))
        yield
    finally:
        for n, cls in saved.items():
            setattr(R, n, cls)


def _build(case, dev, decay, pg=None, seed=0, **kw):
    kind, ckw = CASES[case]
    before = os.environ.get("SIMT_EARLY_SGD")
    os.environ["SIMT_EARLY_SGD"] = "0" if ckw.get("late") else "1"          # read by the constructor
    try:
        with ema_on(decay):
            tr = make(kind, ckw, dev, pg, seed=seed, **kw)
    finally:
        if before is None:
            os.environ.pop("SIMT_EARLY_SGD", None)
        else:
            os.environ["SIMT_EARLY_SGD"] = before
    if kind == "simt":
        assert tr._early_sgd == (not ckw.get("late") and ckw.get("iter_size", 1) == 1), "the schedule under test is not the one the case names"
    return tr


def _masters(tr):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in tr.params.items() if v.is_floating_point()}


def _shadow_words(tr):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.uint32) for k, v in tr.ema.shadow.items()}


_RUNS = {}


def _run(case, dev, decay, steps, host_shadow):
    """One run of `steps` steps, memoised: (loss scalars per step, full_state, final shadow words | None, host shadow words | None, extras).
    host_shadow: synchronise after every step, read the masters and apply the restatement on the host."""
    key = (case, decay, steps, host_shadow)
    if key in _RUNS:
        return _RUNS[key]
    kind, ckw = CASES[case]
    data = batches(kind, ckw, dev, n=steps)
    tr = _build(case, dev, decay)
    sh = ref.Shadow(_masters(tr), decay) if host_shadow else None
    louts = []
    for b in data:
        tr.step(*b)
        louts.append(scalars(tr))
        if sh is not None:
            sh.update(_masters(tr))
    R.finite_losses(tr, f"{case}, step {steps}")
    extras = {}
    if decay is not None:
        sd, esd = tr.state_dict(), tr.ema_state_dict()
        extras = dict(updates=tr.ema_updates, sd={k: (v.dtype, tuple(v.shape)) for k, v in sd.items()},
                      esd={k: (v.dtype, tuple(v.shape)) for k, v in esd.items()},
                      nbt=[(int(sd[k]), int(esd[k])) for k in sd if k.endswith("num_batches_tracked")],
                      applied=set(tr.sgd_names), live=_masters(tr), ema_keys=list(tr.ema_params),
                      long_is_live=all(tr.ema_params[k] is tr.params[k] for k, v in tr.params.items() if not v.is_floating_point()),
                      esd_words={k: v.numpy().view(np.uint32) for k, v in esd.items() if v.is_floating_point()}, keys=list(tr.params))
    res = (louts, full_state(tr), _shadow_words(tr) if decay is not None else None,
           {k: ref.words(v) for k, v in sh.e.items()} if sh is not None else None, extras)
    del tr
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


@pytest.mark.parametrize("case", RUN_CASES)
def test_ema_is_a_pure_observer(dev, case):
    """4 steps with ema_decay = 0.9 against 4 steps without: the loss scalars of every step and everything a resume must reproduce, bitwise."""
    (la, sa, *_), (lb, sb, *_) = _run(case, dev, None, 4, False), _run(case, dev, D, 4, False)
    for i, (a, b) in enumerate(zip(la, lb)):
        assert torch.equal(a, b), f"{case}: the scalars of step {i + 1} differ with the EMA on"
    assert sa.keys() == sb.keys()
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{case}: {len(diff)} of {len(sa)} tensors differ with the EMA on: {diff[:8]}"


@pytest.mark.parametrize("case,steps", [(c, 4) for c in RUN_CASES] + [(LONG_CASE, 12)])
def test_shadow_equals_the_restatement_applied_to_the_masters(dev, case, steps):
    _l, _s, synced, host, x = _run(case, dev, D, steps, True)
    assert x["updates"] == steps and synced.keys() == host.keys() and len(host) > 4
    bad = [k for k in host if not np.array_equal(synced[k], host[k])]
    assert not bad, f"{case}: {len(bad)} of {len(host)} shadow tensors differ from the restatement: {bad[:8]}"
    assert any(k.endswith("running_mean") for k in host) or "vgg" in case                     # running statistics are shadowed
    # the same without the per-step synchronisation and read-back: the launch is ordered by the streams, not by the test
    _l2, _s2, free, _h, x2 = _run(case, dev, D, steps, False)
    bad = [k for k in host if not np.array_equal(free[k], host[k])]
    assert not bad, f"{case}: {len(bad)} shadow tensors differ when nothing synchronises between the steps: {bad[:8]}"
    assert x2["updates"] == steps
    # tensors no optimiser lists compare == with the live ones (BatchNorm affine; conv1 / layer1 / layer2 in the SimT stage)
    untouched = [k for k in host if k not in x["applied"] and "running_" not in k]
    moved = [k for k in x["applied"] if not np.array_equal(synced[k], ref.words(x["live"][k]))]
    assert moved, "no applied tensor's shadow differs from the live one: the run does not exercise the average"
    for k in untouched:
        assert np.array_equal(synced[k].view(np.float32), x["live"][k]), f"{k}: untouched by every optimiser, yet its shadow left the live value"
    # the public surface
    assert x["ema_keys"] == x["keys"] and x["long_is_live"]
    assert x["sd"] == x["esd"] and list(x["sd"]) == list(x["esd"])
    assert all(a == b for a, b in x["nbt"])
    assert all(np.array_equal(x["esd_words"][k], synced[k]) for k in synced)
    if steps == 12:
        assert ref.omd(D, 9) == ref.omd(D, 11) == np.float32(1 - D) and ref.omd(D, 8) > np.float32(1 - D)


def _with_shadow(tr):
    out = full_state(tr)
    out.update({f"ema {k}": v.cpu() for k, v in tr.ema.shadow.items()})
    out["ema_updates"] = torch.tensor(tr.ema_updates)
    return out


@pytest.mark.parametrize("case", ["SimTTrainer", "WarmupSingleTrainer-v3", "SimTTrainer-rccl_one_rank"])
def test_resume_carries_the_shadow(dev, tmp_path, case):
    """3 steps + training_state() + the file + a fresh trainer built from other weights + load_training_state + 3 steps == 6 steps: the shadow,
    ema_updates and everything tests/test_gpu_resume.py compares."""
    kind, ckw = CASES[case]
    with (one_rank_group(dev, 29571) if ckw.get("dp") else contextlib.nullcontext()) as pg:
        data = batches(kind, ckw, dev)
        tr = _build(case, dev, D, pg)
        assert (tr.reducer is not None) == bool(ckw.get("dp"))
        la = []
        for b in data:
            tr.step(*b)
            la.append(scalars(tr))
        a = _with_shadow(tr)
        del tr
        torch.cuda.empty_cache()
        tr = _build(case, dev, D, pg)
        lb = []
        for b in data[:3]:
            tr.step(*b)
            lb.append(scalars(tr))
        ts = tr.training_state()
        assert ts["ema"]["updates"] == 3 and ts["ema"]["decay"] == D and all(not t.is_cuda for t in ts["ema"]["shadow"].values())
        path = str(tmp_path / "run.state")
        tsf.save(path, ts, None, {"world": 1})
        del tr, ts
        torch.cuda.empty_cache()
        ts = tsf.load(path)[0]
        tr = _build(case, dev, D, pg, seed=1)
        tr.load_training_state(ts)
        assert tr.ema_updates == 3
        for b in data[3:]:
            tr.step(*b)
            lb.append(scalars(tr))
        b_ = _with_shadow(tr)
        # a trainer without the EMA refuses the state and is not changed by it
        other = _build(case, dev, None, pg, seed=1)
        with pytest.raises(ValueError, match="ema"):
            other.load_training_state(ts)
        del tr, other
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert a.keys() == b_.keys() and int(a["ema_updates"]) == 6
    diff = [k for k in a if a[k].dtype != b_[k].dtype or not torch.equal(a[k], b_[k])]
    assert not diff, f"{case} resumed after step 3: {len(diff)} of {len(a)} tensors differ: {diff[:8]}"


def test_error_word_leaves_the_shadow_unchanged(dev, monkeypatch):
    """With the plan's sticky fused-BatchNorm error word set (by hand: nothing times out) the optimisers skip their updates and so does the EMA."""
    monkeypatch.setenv("SIMT_BN_GRID", "3")
    size = (4, 768, 768)                                   # (large enough for the plan to fuse BatchNorm launches at this reduced depth)
    tr = _build("SimTTrainer", dev, D, size=size)
    assert tr.plan.fbn_launches > 0 and tr.plan.fbn_err is not None and tr.ema.desc.skip_if == tr.plan.fbn_err.data_ptr()
    img, lab = so.synthetic_batch(*size, R.CD.numpy(), seed=1, block=8)
    img, lab = img.to(dev), lab.to(dev)
    tr.step(img, lab)
    tr.step(img, lab)
    good = _shadow_words(tr)
    assert any(not np.array_equal(good[k], ref.words(v)) for k, v in _masters(tr).items())          # the shadow is an average by now
    tr.plan.fbn_err.fill_(1)
    tr.step(img, lab)
    after = _shadow_words(tr)
    assert all(np.array_equal(good[k], after[k]) for k in good), "the EMA launch wrote while the error word was set"
    with pytest.raises(RuntimeError, match="SIMT_BN_GRID=0"):
        tr.training_state()
    tr.plan.fbn_err.zero_()


# ---- tools ------------------------------------------------------------------------------------------------------------------------------------------
def _tool(which):
    if which == "warmup":
        from simt_amd.tools import trainV1_warmup as tool
        return tool, ["--learning-rate", "2.5e-4"], 0
    from simt_amd.tools import trainV2_simt as tool
    return tool, ["--open-classes", "3", "--learning-rate", "6e-4", "--learning-rate-T", "6e-3"], 3


def _common(which, model):
    tool, extra, K = _tool(which)
    lr = ["--learning-rate", "2.5e-5"] if model == "DeepLabVGG" else []           # (tests/test_gpu_resume.py VGG_LR: six bf16 steps stay finite)
    return tool, extra + lr + ["--model", model, "--synthetic", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
                               "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2"], K


_TOOL_RUNS = {}


def _six_steps(which, model, flag, tmp_path_factory, capsys):
    """Snapshot directory of one 6-step run with (`flag` = True) or without --ema 0.9, memoised per (tool, model)."""
    key = (which, model, flag)
    if key not in _TOOL_RUNS:
        tool, common, _K = _common(which, model)
        snap = str(tmp_path_factory.mktemp(f"{which}_{model}_{'ema' if flag else 'off'}"))
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", "6"] + (["--ema", "0.9"] if flag else []))
        _TOOL_RUNS[key] = (snap, capsys.readouterr().out)
    return _TOOL_RUNS[key]


def _assert_same_file(a, b):
    sa, sb = torch.load(a), torch.load(b)
    assert list(sa) == list(sb) and len(sa) > 0
    bits = lambda t: t.contiguous().view(torch.uint8) if t.dim() else t          # bitwise: a NaN equals itself
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or sa[k].shape != sb[k].shape or not torch.equal(bits(sa[k]), bits(sb[k]))]
    assert not diff, f"{os.path.basename(a)}: {len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


TOOL_CASES = [("simt", "DeepLab"), ("simt", "DeepLabVGG"), ("warmup", "DeepLab"), ("warmup", "DeepLabVGG")]


@pytest.mark.parametrize("which,model", TOOL_CASES)
def test_tool_ema_flag_writes_the_averaged_model_beside_the_unchanged_one(dev, tmp_path, tmp_path_factory, capsys, which, model):
    from PIL import Image

    from simt_amd.tools import make_pseudo_labels as mpl
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    off, out_off = _six_steps(which, model, False, tmp_path_factory, capsys)
    on, out_on = _six_steps(which, model, True, tmp_path_factory, capsys)
    assert os.listdir(off) == ["GTA5_6.pth"] and sorted(os.listdir(on)) == ["GTA5_6.pth", "GTA5_6_ema.pth"]
    assert R._loss_lines(out_on) == R._loss_lines(out_off) and len(R._loss_lines(out_on)) == 6 and "EMA" not in out_off
    _assert_same_file(os.path.join(off, "GTA5_6.pth"), os.path.join(on, "GTA5_6.pth"))
    live, avg = torch.load(os.path.join(on, "GTA5_6.pth")), torch.load(os.path.join(on, "GTA5_6_ema.pth"))
    assert list(live) == list(avg) and all(live[k].dtype == avg[k].dtype and live[k].shape == avg[k].shape for k in live)
    head = "classifier.conv2d_list.0.weight" if model == "DeepLabVGG" else "layer6.conv2d_list.0.weight"
    assert head in live and not torch.equal(live[head], avg[head]) and bool(torch.isfinite(avg[head]).all())
    K = _tool(which)[2]
    if model == "DeepLab":
        from simt_amd.model.deeplab_multi import DeeplabMulti
        m, arch, ev_model = DeeplabMulti(19, K, K > 0), "multi", "v2"
    else:
        from simt_amd.model.deeplab_vgg import DeeplabVGG
        m, arch, ev_model = DeeplabVGG(19 + K), "vgg", "vgg"
    m.load_state_dict(avg, strict=True)
    scales, label_hw = ((48, 96), (64, 128)), (72, 144)
    ev = Evaluator(avg, num_classes=19, open_classes=K, label_hw=label_hw, scales=scales, device=dev, model=ev_model)
    g = torch.Generator().manual_seed(2)
    pred = ev.predict(*[(torch.randn(1, 3, h, w, generator=g) * 50).to(dev) for (h, w) in scales])
    assert tuple(pred.shape[-2:]) == label_hw and int(pred.max()) < 19
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "train", "city"))
    name = "city/city_000000_000019_leftImg8bit.png"
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (96, 192, 3), dtype=np.uint8)).save(os.path.join(root, "train", name))
    open(os.path.join(root, "train.txt"), "w").write(name + "\n")
    mpl.main(["--restore-from", os.path.join(on, "GTA5_6_ema.pth"), "--arch", arch, "--open-classes", str(K), "--data-dir", root,
              "--data-list", os.path.join(root, "train.txt"), "--input-size", "96,48", "--label-size", "144,72", "--out-name", "pseudo_ema",
              "--list-out", os.path.join(root, "pseudo_ema.lst"), "--num-workers", "1"])
    png = np.asarray(Image.open(os.path.join(root, "pseudo_ema", os.path.basename(name))))
    assert png.shape == (72, 144) and png.dtype == np.uint8
    capsys.readouterr()


@pytest.mark.parametrize("which,model", TOOL_CASES)
def test_tool_ema_resumes_through_the_train_state(dev, tmp_path, tmp_path_factory, capsys, which, model):
    """3 + 3 steps through --train-state equal 6 steps, GTA5_6_ema.pth included; the same command line with --ema dropped, or changed, is refused."""
    on, _out = _six_steps(which, model, True, tmp_path_factory, capsys)
    tool, common, _K = _common(which, model)
    snap, state = str(tmp_path / "b"), str(tmp_path / "run.state")
    run = lambda stop, *flags: tool.main(common + ["--snapshot-dir", snap, "--train-state", state, "--num-steps-stop", str(stop)] + list(flags))
    run(3, "--ema", "0.9")
    assert tsf.load(state)[0]["ema"]["updates"] == 3 and tsf.load(state)[2]["ema_keeper"]["best_iter"] == 0
    with pytest.raises(SystemExit, match="ema"):
        run(6)
    with pytest.raises(SystemExit, match="ema decay"):
        run(6, "--ema", "0.99")
    capsys.readouterr()
    run(6, "--ema", "0.9")
    assert "resumed" in capsys.readouterr().out
    assert sorted(os.listdir(snap)) == ["GTA5_3.pth", "GTA5_3_ema.pth", "GTA5_6.pth", "GTA5_6_ema.pth"]
    _assert_same_file(os.path.join(on, "GTA5_6.pth"), os.path.join(snap, "GTA5_6.pth"))
    _assert_same_file(os.path.join(on, "GTA5_6_ema.pth"), os.path.join(snap, "GTA5_6_ema.pth"))
    assert tsf.load(state)[0]["ema"]["updates"] == 6


@pytest.mark.parametrize("which", ["simt", "warmup"])
def test_tool_evaluates_the_ema_and_keeps_its_best_snapshot(dev, tmp_path, capsys, which):
    """A tiny validation list (tests/test_gpu_tools.py): the live model's lines and files as always, an `EMA mIoU` line per evaluation and exactly
    one best file of the `ema_` rotation."""
    Image = pytest.importorskip("PIL.Image")
    from test_gpu_tools import _make_dataset
    tool, extra, _K = _tool(which)
    _make_dataset(tmp_path, Image)
    snap = str(tmp_path / "snap")
    argv = extra + ["--data-dir-target", str(tmp_path), "--data-list-target", str(tmp_path / "pseudo.lst"), "--input-size-target", "129,65",
                    "--batch-size", "2", "--num-steps", "50", "--num-steps-stop", "6", "--save-pred-every", "2", "--print-every", "1",
                    "--from-scratch", "--restore-from", "", "--snapshot-dir", snap, "--data-dir-val", str(tmp_path),
                    "--data-list-val", str(tmp_path / "kit" / "val.txt"), "--gt-dir-val", str(tmp_path / "gt"), "--devkit-dir", str(tmp_path / "kit"),
                    "--num-workers", "2", "--ema", "0.9"]
    tool.main(argv)
    out = capsys.readouterr().out
    assert out.count("Begin evaluation") == 2 and out.count("EMA mIoU: ") == 2 and out.count("===> mIoU:") == 4      # iterations 2 and 4: live, then EMA
    stem = "GTA5_BAPA_warmup_" if which == "warmup" else "GTA5_"
    assert len(glob.glob(os.path.join(snap, stem + "iter*_mIoU*.pth"))) == 1
    best = glob.glob(os.path.join(snap, stem + "ema_iter*_mIoU*.pth"))
    assert len(best) == 1, sorted(os.listdir(snap))
    assert sorted(f for f in os.listdir(snap) if "iter" not in f) == ["GTA5_6.pth", "GTA5_6_ema.pth"]
    sd = torch.load(best[0])
    assert list(sd) == list(torch.load(os.path.join(snap, "GTA5_6.pth")))
