"""The EMA teacher on the GPU (simt_amd/ema_teacher.py, csrc/bn_fold_multi.hip).  Every comparison is between two executions of the
same arithmetic, or against the numpy restatement of the EMA (tests/_ema_ref.py), and therefore BITWISE.

  1. the kernel: simt_bn_fold_multi against simt_bn_fold on the GPU, segment by segment, as 32-bit words; guard words; the refusals;
  2. inert until the first refresh: ema_teacher_every larger than the run == the same trainer without the keyword;
  3. a run with the keyword and nothing synchronising between the steps == the same trainer without it whose frozen model the TEST refreshes
     (synchronise, copy_ of the shadow into fixed_params, fixed.repack(): the launches the refresh replaces) -- scalars of every step, everything
     a resume must reproduce, every pack-list destination of the frozen plan, and the teacher == the host restatement's shadow at the last
     refresh.  A refresh that ran too early, too late, or beside a reader would show here;
  4. the fused-BatchNorm error word; 5. resume between two refreshes and its refusals; 6. the tool.

One departure from the letter of the issue, in 5: it asks for the resumed trainer to be built "from another frozen seed", and in the same breath
for `frozen_sha256` to keep refusing a resume beside another --restore-from -- a trainer built from another frozen model IS refused (asserted
below).  The resumed trainer is therefore built from the same frozen model and its `fixed_params` are then overwritten with those of another
frozen seed (and re-packed) before the load: the load still has to bring the teacher back from the file, nothing from the constructor survives.
"""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _ema_ref as ref
import _operand_coherence as oc
import test_gpu_resume as R
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import train_state as tsf
from simt_amd.ema_teacher import FOLD_CHUNK, refresh_due
from test_gpu_resume import CASES, batches, full_state, make, scalars
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
D = 0.9
GUARD = 16                   # words on either side of every scale / shift
SENTINEL = 0x5EADBEEF
EPS = 1e-5
SEG_C = [1, 63, 64, 65, 255, 256, 257, 2048]          # FOLD_CHUNK = 256: a chunk boundary inside a segment, at a segment's end, one channel past it


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------------
def _planted(Cn, rng):
    """gamma, beta, running_mean, running_var with the special values planted (where Cn allows; Cn = 1 gets running_var = 0)."""
    g = rng.standard_normal(Cn).astype(np.float32)
    b = rng.standard_normal(Cn).astype(np.float32)
    rm = rng.standard_normal(Cn).astype(np.float32)
    rv = (rng.random(Cn) * 2 + 1e-3).astype(np.float32)
    plant = [("rv", 0.0), ("g", -1.5), ("g", -0.0), ("b", -0.0), ("rm", -0.0), ("rm", 1e-41), ("rv", 3.3e38), ("g", 0.0), ("rm", -1e-41),
             ("rv", 1e-41), ("g", 3.0e38), ("rm", 3.0e38), ("b", np.inf), ("g", np.nan)]
    arrs = {"g": g, "b": b, "rm": rm, "rv": rv}
    for i, (name, v) in enumerate(plant):
        if i < Cn:
            arrs[name][(5 * i) % Cn if Cn > 80 else i] = np.float32(v)
    return g, b, rm, rv


class _FoldTable:
    def __init__(self, dev, seed=0):
        rng = np.random.default_rng(seed)
        self.host = [_planted(c, rng) for c in SEG_C]
        self.inp = [[torch.from_numpy(a).to(dev) for a in seg] for seg in self.host]
        guard = lambda c: torch.full((c + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.out = [[guard(c), guard(c)] for c in SEG_C]                  # the multi launch writes here
        self.ref = [[guard(c), guard(c)] for c in SEG_C]                  # simt_bn_fold writes here
        self.segs_host = (L.BnFoldSeg * len(SEG_C))()
        for s, (g, b, rm, rv), (sc, sh), c in zip(self.segs_host, self.inp, self.out, SEG_C):
            s.gamma, s.beta, s.running_mean, s.running_var = g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr()
            s.scale, s.shift, s.C = sc.data_ptr() + 4 * GUARD, sh.data_ptr() + 4 * GUARD, c
        self.segs = torch.from_numpy(np.frombuffer(bytes(self.segs_host), dtype=np.uint8).copy()).to(dev)
        chunks = [(si, ci) for si, c in enumerate(SEG_C) for ci in range((c + FOLD_CHUNK - 1) // FOLD_CHUNK)]
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=dev)
        assert len(chunks) == 6 + 2 + 8 and FOLD_CHUNK == 256
        torch.cuda.synchronize()

    def desc(self):
        d = L.BnFoldDesc()
        d.segs, d.segs_host, d.chunks = self.segs.data_ptr(), self.segs_host, self.chunks.data_ptr()
        d.nsegs, d.nchunks, d.chunk, d.eps = len(SEG_C), self.chunks.shape[0], FOLD_CHUNK, EPS
        return d

    def launch(self, d):
        rc = L.load().simt_bn_fold_multi(C.byref(d), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for pair in self.out for t in pair)


def test_multi_fold_equals_the_single_folds_word_for_word(dev):
    tb = _FoldTable(dev)
    st = torch.cuda.current_stream().cuda_stream
    for (g, b, rm, rv), (sc, sh), c in zip(tb.inp, tb.ref, SEG_C):
        L.call("simt_bn_fold", g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, sc.data_ptr() + 4 * GUARD, sh.data_ptr() + 4 * GUARD, c, st)
    before = [[a.clone() for a in seg] for seg in tb.inp]
    assert tb.launch(tb.desc()) == 0
    for i, (got, want, c) in enumerate(zip(tb.out, tb.ref, SEG_C)):
        for what, a, b in zip(("scale", "shift"), got, want):
            assert bool((a[:GUARD] == SENTINEL).all()) and bool((a[GUARD + c:] == SENTINEL).all()), f"segment {i} (C = {c}): a guard word of {what} was written"
            bad = a[GUARD:GUARD + c] != b[GUARD:GUARD + c]
            assert not bool(bad.any()), (f"segment {i} (C = {c}): {int(bad.sum())} words of {what} differ from simt_bn_fold, first at "
                                         f"{int(bad.int().argmax())}: {int(a[GUARD + int(bad.int().argmax())]) & 0xFFFFFFFF:#010x} vs "
                                         f"{int(b[GUARD + int(bad.int().argmax())]) & 0xFFFFFFFF:#010x}")
            assert not bool((a[GUARD:GUARD + c] == SENTINEL).any()), f"segment {i} (C = {c}): a word of {what} was not written"
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for s0, s1 in zip(before, tb.inp) for x, y in zip(s0, s1)), "an input was written"
    # the planted values are what the test says they are: an infinite scale (running_var = 0 is finite with eps; gamma / tiny is not needed), NaN, -0.0
    sc = tb.out[-1][0][GUARD:GUARD + 2048].view(torch.float32).cpu().numpy()
    sh = tb.out[-1][1][GUARD:GUARD + 2048].view(torch.float32).cpu().numpy()
    assert np.isnan(sc).sum() >= 1 and (sc < 0).sum() > 100 and np.signbit(sc[sc == 0]).any() and not np.isfinite(sh).all()
    assert np.float32(tb.host[-1][3][0]) == 0 and np.isfinite(sc[0])


def test_multi_fold_refusals_write_nothing(dev):
    tb = _FoldTable(dev, seed=1)
    for field, value in (("segs", None), ("segs_host", None), ("chunks", None), ("nchunks", 0), ("nchunks", -1), ("nsegs", 0), ("chunk", 0)):
        d = tb.desc()
        setattr(d, field, value)
        assert tb.launch(d) != 0, f"{field} = {value} was accepted"
        assert tb.untouched(), f"{field} = {value}: an output was written"
    for si, c in ((0, 0), (3, -1), (len(SEG_C) - 1, 0)):
        keep = tb.segs_host[si].C
        tb.segs_host[si].C = c
        assert tb.launch(tb.desc()) != 0, f"a segment with C = {c} was accepted"
        assert tb.untouched(), f"segment {si} with C = {c}: an output was written"
        tb.segs_host[si].C = keep
    keep = tb.segs_host[2].scale
    tb.segs_host[2].scale = None
    assert tb.launch(tb.desc()) != 0 and tb.untouched()
    tb.segs_host[2].scale = keep
    assert L.load().simt_bn_fold_multi(None, None) != 0
    assert tb.launch(tb.desc()) == 0 and not tb.untouched()          # and the table as it was: the launch writes


# ---- trainers -------------------------------------------------------------------------------------------------------------------------------------
TCASES = ["SimTTrainer", "SimTTrainer-late_sgd", "SimTTrainer-iter_size2", "SimTTrainer-rccl_one_rank", "SimTSingleTrainer-v3", "SimTSingleTrainer-vgg"]
SIMT = ("SimTTrainer", "SimTSingleTrainer")
PORT = 29581


@contextlib.contextmanager
def _keywords(**kw):
    """tests/test_gpu_resume.make builds the trainers by name: give the two SimT trainers `kw` for the duration."""
    saved = {n: getattr(R, n) for n in SIMT}
    try:
        for n, cls in saved.items():
            setattr(R, n, functools.partial(cls, **kw))
        yield
    finally:
        for n, cls in saved.items():
            setattr(R, n, cls)


def _build(case, dev, every, pg=None, seed=0, decay=D, **kw):
    """The trainer of a case with ema_decay (None: without) and, if `every` is not None, ema_teacher_every."""
    kind, ckw = CASES[case]
    before = os.environ.get("SIMT_EARLY_SGD")
    os.environ["SIMT_EARLY_SGD"] = "0" if ckw.get("late") else "1"          # read by the constructor
    try:
        kws = {} if decay is None else {"ema_decay": decay}
        if every is not None:
            kws["ema_teacher_every"] = every
        with _keywords(**kws):
            tr = make(kind, ckw, dev, pg, seed=seed, **kw)
    finally:
        if before is None:
            os.environ.pop("SIMT_EARLY_SGD", None)
        else:
            os.environ["SIMT_EARLY_SGD"] = before
    if kind == "simt":
        assert tr._early_sgd == (not ckw.get("late") and ckw.get("iter_size", 1) == 1), "the schedule under test is not the one the case names"
    assert (tr.reducer is not None) == bool(ckw.get("dp"))
    return tr


def _group(case, dev):
    return one_rank_group(dev, PORT) if CASES[case][1].get("dp") else contextlib.nullcontext()


def _words(d):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().view(np.uint32).copy() for k, v in d.items() if v.is_floating_point()}


def _floats(d):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items() if v.is_floating_point()}


def _frozen_state(tr):
    """full_state plus everything the teacher adds to what a resume must reproduce."""
    out = full_state(tr)
    out.update({f"frozen {k}": v.cpu() for k, v in tr.fixed_params.items()})
    out.update({f"ema {k}": v.cpu() for k, v in tr.ema.shadow.items()})
    out["ema_updates"] = torch.tensor(tr.ema_updates)
    for i, dsts in enumerate(oc.snapshot(tr.fixed)):
        out.update({f"frozen operand {i}.{j}": t.cpu() for j, t in enumerate(dsts)})
    return out


def _refresh_by_hand(tr):
    """The parent's own launches: synchronise, copy the shadow into the frozen model, re-pack its plan."""
    torch.cuda.synchronize()
    for k, v in tr.fixed_params.items():
        if v.is_floating_point():
            v.copy_(tr.ema_params[k][:v.shape[0]] if v.dim() else tr.ema_params[k])          # (DeeplabVGG: the classifier's leading rows)
    tr.fixed.repack()
    torch.cuda.synchronize()


_RUNS = {}


def _run(case, dev, mode, every=None, steps=4):
    """One memoised run of `steps` steps.  mode "free": the trainer with ema_teacher_every = `every` (None: EMA only), nothing synchronises between
    the steps.  mode "by_hand": EMA only; after every step the test synchronises, feeds the host restatement of the shadow and, where a run with
    `every` refreshes, refreshes by hand.  -> dict(louts, state, frozen0 / teacher words, host shadow at the last / first refresh, ...)."""
    key = (case, mode, every, steps)
    if key in _RUNS:
        return _RUNS[key]
    kind, ckw = CASES[case]
    with _group(case, dev) as pg:
        data = batches(kind, ckw, dev, n=steps)
        tr = _build(case, dev, every if mode == "free" else None, pg)
        res = dict(frozen0=_floats(tr.fixed_params), applied=list(tr.sgd_names), louts=[], first=None, last=None, refreshed_at=[])
        sh = ref.Shadow({k: v for k, v in _floats(tr.params).items()}, D) if mode == "by_hand" else None
        for i, b in enumerate(data):
            tr.step(*b)
            res["louts"].append(scalars(tr))
            if sh is not None:
                sh.update(_floats(tr.params))
                if every is not None and refresh_due(sh.updates, every):
                    _refresh_by_hand(tr)
                    res["last"] = {k: ref.words(v).copy() for k, v in sh.e.items()}
                    res["first"] = res["first"] or {k: v.copy() for k, v in sh.e.items()}
                    res["refreshed_at"].append(i + 1)
        R.finite_losses(tr, f"{case}, step {steps}")
        res["state"] = _frozen_state(tr)
        res["teacher"] = _words(tr.fixed_params)
        res["refreshes"] = tr.teacher_refreshes if mode == "free" and every is not None else len(res["refreshed_at"])
        res["updates"] = tr.ema_updates
        if mode == "free" and every is not None:
            sd = tr.teacher_state_dict()
            res["tsd"] = {k: (v.dtype, tuple(v.shape), v.is_cuda) for k, v in sd.items()}
            res["surface"] = tr.teacher_params is tr.fixed_params and list(sd) == list(tr.fixed_params)
            res["launches"] = [getattr(fn, "__name__", "?") for fn, _a in tr.teacher.launches]
            res["folds"] = sum(1 for it in tr.fixed._pack_items_raw if it.fn is L.load().simt_bn_fold)
        del tr
        torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


def _assert_same(a, b, what, louts=True):
    if louts:
        for i, (x, y) in enumerate(zip(a["louts"], b["louts"])):
            assert torch.equal(x, y), f"{what}: the scalars of step {i + 1} differ: {x.view(torch.float32).tolist()} vs {y.view(torch.float32).tolist()}"
    sa, sb = a["state"], b["state"]
    assert sa.keys() == sb.keys()
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{what}: {len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


@pytest.mark.parametrize("case", TCASES)
def test_inert_until_the_first_refresh(dev, case):
    """ema_teacher_every = 100 over 4 steps: no refresh falls due, and the run is bit for bit the same trainer's without the keyword -- the loss
    scalars of every step, full_state, the frozen model and every packed operand of its plan."""
    a, b = _run(case, dev, "free", 100), _run(case, dev, "free", None)
    assert a["refreshes"] == 0 and a["updates"] == 4
    _assert_same(a, b, f"{case}, ema_teacher_every = 100 against no keyword")
    assert all(np.array_equal(a["teacher"][k], ref.words(v)) for k, v in a["frozen0"].items()), "the frozen model moved without a refresh"


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("case", TCASES)
def test_refresh_equals_the_launches_it_replaces_and_nothing_races_it(dev, case, every):
    a, b, off = _run(case, dev, "free", every), _run(case, dev, "by_hand", every), _run(case, dev, "free", None)
    assert a["refreshes"] == 4 // every == len(b["refreshed_at"]) and b["refreshed_at"] == list(range(every, 5, every)) and a["updates"] == 4
    # ---- the condition (not a measurement): the frozen model was drawn from another seed than the student, so the FIRST refresh changes the bf16
    # rounding of >= 0.99 of the elements of every applied weight tensor the frozen model has -- its packed operand is another one -- and the
    # step behind it computes other scalars than the run whose frozen model never moves.  Otherwise the case shows nothing.
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    # (conv weights: the tensors that HAVE a bf16 operand; DeepLabv3's trainable BatchNorm weights enter the fp32 scales and are held by the
    # equalities below)
    names = [n for n in a["applied"] if n in a["frozen0"] and n.endswith(".weight") and a["frozen0"][n].ndim == 4]
    assert names, "the frozen model shares no applied weight with the student"
    rows = {n: a["frozen0"][n].shape[0] for n in names}
    first = {n: b["first"][n][:rows[n]] for n in names}
    oc.assert_visible(oc.rounding_changed(t({n: a["frozen0"][n] for n in names}), t(first)), f"{case}, first refresh (behind step {every})")
    assert all(torch.equal(x, y) for x, y in zip(a["louts"][:every], off["louts"][:every])), "the scalars differ BEFORE the first refresh"
    assert not torch.equal(a["louts"][every], off["louts"][every]), (f"{case}: the scalars of step {every + 1}, the first behind a refresh, equal "
                                                                     "those of a run without the teacher: the case shows nothing")
    # ---- the refresh == the parent's launches, without a synchronisation anywhere
    _assert_same(a, b, f"{case}, every {every}: the stream-ordered refresh against synchronise + copy_ + fixed.repack()")
    # ---- the teacher is the host restatement's shadow at the last refresh, word for word
    bad = [k for k, w in a["teacher"].items() if not np.array_equal(w.reshape(-1), b["last"][k].reshape(-1)[:w.size])]
    assert not bad and len(a["teacher"]) > 4, f"{case}: {len(bad)} teacher tensors differ from the restatement's shadow at update {b['refreshed_at'][-1]}: {bad[:8]}"
    assert any(k.endswith("running_mean") for k in a["teacher"]) or "vgg" in case
    # ---- the public surface and the launch list
    assert a["surface"] and all(not cuda for (_d, _s, cuda) in a["tsd"].values())
    want = ["simt_ema_multi"] + (["simt_bn_fold_multi"] if a["folds"] else [])
    assert a["launches"][:len(want)] == want and "simt_bn_fold" not in a["launches"] and a["launches"].count("simt_pack_weight_multi") == 1
    assert (a["folds"] == 0) == ("vgg" in case)


@pytest.mark.parametrize("case", ["SimTTrainer", "SimTSingleTrainer-v3", "SimTSingleTrainer-vgg"])
def test_teacher_state_dict_is_the_closed_set_models(dev, case):
    """Keys in order, shapes and dtypes of the closed-set model's state_dict() (what strict=True asks for), on the host."""
    a = _run(case, dev, "free", 1)
    kind, ckw = CASES[case]
    if kind == "simt":
        want = {k: tuple(s) for k, s in so.state_shapes(19, 0, False, layers=R.SMALL).items()}
    elif ckw["model"] == "v3":
        want = {k: tuple(s) for k, s in R.v3_state_shapes(19, 0, False, (1, 2, 2), 64, 64).items()}
    else:
        lay = [(i, ci if ci == 3 else max(ci, 64), max(co, 64), d, p) for (i, ci, co, d, p) in R.VGG_SMALL]
        want = {k: tuple(v.shape) for k, v in R._vgg_state(19, lay, 6).items()}
    assert list(a["tsd"]) == list(want) and all(a["tsd"][k][1] == s for k, s in want.items())
    assert all(dt == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, (dt, _s, _c) in a["tsd"].items())


def test_error_word_keeps_the_last_good_teacher(dev, monkeypatch):
    """With the plan's sticky fused-BatchNorm error word set (by hand: nothing times out) a refresh leaves the frozen model unchanged word for
    word; with the word cleared the next refresh moves it."""
    monkeypatch.setenv("SIMT_BN_GRID", "3")
    size = (4, 768, 768)                                   # (large enough for the plan to fuse BatchNorm launches at this reduced depth)
    tr = _build("SimTTrainer", dev, 1, size=size)
    assert tr.plan.fbn_launches > 0 and tr.plan.fbn_err is not None and tr.teacher.copy_desc.skip_if == tr.plan.fbn_err.data_ptr()
    img, lab = so.synthetic_batch(*size, R.CD.numpy(), seed=1, block=8)
    img, lab = img.to(dev), lab.to(dev)
    start = _words(tr.fixed_params)
    tr.step(img, lab)
    tr.step(img, lab)
    good, operands = _words(tr.fixed_params), oc.snapshot(tr.fixed)
    assert tr.teacher_refreshes == 2 and any(not np.array_equal(good[k], start[k]) for k in good)
    assert all(np.array_equal(good[k], w) for k, w in _words(tr.ema.shadow).items() if k in good)
    tr.plan.fbn_err.fill_(1)
    tr.step(img, lab)
    after = _words(tr.fixed_params)
    assert all(np.array_equal(good[k], after[k]) for k in good), "the refresh wrote the frozen model while the error word was set"
    moved, _ = oc.compare(tr.fixed, operands, "the operands of the last good teacher")
    assert not moved, moved[:4]
    with pytest.raises(RuntimeError, match="SIMT_BN_GRID=0"):
        tr.training_state()
    tr.plan.fbn_err.zero_()
    tr.step(img, lab)
    again = _words(tr.fixed_params)
    assert any(not np.array_equal(good[k], again[k]) for k in good), "the refresh behind the cleared word did not move the frozen model"
    assert all(np.array_equal(again[k], w) for k, w in _words(tr.ema.shadow).items() if k in again)


# ---- 5. resume ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["SimTTrainer", "SimTTrainer-rccl_one_rank", "SimTSingleTrainer-vgg"])
def test_resume_between_two_refreshes(dev, tmp_path, case):
    """N = 2: 3 steps + training_state() + the file + a trainer built from other weights whose frozen model is then overwritten with another
    frozen seed's + load_training_state + 3 steps == 6 steps.  The cut falls between the refreshes behind steps 2 and 4: a resume that rebuilt the
    teacher from the shadow (update 3), or kept the constructor's frozen model, fails."""
    kind, ckw = CASES[case]
    a = _run(case, dev, "free", 2, steps=6)
    assert a["refreshes"] == 3
    with _group(case, dev) as pg:
        data = batches(kind, ckw, dev)
        tr = _build(case, dev, 2, pg)
        louts = []
        for b in data[:3]:
            tr.step(*b)
            louts.append(scalars(tr))
        ts = tr.training_state()
        assert ts["teacher"]["every"] == 2 and ts["teacher"]["refreshes"] == 1 and all(not t.is_cuda for t in ts["teacher"]["params"].values())
        assert ts["frozen_sha256"] == tr.frozen_sha256 != tsf.state_sha256(tr.fixed_params)          # the model the run STARTED beside
        w = next(k for k in ts["teacher"]["params"] if k in tr.sgd_names and k.endswith(".weight"))
        rows = ts["teacher"]["params"][w].shape[0]
        assert not torch.equal(ts["teacher"]["params"][w], ts["ema"]["shadow"][w][:rows]), "the cut does not fall between two refreshes"
        path = str(tmp_path / "run.state")
        tsf.save(path, ts, None, {"world": 1})
        del tr, ts
        torch.cuda.empty_cache()
        ts = tsf.load(path)[0]
        # another frozen model is refused as ever ...
        stranger = _build(case, dev, 2, pg, seed=1, frozen_seed=1)
        with pytest.raises(ValueError, match="frozen_sha256"):
            stranger.load_training_state(ts)
        # ... so: the same one, then its tensors replaced by the stranger's (see the module docstring)
        tr = _build(case, dev, 2, pg, seed=1)
        for k, v in tr.fixed_params.items():
            v.copy_(stranger.fixed_params[k])
        tr.fixed.repack()
        del stranger
        tr.load_training_state(ts)
        assert tr.teacher_refreshes == 1 and tr.ema_updates == 3
        for b in data[3:]:
            tr.step(*b)
            louts.append(scalars(tr))
        res = dict(louts=louts, state=_frozen_state(tr))
        assert tr.teacher_refreshes == 3
        # the refusals: the keyword dropped, added, N changed -- the field is named and nothing is changed
        for other, state, names in ((_build(case, dev, None, pg, seed=1), ts, ("ema_teacher", "does not move")),
                                    (_build(case, dev, 1, pg, seed=1), ts, ("ema_teacher every", "state: 2", "this trainer: 1"))):
            before = _frozen_state(other)
            with pytest.raises(ValueError) as e:
                other.load_training_state(state)
            assert all(n in str(e.value) for n in names), str(e.value)
            after = _frozen_state(other)
            assert all(torch.equal(before[k], after[k]) for k in before), "a refused load changed the trainer"
            del other
        plain = _build(case, dev, None, pg)
        plain.step(*data[0])
        ts_plain = plain.training_state()
        with pytest.raises(ValueError, match="ema_teacher"):
            tr.load_training_state(ts_plain)
        del tr, plain
        torch.cuda.empty_cache()
    _assert_same(a, res, f"{case} resumed after step 3 (between the refreshes behind steps 2 and 4)")


# ---- 6. the tool ----------------------------------------------------------------------------------------------------------------------------------
def _tool_args(model, tmp_path_factory):
    """The command line of tests/test_gpu_ema.py's tool cases.  --model DeepLab draws student and frozen model from ONE generator, so their
    shared tensors are equal: it is given a checkpoint with trained-like weights and --not-restore-last, which leaves the student's classifiers at
    their own initial values.  The one-output models are two modules drawn one after the other from the seed: different weights as they are."""
    from simt_amd import model_spec as ms
    from simt_amd.tools import trainV2_simt as tool
    lr = ["--learning-rate", "2.5e-5"] if model == "DeepLabVGG" else ["--learning-rate", "6e-4"]
    argv = ["--open-classes", "3", "--learning-rate-T", "6e-3"] + lr + ["--model", model, "--synthetic", "--input-size-target", "129,65",
                                                                          "--batch-size", "2", "--num-steps", "50", "--save-pred-every", "100",
                                                                          "--print-every", "1", "--from-scratch", "--num-workers", "2"]
    if model == "DeepLab":
        ckpt = str(tmp_path_factory.mktemp("ckpt") / "frozen.pth")
        torch.save(ms.trained_like_init(ms.state_shapes(19, 0, False), seed=77), ckpt)
        return tool, argv + ["--restore-from", ckpt, "--not-restore-last"]
    return tool, argv + ["--restore-from", ""]


@pytest.mark.parametrize("model", ["DeepLab", "DeepLabv3", "DeepLabVGG"])
def test_tool_ema_teacher_flag(dev, tmp_path, tmp_path_factory, capsys, model):
    """--ema 0.9 --ema-teacher 2, 6 synthetic steps: the loss lines of iterations 0 and 1 are the flag-off run's, the line of iteration 2 (the
    first behind a refresh) is not; 3 + 3 steps through --train-state equal the 6 -- loss lines and every tensor of both final snapshots; the
    same command line with the flag dropped or N changed is refused."""
    from test_gpu_ema import _assert_same_file
    tool, common = _tool_args(model, tmp_path_factory)

    def run(tag, stop, *flags):
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop), "--ema", "0.9"] + list(flags))
        return capsys.readouterr().out, snap

    out_off, _ = run("off", 6)
    out_on, snap_on = run("on", 6, "--ema-teacher", "2")
    off, on = R._loss_lines(out_off), R._loss_lines(out_on)
    with capsys.disabled():
        print("\n".join(["", "flag off:"] + off + ["--ema-teacher 2:"] + on))
    assert len(off) == len(on) == 6 and "EMA teacher" not in out_off
    assert sum("EMA teacher" in ln and "N = 2" in ln for ln in out_on.splitlines()) == 1
    assert on[:2] == off[:2], "the loss lines differ before the first refresh"
    assert on[2] != off[2], "the loss line of the third iteration, the first behind a refresh, equals the flag-off run's"
    state = str(tmp_path / "run.state")
    out_b1, snap_b = run("b", 3, "--ema-teacher", "2", "--train-state", state)
    assert R._loss_lines(out_b1) == on[:3]
    saved = tsf.load(state)[0]["teacher"]
    assert saved["every"] == 2 and saved["refreshes"] == 1
    with pytest.raises(SystemExit, match="ema_teacher"):
        run("b", 6, "--train-state", state)
    with pytest.raises(SystemExit, match="ema_teacher every"):
        run("b", 6, "--ema-teacher", "3", "--train-state", state)
    capsys.readouterr()
    out_b2, _ = run("b", 6, "--ema-teacher", "2", "--train-state", state)
    assert "resumed" in out_b2 and R._loss_lines(out_b2) == on[3:], (on, out_b2)
    for f in ("GTA5_6.pth", "GTA5_6_ema.pth"):
        _assert_same_file(os.path.join(snap_on, f), os.path.join(snap_b, f))
    assert tsf.load(state)[0]["teacher"]["refreshes"] == 3
