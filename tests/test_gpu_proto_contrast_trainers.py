"""The prototype contrastive term in the warm-up trainer and the tool (keywords proto_contrast / proto_contrast_temp /
proto_contrast_min_ratio of WarmupTrainer, --proto-contrast of trainV1_warmup).  All on the reduced DeepLab-v2 at online_labels = 0, where the
teacher finds five or six classes (profiles/proto_denoise.txt, section 4).

  (a) without the keyword none of the four launches is issued, nothing is allocated, the plan has no seed and the train state no new field; the
      launch list of proto_contrast = 0 without the four new names IS the keyword-less list;
  (b) proto_contrast = 0: three steps equal the trainer without the keyword, as values;
  (c) the four entry points run again by the test on copies of the pass's `label`, student features, eta and n, taken directly in front of the
      trainer's own launches, give the trainer's cell labels, seed, d, partials, scalars, seen set and N bit for bit, and the cell labels are the
      restatement's -- plain, class-balanced, weighted, online_mix, online_source (both passes), iter_size = 2, bf16 and fp32;
  (d) the term moves the trunk and, in the pass itself, no head gradient;
  (e) a one-rank RCCL group is the single-GPU trainer; resume 3 + 3 == 6; the refusals name the field or the keyword;
  (f) the tool prints ` pc = `, resumes, and refuses --model DeepLabv3 --proto-contrast."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _proto_contrast_ref as pr
import test_gpu_feat_dist as FD
import test_gpu_online_labels as O
import test_gpu_proto_trainers as PT
import test_gpu_source_mix as SM
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import proto_contrast as PC
from simt_amd import train_state as tsf
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
PORT = 29619
B, H, W = O.SIZE
PROTO = dict(proto_denoise=PT.TEMP, proto_momentum=PT.MOM)
LAM, TEMP, RATIO = 0.5, 0.2, 0.6
ON = dict(PROTO, proto_contrast=LAM, proto_contrast_temp=TEMP, proto_contrast_min_ratio=RATIO)
MODES = {"plain": dict(online_labels=0.0), "balanced": dict(online_labels=0.0, online_labels_balanced=0.5, online_labels_momentum=0.5),
         "weighted": dict(online_labels=0.0, online_labels_weighted="item"), "mix": dict(online_labels=0.0, online_mix=0.5, online_mix_seed=11),
         "dacs": dict(online_labels=0.0, online_labels_weighted="batch", online_source=True, online_mix=0.5, online_mix_seed=11),
         "source": dict(online_labels=0.0, online_source=True)}
NEW = ("simt_cell_labels", "simt_proto_contrast_prep", "simt_proto_contrast", "simt_proto_contrast_finalize")


def _calls_of_a_step(tr, dev, monkeypatch, src=None):
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    PT._step(tr, O._views(dev, 1)[0], src, 1)
    torch.cuda.synchronize()
    monkeypatch.setattr(L, "call", real_call)
    return calls


# ---- (a), (b) ------------------------------------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_nothing_is_launched_or_allocated(dev, monkeypatch):
    src = SM._sources(dev, 1)[0]
    off = O._trainer("v2", dev, **PROTO, **MODES["source"])
    assert off.proto_contrast is None and off.plan.feat_seed is None and off.plan.feat_grad_seed is False
    assert not [k for k in vars(off) if k.startswith("pc_")] and not hasattr(off, "proto_contrast_temp")
    hy = off.training_state()["hyper"]
    assert not [k for k in hy if k.startswith("proto_contrast")]
    calls_off = _calls_of_a_step(off, dev, monkeypatch, src)
    assert calls_off and not set(calls_off) & set(NEW) and not [k for k in off.losses() if "proto_contrast" in k]
    zero = O._trainer("v2", dev, **PROTO, proto_contrast=0.0, **MODES["source"])
    calls_zero = _calls_of_a_step(zero, dev, monkeypatch, src)
    assert [calls_zero.count(n) for n in NEW] == [2, 2, 2, 2], "four launches per pass"
    assert [n for n in calls_zero if n not in NEW] == calls_off, "the keyword changed the launches around its own"
    order = [n for n in calls_zero if n in NEW]
    assert order == list(NEW) * 2
    # in each pass the four lie behind the head's gradient launch and the label launch of the target pass
    first_label = min(i for i, n in enumerate(calls_zero) if n.startswith("simt_online_label"))
    idx = [i for i, n in enumerate(calls_zero) if n == "simt_cell_labels"]
    assert idx[0] < first_label < idx[1], "the source pass's launches do not lie in front of the teacher's label launch, or the target's behind it"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_lambda_zero_is_the_trainer_without_the_keyword(dev, dtype):
    kw = MODES["source"]
    base = PT._run("v2", dev, dtype, 3, **PROTO, **kw)
    got = PT._run("v2", dev, dtype, 3, **PROTO, proto_contrast=0.0, **kw)
    O._assert_same(got, base, "proto_contrast = 0")
    assert torch.equal(PT._bits(got["eta"]), PT._bits(base["eta"])) and torch.equal(got["n"], base["n"])
    for a, b in zip(got["per_step"], base["per_step"]):
        assert a["proto_contrast"] == 0.0 and a["source_proto_contrast"] == 0.0 and "proto_contrast" not in b
        assert {k: v for k, v in a.items() if "proto_contrast" not in k} == b
    assert got["per_step"][-1]["proto_contrast_cells"] > 0, "no valid cell: the comparison shows nothing"


# ---- (c) the trainer's launches == the test's -------------------------------------------------------------------------------------------------------------
def _capture(tr):
    """Wraps the trainer's `_pc_launches`: in front of them (same stream) the inputs are copied, behind them the outputs."""
    caps = []
    real = tr._pc_launches

    def launches(st, source=False):
        c = dict(source=source, label=tr.label.clone(), fs=tr.plan.block_io[-1]["z"].clone(), eta=tr.proto_eta.clone(), n=tr.proto_n.clone())
        real(st, source)
        c.update(lab=tr.pc_lab.clone(), lab_part=tr.pc_lab_part.clone(), phat=tr.pc_phat.clone(), hdr=tr.pc_hdr.clone(), seed=tr.plan.feat_seed.clone(),
                 d=tr.pc_d.clone(), part=tr.pc_part.clone(), out=tr.pc_out.clone(), seeded=tr.plan.feat_seed_desc.res)
        caps.append(c)
    tr._pc_launches = launches
    return caps


def _relaunch(tr, c):
    """The four entry points, by the test, into buffers of its own (outputs pre-filled with junk)."""
    M, D = c["fs"].shape
    h, w = tr.plan.feat_hw
    nan = float("nan")
    own = dict(lab=torch.full_like(c["lab"], 0xEE), lab_part=torch.full_like(c["lab_part"], -7), phat=torch.full_like(c["phat"], nan),
               hdr=torch.full_like(c["hdr"], -7), seed=torch.full_like(c["seed"], nan), d=torch.full_like(c["d"], nan),
               part=torch.full_like(c["part"], nan), out=torch.full_like(c["out"], nan))
    st = ops.stream_ptr()
    cl = PC.fill_cell_labels(c["label"], own["lab"], own["lab_part"], c["n"], B, H, W, h, w, tr.C, RATIO)
    d = PC.fill_contrast(c["fs"], own["lab"], c["eta"], c["n"], own["phat"], own["hdr"], own["seed"], own["d"], own["part"], own["out"], M, D, tr.C,
                         tr.dtype, LAM, TEMP, 1.0 / tr.hp.iter_size)
    L.call("simt_cell_labels", C.byref(cl), st)
    for name in NEW[1:]:
        L.call(name, C.byref(d), st)
    torch.cuda.synchronize()
    return own


CASES = [("plain", BF, 1), ("plain", F32, 1), ("balanced", BF, 1), ("weighted", BF, 1), ("mix", BF, 1), ("dacs", BF, 1), ("dacs", F32, 2), ("source", BF, 2)]


@pytest.mark.parametrize("mode,dtype,its", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_trainer_launches_equal_the_entry_points(dev, mode, dtype, its):
    kw = MODES[mode]
    source = bool(kw.get("online_source"))
    data = O._views(dev, 2, its)
    src = SM._sources(dev, 2, its) if source else [None, None]
    tr = O._trainer("v2", dev, dtype, None, its, **ON, **kw)
    assert tr.plan.feat_seed is not None and tr.plan.feat_seed.shape == tr.plan.block_io[-1]["z"].shape == (B * tr.h * tr.w, 2048)
    caps = _capture(tr)
    for mb, sb in zip(data, src):
        PT._step(tr, mb, sb, its)
    torch.cuda.synchronize()
    assert len(caps) == 2 * its * (2 if source else 1) and [c["source"] for c in caps] == ([True, False] if source else [False]) * 2 * its
    assert all(c["seeded"] == tr.plan.feat_seed.data_ptr() for c in caps), "a backward ran without the seed"
    h, w = tr.plan.feat_hw
    live = 0
    for i, c in enumerate(caps):
        mine = _relaunch(tr, c)
        for q in ("lab", "lab_part", "phat", "hdr", "seed", "d", "part", "out"):
            assert torch.equal(PT._bits(mine[q]), PT._bits(c[q])), f"pass {i}: {q}: the test's launch differs from the trainer's"
        want, cells = pr.cell_labels_ref(c["label"].cpu().numpy(), h, w, tr.C, RATIO, c["n"].cpu().numpy())
        assert np.array_equal(c["lab"].cpu().numpy(), want) and int(c["lab_part"].sum()) == cells, f"pass {i}: the cell labels are not the restatement's"
        if c["source"]:          # the source pass trains on the ground truth it was given
            given = src[i // (2 * its)][(i // 2) % its][1]
            assert torch.equal(c["label"], given.to(c["label"].device))
        N, nseen = int(c["hdr"][2]), int(c["hdr"][3])
        assert nseen == int((c["n"] > 0).sum()) and float(c["out"][2]) == N
        if i == 0:
            assert nseen == 0 or not c["source"], "the first source pass saw a prototype"
        if N > 0:
            live += 1
            assert nseen >= 2 and bool(torch.isfinite(c["seed"].float()).all()) and bool((c["seed"] != 0).any()) and float(c["out"][0]) > 0
        else:
            assert not bool(c["seed"].float().abs().sum()) and not bool(c["d"].abs().sum()) and not bool(c["out"].abs().sum())
    assert live >= len(caps) // 2, f"only {live} of {len(caps)} captured passes had a valid cell"
    last = [c for c in caps if not c["source"]][-1]
    l = tr.losses()
    assert l["proto_contrast"] == float(last["out"][0]) and l["proto_contrast_cells"] == int(last["hdr"][2])
    if source:
        assert l["source_proto_contrast"] == float([c for c in caps if c["source"]][-1]["out"][0])
    else:
        assert "source_proto_contrast" not in l


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_term_moves_the_trunk_and_no_head_gradient(dev):
    """Same start, same batch: in the first pass with a valid cell (the target pass of step 1 reads the prototypes AFTER the teacher's update) the
    gradients of both heads are the keyword-less trainer's bit for bit and trunk gradients differ; after step 2 trunk weights differ."""
    kw = MODES["plain"]
    data = O._views(dev, 2)
    a, b = O._trainer("v2", dev, BF, **PROTO, **kw), O._trainer("v2", dev, BF, **ON, **kw)
    heads = ("layer5", "layer6")
    for i, mb in enumerate(data):
        PT._step(a, mb, None, 1)
        PT._step(b, mb, None, 1)
        torch.cuda.synchronize()
        if i == 0:
            assert b.losses()["proto_contrast"] > 0 and b.losses()["proto_contrast_cells"] > 0
            assert set(a.plan.grads) == set(b.plan.grads)
            moved = [k for k in a.plan.grads if not torch.equal(a.plan.grads[k], b.plan.grads[k])]
            assert moved and not [k for k in moved if k.startswith(heads)], f"head gradients differ: {[k for k in moved if k.startswith(heads)][:4]}"
            assert all(torch.equal(a.params[k], b.params[k]) for k in a.params if k.startswith(heads))
    trunk = [k for k in a.params if k.endswith("conv1.weight") and not k.startswith(heads)]
    assert any(not torch.equal(a.params[k], b.params[k]) for k in trunk), "the term moved no trunk weight"
    assert all(bool(torch.isfinite(v).all()) for v in b.params.values() if v.is_floating_point())


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_rank_rccl_group_equals_the_single_gpu_trainer(dev):
    kw = dict(ON, **MODES["dacs"])
    one = PT._run("v2", dev, BF, 3, **kw)
    with one_rank_group(dev, PORT) as pg:
        dp = PT._run("v2", dev, BF, 3, pg=pg, **kw)
    O._assert_same(dp, one, "one-rank RCCL group")
    assert dp["per_step"] == one["per_step"] and one["per_step"][-1]["proto_contrast"] > 0


def test_resume_and_the_refusals(dev, tmp_path):
    kw = dict(ON, **MODES["plain"])
    data = O._views(dev, 6)

    def steps(tr, lo, hi, out):
        for mb in data[lo:hi]:
            PT._step(tr, mb, None, 1)
            out["scalars"].append(PT.R.scalars(tr))
            out["labels"].append(tr.label.clone())
            out["read"].append(tr.losses())

    a = dict(scalars=[], labels=[], read=[])
    tr = O._trainer("v2", dev, **kw)
    steps(tr, 0, 6, a)
    a["state"] = O._state(tr)
    del tr
    b = dict(scalars=[], labels=[], read=[])
    tr = O._trainer("v2", dev, **kw)
    steps(tr, 0, 3, b)
    ts = tr.training_state()
    hy = ts["hyper"]
    assert (hy["proto_contrast"], hy["proto_contrast_temp"], hy["proto_contrast_min_ratio"]) == (LAM, TEMP, RATIO)
    assert not [k for k in ts["accumulators"] if "contrast" in k or k.startswith("pc_")], "a new accumulator"
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = O._trainer("v2", dev, **kw)
    tr.load_training_state(ts)
    assert tr.it_done == 3
    steps(tr, 3, 6, b)
    b["state"] = O._state(tr)
    assert b["read"] == a["read"] and a["read"][-1]["proto_contrast"] > 0
    O._assert_same(a, b, "resumed after step 3")
    base = dict(PROTO, **MODES["plain"])
    for other, named in [(base, r"proto_contrast \(state: 0\.5, this trainer: None\)"),
                         (dict(kw, proto_contrast=0.25), r"proto_contrast \(state: 0\.5, this trainer: 0\.25\)"),
                         (dict(kw, proto_contrast_temp=0.1), r"proto_contrast_temp \(state: 0\.2, this trainer: 0\.1\)"),
                         (dict(kw, proto_contrast_min_ratio=0.75), r"proto_contrast_min_ratio \(state: 0\.6, this trainer: 0\.75\)")]:
        with pytest.raises(ValueError, match=named):
            O._trainer("v2", dev, **other).load_training_state(ts)
    off = O._trainer("v2", dev, **base)
    with pytest.raises(ValueError, match=r"proto_contrast \(state: None, this trainer: 0\.5\)"):
        tr.load_training_state(off.training_state())


def test_keyword_refusals(dev):
    im = FD._imnet()
    for kw, named in [(dict(online_labels=0.5, proto_contrast=0.1), "^proto_contrast needs proto_denoise"),
                      (dict(proto_contrast=0.1), "^proto_contrast needs proto_denoise"),
                      (dict(online_labels=0.5, online_source=True, proto_denoise=1.0, proto_contrast=0.1, feat_dist=0.005, feat_dist_state=im),
                       "^proto_contrast with feat_dist"),
                      (dict(online_labels=0.5, proto_denoise=1.0, proto_contrast=-1.0), "^proto_contrast -1.0"),
                      (dict(online_labels=0.5, proto_denoise=1.0, proto_contrast=0.1, proto_contrast_temp=0.0), "^proto_contrast_temp 0.0"),
                      (dict(online_labels=0.5, proto_denoise=1.0, proto_contrast=0.1, proto_contrast_min_ratio=0.5), "^proto_contrast_min_ratio 0.5"),
                      (dict(online_labels=0.5, proto_denoise=1.0, proto_contrast_temp=0.1), "^proto_contrast_temp needs proto_contrast")]:
        with pytest.raises(ValueError, match=named):
            O._trainer("v2", dev, **kw)
    for model in ("v3", "vgg"):
        with pytest.raises(ValueError, match="^proto_contrast: the prototype contrastive term is built for DeepLab-v2"):
            O._trainer(model, dev, online_labels=0.5, proto_denoise=1.0, proto_contrast=0.1)


# ---- (f) the tool ----------------------------------------------------------------------------------------------------------------------------------------
def test_tool_trains_with_the_flag_and_resumes(dev, tmp_path, capsys, monkeypatch):
    """trainV1_warmup --online-labels 0 --online-source --proto-denoise --proto-contrast 0.5 on generated files, B = 2, 129,65: ` pc = ` in every
    loss line, no nan, four launches per pass; 2 + 2 == 4 through --train-state in the loss lines and the final snapshot; a resume with the flag
    dropped is refused by name, and so is --model DeepLabv3 with the flag."""
    from simt_amd.tools import trainV1_warmup as tool
    sets = FD._data_sets(tmp_path)
    common = ["--learning-rate", "2.5e-4", "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50", "--save-pred-every", "100",
              "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2", "--random-mirror", "--online-labels", "0",
              "--online-source", "--proto-denoise"] + sets
    flag = ["--proto-contrast", "0.5"]
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run(tag, stop, *more):
        del calls[:]
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_4.pth")

    out_a, snap_a = run("a", 4, *flag)
    lines = FD._loss_lines(out_a)
    assert len(lines) == 4 and not re.search(r"= nan", out_a), out_a
    assert all(re.search(r" proto = \d+/19 moved \d\.\d{4} pc = \d+\.\d{4} \(\d+\)  lr = ", ln) for ln in lines), lines
    assert [calls.count(n) for n in NEW] == [8, 8, 8, 8]
    assert out_a.count("prototype contrast: every pass adds 0.5 * the mean over the valid layer-4 cells") == 1 and "not checked against SePiCo" in out_a
    state = str(tmp_path / "run.state")
    out_b1, _ = run("b", 2, *flag, "--train-state", state)
    assert FD._loss_lines(out_b1) == lines[:2]
    out_b2, snap_b = run("b", 4, *flag, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_b2), out_b2
    assert FD._loss_lines(out_b2) == lines[2:], (out_a, out_b2)
    sa, sb = torch.load(snap_a), torch.load(snap_b)
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(SystemExit, match="proto_contrast"):          # dropped
        tool.main(common + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        tool.main(common + flag + ["--model", "DeepLabv3", "--snapshot-dir", str(tmp_path / "c"), "--num-steps-stop", "1"])
    assert e.value.code == 2 and "--proto-contrast with --model DeepLabv3" in capsys.readouterr().err
