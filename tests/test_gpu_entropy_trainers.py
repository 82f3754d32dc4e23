"""The entropy term of the target pass in the warm-up trainers (keywords entropy_min / entropy_eta / entropy_after of WarmupTrainer
and WarmupSingleTrainer).

  (a) entropy_after beyond the steps run: the trainer without the keywords, bit for bit (labels, scalars, every tensor of the state, losses());
  (b) the term on, iter_size = 1: the two entry points run again by the test, into workspaces of its own, on copies of the trainer's logits,
      labels, weights and map taken directly behind the trainer's own head launches (the backward is free to reuse `plan.dlogits`, so the copies
      are taken in front of it) == the trainer's hout[:16] and gradient, bit for bit -- with online_labels_weighted + online_source +
      online_mix (the [2B] table and the source mix's map) and class-balanced (NULL weights); the source pass issues the plain launches;
  (c) iter_size = 2 with the switch between two steps, and a one-rank RCCL group;
  (d) resume 3 + 3 == 6 with entropy_after = 4, so the switch lies behind the resume; the refusals name the field.
"""
import ctypes as C

import pytest
import torch

import test_gpu_online_labels as O
import test_gpu_resume as R
import test_gpu_source_mix as SM
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
PORT = 29611
B, H, W = O.SIZE
LAM, ETA = 0.5, 2.0          # a lambda at which the term moves the weights visibly within three steps
DACS = dict(online_labels_weighted="batch", online_source=True, online_mix=0.5, online_mix_seed=11)
BALANCED = dict(online_labels_balanced=0.5, online_labels_momentum=0.5)


def _step(tr, mb, sb, its):
    one = its == 1
    kw = {}
    if sb is not None:
        kw.update(source_image=sb[0][0] if one else [s[0] for s in sb], source_label=sb[0][1] if one else [s[1] for s in sb])
    tr.step(mb[0][0] if one else [m[0] for m in mb], None, teacher_image=mb[0][1] if one else [m[1] for m in mb], **kw)


def _run(model, dev, dtype, steps, pg=None, its=1, **kw):
    """-> dict(labels, scalars, state, losses, per_step) of a trainer built with **kw."""
    data = O._views(dev, steps, its)
    src = SM._sources(dev, steps, its) if kw.get("online_source") else [None] * steps
    tr = O._trainer(model, dev, dtype, pg, its, **kw)
    res = dict(labels=[], scalars=[], per_step=[])
    for mb, sb in zip(data, src):
        _step(tr, mb, sb, its)
        torch.cuda.synchronize()
        res["labels"].append(tr.label.clone())
        res["scalars"].append(R.scalars(tr))
        res["per_step"].append(tr.losses())
    res["losses"] = res["per_step"][-1]
    res["state"] = O._state(tr)
    del tr
    torch.cuda.empty_cache()
    return res


# ---- (a) the switch beyond the run -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", O.MODELS)
def test_switch_beyond_the_run_is_the_trainer_without_the_keywords(dev, model, dtype):
    kw = dict(online_labels=0.5, **DACS)
    base = _run(model, dev, dtype, 3, **kw)
    got = _run(model, dev, dtype, 3, entropy_min=LAM, entropy_eta=0.5, entropy_after=100, **kw)
    O._assert_same(got, base, f"{model} entropy_after = 100")
    assert got["per_step"] == base["per_step"] and "entropy2" not in got["losses"] and "entropy1" not in got["losses"]


# ---- (b) the term on: the trainer's launches == the test's ------------------------------------------------------------------------------------------
def _relaunch(tr, cap, dev):
    """simt_head_loss_entropy / simt_head_grad_entropy by the test: the trainer's descriptor with the logits, labels, weights and map replaced by
    the copies `cap` holds and every output and workspace by buffers of the test's own.  -> (hout[:16] bits, [gradient bits per head])."""
    hd = L.HeadDesc.from_buffer_copy(tr.head_desc)
    two = not hd.single
    part, keys, hout, g1 = torch.zeros_like(tr.part), torch.zeros_like(tr.keys), torch.full_like(tr.hout, -3.0), torch.zeros_like(tr.g1)
    grads = [torch.full_like(g, 7.0) for g in cap["grads"]]
    lab = cap["label"]
    hd.pred2, hd.label = cap["logits"][-1].data_ptr(), lab.data_ptr()
    hd.dpred2_t = grads[-1].data_ptr()
    if two:
        hd.pred1, hd.dpred1_t = cap["logits"][0].data_ptr(), grads[0].data_ptr()
    hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
    conf = lws = None
    if hd.conf_out:
        conf = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        hd.conf_out = conf.data_ptr()
    if hd.label_ws:
        lws = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        hd.label_ws = lws.data_ptr()
    w, item = cap["w"], cap["item"]
    args = (None if w is None else w.data_ptr(), 0 if w is None else w.numel(), None if item is None else item.data_ptr())
    rec = L.HeadEntropy(LAM, ETA)
    st = ops.stream_ptr()
    L.call("simt_head_loss_entropy", C.byref(hd), *args, C.byref(rec), st)
    L.call("simt_head_grad_entropy", C.byref(hd), *args, C.byref(rec), st)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)          # noqa: E731
    return hout[:16].view(torch.int32).clone(), [bits(g) for g in grads], (part, keys, g1, conf, lws)


def _capture(tr, model):
    """Wraps the trainer's `_head_grad`: directly behind it (same stream) the logits, labels, weights, map and gradients are copied."""
    cap = {}
    real = tr._head_grad

    def head_grad(st):
        real(st)
        if model == "v2":
            cap["logits"] = [tr.plan.out["x1"].clone(), tr.plan.out["x2"].clone()]
            cap["grads"] = [tr.plan.dlogits["x1"].clone(), tr.plan.dlogits["x2"].clone()]
        else:
            cap["logits"], cap["grads"] = [tr.pred.clone()], [tr.plan.dlogits["x"].clone()]
        cap["label"], cap["hout"] = tr.label.clone(), tr.hout[:16].clone()
        weighted = getattr(tr, "online_labels_weighted", None) is not None
        table = (tr.label_w if tr._source_table() else tr.label_q) if weighted else None
        cap["w"] = None if table is None else table.clone()
        cap["item"] = None if (not weighted or tr.w_item is None) else tr.w_item.clone()
    tr._head_grad = head_grad
    return cap


@pytest.mark.parametrize("how", ["dacs", "balanced"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", O.MODELS)
def test_trainer_launches_equal_the_entry_points(dev, model, dtype, how, monkeypatch):
    # (class-balanced at tau = 0: every pixel keeps its label -- above a from-scratch model's confidences no pixel would, and the cross-entropy
    # over zero pixels is NaN as nn.CrossEntropyLoss's is)
    kw = dict(online_labels=0.5, **DACS) if how == "dacs" else dict(online_labels=0.0, **BALANCED)
    data = O._views(dev, 2)
    src = SM._sources(dev, 2) if how == "dacs" else [None, None]
    tr = O._trainer(model, dev, dtype, entropy_min=LAM, entropy_eta=ETA, entropy_after=1, **kw)
    cap = _capture(tr, model)
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    _step(tr, data[0], src[0], 1)          # iteration 0: in front of the switch
    torch.cuda.synchronize()
    assert not any("entropy" in n for n in calls) and "entropy2" not in tr.losses()
    calls.clear()
    _step(tr, data[1], src[1], 1)          # iteration 1: the term is on
    torch.cuda.synchronize()
    heads = [n for n in calls if n.startswith("simt_head_")]
    want = (["simt_head_loss", "simt_head_grad"] if how == "dacs" else []) + ["simt_head_loss_entropy", "simt_head_grad_entropy"]
    assert heads == want, heads          # the source pass keeps the plain launches
    monkeypatch.undo()
    assert torch.equal(cap["hout"].view(torch.int32), tr.hout[:16].view(torch.int32))
    if how == "dacs":
        assert cap["w"].numel() == 2 * B and cap["item"] is not None and bool((cap["w"][B:] == 1).all())
    else:
        assert cap["w"] is None and cap["item"] is None
    hout, grads, _keep = _relaunch(tr, cap, dev)
    assert torch.equal(hout, cap["hout"].view(torch.int32)), (hout.view(torch.float32).tolist(), cap["hout"].tolist())
    for k, (g, t) in enumerate(zip(grads, cap["grads"])):
        t = t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)
        QP = tr.QP          # (the launch writes columns [0, QP); the pitch columns behind them keep what the buffer held)
        assert torch.equal(g[:, :QP], t[:, :QP]), f"head {k}: {int((g[:, :QP] != t[:, :QP]).sum())} gradient words differ from the trainer's"
        assert bool((cap["grads"][k].float() != 0).any())
    v = tr.hout[:16].cpu().tolist()
    l = tr.losses()
    assert 0.0 < v[3] < 1.5 and l["entropy2"] == v[3] and (("entropy1" in l and l["entropy1"] == v[2] > 0.0) if model == "v2" else "entropy1" not in l)
    lam_seg = float(tr.head_desc.lambda_seg)
    total = v[1] + LAM * v[3] + (lam_seg * v[0] + LAM * lam_seg * v[2] if model == "v2" else 0.0)
    assert abs(v[14] - total) <= 1e-5 * (1 + abs(total)) and l["total"] == v[14]


# ---- (c) iter_size = 2, one-rank RCCL group ----------------------------------------------------------------------------------------------------------
def test_iter_size_2_switches_between_two_steps(dev):
    kw = dict(online_labels=0.5, **DACS)
    base = _run("v2", dev, BF, 2, its=2, **kw)
    got = _run("v2", dev, BF, 2, its=2, entropy_min=LAM, entropy_after=1, **kw)
    assert torch.equal(got["scalars"][0], base["scalars"][0]) and got["per_step"][0] == base["per_step"][0]
    assert not torch.equal(got["scalars"][1], base["scalars"][1]) and "entropy2" in got["per_step"][1] and "entropy2" not in got["per_step"][0]
    assert any(not torch.equal(got["state"][k], base["state"][k]) for k in base["state"] if k.startswith("model "))
    assert all(v == v and abs(v) != float("inf") for k, v in got["losses"].items() if not isinstance(v, list))


def test_one_rank_rccl_group_equals_the_single_gpu_trainer(dev):
    kw = dict(online_labels=0.5, entropy_min=LAM, **DACS)
    one = _run("v3", dev, BF, 3, **kw)
    with one_rank_group(dev, PORT) as pg:
        dp = _run("v3", dev, BF, 3, pg=pg, **kw)
    O._assert_same(dp, one, "one-rank RCCL group")
    assert dp["per_step"] == one["per_step"] and "entropy2" in one["losses"]


# ---- (d) resume --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", O.MODELS)
def test_resume_in_front_of_the_switch(dev, tmp_path, model):
    kw = dict(online_labels=0.5, entropy_min=LAM, entropy_eta=ETA, entropy_after=4, **DACS)
    data, src = O._views(dev, 6), SM._sources(dev, 6)

    def steps(tr, lo, hi, out):
        for mb, sb in list(zip(data, src))[lo:hi]:
            _step(tr, mb, sb, 1)
            out["scalars"].append(R.scalars(tr))
            out["labels"].append(tr.label.clone())
            out["read"].append(tr.losses())

    a = dict(scalars=[], labels=[], read=[])
    tr = O._trainer(model, dev, **kw)
    steps(tr, 0, 6, a)
    a["state"] = O._state(tr)
    assert ["entropy2" in r for r in a["read"]] == [False] * 4 + [True] * 2
    del tr
    b = dict(scalars=[], labels=[], read=[])
    tr = O._trainer(model, dev, **kw)
    steps(tr, 0, 3, b)
    ts = tr.training_state()
    assert (ts["hyper"]["entropy_min"], ts["hyper"]["entropy_eta"], ts["hyper"]["entropy_after"]) == (LAM, ETA, 4)
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = O._trainer(model, dev, **kw)
    tr.load_training_state(ts)
    assert tr.it_done == 3 and "entropy2" not in tr.losses()
    steps(tr, 3, 6, b)
    b["state"] = O._state(tr)
    assert b["read"] == a["read"]
    O._assert_same(a, b, f"{model} resumed after step 3")
    if model != "v2":
        return
    base = dict(online_labels=0.5, **DACS)
    for other, named in [(base, r"entropy_min \(state: 0\.5, this trainer: None\)"),
                         (dict(kw, entropy_min=0.25), r"entropy_min \(state: 0\.5, this trainer: 0\.25\)"),
                         (dict(kw, entropy_eta=0.5), r"entropy_eta \(state: 2\.0, this trainer: 0\.5\)"),
                         (dict(kw, entropy_after=2), r"entropy_after \(state: 4, this trainer: 2\)")]:
        with pytest.raises(ValueError, match=named):
            O._trainer(model, dev, **other).load_training_state(ts)
    off = O._trainer(model, dev, **base)
    ots = off.training_state()
    assert not any(k.startswith("entropy") for k in ots["hyper"])
    with pytest.raises(ValueError, match=r"entropy_min \(state: None, this trainer: 0\.5\)"):
        tr.load_training_state(ots)


def test_keyword_refusals(dev):
    for kw, named in [(dict(entropy_min=0.005), "entropy_min needs online_labels"),
                      (dict(online_labels=0.5, entropy_min=0.0), "entropy_min 0.0"),
                      (dict(online_labels=0.5, entropy_min=float("nan")), "entropy_min nan"),
                      (dict(online_labels=0.5, entropy_min=0.005, entropy_eta=0.0), "entropy_eta 0.0"),
                      (dict(online_labels=0.5, entropy_min=0.005, entropy_after=-1), "entropy_after -1"),
                      (dict(online_labels=0.5, entropy_after=3), "entropy_after needs entropy_min")]:
        for model in ("v2", "vgg"):
            with pytest.raises(ValueError, match=named):
                O._trainer(model, dev, **kw)
    plain = O._trainer("v2", dev, online_labels=0.5)
    assert plain.entropy_min is None and not hasattr(plain, "entropy_rec") and "entropy2" not in plain.losses()
