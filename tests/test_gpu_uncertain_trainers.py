"""The uncertainty rectification in WarmupTrainer (keyword uncertainty_rectify), at tests/test_gpu_entropy_trainers.py's geometry.

  (a) the two entry points run again by the test, into workspaces of its own, on copies of the trainer's logits, labels, weights and map taken
      directly behind the trainer's own head launches == the trainer's hout[:16] and gradient, bit for bit -- with labels given (no teacher),
      with online_labels, with online_labels_weighted + online_mix, and with online_source on top (the [2B] table; the source pass issues the
      plain launches), bf16 and fp32;
  (b) iter_size = 2, and a one-rank RCCL group;
  (c) one fp32 step's classifier update against the float64 restatement under the classifier bound of tests/test_gpu_configs.py;
  (d) resume 3 + 3 == 6; the refusals name the field.

Keyword None is the parent's trainer: every existing trainer test runs without it.
"""
import ctypes as C

import pytest
import torch

import _uncertain_ref as ur
import test_gpu_entropy_trainers as ET
import test_gpu_online_labels as O
import test_gpu_resume as R
import test_gpu_source_mix as SM
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from simt_amd.step import Hyper, WarmupTrainer
from test_gpu_configs import _update_bound
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
PORT = 29631
B, H, W = O.SIZE
CD = so.load_class_dist()
LAM = 1.0
WMIX = dict(online_labels_weighted="item", online_mix=0.5, online_mix_seed=11)
# ("online" at tau = 0: every pixel keeps its label -- above a from-scratch model's confidences no pixel would, and the cross-entropy over zero
# pixels is NaN as nn.CrossEntropyLoss's is; the weighted rule labels every pixel whatever the threshold)
HOW = {"labels": {}, "online": dict(online_labels=0.0), "weighted_mix": dict(online_labels=0.5, **WMIX),
       "source": dict(online_labels=0.5, online_source=True, **WMIX)}


def _labels(dev, n, its=1):
    """The labels of the steps without a teacher: the synthetic batches' own, with a band of 255s."""
    out = []
    for i in range(n):
        mb = []
        for j in range(its):
            _img, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=700 + 10 * i + j, block=8)
            lab[:, H // 4] = 255
            mb.append(lab.contiguous().to(dev))
        out.append(mb)
    return out


def _step(tr, mb, sb, lb, its):
    """One step: with a teacher ET._step; else the strong images with the given labels."""
    if tr.online_labels is not None:
        return ET._step(tr, mb, sb, its)
    tr.step(mb[0][0] if its == 1 else [m[0] for m in mb], lb[0] if its == 1 else list(lb))


def _run(dev, dtype, steps, how, pg=None, its=1, **kw):
    kw = dict(HOW[how], **kw)
    data, labs = O._views(dev, steps, its), _labels(dev, steps, its)
    src = SM._sources(dev, steps, its) if kw.get("online_source") else [None] * steps
    tr = O._trainer("v2", dev, dtype, pg, its, **kw)
    res = dict(labels=[], scalars=[], per_step=[])
    for mb, sb, lb in zip(data, src, labs):
        _step(tr, mb, sb, lb, its)
        torch.cuda.synchronize()
        res["labels"].append(tr.label.clone())
        res["scalars"].append(R.scalars(tr))
        res["per_step"].append(tr.losses())
    res["losses"] = res["per_step"][-1]
    res["state"] = O._state(tr)
    del tr
    torch.cuda.empty_cache()
    return res


def _relaunch(tr, cap, dev, lam):
    """simt_head_loss_uncertain / simt_head_grad_uncertain by the test: the trainer's descriptor with the logits, labels, weights and map
    replaced by the copies `cap` holds and every output and workspace by buffers of the test's own.  -> (hout[:16] bits, [gradient bits])."""
    hd = L.HeadDesc.from_buffer_copy(tr.head_desc)
    part, keys, hout, g1 = torch.zeros_like(tr.part), torch.zeros_like(tr.keys), torch.full_like(tr.hout, -3.0), torch.zeros_like(tr.g1)
    grads = [torch.full_like(g, 7.0) for g in cap["grads"]]
    hd.pred1, hd.pred2, hd.label = cap["logits"][0].data_ptr(), cap["logits"][1].data_ptr(), cap["label"].data_ptr()
    hd.dpred1_t, hd.dpred2_t = grads[0].data_ptr(), grads[1].data_ptr()
    hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
    keep = [part, keys, g1]
    for f in ("conf_out", "label_ws"):
        if getattr(hd, f):
            keep.append(torch.zeros(B, H, W, dtype=torch.uint8, device=dev))
            setattr(hd, f, keep[-1].data_ptr())
    w, item = cap["w"], cap["item"]
    args = (None if w is None else w.data_ptr(), 0 if w is None else w.numel(), None if item is None else item.data_ptr())
    rec = L.HeadUncertainty(lam)
    st = ops.stream_ptr()
    L.call("simt_head_loss_uncertain", C.byref(hd), *args, C.byref(rec), st)
    L.call("simt_head_grad_uncertain", C.byref(hd), *args, C.byref(rec), st)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)          # noqa: E731
    return hout[:16].view(torch.int32).clone(), [bits(g) for g in grads], keep


# ---- (a) the trainer's launches == the test's ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_trainer_launches_equal_the_entry_points(dev, dtype, how, monkeypatch):
    kw = HOW[how]
    data, labs = O._views(dev, 1), _labels(dev, 1)
    src = SM._sources(dev, 1) if kw.get("online_source") else [None]
    tr = O._trainer("v2", dev, dtype, uncertainty_rectify=LAM, **kw)
    cap = ET._capture(tr, "v2")
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    _step(tr, data[0], src[0], labs[0], 1)
    torch.cuda.synchronize()
    heads = [n for n in calls if n.startswith("simt_head_")]
    want = (["simt_head_loss", "simt_head_grad"] if how == "source" else []) + ["simt_head_loss_uncertain", "simt_head_grad_uncertain"]
    assert heads == want, heads          # the source pass keeps the plain launches
    monkeypatch.undo()
    assert torch.equal(cap["hout"].view(torch.int32), tr.hout[:16].view(torch.int32))
    if how == "source":
        assert cap["w"].numel() == 2 * B and cap["item"] is not None and bool((cap["w"][B:] == 1).all())
    elif how == "weighted_mix":
        assert cap["w"].numel() == B and cap["item"] is not None
    else:
        assert cap["w"] is None and cap["item"] is None
    hout, grads, _keep = _relaunch(tr, cap, dev, LAM)
    assert torch.equal(hout, cap["hout"].view(torch.int32)), (hout.view(torch.float32).tolist(), cap["hout"].tolist())
    for k, (g, t) in enumerate(zip(grads, cap["grads"])):
        t = t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)
        QP = tr.QP          # (the launch writes columns [0, QP); the pitch columns behind them keep what the buffer held)
        assert torch.equal(g[:, :QP], t[:, :QP]), f"head {k}: {int((g[:, :QP] != t[:, :QP]).sum())} gradient words differ from the trainer's"
        assert bool((cap["grads"][k].float() != 0).any())
    v = tr.hout[:16].cpu().tolist()
    l = tr.losses()
    assert (l["loss_seg1"], l["loss_seg2"], l["uncertainty1"], l["uncertainty2"], l["rectify1"], l["rectify2"]) == tuple(v[:6])
    assert v[2] > 0.0 and v[3] > 0.0 and 0.0 < v[4] < 1.0 and 0.0 < v[5] < 1.0, v
    lam_seg = float(tr.head_desc.lambda_seg)
    total = v[1] + LAM * v[3] + lam_seg * (v[0] + LAM * v[2])
    assert abs(v[14] - total) <= 1e-5 * (1 + abs(total)) and l["total"] == v[14]
    if how == "source":
        assert "source_seg2" in l


# ---- (b) iter_size = 2, one-rank RCCL group -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["labels", "source"])
def test_iter_size_2_differs_from_the_trainer_without_and_stays_finite(dev, how):
    base = _run(dev, BF, 2, how, its=2)
    got = _run(dev, BF, 2, how, its=2, uncertainty_rectify=LAM)
    assert "uncertainty2" in got["per_step"][0] and "uncertainty2" not in base["per_step"][0]
    assert not torch.equal(got["scalars"][0], base["scalars"][0])
    assert any(not torch.equal(got["state"][k], base["state"][k]) for k in base["state"] if k.startswith("model "))
    assert all(v == v and abs(v) != float("inf") for k, v in got["losses"].items() if not isinstance(v, list))
    again = _run(dev, BF, 2, how, its=2, uncertainty_rectify=LAM)
    O._assert_same(again, got, f"iter_size 2 {how}: a second run")


def test_one_rank_rccl_group_equals_the_single_gpu_trainer(dev):
    one = _run(dev, BF, 3, "source", uncertainty_rectify=LAM)
    with one_rank_group(dev, PORT) as pg:
        dp = _run(dev, BF, 3, "source", pg=pg, uncertainty_rectify=LAM)
    O._assert_same(dp, one, "one-rank RCCL group")
    assert dp["per_step"] == one["per_step"] and "uncertainty2" in one["losses"]


# ---- (c) one step against float64 ----------------------------------------------------------------------------------------------------------------------
ORACLE_LAYERS = (1, 1, 2, 1)
CLASSIFIER_KEYS = ("layer6.conv2d_list.1.weight", "layer6.conv2d_list.0.bias", "layer5.conv2d_list.0.weight", "layer5.conv2d_list.1.bias")


def test_classifier_update_vs_float64(dev, monkeypatch):
    """One fp32 step with labels given against oracle.simt_oracle.OracleWarmupTrainer in float64 whose loss is the restatement's (the
    module's `warmup_losses` replaced for the test): losses 1e-4 * (1 + |ref|), classifier updates within test_gpu_configs._update_bound.  The
    float64 step WITHOUT the rectification must miss that bound, or the case shows nothing."""
    st = so.recipe_state(so.state_shapes(19, 0, False, layers=ORACLE_LAYERS), seed=77, head_scale=8.0)
    Bo, Ho, Wo = 2, 97, 97
    x, lab = so.synthetic_batch(Bo, Ho, Wo, CD.numpy(), seed=500, block=16)
    hp = dict(open_classes=0, lr=2.5e-4)
    plain = so.OracleWarmupTrainer(st, so.Hyper(**hp), layers=ORACLE_LAYERS, dtype=torch.float64)
    plain.step(x, lab, 0)
    kept = {}

    def losses(p1, p2, label, lambda_seg, size):
        r = ur.uncertain_losses(p1, p2, label, None, None, lambda_seg, False, 19, LAM)
        kept.update({k: (float(v.detach()) if torch.is_tensor(v) else v) for k, v in r.items()})
        return r["total"], r["r1"], r["r2"]
    monkeypatch.setattr(so, "warmup_losses", losses)
    o64 = so.OracleWarmupTrainer(st, so.Hyper(**hp), layers=ORACLE_LAYERS, dtype=torch.float64)
    o64.step(x, lab, 0)
    monkeypatch.undo()
    tr = WarmupTrainer(st, Hyper(**hp), Bo, Ho, Wo, dtype=F32, device=dev, layers=ORACLE_LAYERS, uncertainty_rectify=LAM)
    tr.step(x.to(dev), lab.to(dev), 0)
    l = tr.losses()
    print(f"[uncertain] trainer {l}; float64 {kept}")
    for a, b in (("total", "total"), ("loss_seg1", "r1"), ("loss_seg2", "r2"), ("uncertainty1", "k1"), ("uncertainty2", "k2"),
                 ("rectify1", "m1"), ("rectify2", "m2")):
        assert abs(l[a] - kept[b]) <= 1e-4 * (1 + abs(kept[b])), (a, l[a], kept[b])
    shown = 0
    for k in CLASSIFIER_KEYS:
        p0, v, p64 = st[k].double(), tr.params[k].detach().cpu().double(), o64.st[k].detach()
        du = (p64 - p0).norm().item()
        rel = (v - p64).norm().item() / max(du, 1e-30)
        rel_plain = (plain.st[k].detach() - p64).norm().item() / max(du, 1e-30)
        print(f"[uncertain] {k}: |update| {du:.3e}, gpu-vs-float64 / |update| {rel:.3e}, the step without the keyword {rel_plain:.3e}")
        assert du > 0 and rel <= _update_bound(k), (k, rel)
        shown += rel_plain > _update_bound(k)
    assert shown == len(CLASSIFIER_KEYS), "the step without the rectification passes the bound: the case shows nothing"


# ---- (d) resume ----------------------------------------------------------------------------------------------------------------------------------------
def test_resume_3_plus_3(dev, tmp_path):
    kw = dict(HOW["source"], uncertainty_rectify=LAM)
    data, src = O._views(dev, 6), SM._sources(dev, 6)

    def steps(tr, lo, hi, out):
        for mb, sb in list(zip(data, src))[lo:hi]:
            ET._step(tr, mb, sb, 1)
            out["scalars"].append(R.scalars(tr))
            out["labels"].append(tr.label.clone())
            out["read"].append(tr.losses())

    a = dict(scalars=[], labels=[], read=[])
    tr = O._trainer("v2", dev, **kw)
    steps(tr, 0, 6, a)
    a["state"] = O._state(tr)
    assert all("uncertainty2" in r and "rectify2" in r for r in a["read"])
    del tr
    b = dict(scalars=[], labels=[], read=[])
    tr = O._trainer("v2", dev, **kw)
    steps(tr, 0, 3, b)
    ts = tr.training_state()
    assert ts["hyper"]["uncertainty_rectify"] == LAM
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = O._trainer("v2", dev, **kw)
    tr.load_training_state(ts)
    assert tr.it_done == 3
    steps(tr, 3, 6, b)
    b["state"] = O._state(tr)
    assert b["read"] == a["read"]
    O._assert_same(a, b, "resumed after step 3")
    for other, named in [(HOW["source"], r"uncertainty_rectify \(state: 1\.0, this trainer: None\)"),
                         (dict(kw, uncertainty_rectify=0.5), r"uncertainty_rectify \(state: 1\.0, this trainer: 0\.5\)")]:
        with pytest.raises(ValueError, match=named):
            O._trainer("v2", dev, **other).load_training_state(ts)
    off = O._trainer("v2", dev, **HOW["source"])
    ots = off.training_state()
    assert "uncertainty_rectify" not in ots["hyper"]
    with pytest.raises(ValueError, match=r"uncertainty_rectify \(state: None, this trainer: 1\.0\)"):
        tr.load_training_state(ots)


def test_keyword_refusals(dev):
    for kw, named in [(dict(uncertainty_rectify=-1.0), "uncertainty_rectify -1.0"), (dict(uncertainty_rectify=float("nan")), "uncertainty_rectify nan"),
                      (dict(online_labels=0.5, entropy_min=0.005, uncertainty_rectify=1.0), "uncertainty_rectify beside entropy_min")]:
        with pytest.raises(ValueError, match=named):
            O._trainer("v2", dev, **kw)
    for model in ("v3", "vgg"):
        with pytest.raises(ValueError, match="uncertainty_rectify: .*one head"):
            O._trainer(model, dev, uncertainty_rectify=1.0)
    plain = O._trainer("v2", dev)
    assert plain.uncertainty_rectify is None and not hasattr(plain, "uncertainty_rec") and "uncertainty2" not in plain.losses()
