"""Quality-weighted online labels in the warm-up trainers (keyword online_labels_weighted of WarmupTrainer / WarmupSingleTrainer).

  (a) online_labels = 0.0: every confidence is above the threshold, every weight is exactly 1, and the trainer WITH the keyword (either mode,
      with and without online_mix) is the trainer without it, bit for bit, over three steps;
  (b) a general threshold (the median confidence): `label_quality` == the numpy restatement applied to the per-item counts of a
      simt_online_label(T) the test launches on the trainer's own teacher output; the loss scalars == the float64 restatement of
      tests/_weighted_ref.py on the trainer's logits, labels, weights and map; with online_mix in "item" mode the trainer's map ==
      simt_class_mix_items on the widened bytes with the same draws;
  (c) resume: 3 + save + load + 3 == 6, bitwise, with the keyword and online_mix; the refusals;
  (d) iter_size = 2, and a one-rank RCCL group.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import _weighted_ref as wr
import test_gpu_online_labels as O
import test_gpu_resume as R
from simt_amd import _lib as L
from simt_amd import online_labels as ol
from simt_amd import ops
from simt_amd import train_state as tsf
from simt_amd.data import class_mix
from test_gpu_online_mix import _presence_launch
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
PORT = 29597
B, H, W = O.SIZE
SEED = 11


def _mixkw(mix):
    return {} if mix is None else dict(online_mix=mix, online_mix_seed=SEED)


def _three_steps(model, dev, dtype, data, pg=None, its=1, **kw):
    """-> dict(labels, scalars, state, losses, calls) of a trainer built with **kw over `data`."""
    tr = O._trainer(model, dev, dtype, pg, its, **kw)
    res = dict(labels=[], scalars=[], q=[])
    for mb in data:
        strong = [m[0] for m in mb] if its > 1 else mb[0][0]
        weak = [m[1] for m in mb] if its > 1 else mb[0][1]
        tr.step(strong, None, teacher_image=weak)
        torch.cuda.synchronize()
        res["labels"].append(tr.label.clone())
        res["scalars"].append(R.scalars(tr))
        if kw.get("online_labels_weighted") is not None:
            res["q"].append(tr.label_q.cpu().tolist())
    res["losses"] = tr.losses()
    res["state"] = O._state(tr)
    del tr
    torch.cuda.empty_cache()
    return res


# ---- (a) tau = 0: every weight is 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [None, 1.0], ids=["plain", "mix"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", O.MODELS)
def test_unit_weights_equal_the_trainer_without_the_keyword(dev, model, dtype, mix):
    data = O._views(dev, 3)
    base = _three_steps(model, dev, dtype, data, online_labels=0.0, **_mixkw(mix))
    assert "label_quality" not in base["losses"] and base["losses"]["labelled"] == 1.0
    for mode in ol.WEIGHTED_MODES:
        got = _three_steps(model, dev, dtype, data, online_labels=0.0, online_labels_weighted=mode, **_mixkw(mix))
        assert got["q"] == [[1.0] * B] * 3 and got["losses"]["label_quality"] == [1.0] * B and got["losses"]["labelled"] == 1.0
        O._assert_same(got, base, f"{model} tau = 0, {mode}, mix {mix}")
        assert {k: v for k, v in got["losses"].items() if k != "label_quality"} == base["losses"]


# ---- (b) a general threshold -------------------------------------------------------------------------------------------------------------------------
def _logits(tr, model):
    """The student's low-res logits of the last forward as [B][C][h][w] host tensors: (pred1 | None, pred2)."""
    def nchw(t, ld):
        return t.view(B, tr.h, tr.w, ld)[..., :19].permute(0, 3, 1, 2).float().cpu().contiguous()
    if model == "v2":
        return nchw(tr.plan.out["x1"], tr.plan.ldp["x1"]), nchw(tr.plan.out["x2"], tr.plan.ldp["x2"])
    return None, nchw(tr.pred, tr.ldp)


def _kept_per_item(tr, tau, dev):
    """simt_online_label at `tau` on the trainer's own teacher output -> the per-item numbers of non-255 labels, and the labels."""
    one = tr.online_desc
    lab = torch.full((B, H, W), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(20, dtype=torch.int64, device=dev)
    d = L.OnlineLabelDesc()
    d.fix, d.label, d.counts = one.fix, lab.data_ptr(), cnt.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = one.B, one.h, one.w, one.ld, one.H, one.W, one.C, one.family, tau
    L.call("simt_online_label", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    return (lab != 255).view(B, -1).sum(1).cpu().numpy(), lab


def _items_of_the_existing_mix(x, lab64, apply, rank, dev):
    """simt_label_presence + simt_class_mix_items on int64 labels -> the item map (device)."""
    _words, part = _presence_launch(lab64, 19, dev)
    xo, lo = torch.empty_like(x), torch.empty_like(lab64)
    items = torch.full((B, H, W), 0xEE, dtype=torch.uint8, device=dev)
    e = L.ClassMixDesc()
    e.x, e.lab, e.x_out, e.lab_out, e.part = x.data_ptr(), lab64.data_ptr(), xo.data_ptr(), lo.data_ptr(), part.data_ptr()
    e.B, e.h, e.w, e.n_classes = B, H, W, 19
    table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
    table[:B, :19] = rank
    C.memmove(e.rank, table.ctypes.data, table.nbytes)
    for i in range(B):
        e.partner[i], e.apply[i] = (i + 1) % B, 1 if apply[i] else 0
    L.call("simt_class_mix_items", C.byref(e), items.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    return items, lo


@pytest.mark.parametrize("mode,mix", [("batch", None), ("item", 1.0)], ids=["batch", "item-mix"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", O.MODELS)
def test_general_threshold_weights_losses_and_map(dev, model, dtype, mode, mix):
    data = O._views(dev, 2)
    comp = O.Composition(model, dev, dtype)
    tau = comp.threshold(data[0][0][1])
    del comp
    tr = O._trainer(model, dev, dtype, online_labels=tau, online_labels_weighted=mode, **_mixkw(mix))
    rng = class_mix.generator(SEED, 0)
    half = model == "v3"
    lam = float(tr.head_desc.lambda_seg)
    for step, mb in enumerate(data):
        strong, weak = mb[0]
        tr.step(strong, None, teacher_image=weak)
        torch.cuda.synchronize()
        kept, lab_t = _kept_per_item(tr, tau, dev)
        share = kept / float(H * W)
        print(f"{model} {mode} step {step}: tau = {tau!r}, kept shares {share.tolist()}, q = {tr.label_q.tolist()}")
        assert all(0.1 < s < 0.9 for s in share), share
        want_q = ol.label_quality(kept, H * W, mode)
        got_q = tr.label_q.cpu().numpy()
        assert (got_q.view(np.uint32) == want_q.view(np.uint32)).all(), (got_q.tolist(), want_q.tolist())
        assert (tr.conf_part.long().sum(1).cpu().numpy() == kept).all()
        # the labels: the arg-max everywhere (the labels at tau wherever that launch kept one)
        all_kept, lab_all = _kept_per_item(tr, float("-inf"), dev)
        keep = lab_t != 255
        assert bool((lab_all[keep] == lab_t[keep]).all()) and int(all_kept.sum()) > int(kept.sum())
        item = None
        if mix is None:
            assert torch.equal(tr.label, lab_all) and tr.w_item is None
        else:
            assert torch.equal(tr.lab8.long(), lab_all)
            apply, rank = class_mix.draw_batch(rng, B, 19, mix)
            want_items, want_lab = _items_of_the_existing_mix(strong.contiguous(), lab_all, apply, rank, dev)
            assert torch.equal(tr.label, want_lab)
            assert torch.equal(tr.w_item, want_items), f"{int((tr.w_item != want_items).sum())} bytes of the item map differ from simt_class_mix_items"
            assert bool((want_items != torch.arange(B, device=dev, dtype=torch.uint8).view(B, 1, 1)).any()), "nothing was pasted"
            item = tr.w_item.cpu()
        p1, p2 = _logits(tr, model)
        ref = wr.weighted_ref(p1, p2, tr.label.cpu(), got_q, item, lam, half, torch.float64)
        v = tr.hout[:16].cpu().tolist()
        for i, k in ((1, "l2"), (14, "total")) + ((((0, "l1"),)) if model == "v2" else ()):
            want = float(ref[k])
            assert abs(v[i] - want) <= 1e-4 * (1 + abs(want)), (model, mode, k, v[i], want)
        assert int(v[6]) == ref["N"]
        # the weights matter: the same restatement with unit weights is another number
        unit = wr.weighted_ref(p1, p2, tr.label.cpu(), np.ones(B, np.float32), None, lam, half, torch.float64)
        assert abs(float(unit["total"]) - float(ref["total"])) > 1e-4 * (1 + abs(float(ref["total"])))
    l = tr.losses()
    assert l["label_quality"] == tr.label_q.cpu().tolist() and 0.1 < l["labelled"] < 0.9
    assert l["loss_seg2" if model == "v2" else "loss_seg"] == tr.hout[1].item()


def test_keyword_refusals(dev):
    for kw, named in [(dict(online_labels_weighted="batch"), "online_labels_weighted needs online_labels"),
                      (dict(online_labels=0.5, online_labels_weighted="both"), "online_labels_weighted 'both'"),
                      (dict(online_labels=0.5, online_labels_weighted=True), "online_labels_weighted True"),
                      (dict(online_labels=0.5, online_labels_weighted="item", online_labels_balanced=0.5),
                       "online_labels_weighted cannot be combined with online_labels_balanced in this version")]:
        for model in ("v2", "vgg"):
            with pytest.raises(ValueError, match=named):
                O._trainer(model, dev, **kw)
    plain = O._trainer("v2", dev, online_labels=0.5)
    assert plain.online_labels_weighted is None and not hasattr(plain, "conf_part") and "label_quality" not in plain.losses()


# ---- (c) resume --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", O.MODELS)
def test_resume_with_the_keyword_and_the_mix(dev, tmp_path, model):
    data = O._views(dev, 6)
    tau = O.Composition(model, dev, BF).threshold(data[0][0][1])
    kw = dict(online_labels=tau, online_labels_weighted="item", **_mixkw(0.5))

    def steps(tr, part, out):
        for mb in part:
            tr.step(mb[0][0], None, teacher_image=mb[0][1])
            out["scalars"].append(R.scalars(tr))
            l = tr.losses()
            out["read"].append((l["labelled"], l["label_quality"]))
            out["labels"].append(tr.label.clone())
            out["maps"].append(tr.w_item.clone())

    a = dict(scalars=[], read=[], labels=[], maps=[])
    tr = O._trainer(model, dev, **kw)
    steps(tr, data, a)
    a["state"] = O._state(tr)
    print(f"{model}: tau = {tau!r}, (labelled, q) {a['read']}")
    assert len({tuple(q) for _l, q in a["read"]}) > 1 and all(0.0 < v <= 1.0 for _l, q in a["read"] for v in q)
    del tr
    b = dict(scalars=[], read=[], labels=[], maps=[])
    tr = O._trainer(model, dev, **kw)
    steps(tr, data[:3], b)
    ts = tr.training_state()
    assert ts["hyper"]["online_labels_weighted"] == "item" and ts["hyper"]["online_mix"] == 0.5 and "mix_rng" in ts
    assert set(ts["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported", "label_quality"}
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = O._trainer(model, dev, **kw)
    tr.load_training_state(ts)
    assert tr.it_done == 3 and tr.losses()["label_quality"] == a["read"][2][1]
    steps(tr, data[3:], b)
    b["state"] = O._state(tr)
    assert b["read"] == a["read"] and all(torch.equal(x, y) for x, y in zip(a["maps"], b["maps"]))
    O._assert_same(a, b, f"{model} resumed after step 3")
    if model != "v2":
        return
    # the refusals: the keyword added, dropped or changed
    for other, named in [(dict(online_labels=tau, **_mixkw(0.5)), r"online_labels_weighted \(state: 'item', this trainer: None\)"),
                         (dict(kw, online_labels_weighted="batch"), r"online_labels_weighted \(state: 'item', this trainer: 'batch'\)")]:
        with pytest.raises(ValueError, match=named):
            O._trainer(model, dev, **other).load_training_state(ts)
    off = O._trainer(model, dev, online_labels=tau, **_mixkw(0.5))
    ots = off.training_state()
    assert "online_labels_weighted" not in ots["hyper"] and set(ots["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported"}
    with pytest.raises(ValueError, match=r"online_labels_weighted \(state: None, this trainer: 'item'\)"):
        tr.load_training_state(ots)


# ---- (d) iter_size = 2, one-rank RCCL group ----------------------------------------------------------------------------------------------------------
def test_iter_size_2(dev):
    """Two micro-batches per step at tau = 0: the trainer without the keyword, bit for bit; `label_quality` is the last micro-batch's."""
    data = O._views(dev, 2, its=2)
    base = _three_steps("v2", dev, BF, data, its=2, online_labels=0.0, **_mixkw(1.0))
    got = _three_steps("v2", dev, BF, data, its=2, online_labels=0.0, online_labels_weighted="item", **_mixkw(1.0))
    O._assert_same(got, base, "iter_size 2")
    assert got["losses"]["label_quality"] == [1.0] * B


def test_one_rank_rccl_group_equals_the_single_gpu_trainer(dev):
    data = O._views(dev, 3)
    tau = O.Composition("v3", dev, BF).threshold(data[0][0][1])
    kw = dict(online_labels=tau, online_labels_weighted="item", **_mixkw(1.0))
    one = _three_steps("v3", dev, BF, data, **kw)
    with one_rank_group(dev, PORT) as pg:
        dp = _three_steps("v3", dev, BF, data, pg=pg, **kw)
    O._assert_same(dp, one, "one-rank RCCL group")
    assert dp["q"] == one["q"] and dp["losses"] == one["losses"] and len({tuple(q) for q in one["q"]}) > 1
