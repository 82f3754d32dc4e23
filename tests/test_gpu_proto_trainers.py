"""The prototype weights in the warm-up trainers (keywords proto_denoise / proto_momentum of WarmupTrainer and WarmupSingleTrainer).

  (a) without the keyword no simt_proto launch is issued and every label descriptor reads the teacher's own output;
  (b) with it: step 1 -- no class seen -- is the keyword-less trainer's, labels and weights bit for bit; from step 2 the labels differ;
  (c) the three entry points run again by the test on copies of the trainer's features, teacher output, prototypes and counts, taken directly
      in front of the trainer's own launches, give the trainer's rectified map, eta and n bit for bit, and the label launch of the trainer's
      mode on THAT map gives the trainer's label map -- plain, class-balanced, weighted, with online_mix, with online_source, iter_size = 2;
  (d) a one-rank RCCL group is the single-GPU trainer; resume 3 + 3 == 6; the refusals name the field.
"""
import ctypes as C

import pytest
import torch

import test_gpu_online_labels as O
import test_gpu_resume as R
import test_gpu_source_mix as SM
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import proto as P
from simt_amd import train_state as tsf
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
PORT = 29617
B, H, W = O.SIZE
TEMP, MOM = 0.5, 0.9
MODES = {"plain": dict(online_labels=0.3), "plain0": dict(online_labels=0.0), "balanced": dict(online_labels=0.0, online_labels_balanced=0.5, online_labels_momentum=0.5),
         "weighted": dict(online_labels=0.3, online_labels_weighted="item"), "mix": dict(online_labels=0.3, online_mix=0.5, online_mix_seed=11),
         "dacs": dict(online_labels=0.3, online_labels_weighted="batch", online_source=True, online_mix=0.5, online_mix_seed=11)}


def _step(tr, mb, sb, its):
    one = its == 1
    kw = {}
    if sb is not None:
        kw.update(source_image=sb[0][0] if one else [s[0] for s in sb], source_label=sb[0][1] if one else [s[1] for s in sb])
    tr.step(mb[0][0] if one else [m[0] for m in mb], None, teacher_image=mb[0][1] if one else [m[1] for m in mb], **kw)


def _run(model, dev, dtype, steps, pg=None, its=1, **kw):
    data = O._views(dev, steps, its)
    src = SM._sources(dev, steps, its) if kw.get("online_source") else [None] * steps
    tr = O._trainer(model, dev, dtype, pg, its, **kw)
    res = dict(labels=[], scalars=[], per_step=[], states=[])
    for mb, sb in zip(data, src):
        _step(tr, mb, sb, its)
        torch.cuda.synchronize()
        res["labels"].append(tr.label.clone())
        res["scalars"].append(R.scalars(tr))
        res["per_step"].append(tr.losses())
        res["states"].append({k: v.clone() for k, v in tr.params.items()})
    res["state"] = O._state(tr)
    if kw.get("proto_denoise") is not None:
        res["eta"], res["n"] = tr.proto_eta.clone(), tr.proto_n.clone()
    del tr
    torch.cuda.empty_cache()
    return res


# ---- (a), (b) ------------------------------------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_nothing_is_launched_or_re_pointed(dev, monkeypatch):
    tr = O._trainer("v2", dev, online_labels=0.3)
    assert tr.proto_denoise is None and not hasattr(tr, "proto_map") and tr.online_desc.fix == tr.fixp.data_ptr()
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    _step(tr, O._views(dev, 1)[0], None, 1)
    torch.cuda.synchronize()
    assert calls and not any("proto" in n for n in calls) and "proto_seen" not in tr.losses()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", O.MODELS)
def test_step_one_is_the_trainer_without_the_keyword_and_step_two_is_not(dev, model, dtype):
    # (DeepLab-v2 at tau = 0: above 0.3 the reduced model's teacher keeps ONE class -- measured: proto_seen 1, labelled 0.002 -- and with one
    # prototype every class takes the same distance, so the rule is the identity whatever the code does; at 0 it finds five classes and the
    # weights move a tenth of the cells at step 2)
    kw = dict(online_labels=0.0) if model == "v2" else MODES["plain"]
    base = _run(model, dev, dtype, 3, **kw)
    got = _run(model, dev, dtype, 3, proto_denoise=TEMP, proto_momentum=MOM, **kw)
    assert torch.equal(got["labels"][0], base["labels"][0]) and torch.equal(got["scalars"][0], base["scalars"][0])
    for k, v in base["states"][0].items():
        assert torch.equal(got["states"][0][k], v), f"{k} differs after step 1"
    assert not torch.equal(got["labels"][1], base["labels"][1]), "the prototypes moved no label of step 2"
    first, last = got["per_step"][0], got["per_step"][-1]
    assert first["proto_changed"] == 0.0 and 0 < first["proto_seen"] <= 19 and last["proto_seen"] >= first["proto_seen"]
    assert 0.0 < last["proto_changed"] <= 1.0 and bool(torch.isfinite(got["eta"][got["n"] > 0]).all())
    assert {k: v for k, v in first.items() if not k.startswith("proto_")} == base["per_step"][0]


# ---- (c) the trainer's launches == the test's -------------------------------------------------------------------------------------------------------------
def _capture(tr):
    """Wraps the trainer's `_proto_launches`: in front of them (same stream) the inputs are copied, behind them the outputs."""
    cap = {}
    real = tr._proto_launches

    def launches(st):
        cap.update(F=tr.proto_feat.clone(), P=tr.fixp.clone(), eta0=tr.proto_eta.clone(), n0=tr.proto_n.clone(),
                   thr=tr.label_thr.clone() if getattr(tr, "online_labels_balanced", None) is not None else None)
        real(st)
        cap.update(map=tr.proto_map.clone(), eta=tr.proto_eta.clone(), n=tr.proto_n.clone(), lab=tr.proto_lab.clone(),
                   changed=tr.proto_changed_part.clone())
    tr._proto_launches = launches
    return cap


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32) if t.is_floating_point() else t


def _relaunch(tr, cap):
    """The three entry points and the label launch of the trainer's mode, by the test, into buffers of its own."""
    M, D = cap["F"].shape
    Cn, ldp = tr.C, tr.ldf
    out, eta, n = torch.full_like(cap["map"], -3.0), cap["eta0"].clone(), cap["n0"].clone()
    lab, changed, ws = torch.zeros_like(cap["lab"]), torch.zeros_like(cap["changed"]), torch.zeros_like(tr.proto_ws)
    st = ops.stream_ptr()
    r = P.fill_rectify(cap["F"], D, D, cap["P"], out, ldp, eta, n, lab, changed, M, Cn, tr.dtype, tr._family, TEMP, tr.online_labels)
    L.call("simt_proto_rectify", C.byref(r), st)
    L.call("simt_proto_accumulate", C.byref(P.fill_accumulate(cap["F"], D, D, lab, ws, M, Cn, tr.dtype)), st)
    L.call("simt_proto_update", C.byref(P.fill_update(ws, eta, n, M, D, Cn, MOM)), st)
    # the label launch of the trainer's mode on the test's map
    mix = tr.online_mix is not None
    if getattr(tr, "online_labels_weighted", None) is not None:
        name, desc = ("simt_online_label_w_u8" if mix else "simt_online_label_w"), tr.online_w_desc
    elif tr.online_labels_balanced is not None:
        name, desc = ("simt_online_label_cb_u8", tr.online_cb_u8_desc) if mix else ("simt_online_label_cb", tr.online_cb_desc)
    else:
        name, desc = ("simt_online_label_u8", tr.online_u8_desc) if mix else ("simt_online_label", tr.online_desc)
    assert desc.fix == tr.proto_map.data_ptr(), f"{name}: the trainer's descriptor does not read the rectified map"
    d = type(desc).from_buffer_copy(desc)
    own = {"label": torch.zeros_like(tr.label), "counts": torch.zeros_like(tr.label_counts)}
    if mix:
        own.update(lab8=torch.zeros_like(tr.lab8), part=torch.zeros_like(tr.mix_part))
    if hasattr(tr, "conf_part"):
        own["conf_part"] = torch.zeros_like(tr.conf_part)
    if cap["thr"] is not None:
        own.update(hist=torch.zeros_like(tr.label_hist), thr=cap["thr"].clone())
    d.fix = out.data_ptr()
    for field, _t in d._fields_:
        if field in own:
            setattr(d, field, own[field].data_ptr())
    L.call(name, C.byref(d), st)
    torch.cuda.synchronize()
    return dict(map=out, eta=eta, n=n, lab=lab, changed=changed, labels=own["lab8"] if mix else own["label"])


CASES = [(m, d, "plain0" if m == "v2" else "plain", 1) for m in O.MODELS for d in (BF, F32)] + [("v2", BF, "balanced", 1), ("vgg", BF, "weighted", 1), ("v3", BF, "mix", 1),
                                                                       ("v2", BF, "dacs", 1), ("v3", F32, "dacs", 2)]


@pytest.mark.parametrize("model,dtype,mode,its", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_trainer_launches_equal_the_entry_points(dev, model, dtype, mode, its):
    kw = MODES[mode]
    data = O._views(dev, 2, its)
    src = SM._sources(dev, 2, its) if kw.get("online_source") else [None, None]
    tr = O._trainer(model, dev, dtype, None, its, proto_denoise=TEMP, proto_momentum=MOM, **kw)
    assert tr.proto_feat.shape == (B * tr.h * tr.w, {"v2": 2048, "v3": tr.proto_feat.shape[1], "vgg": tr.proto_feat.shape[1]}[model])
    cap = _capture(tr)
    for mb, sb in zip(data, src):
        _step(tr, mb, sb, its)
    torch.cuda.synchronize()
    assert int((cap["n0"] > 0).sum()) > 0, "the captured micro-batch saw no prototype"
    mine = _relaunch(tr, cap)
    for q in ("map", "eta", "n", "lab", "changed"):
        assert torch.equal(_bits(mine[q]), _bits(cap[q])), f"{q}: the test's launch differs from the trainer's"
    assert torch.equal(_bits(tr.proto_eta), _bits(cap["eta"])) and not torch.equal(_bits(cap["map"]), _bits(cap["P"]))
    if mode == "plain0":          # several classes seen: the weights move cells, not only the rounding of the renormalisation
        assert int((cap["n0"] > 0).sum()) > 1 and int(cap["changed"].sum()) > 0
    theirs = tr.lab8 if tr.online_mix is not None else tr.label
    assert torch.equal(mine["labels"], theirs), f"{int((mine['labels'] != theirs).sum())} labels differ from the trainer's"
    l = tr.losses()
    assert l["proto_seen"] == int((cap["n"] > 0).sum()) and l["proto_changed"] == int(cap["changed"].sum()) / float(cap["F"].shape[0])


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_rank_rccl_group_equals_the_single_gpu_trainer(dev):
    kw = dict(proto_denoise=TEMP, proto_momentum=MOM, **MODES["dacs"])
    one = _run("v3", dev, BF, 3, **kw)
    with one_rank_group(dev, PORT) as pg:
        dp = _run("v3", dev, BF, 3, pg=pg, **kw)
    O._assert_same(dp, one, "one-rank RCCL group")
    assert dp["per_step"] == one["per_step"] and torch.equal(_bits(dp["eta"]), _bits(one["eta"])) and torch.equal(dp["n"], one["n"])


@pytest.mark.parametrize("model", O.MODELS)
def test_resume_and_the_refusals(dev, tmp_path, model):
    kw = dict(proto_denoise=TEMP, proto_momentum=MOM, **MODES["plain"])
    data = O._views(dev, 6)

    def steps(tr, lo, hi, out):
        for mb in data[lo:hi]:
            _step(tr, mb, None, 1)
            out["scalars"].append(R.scalars(tr))
            out["labels"].append(tr.label.clone())
            out["read"].append(tr.losses())

    a = dict(scalars=[], labels=[], read=[])
    tr = O._trainer(model, dev, **kw)
    steps(tr, 0, 6, a)
    a["state"], eta_a, n_a = O._state(tr), tr.proto_eta.clone(), tr.proto_n.clone()
    del tr
    b = dict(scalars=[], labels=[], read=[])
    tr = O._trainer(model, dev, **kw)
    steps(tr, 0, 3, b)
    ts = tr.training_state()
    assert (ts["hyper"]["proto_denoise"], ts["hyper"]["proto_momentum"]) == (TEMP, MOM)
    assert {"proto_eta", "proto_n", "proto_changed_part"} <= set(ts["accumulators"])
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = O._trainer(model, dev, **kw)
    tr.load_training_state(ts)
    assert tr.it_done == 3 and {k: v for k, v in tr.losses().items() if k.startswith("proto")} == {k: v for k, v in b["read"][-1].items() if k.startswith("proto")}
    steps(tr, 3, 6, b)
    b["state"] = O._state(tr)
    assert b["read"] == a["read"]
    O._assert_same(a, b, f"{model} resumed after step 3")
    assert torch.equal(_bits(tr.proto_eta), _bits(eta_a)) and torch.equal(tr.proto_n, n_a)
    if model != "v2":
        return
    base = MODES["plain"]
    for other, named in [(base, r"proto_denoise \(state: 0\.5, this trainer: None\)"),
                         (dict(kw, proto_denoise=1.0), r"proto_denoise \(state: 0\.5, this trainer: 1\.0\)"),
                         (dict(kw, proto_momentum=0.99), r"proto_momentum \(state: 0\.9, this trainer: 0\.99\)")]:
        with pytest.raises(ValueError, match=named):
            O._trainer(model, dev, **other).load_training_state(ts)
    off = O._trainer(model, dev, **base)
    ots = off.training_state()
    assert not any(k.startswith("proto") for k in ots["hyper"]) and not any(k.startswith("proto") for k in ots["accumulators"])
    with pytest.raises(ValueError, match=r"proto_denoise \(state: None, this trainer: 0\.5\)"):
        tr.load_training_state(ots)


def test_keyword_refusals(dev):
    for kw, named in [(dict(proto_denoise=1.0), "proto_denoise needs online_labels"),
                      (dict(online_labels=0.5, proto_denoise=0.0), "proto_denoise 0.0"),
                      (dict(online_labels=0.5, proto_denoise=float("nan")), "proto_denoise nan"),
                      (dict(online_labels=0.5, proto_denoise=1.0, proto_momentum=1.0), "proto_momentum 1.0"),
                      (dict(online_labels=0.5, proto_momentum=0.9), "proto_momentum needs proto_denoise")]:
        for model in ("v2", "vgg"):
            with pytest.raises(ValueError, match=named):
                O._trainer(model, dev, **kw)
