"""The labelled source batch on the GPU (simt_source_mix / simt_source_mix_items in csrc/class_mix.hip, simt_head_loss_weighted_n /
simt_head_grad_weighted_n in csrc/head_loss.hip, the keyword online_source of the warm-up trainers, --online-source of trainV1_warmup).  The
yardsticks are the launches that existed before the keyword and the restatements of tests/_source_mix_ref.py and tests/_weighted_ref.py,
never the code under test:

  (a) the launch, bit for bit against the restatement and against simt_label_presence + simt_class_mix_items on the concatenated 2B-item batch;
      refusals;
  (b) the head launches with a table longer than the batch: nw = B against the existing weighted launches, entry B = 1 against the unweighted
      ones, entry B = 0.5 exactly half, a random map over 2B entries under the float64 bar of tests/_head_bar.py;
  (c) the trainers with online_source against a trainer WITHOUT any keyword and with iter_size doubled (its head's gscale set back to
      1 / iter_size) that is fed the source pair and then the pair the existing launches make from a separate teacher plan;
  (d) the tool on a generated source set and target set; without the flag its loss lines are the parent commit's, recorded in
      tests/golden/online_source_flag_off.json."""
import contextlib
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as cref
import _head_bar as hb
import _source_mix_ref as sref
import _weighted_ref as wr
import test_gpu_online_labels as OL
import test_gpu_online_mix as M
import test_gpu_online_weighted as WT
import test_gpu_resume as R
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from test_gpu_online_labels_cb import BalancedComposition
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
CD = so.load_class_dist()
NEW = ("simt_source_mix", "simt_source_mix_items", "simt_head_loss_weighted_n", "simt_head_grad_weighted_n")
FILL_X, FILL_LAB, FILL_ITEM = 0x5A5A5A5A, -3, 0xEE


# ---- (a) the launch ----------------------------------------------------------------------------------------------------------------------------------
def _desc(xs, labs, part_s, xt, lab8, x_out, lab_out, B, h, w, Cn, apply, rank):
    d = L.SourceMixDesc()
    d.xs, d.labs, d.part_s, d.xt, d.lab8 = xs.data_ptr(), labs.data_ptr(), part_s.data_ptr(), xt.data_ptr(), lab8.data_ptr()
    d.x_out, d.lab_out = x_out.data_ptr(), lab_out.data_ptr()
    d.B, d.h, d.w, d.n_classes = B, h, w, Cn
    table = np.full((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), 0xEE, dtype=np.uint8)          # garbage beyond B and beyond C
    table[:B, :Cn] = rank
    C.memmove(d.rank, table.ctypes.data, table.nbytes)
    for i in range(L.CLASS_MIX_MAX):
        d.apply[i] = (1 if apply[i] else 0) if i < B else 0xEE
    return d


def _presence(labs, Cn, dev):
    B = labs.shape[0]
    part = torch.full((B, L.CLASS_MIX_PARTS), -1, dtype=torch.int32, device=dev)
    L.call("simt_label_presence", ops._p(labs), B, labs[0].numel(), Cn, ops._p(part), ops.stream_ptr())
    return part


def _concatenated(xs, labs, xt, lab8, apply, rank, Cn, dev):
    """The EXISTING launches on the 2B-item batch [xt; xs], [widened lab8; labs] with partner[i] = B + i and the source items' apply = 0:
    simt_label_presence + simt_class_mix_items -> (x_out, lab_out, item map) of the first B items, device tensors."""
    B, _c, h, w = xs.shape
    x2 = torch.cat([xt, xs]).contiguous()
    lab2 = torch.cat([lab8.long(), labs]).contiguous()
    part = _presence(lab2, Cn, dev)
    x_out, lab_out = torch.empty_like(x2), torch.empty_like(lab2)
    item = torch.full((2 * B, h, w), FILL_ITEM, dtype=torch.uint8, device=dev)
    d = L.ClassMixDesc()
    d.x, d.lab, d.x_out, d.lab_out, d.part = x2.data_ptr(), lab2.data_ptr(), x_out.data_ptr(), lab_out.data_ptr(), part.data_ptr()
    d.B, d.h, d.w, d.n_classes = 2 * B, h, w, Cn
    table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
    table[:B, :Cn] = rank
    table[B:2 * B, :Cn] = rank
    C.memmove(d.rank, table.ctypes.data, table.nbytes)
    for i in range(2 * B):
        d.partner[i] = B + i if i < B else i
        d.apply[i] = 1 if (i < B and apply[i]) else 0
    L.call("simt_class_mix_items", C.byref(d), item.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    return x_out[:B], lab_out[:B], item[:B]


@pytest.mark.parametrize("geo", sref.GEOMETRIES, ids=lambda g: "B{}-{}x{}-C{}".format(*g[:4]))
def test_source_mix_equals_the_restatement_and_the_existing_launches(dev, geo):
    B, h, w, Cn, seed = geo
    for case in sref.CASES:
        xs_np, labs_np, xt_np, lab8_np, apply, rank = sref.inputs(B, h, w, Cn, seed, case)
        masks = sref.conditions(labs_np, apply, rank, Cn)
        xs, xt, labs = torch.from_numpy(xs_np).to(dev), torch.from_numpy(xt_np).to(dev), torch.from_numpy(labs_np).to(dev)
        lbuf, lab8, _off = M._aligned_u8(B * h * w, dev, 0)
        lab8.copy_(torch.from_numpy(lab8_np).reshape(-1))
        part_s = _presence(labs, Cn, dev)
        before = (xs.clone(), xt.clone(), labs.clone(), lbuf.clone(), part_s.clone())
        outs = []
        for items in (False, True):
            x_out = torch.full_like(xt, FILL_X)
            lab_out = torch.full((B, h, w), FILL_LAB, dtype=torch.int64, device=dev)
            ibuf = torch.full((B * h * w + 8,), FILL_ITEM, dtype=torch.uint8, device=dev)
            ioff = (-ibuf.data_ptr()) % 4 + 4
            d = _desc(xs, labs, part_s, xt, lab8, x_out, lab_out, B, h, w, Cn, apply, rank)
            if items:
                L.call("simt_source_mix_items", C.byref(d), ibuf.data_ptr() + ioff, ops.stream_ptr())
            else:
                L.call("simt_source_mix", C.byref(d), ops.stream_ptr())
            torch.cuda.synchronize()
            outs.append((x_out, lab_out, ibuf, ioff))
        for t, b in zip((xs, xt, labs, lbuf, part_s), before):
            assert torch.equal(t, b), f"{case}: an input was written"
        (x0, l0, i0, _o), (x1, l1, ibuf, ioff) = outs
        assert bool((i0 == FILL_ITEM).all()), "the plain launch wrote a map"
        assert torch.equal(x0, x1) and torch.equal(l0, l1), f"{case}: the _items flavour's x_out / lab_out differ from the plain one's"
        assert bool((ibuf[:ioff] == FILL_ITEM).all()) and bool((ibuf[ioff + B * h * w:] == FILL_ITEM).all()), "guard bytes of the map written"
        item = ibuf[ioff:ioff + B * h * w].view(B, h, w)
        want_x, want_lab, want_item = sref.mix(xs_np, labs_np, xt_np, lab8_np, apply, rank, Cn)
        assert want_x.dtype == np.int32 and want_lab.dtype == np.int64
        assert (l1.cpu().numpy() == want_lab).all(), f"{case}: {int((l1.cpu().numpy() != want_lab).sum())} labels differ from the restatement"
        assert (x1.cpu().numpy() == want_x).all(), f"{case}: {int((x1.cpu().numpy() != want_x).sum())} image words differ from the restatement"
        assert (item.cpu().numpy() == want_item).all(), f"{case}: {int((item.cpu().numpy() != want_item).sum())} bytes of the map differ"
        ex_x, ex_lab, ex_item = _concatenated(xs, labs, xt, lab8.view(B, h, w), apply, rank, Cn, dev)
        assert torch.equal(x1, ex_x) and torch.equal(l1, ex_lab) and torch.equal(item, ex_item), f"{case}: differs from the existing launches"
        if case == "none":
            assert not masks.any() and torch.equal(x1, xt) and bool((l1 == 255).all())
        else:
            assert masks.any() and bool((l1[torch.from_numpy(~masks).to(dev)] == 255).all())          # lab8 is all 255: only pasted pixels are labelled
            assert bool((l1[torch.from_numpy(masks).to(dev)] < Cn).all())
        if case == "one class":
            assert set(l1[0].unique().tolist()) == {Cn - 1, 255}


def test_source_mix_refusals_write_nothing(dev):
    B, h, w, Cn, seed = sref.GEOMETRIES[1]
    xs_np, labs_np, xt_np, lab8_np, apply, rank = sref.inputs(B, h, w, Cn, seed, "mixed")
    n = B * 3 * h * w
    x2 = torch.from_numpy(np.concatenate([xs_np.reshape(-1), xt_np.reshape(-1), xt_np.reshape(-1)])).to(dev)          # xs, xt, room behind
    xs, xt = x2[:n], x2[n:2 * n]
    lab2 = torch.from_numpy(np.concatenate([labs_np.reshape(-1), labs_np.reshape(-1)])).to(dev)
    labs = lab2[:B * h * w]
    _lbuf, lab8, _off = M._aligned_u8(B * h * w, dev, 255)
    part_s = _presence(labs.view(B, h, w), Cn, dev)
    x_out = torch.full((n + 4,), FILL_X, dtype=torch.int32, device=dev)
    lab_out = torch.full((B * h * w + 2,), FILL_LAB, dtype=torch.int64, device=dev)
    item = torch.full((B * h * w + 4,), FILL_ITEM, dtype=torch.uint8, device=dev)
    x_before, lab_before = x2.clone(), lab2.clone()

    def desc(**kw):
        d = _desc(xs, labs, part_s, xt, lab8, x_out, lab_out, B, h, w, Cn, apply, rank)
        for k, v in kw.items():
            if k != "rank00":
                setattr(d, k, v)
        if "rank00" in kw:
            d.rank[0][0] = kw["rank00"]
        return d
    nb = n * 4
    bad = [desc(xs=None), desc(labs=None), desc(part_s=None), desc(xt=None), desc(lab8=None), desc(x_out=None), desc(lab_out=None),
           desc(xs=xs.data_ptr() + 4), desc(labs=labs.data_ptr() + 8), desc(xt=xt.data_ptr() + 8), desc(lab8=lab8.data_ptr() + 4),
           desc(x_out=x_out.data_ptr() + 8), desc(lab_out=lab_out.data_ptr() + 8), desc(part_s=part_s.data_ptr() + 2),
           desc(B=0), desc(B=33), desc(n_classes=0), desc(n_classes=33), desc(h=0), desc(w=-1), desc(h=65536, w=32768), desc(rank00=19),
           desc(x_out=xs.data_ptr()), desc(x_out=xs.data_ptr() + 16), desc(x_out=xt.data_ptr()), desc(x_out=xt.data_ptr() + nb - 16),
           desc(lab_out=labs.data_ptr())]
    for name in ("simt_source_mix", "simt_source_mix_items"):
        extra = (item.data_ptr(),) if name.endswith("items") else ()
        for d in bad:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(d), *extra, ops.stream_ptr())
        with pytest.raises(L.SimtHipError):
            L.call(name, None, *extra, ops.stream_ptr())
    for bad_map in (None, item.data_ptr() + 1):
        with pytest.raises(L.SimtHipError):
            L.call("simt_source_mix_items", C.byref(desc()), bad_map, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((x_out == FILL_X).all()) and bool((lab_out == FILL_LAB).all()) and bool((item == FILL_ITEM).all())
    assert torch.equal(x2, x_before) and torch.equal(lab2, lab_before)
    L.call("simt_source_mix_items", C.byref(desc()), item.data_ptr(), ops.stream_ptr())          # the descriptor itself is sound
    L.call("simt_source_mix", C.byref(desc(x_out=xt.data_ptr() + nb)), ops.stream_ptr())         # adjacent is not overlapping
    torch.cuda.synchronize()
    assert bool((x_out[-4:] == FILL_X).all()) and bool((lab_out[-2:] == FILL_LAB).all()) and bool((item[-4:] == FILL_ITEM).all())
    assert bool((item[:-4] != FILL_ITEM).all()) and torch.equal(x2[2 * n:], x_out[:-4])


# ---- (b) the head launches with a table longer than the batch ---------------------------------------------------------------------------------------
HEADS = [("straddle", False, False), ("straddle", True, True), ("rows", False, False)]


def _relaunch(base, w, nw, item, dev):
    """The _n launches on the descriptor and buffers of a finished WT._head run -> that run's dict with the new outputs."""
    hd = base["desc"]
    _p1, _p2, _lab, _part, _keys, hout, _g1, dp, dt, conf = base["keep"]
    for t in dp:
        t.fill_(5.0)
    wd = torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev)
    it = None if item is None else item.to(dev).contiguous()
    ip = None if it is None else it.data_ptr()
    st = ops.stream_ptr()
    L.call("simt_head_loss_weighted_n", C.byref(hd), wd.data_ptr(), nw, ip, st)
    L.call("simt_head_grad_weighted_n", C.byref(hd), wd.data_ptr(), nw, ip, st)
    torch.cuda.synchronize()
    return dict(base, hout=hout[:16].cpu(), dp1=dp[0].cpu(), dp2=dp[1].cpu(), dt1=dt[0].cpu(), dt2=dt[1].cpu(), conf=conf.cpu())


def _same_bits(a, b, single, what):
    assert torch.equal(WT._bits(a["hout"]), WT._bits(b["hout"])), (what, a["hout"].tolist(), b["hout"].tolist())
    assert torch.equal(a["conf"], b["conf"])
    for (n, x), (_n, y) in zip(WT._grads(a, single), WT._grads(b, single)):
        assert torch.equal(WT._bits(x), WT._bits(y)), f"{what} {n}: {int((WT._bits(x) != WT._bits(y)).sum())} of {x.numel()} elements differ"


@pytest.mark.parametrize("c", HEADS, ids=WT._HID)
def test_head_n_exact_properties(dev, c):
    case, half, single = c
    B, _h, _w, H, W, _Q, _Cn = wr.CASES[case]
    p1, p2, lab, wt, item, base = WT._base(dev, c)
    # nw = B: the existing weighted launches, bit for bit -- general weights, the map with its block of bytes >= B (clamped to B - 1)
    old = WT._head(dev, case, half, single, p1, p2, lab, w=wt, w_item=item)
    _same_bits(_relaunch(old, wt, B, item, dev), old, single, "nw = B with the map")
    old = WT._head(dev, case, half, single, p1, p2, lab, w=wt)
    _same_bits(_relaunch(old, wt, B, None, dev), old, single, "nw = B without a map")
    assert not torch.equal(WT._bits(old["dp2"]), WT._bits(base["dp2"]))
    # a constant map B with w[B] = 1: the unweighted launches, bit for bit (the entries in front of it are not read)
    const = torch.full((B, H, W), B, dtype=torch.uint8)
    table = np.concatenate([wt, [1.0], np.full(B - 1, 0.25)]).astype(np.float32)
    scratch = WT._head(dev, case, half, single, p1, p2, lab)
    one = _relaunch(scratch, table, 2 * B, const, dev)
    _same_bits(one, base, single, "w[B] = 1")
    # w[B] = 0.5: exactly half
    table[B] = 0.5
    hf = _relaunch(scratch, table, 2 * B, const, dev)
    for i in ((1, 14) if single else (0, 1, 14)):
        assert float(hf["hout"][i]) == 0.5 * float(base["hout"][i]), (i, float(hf["hout"][i]), float(base["hout"][i]))
    assert float(hf["hout"][6]) == float(base["hout"][6]) and float(hf["hout"][15]) == float(base["hout"][15])
    for (n, a), (_n, b) in zip(WT._grads(hf, single), WT._grads(base, single)):
        assert bool((a.float() == 0.5 * b.float()).all()), f"w[B] = 0.5 {n}: {int((a.float() != 0.5 * b.float()).sum())} elements are not half"
    # the clamp bound is nw - 1: a byte beyond the table reads its last entry
    beyond = torch.full((B, H, W), 200, dtype=torch.uint8)
    table = np.concatenate([wt, np.full(B - 1, 0.25), [1.0]]).astype(np.float32)
    _same_bits(_relaunch(scratch, table, 2 * B, beyond, dev), base, single, "a byte beyond the table")


def _map_2b(B, H, W, seed):
    """A blocky random map over 2B entries that names every entry, with one block of bytes >= 2B (clamped to 2B - 1)."""
    g = torch.Generator().manual_seed(seed)
    by, bx = (H + 12) // 13, (W + 6) // 7
    blocks = torch.randint(0, 2 * B, (B, by, bx), generator=g)
    blocks[0, 0, 0] = 2 * B + 3
    item = blocks.repeat_interleave(13, 1).repeat_interleave(7, 2)[:, :H, :W].to(torch.uint8).contiguous()
    assert set(item.unique().tolist()) >= set(range(2 * B))
    return item


@pytest.mark.parametrize("c", HEADS, ids=WT._HID)
def test_head_n_vs_float64(dev, c, monkeypatch):
    """General weights over 2B entries and a random map against tests/_weighted_ref.py -- its `pixel_weights` told that the table has nw
    entries -- under tests/_head_bar.py as it stands: losses within 1e-4 * (1 + |ref|), gradients under the per-element bar."""
    case, half, single = c
    B, _h, _w, H, W, Q, Cn = wr.CASES[case]
    p1, p2, lab, wt, _item, _b = WT._base(dev, c)
    nw = 2 * B
    g = torch.Generator().manual_seed(77 + H)
    table = np.concatenate([wt, (torch.rand(B, generator=g) * 0.9 + 0.1).numpy()]).astype(np.float32)
    assert len(set(table.tolist())) == nw
    item = _map_2b(B, H, W, 5 + H)
    gather = wr.pixel_weights
    monkeypatch.setattr(wr, "pixel_weights", lambda w, w_item, _B, H_, W_, dtype: gather(w, w_item, nw, H_, W_, dtype))
    got = _relaunch(WT._head(dev, case, half, single, p1, p2, lab), table, nw, item, dev)
    r64, r32 = hb.ref_pair(("weighted_n refs", c), lambda dt: wr.weighted_ref(None if single else p1, p2, lab, table, item, 0.1, half, dt, Cn))
    for i, k in ((1, "l2"), (14, "total")) + (() if single else ((0, "l1"),)):
        want = float(r64[k])
        print(f"[weighted_n] {WT._HID(c)} hout[{i}] = {float(got['hout'][i])!r}, float64 {want!r}")
        assert abs(float(got["hout"][i]) - want) <= 1e-4 * (1 + abs(want)), (k, float(got["hout"][i]), want)
    assert int(got["hout"][6]) == r64["N"] and int(got["hout"][15]) == 2
    for hd_, f32, bf in (("dpred2", got["dp2"], got["dt2"]),) + (() if single else (("dpred1", got["dp1"], got["dt1"]),)):
        hb.trainer_form("n " + WT._HID(c), hd_, f32, bf, got["back"], Q, got["QP"], r64[hd_], r32[hd_], 1.0)
    # the entries behind B - 1 matter: the same map clamped to B - 1 gives another loss
    monkeypatch.setattr(wr, "pixel_weights", gather)
    low = wr.weighted_ref(None if single else p1, p2, lab, table[:B], item, 0.1, half, torch.float64, Cn)
    assert abs(float(low["total"]) - float(r64["total"])) > 1e-4 * (1 + abs(float(r64["total"]))), "the case shows nothing"


def test_head_n_refusals_write_nothing(dev):
    c = HEADS[0]
    B = wr.CASES[c[0]][0]
    _p1, _p2, _lab, wt, _item, base = WT._base(dev, c)
    hd, hout = base["desc"], base["keep"][5]
    keep = hout.clone()
    hout.fill_(-3.0)
    wd = torch.from_numpy(np.concatenate([wt, wt])).to(dev)
    st = ops.stream_ptr()
    try:
        for name in ("simt_head_loss_weighted_n", "simt_head_grad_weighted_n"):
            for nw in (B - 1, 0, -1, L.HEAD_WEIGHTS_MAX + 1):
                with pytest.raises(L.SimtHipError):
                    L.call(name, C.byref(hd), wd.data_ptr(), nw, None, st)
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(hd), None, 2 * B, None, st)
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(hd), wd.data_ptr() + 2, 2 * B, None, st)
            with pytest.raises(L.SimtHipError):
                L.call(name, None, wd.data_ptr(), 2 * B, None, st)
            hd.mode = 0
            try:
                with pytest.raises(L.SimtHipError):
                    L.call(name, C.byref(hd), wd.data_ptr(), 2 * B, None, st)
            finally:
                hd.mode = 1
        torch.cuda.synchronize()
        assert bool((hout == -3.0).all())
    finally:
        hout.copy_(keep)


# ---- (c) trainers ----------------------------------------------------------------------------------------------------------------------------------
SIZE, MODELS = OL.SIZE, OL.MODELS
PORT = 29597
MIX_P, MIX_SEED = 0.5, 11
PORTION, MOMENTUM = 0.5, 0.5


def _sources(dev, n, its=1):
    """n steps of `its` labelled source pairs: synthetic batches of seeds of their own, with a band of 255s."""
    B, H, W = SIZE
    out = []
    for i in range(n):
        mb = []
        for j in range(its):
            img, lab = so.synthetic_batch(B, H, W, CD.numpy(), seed=4000 + 10 * i + j, block=8)
            lab[:, H // 3] = 255
            mb.append((img.contiguous().to(dev), lab.contiguous().to(dev)))
        out.append(mb)
    return out


_RUNS = {}


def _run(model, dev, dtype, mode, mix=True, steps=3, its=1, dp=False, balanced=False, weighted=None, tau=None, first=None):
    """One memoised run.  mode "source": the trainer with online_labels and online_source (and online_mix when `mix`).  mode "composition":
    a trainer WITHOUT any keyword and with iter_size DOUBLED, its head's gscale set back to 1 / its, fed per micro-batch the source pair and
    then the pair the existing launches make from a separate teacher plan (the source mix: simt_label_presence + simt_class_mix_items on
    the concatenated batch) with the same draws.  first: a dict of a finished run to continue from its train state (resume).
    -> dict(tau, labels, inputs, scalars, state, shares, mixed, losses, nbt)."""
    key = (model, dtype, mode, mix, steps, its, dp, balanced, weighted, tau)
    if first is None and key in _RUNS:
        return _RUNS[key]
    data, src = OL._views(dev, steps, its), _sources(dev, steps, its)
    if tau is None:
        probe = OL.Composition(model, dev, dtype)
        tau = probe.threshold(data[0][0][1])
        del probe
    res = dict(tau=tau, labels=[], inputs=[], scalars=[], shares=[], mixed=[], kept=[])
    rng = cref.generator(MIX_SEED, 0)
    with (one_rank_group(dev, PORT) if dp else contextlib.nullcontext()) as pg:
        if mode == "source":
            kw = dict(online_labels=tau, online_source=True)
            if mix:
                kw.update(online_mix=MIX_P, online_mix_seed=MIX_SEED)
            if balanced:
                kw.update(online_labels_balanced=PORTION, online_labels_momentum=MOMENTUM)
            if weighted is not None:
                kw.update(online_labels_weighted=weighted)
            tr = OL._trainer(model, dev, dtype, pg, its, **kw)
            comp = None
        else:
            comp = BalancedComposition(model, dev, dtype, tau, PORTION, MOMENTUM) if balanced else OL.Composition(model, dev, dtype)
            tr = OL._trainer(model, dev, dtype, pg, 2 * its)
            tr.head_desc.gscale = 1.0 / its          # the two passes of a micro-batch are SUMMED (DACS), not averaged
            assert not hasattr(tr, "fixed") and not tr.online_source and not hasattr(tr, "source_hout")
        nbt0 = {k: int(v) for k, v in tr.state_dict().items() if k.endswith("num_batches_tracked")}
        start = 0
        if first is not None:
            tr.load_training_state(first["ts"])
            start = first["steps"]
        for mb, sb in list(zip(data, src))[start:]:
            if mode == "source":
                one = its == 1
                tr.step(mb[0][0] if one else [m[0] for m in mb], None, teacher_image=mb[0][1] if one else [m[1] for m in mb],
                        source_image=sb[0][0] if one else [s[0] for s in sb], source_label=sb[0][1] if one else [s[1] for s in sb])
            else:
                images, labels = [], []
                for (strong, weak), (sx, sl) in zip(mb, sb):
                    lab = (comp.label_balanced(weak) if balanced else comp.label(weak, tau)).clone()
                    res["shares"].append(float((lab != 255).float().mean()))
                    x = strong
                    if mix:
                        apply, rank = cref.draws(rng, SIZE[0], 19, MIX_P)
                        x, lab2, _item = _concatenated(sx, sl, strong.contiguous(), lab.to(torch.uint8), apply, rank, 19, dev)
                        res["mixed"].append(bool(apply.any()) and not torch.equal(lab2, lab))
                        lab = lab2
                    images += [sx, x]
                    labels += [sl, lab]
                tr.step(images, labels)
            torch.cuda.synchronize()
            res["labels"].append(tr.label.clone())                         # (iter_size > 1: the last micro-batch's target pass)
            res["inputs"].append(tr.plan.x_in.clone())
            res["scalars"].append(R.scalars(tr))
            if mode == "source":
                res["kept"].append(tr.source_hout.clone())
        # (label_thresholds / label_quality are lists: finite_losses takes scalars)
        res["losses"] = tr.losses() if (balanced or weighted is not None) else R.finite_losses(tr, f"{model} {mode}")
        res["state"] = OL._state(tr)
        res["nbt"] = {k: int(v) - nbt0[k] for k, v in tr.state_dict().items() if k.endswith("num_batches_tracked")}
        res["ts"], res["steps"] = (tr.training_state() if mode == "source" else None), steps
        del tr
    del comp
    torch.cuda.empty_cache()
    if first is None:
        _RUNS[key] = res
    return res


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "plain"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", MODELS)
def test_source_trainer_equals_the_composition(dev, model, dtype, mix):
    """3 steps, a weak view for the teacher: the student's input, the labels, the loss scalars and every tensor of the state."""
    comp = _run(model, dev, dtype, "composition", mix=mix)
    print(f"{model}: tau = {comp['tau']!r}, kept shares {comp['shares']}, mixed {comp['mixed']}")
    assert all(0.1 < s < 0.9 for s in comp["shares"]), comp["shares"]
    assert not mix or any(comp["mixed"]), "no step of the composition pasted anything: the draws never applied"
    got = _run(model, dev, dtype, "source", mix=mix)
    M._assert_same(got, comp, f"{model} online source")
    # `labelled` stays the share of the teacher's labels BEFORE the mix; the source pass's losses are kept
    assert abs(got["losses"]["labelled"] - sum(comp["shares"]) / 3) < 1e-6 and "source_seg2" not in comp["losses"]
    assert got["losses"]["source_seg2"] == float(got["kept"][-1][1]) and got["losses"]["source_seg2"] > 0
    assert got["losses"]["source_seg1"] == float(got["kept"][-1][0]) and (model != "v2" or got["losses"]["source_seg1"] > 0)
    # num_batches_tracked: two train-mode forwards per micro-batch, for the BatchNorms that run
    assert set(got["nbt"].values()) <= {0, 6} and got["nbt"] == comp["nbt"] and (model == "vgg" or 6 in got["nbt"].values())


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_source_trainer_iter_size_2(dev, model):
    comp = _run(model, dev, BF, "composition", its=2)
    assert any(comp["mixed"])
    got = _run(model, dev, BF, "source", its=2)
    M._assert_same(got, comp, f"{model} iter_size 2")
    assert set(got["nbt"].values()) <= {0, 12} and 12 in got["nbt"].values()


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_source_trainer_with_balanced_thresholds(dev, model):
    comp = _run(model, dev, BF, "composition", balanced=True)
    got = _run(model, dev, BF, "source", balanced=True)
    M._assert_same(got, comp, f"{model} class-balanced")
    assert len(got["losses"]["label_thresholds"]) == 19


def test_source_trainer_one_rank_rccl_group(dev):
    M._assert_same(_run("v2", dev, BF, "source", dp=True), _run("v2", dev, BF, "source"), "one-rank RCCL group")
    M._assert_same(_run("v3", dev, BF, "source", dp=True, mix=False), _run("v3", dev, BF, "source", mix=False), "one-rank RCCL group, no mix")


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "plain"])
@pytest.mark.parametrize("model", MODELS)
def test_quality_weights_at_threshold_zero_change_nothing(dev, model, mix):
    """online_labels = 0: q = 1 and the source entries are 1, so the weighted keyword trainer -- the _n head launches over the [2B] table and
    simt_source_mix_items with the mix -- equals the unweighted keyword trainer bit for bit."""
    plain = _run(model, dev, BF, "source", mix=mix, tau=0.0)
    got = _run(model, dev, BF, "source", mix=mix, tau=0.0, weighted="batch")
    M._assert_same(got, plain, f"{model} weighted at 0")
    assert got["losses"]["label_quality"] == [1.0] * SIZE[0] and got["losses"]["labelled"] == 1.0


def test_weighted_source_trainer_launches_the_n_form_and_the_item_map(dev, monkeypatch):
    data, src = OL._views(dev, 1), _sources(dev, 1)
    (strong, weak), (sx, sl) = data[0][0], src[0][0]
    tau = OL.Composition("v2", dev, BF).threshold(weak)
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    B = SIZE[0]
    for mode in ("batch", "item"):
        del calls[:]
        tr = OL._trainer("v2", dev, online_labels=tau, online_source=True, online_mix=1.0, online_labels_weighted=mode)
        tr.step(strong, None, teacher_image=weak, source_image=sx, source_label=sl)
        torch.cuda.synchronize()
        assert calls.count("simt_source_mix_items") == 1 and calls.count("simt_head_loss_weighted_n") == 1 == calls.count("simt_head_grad_weighted_n")
        assert calls.count("simt_head_loss") == 1 == calls.count("simt_head_grad") and "simt_class_mix_u8" not in calls          # the source pass
        assert calls.count("simt_label_presence") == 1 and "simt_source_mix" not in calls
        table = tr.label_w.cpu()
        assert table.shape == (2 * B,) and table[B:].tolist() == [1.0] * B and tr.label_q.data_ptr() == tr.label_w.data_ptr()
        assert all(0.0 < q < 1.0 for q in table[:B].tolist())
        own = torch.arange(B, device=dev, dtype=torch.uint8).view(B, 1, 1)
        pasted = tr.w_item != own
        assert bool(pasted.any()) and torch.equal(tr.w_item[pasted], (own + B).expand_as(tr.w_item)[pasted])
        assert torch.equal(tr.label[pasted], sl[pasted]) and torch.equal(tr.plan.x_in[:, 0][pasted], sx[:, 0][pasted])
        l = tr.losses()
        assert l["label_quality"] == table[:B].tolist() and l["source_seg2"] > 0
        del tr
    # without the mix the weighted head launches are the ones they were: no map, the [B] table
    del calls[:]
    tr = OL._trainer("v2", dev, online_labels=tau, online_source=True, online_labels_weighted="batch")
    tr.step(strong, None, teacher_image=weak, source_image=sx, source_label=sl)
    torch.cuda.synchronize()
    assert calls.count("simt_head_loss_weighted") == 1 and not set(calls) & set(NEW) and not hasattr(tr, "label_w")


def test_step_arguments_and_the_plain_trainers(dev, monkeypatch):
    data, src = OL._views(dev, 1), _sources(dev, 1)
    (strong, weak), (sx, sl) = data[0][0], src[0][0]
    tau = OL.Composition("v2", dev, BF).threshold(weak)
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    online = OL._trainer("v2", dev, online_labels=tau, online_mix=1.0)
    plain = OL._trainer("v2", dev)
    online.step(strong, None, teacher_image=weak)
    plain.step(strong, online.label.clone())
    torch.cuda.synchronize()
    assert not set(calls) & set(NEW), "a trainer without the keyword launched a new symbol"
    for tr in (online, plain):
        assert tr.online_source is False
        assert not any(hasattr(tr, a) for a in ("source_hout", "src_x", "src_lab", "_src_stage", "src_part", "source_mix_desc", "label_w"))
        with pytest.raises(ValueError, match="online_source"):
            tr.step(strong, None if tr is online else sl, source_image=sx, source_label=sl)
    assert "online_source" not in online.training_state()["hyper"] and "source_seg2" not in online.losses()
    with pytest.raises(ValueError, match="^online_source needs online_labels"):
        OL._trainer("v2", dev, online_source=True)
    with pytest.raises(ValueError, match="^online_source 1"):
        OL._trainer("v2", dev, online_labels=tau, online_source=1)
    tr = OL._trainer("v2", dev, online_labels=tau, online_source=True)
    with pytest.raises(ValueError, match="online_source"):
        tr.step(strong, None, teacher_image=weak)
    with pytest.raises(ValueError, match="pass label=None"):
        tr.step(strong, sl, source_image=sx, source_label=sl)
    # the bad-label counter covers the source labels
    bad = sl.clone()
    bad[0, 0, :3] = 19
    tr.step(strong, None, teacher_image=weak, source_image=sx, source_label=bad)
    with pytest.raises(ValueError, match=r"^3 label value\(s\) outside \[0, 19\)"):
        tr.losses()


def test_source_pair_that_the_launches_cannot_read_goes_through_the_staging_pair(dev):
    """The mix reads the caller's source tensors where they lie; a non-contiguous view, a misaligned base and a host tensor give what the
    contiguous device tensors give, through a staging pair allocated on first need."""
    data, src = OL._views(dev, 1), _sources(dev, 1)
    (strong, weak), (sx, sl) = data[0][0], src[0][0]
    tau = OL.Composition("v2", dev, BF).threshold(weak)
    kw = dict(online_labels=tau, online_source=True, online_mix=1.0, online_mix_seed=3)
    B, H, W = SIZE
    wide_x, wide_l = torch.zeros(B, 3, H, W + 3, device=dev), torch.zeros(B, H, W + 3, dtype=torch.int64, device=dev)
    wide_x[..., :W], wide_l[..., :W] = sx, sl
    flat_x, flat_l = torch.zeros(sx.numel() + 1, device=dev), torch.zeros(sl.numel() + 1, dtype=torch.int64, device=dev)
    flat_x[1:], flat_l[1:] = sx.reshape(-1), sl.reshape(-1)
    outs = []
    for x, l in ((sx, sl), (wide_x[..., :W], wide_l[..., :W]), (flat_x[1:].view(B, 3, H, W), flat_l[1:].view(B, H, W)), (sx.cpu(), sl.cpu()),
                 (sx, sl.int())):
        tr = OL._trainer("v2", dev, **kw)
        assert tr._src_stage == [None, None]
        tr.step(strong, None, teacher_image=weak, source_image=x, source_label=l)
        torch.cuda.synchronize()
        outs.append((tr.plan.x_in.clone(), tr.label.clone(), R.scalars(tr), tr.source_hout.clone(), [t is not None for t in tr._src_stage]))
        if x is sx and l is sl:
            assert tr.src_x.data_ptr() == sx.data_ptr() and tr.src_lab.data_ptr() == sl.data_ptr()          # read where the caller left them
        del tr
    assert [o[4] for o in outs] == [[False, False], [True, True], [True, True], [True, True], [False, True]]
    for o in outs[1:]:
        assert torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(o[1], outs[0][1])
        assert torch.equal(o[2], outs[0][2]) and torch.equal(o[3], outs[0][3])
    assert not torch.equal(outs[0][0], strong), "online_mix = 1 pasted nothing"


def test_resume(dev, tmp_path):
    """3 steps + save + a new trainer + load + 3 steps == 6 steps, draws and the kept source losses included; the refusals of the train state."""
    whole = _run("v2", dev, BF, "source", steps=6)
    half = _run("v2", dev, BF, "source", steps=3)
    assert half["ts"]["hyper"]["online_source"] is True and "source_hout" in half["ts"]["accumulators"]
    path = str(tmp_path / "run.state")
    tsf.save(path, half["ts"], None, {"world": 1})
    ts, _k, _l = tsf.load(path)
    rest = _run("v2", dev, BF, "source", steps=6, tau=half["tau"], first=dict(ts=ts, steps=3))
    assert whole["tau"] == half["tau"]
    for k in ("labels", "inputs", "scalars", "kept"):
        rest[k] = half[k] + rest[k]
    M._assert_same(rest, whole, "resumed after step 3")
    assert all(torch.equal(a, b) for a, b in zip(rest["kept"], whole["kept"]))
    tr = OL._trainer("v2", dev, online_labels=half["tau"], online_mix=MIX_P, online_mix_seed=MIX_SEED)
    with pytest.raises(ValueError, match=r"online_source \(state: True, this trainer: None\)"):
        tr.load_training_state(ts)
    other = OL._trainer("v2", dev, online_labels=half["tau"], online_mix=MIX_P, online_mix_seed=MIX_SEED, online_source=True)
    with pytest.raises(ValueError, match=r"online_source \(state: None, this trainer: True\)"):
        other.load_training_state(tr.training_state())
    other.load_training_state(ts)
    assert other.it_done == 3 and other.source_hout.tolist() == half["kept"][-1].tolist()


# ---- (d) the tool ----------------------------------------------------------------------------------------------------------------------------------
def _data_sets(root):
    """A four-image GTA5-shaped source set (images/, labels/ with GTA5 ids, an unmapped id and 255 among them) and a four-image target set
    listed by image alone; frames of 160 x 96, so the loaders resize."""
    from PIL import Image
    g = np.random.default_rng(3)
    ids = np.array([7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 26, 1, 255], dtype=np.uint8)
    for sub in ("source/images", "source/labels", "target/leftImg8bit"):
        os.makedirs(root / sub)
    names = [f"{n:05d}.png" for n in range(4)]
    for n, name in enumerate(names):
        blocks = ids[g.integers(0, len(ids), (6, 8))]
        Image.fromarray(np.kron(blocks, np.ones((16, 20), dtype=np.uint8))).save(root / "source/labels" / name)
        colour = (blocks[..., None].astype(np.int64) * np.array([37, 91, 53]) % 256).astype(np.uint8)
        noise = g.integers(0, 40, (96, 160, 3), dtype=np.uint8)
        Image.fromarray(np.kron(colour, np.ones((16, 20, 1), dtype=np.uint8)) // 2 + noise).save(root / "source/images" / name)
        Image.fromarray(g.integers(0, 256, (6, 8, 3), dtype=np.uint8).repeat(16, 0).repeat(20, 1) // 2 + noise).save(root / "target/leftImg8bit" / name)
    open(root / "source.txt", "w").write("".join(n + "\n" for n in names))
    open(root / "target.txt", "w").write("".join("leftImg8bit/" + n + "\n" for n in names))
    return ["--data-dir", str(root / "source"), "--data-list", str(root / "source.txt"), "--data-dir-target", str(root / "target"),
            "--data-list-target", str(root / "target.txt")]


TOOL_MODELS = ["DeepLab", "DeepLabv3"]
TOOL_FLAGS = ["--online-source", "--online-mix", "--online-labels-weighted"]
FLAG_OFF_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "online_source_flag_off.json")


def _tool_common(tool_model, sets):
    return ["--learning-rate", "2.5e-4", "--model", tool_model, "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
            "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--num-workers", "2", "--random-mirror",
            "--online-labels", "0"] + sets


def _flag_off_run(tool, tool_model, root, sets):
    """THE flag-off command: the tool test's command without --online-source (the in-batch mix with the quality weights), four steps, with a
    --data-dir that does not exist.  -> (its output, its train-state file).  The parent commit's loss lines for exactly this call are
    tests/golden/online_source_flag_off.json (recorded by importing this function beside the parent's package on an MI355X)."""
    off = [a if a != str(root / "source") else str(root / "nowhere") for a in _tool_common(tool_model, sets)]
    state = str(root / "off.state")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tool.main(off + TOOL_FLAGS[1:] + ["--snapshot-dir", str(root / "o"), "--num-steps-stop", "4", "--train-state", state])
    return buf.getvalue(), state


@pytest.mark.parametrize("tool_model", TOOL_MODELS)
def test_tool_trains_on_a_source_set_and_resumes(dev, tmp_path, capsys, monkeypatch, tool_model):
    """trainV1_warmup --online-labels 0 --online-source --online-mix --online-labels-weighted on generated files, B = 2, 129,65: six steps with
    ` src = ` in every loss line and no nan; 3 + 3 == 6 through --train-state in the loss lines and in every tensor of the final snapshot;
    without the flag the loss lines equal the parent commit's for the same command (tests/golden/online_source_flag_off.json), none of the
    new symbols is launched and no source file is opened; a resume with the flag added or dropped is refused."""
    from simt_amd.tools import trainV1_warmup as tool
    sets = _data_sets(tmp_path)
    common = _tool_common(tool_model, sets)
    flags = TOOL_FLAGS
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
    lines = R._loss_lines(out_a)
    assert len(lines) == 6 and not re.search(r"= nan", out_a), out_a
    assert all(re.search(r" q = 1\.000\.\.1\.000 src = \d+\.\d{3}  lr = ", ln) for ln in lines), lines
    assert len({re.search(r" src = (\S+)", ln).group(1) for ln in lines}) > 1, "the source loss never moved"
    assert calls.count("simt_source_mix_items") == 6 and calls.count("simt_head_loss_weighted_n") == 6 and calls.count("simt_label_presence") == 6
    assert "simt_class_mix_u8" not in calls and "simt_class_mix_u8_items" not in calls
    assert out_a.count("online source: one optimiser step = (1) supervised cross-entropy on a labelled source batch of ") == 1
    out_b1, _ = run("b", 3, *flags, "--train-state", state)
    assert R._loss_lines(out_b1) == lines[:3]
    out_b2, snap_b = run("b", 6, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 3\b", out_b2), out_b2
    assert R._loss_lines(out_b2) == lines[3:], (out_a, out_b2)
    R._same_snapshot(snap_a, snap_b)
    with pytest.raises(SystemExit, match="online_source"):          # dropped
        tool.main(common + flags[1:] + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "8", "--train-state", state])
    capsys.readouterr()
    # the flag-off run: the parent commit's loss lines, the launches it made before the flag existed, and --data-dir / --data-list are not read
    del calls[:]
    out_o, state_off = _flag_off_run(tool, tool_model, tmp_path, sets)
    parent = json.load(open(FLAG_OFF_GOLDEN))[tool_model]
    assert len(parent) == 4 and R._loss_lines(out_o) == parent, (R._loss_lines(out_o), parent)
    assert not set(calls) & set(NEW) and calls.count("simt_class_mix_u8") == 4 and "online source" not in out_o and " src = " not in out_o
    with pytest.raises(SystemExit, match="online_source"):          # added
        tool.main(common + flags + ["--snapshot-dir", str(tmp_path / "o"), "--num-steps-stop", "6", "--train-state", state_off])
    capsys.readouterr()
