"""Quality-weighted online labels on the GPU, launch by launch (csrc/label_sweep.hip, csrc/head_loss.hip, csrc/class_mix.hip).

  labels   simt_online_label_w / _w_u8 against the launches they replace: labels (and presence words) == those at threshold -inf, counts ==
           those at T, row sums of conf_part == the per-item non-255 counts at T; guard bands, garbage prefill, refusals;
  quality  simt_label_quality against online_labels.label_quality, bit for bit;
  mix      simt_class_mix_u8_items: x_out / lab_out == simt_class_mix_u8, the map == simt_class_mix_items on the widened bytes;
  head     simt_head_loss_weighted / simt_head_grad_weighted: (a) w = 1 == the unweighted launches, (b) w = 0.5 exactly half, (c) per-item
           powers of two scale the item's gradient rows exactly, (d) a constant map == the gathered table, (e) general weights and a random
           map against the float64 restatement of tests/_weighted_ref.py under the bars of tests/_head_bar.py.

(a)-(d) compare executions of the same arithmetic, or scalings by powers of two, and are BITWISE.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _class_mix_ref as ref
import _head_bar as hb
import _weighted_ref as wr
import test_gpu_online_mix as M
from _launch_oracle import SENTINEL
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import online_labels as ol
from simt_amd import ops
from test_gpu_online_labels import GARBAGE, GEOMETRIES, GUARD, THRESHOLDS, _desc, _input

pytestmark = pytest.mark.gpu
CD = so.load_class_dist()
BF = torch.bfloat16
_ID = lambda g: "fam{}-{}x{}x{}to{}x{}-C{}-ld{}".format(*g)          # noqa: E731
WORD = 0xDEADBEEF - (1 << 32)                                        # garbage for int32 words (negative: no count equals it)


# ---- the label launches ------------------------------------------------------------------------------------------------------------------------------
def _w_desc(view, label, counts, conf_part, geo, thr):
    family, B, h, w, H, W, Cn, ld = geo
    d = L.OnlineLabelWDesc()
    d.fix, d.label, d.counts, d.conf_part = view.data_ptr(), label.data_ptr(), counts.data_ptr(), conf_part.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, ld, H, W, Cn, family, thr
    return d


def _w_u8_desc(view, lab8, counts, part, conf_part, geo, thr):
    family, B, h, w, H, W, Cn, ld = geo
    d = L.OnlineLabelWU8Desc()
    d.fix, d.lab8, d.counts, d.part, d.conf_part = view.data_ptr(), lab8.data_ptr(), counts.data_ptr(), part.data_ptr(), conf_part.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, ld, H, W, Cn, family, thr
    return d


def _parent(view, geo, thr, dev):
    """simt_online_label at `thr` -> (labels [B][H][W] int64, counts)."""
    family, B, h, w, H, W, Cn, ld = geo
    lab = torch.full((B, H, W), GARBAGE, dtype=torch.int64, device=dev)
    cnt = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
    L.call("simt_online_label", C.byref(_desc(view, lab, cnt, family, B, h, w, ld, H, W, Cn, thr)), ops.stream_ptr())
    torch.cuda.synchronize()
    return lab, cnt


def _parts_buffer(B, rows, dev):
    """[guard | B * rows | guard] words of garbage -> (buffer, view)."""
    buf = torch.full((2 * GUARD + B * rows,), WORD, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + B * rows]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=_ID)
def test_label_w_equals_the_launches_it_replaces(dev, geo):
    family, B, h, w, H, W, Cn, ld = geo
    buf, view = _input(family, B, h, w, Cn, ld, dev, seed=sum(geo))
    before = buf.clone()
    P, rows = B * H * W, M._rows(family, B, H, W)
    all_lab, _all_cnt = _parent(view, geo, float("-inf"), dev)
    shares = []
    for thr in THRESHOLDS:
        want_lab, want_cnt = _parent(view, geo, thr, dev)
        lab = torch.full((2 * GUARD + P,), GARBAGE, dtype=torch.int64, device=dev)
        counts = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
        cbuf, conf_part = _parts_buffer(B, rows, dev)
        d = _w_desc(view, lab[GUARD:], counts, conf_part, geo, thr)
        L.call("simt_online_label_w", C.byref(d), ops.stream_ptr())
        torch.cuda.synchronize()
        got = lab[GUARD:GUARD + P].view(B, H, W)
        assert torch.equal(got, all_lab), f"threshold {thr}: {int((got != all_lab).sum())} labels differ from simt_online_label(-inf)"
        assert torch.equal(counts, want_cnt) and int(counts.sum()) == P, (thr, counts.tolist(), want_cnt.tolist())
        kept = (want_lab != 255).reshape(B, -1).sum(1)
        sums = conf_part.view(B, rows).long().sum(1)
        assert torch.equal(sums, kept), (thr, sums.tolist(), kept.tolist())
        assert bool((conf_part != WORD).all()), "a word of conf_part kept its garbage"          # (no count can equal the negative pattern)
        assert bool((lab[:GUARD] == GARBAGE).all()) and bool((lab[GUARD + P:] == GARBAGE).all()), "label guard words written"
        assert bool((cbuf[:GUARD] == WORD).all()) and bool((cbuf[GUARD + B * rows:] == WORD).all()), "conf_part guard words written"
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the input was written"
        if thr == 0.5:
            shares = (kept.double() / (H * W)).tolist()
            L.call("simt_online_label_w", C.byref(d), ops.stream_ptr())          # counts accumulate, conf_part is overwritten
            torch.cuda.synchronize()
            assert torch.equal(counts, 2 * want_cnt) and torch.equal(conf_part.view(B, rows).long().sum(1), kept)
        if thr != thr:
            assert int(sums.sum()) == 0 and int(counts[Cn]) == P, "a NaN threshold counts nothing as confident"
    if h > 2:
        assert any(0.1 < s < 0.9 for s in shares), f"T = 0.5 keeps {shares}: the input keeps everything or nothing"


@pytest.mark.parametrize("geo", GEOMETRIES, ids=_ID)
def test_label_w_u8_equals_the_launches_it_replaces(dev, geo):
    family, B, h, w, H, W, Cn, ld = geo
    buf, view = _input(family, B, h, w, Cn, ld, dev, seed=sum(geo))
    P, rows = B * H * W, M._rows(family, B, H, W)

    def parent(thr):
        _b, lab8, _o = M._aligned_u8(P, dev, 0x77)
        cnt = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
        part = torch.full((B, rows), WORD, dtype=torch.int32, device=dev)
        L.call("simt_online_label_u8", C.byref(M._u8_desc(view, lab8, cnt, part, family, B, h, w, ld, H, W, Cn, thr)), ops.stream_ptr())
        torch.cuda.synchronize()
        return lab8.clone(), cnt, part
    all_lab, _c, all_part = parent(float("-inf"))
    shares = []
    for thr in THRESHOLDS:
        want_lab, want_cnt, _p = parent(thr)
        lbuf, lab8, off = M._aligned_u8(P, dev, 0x77)
        counts = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
        pbuf, part = _parts_buffer(B, rows, dev)
        cbuf, conf_part = _parts_buffer(B, rows, dev)
        L.call("simt_online_label_w_u8", C.byref(_w_u8_desc(view, lab8, counts, part, conf_part, geo, thr)), ops.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(lab8, all_lab), f"threshold {thr}: bytes differ from simt_online_label_u8(-inf)"
        assert torch.equal(part.view(B, rows), all_part), f"threshold {thr}: presence words differ from simt_online_label_u8(-inf)"
        assert torch.equal(counts, want_cnt) and int(counts.sum()) == P
        kept = (want_lab != 255).view(B, -1).sum(1)
        assert torch.equal(conf_part.view(B, rows).long().sum(1), kept)
        assert bool((lbuf[:off] == 0x77).all()) and bool((lbuf[off + P:] == 0x77).all()), "byte guard written"
        for g, n in ((pbuf, "part"), (cbuf, "conf_part")):
            assert bool((g[:GUARD] == WORD).all()) and bool((g[GUARD + B * rows:] == WORD).all()), f"{n} guard words written"
        if thr == 0.5:
            shares = (kept.double() / (H * W)).tolist()
    if h > 2:
        assert any(0.1 < s < 0.9 for s in shares), shares


def test_label_w_refusals_write_nothing(dev):
    geo = GEOMETRIES[0]
    family, B, h, w, H, W, Cn, ld = geo
    _buf, view = _input(family, B, h, w, Cn, ld, dev, seed=1)
    P, rows = B * H * W, M._rows(family, B, H, W)
    lab = torch.full((P + 1,), GARBAGE, dtype=torch.int64, device=dev)
    _lb, lab8, _o = M._aligned_u8(P, dev, 0x77)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    part = torch.full((40, rows), WORD, dtype=torch.int32, device=dev)
    conf_part = torch.full((40, rows), WORD, dtype=torch.int32, device=dev)

    def make(u8, **kw):
        g = dict(family=family, B=B, h=h, w=w, H=H, W=W, C=Cn, ld=ld)
        g.update({k: v for k, v in kw.items() if k in g})
        geo_ = (g["family"], g["B"], g["h"], g["w"], g["H"], g["W"], g["C"], g["ld"])
        d = _w_u8_desc(view, lab8, counts, part, conf_part, geo_, 0.5) if u8 else _w_desc(view, lab, counts, conf_part, geo_, 0.5)
        for k in ("fix", "label", "lab8", "counts", "part", "conf_part"):
            if k in kw:
                setattr(d, k, kw[k])
        return d
    common = [dict(fix=None), dict(counts=None), dict(conf_part=None), dict(conf_part=conf_part.data_ptr() + 2), dict(C=25), dict(family=2),
              dict(family=-1), dict(B=0), dict(B=33), dict(H=0), dict(w=0), dict(C=0), dict(H=65536, W=32768),
              dict(family=1, B=1, h=32768, w=32768, ld=4, C=3)]
    for kw in common + [dict(label=None), dict(label=lab.data_ptr() + 4), dict(C=256, ld=256)]:
        with pytest.raises(L.SimtHipError):
            L.call("simt_online_label_w", C.byref(make(False, **kw)), ops.stream_ptr())
    for kw in common + [dict(lab8=None), dict(lab8=lab8.data_ptr() + 4), dict(part=None), dict(part=part.data_ptr() + 2), dict(C=33, ld=36)]:
        with pytest.raises(L.SimtHipError):
            L.call("simt_online_label_w_u8", C.byref(make(True, **kw)), ops.stream_ptr())
    for name in ("simt_online_label_w", "simt_online_label_w_u8", "simt_label_quality"):
        with pytest.raises(L.SimtHipError):
            L.call(name, None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((lab == GARBAGE).all()) and bool((lab8 == 0x77).all()) and int(counts.sum()) == 0
    assert bool((part == WORD).all()) and bool((conf_part == WORD).all())
    L.call("simt_online_label_w", C.byref(make(False)), ops.stream_ptr())          # the descriptors themselves are sound
    L.call("simt_online_label_w_u8", C.byref(make(True)), ops.stream_ptr())
    torch.cuda.synchronize()
    assert int(counts.sum()) == 2 * P and bool((lab[:P] != GARBAGE).all()) and int(lab[P]) == GARBAGE


# ---- simt_label_quality ------------------------------------------------------------------------------------------------------------------------------
def _quality(conf_part, H, W, mode, dev, q=None):
    B, rows = conf_part.shape
    cp = torch.from_numpy(conf_part.view(np.int32)).to(dev)
    q = torch.full((B + 2,), -7.0, device=dev) if q is None else q
    d = L.LabelQualityDesc()
    d.conf_part, d.q, d.B, d.rows, d.H, d.W, d.mode = cp.data_ptr(), q.data_ptr() + 4, B, rows, H, W, L.LABEL_QUALITY_MODES[mode]
    L.call("simt_label_quality", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert float(q[0]) == -7.0 and float(q[B + 1]) == -7.0, "guard floats written"
    return q[1:B + 1].cpu().numpy()


@pytest.mark.parametrize("mode", ["item", "batch"])
@pytest.mark.parametrize("B,rows,H,W", [(1, 1, 7, 5), (3, 17, 65, 129), (4, 512, 768, 768), (32, 1024, 5000, 5000), (2, 65, 4096, 8192)])
def test_label_quality_equals_the_restatement_bit_for_bit(dev, mode, B, rows, H, W):
    rng = np.random.default_rng(B * rows + H)
    N = H * W
    n = rng.integers(0, N + 1, B)
    n[0] = N                                              # every pixel confident
    if B > 1:
        n[1] = 0                                          # a row of zeros
    if B > 2 and N > (1 << 24) + 1:
        n[2] = (1 << 24) + 1                              # a count no float32 holds
    conf_part = np.zeros((B, rows), dtype=np.uint32)
    for b in range(B):                                    # spread n[b] over the row at random (words up to 2^32 - 1)
        cuts = np.sort(rng.integers(0, int(n[b]) + 1, rows - 1)) if rows > 1 else np.array([], dtype=np.int64)
        conf_part[b] = np.diff(np.concatenate([[0], cuts, [int(n[b])]])).astype(np.uint32)
    assert (conf_part.astype(np.int64).sum(1) == n).all()
    got = _quality(conf_part, H, W, mode, dev)
    want = ol.label_quality(n, N, mode)
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (got.tolist(), want.tolist())
    assert got[0] == 1.0 or mode == "batch"
    if mode == "item" and B > 1:
        assert got[1] == 0.0


def test_label_quality_refusals_write_nothing(dev):
    cp = torch.zeros(2, 3, dtype=torch.int32, device=dev)
    q = torch.full((2,), -7.0, device=dev)

    def desc(**kw):
        a = dict(conf_part=cp.data_ptr(), q=q.data_ptr(), B=2, rows=3, H=4, W=4, mode=0)
        a.update(kw)
        d = L.LabelQualityDesc()
        for k, v in a.items():
            setattr(d, k, v)
        return d
    for kw in (dict(conf_part=None), dict(q=None), dict(q=q.data_ptr() + 2), dict(B=0), dict(B=33), dict(rows=0), dict(rows=1025), dict(H=0),
               dict(H=65536, W=32768), dict(mode=2), dict(mode=-1)):
        with pytest.raises(L.SimtHipError):
            L.call("simt_label_quality", C.byref(desc(**kw)), ops.stream_ptr())
    torch.cuda.synchronize()
    assert q.tolist() == [-7.0, -7.0]


# ---- simt_class_mix_u8_items -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 8, 12, 19, 70, "mixed"), (3, 7, 9, 19, 64, "mixed"), (2, 7, 9, 19, 5, "all"), (2, 8, 12, 19, 3, "none"),
                                  (32, 5, 5, 32, 65, "mixed"), (4, 67, 65, 7, 9, "mixed")], ids=lambda c: "B{}-{}x{}-C{}-rows{}-{}".format(*c))
def test_class_mix_u8_items_equals_both_parents(dev, case):
    """x_out / lab_out == simt_class_mix_u8; the map == simt_class_mix_items on the widened bytes with the same draws.  h * w % 4 != 0 takes
    the scalar flavour and its tail; "mixed" holds an item with apply = 0."""
    B, h, w, Cn, rows, how = case
    x_np, lab_np = M._mix_batch(B, h, w, Cn, seed=sum(case[:5]), blank=1 if B > 2 else None)
    apply, rank = ref.draws(ref.generator(5, 0), B, Cn, 0.5)
    apply = {"none": np.zeros(B, bool), "all": np.ones(B, bool), "mixed": apply}[how]
    if how == "mixed":
        apply[0], apply[1], apply[-1] = True, False, True
    x = torch.from_numpy(x_np).to(dev)
    _lbuf, lab8, _off = M._aligned_u8(B * h * w, dev, 0)
    lab8.copy_(torch.from_numpy(lab_np).reshape(-1))
    part = torch.from_numpy(M._spread_part(lab_np, Cn, rows).view(np.int32)).to(dev)
    outs = []
    for items in (False, True):
        x_out = torch.full_like(x, 0x5A5A5A5A)
        lab_out = torch.full((B, h, w), -3, dtype=torch.int64, device=dev)
        ibuf = torch.full((B * h * w + 8,), 0xEE, dtype=torch.uint8, device=dev)
        ioff = (-ibuf.data_ptr()) % 4 + 4
        d = M._u8_mix_desc(x, lab8, x_out, lab_out, part, B, h, w, Cn, rows, apply, rank)
        if items:
            L.call("simt_class_mix_u8_items", C.byref(d), ibuf.data_ptr() + ioff, ops.stream_ptr())
        else:
            L.call("simt_class_mix_u8", C.byref(d), ops.stream_ptr())
        torch.cuda.synchronize()
        outs.append((x_out, lab_out, ibuf, ioff))
    (x0, l0, _i0, _o0), (x1, l1, ibuf, ioff) = outs
    assert torch.equal(x0, x1) and torch.equal(l0, l1), "x_out / lab_out differ from simt_class_mix_u8"
    assert bool((ibuf[:ioff] == 0xEE).all()) and bool((ibuf[ioff + B * h * w:] == 0xEE).all()), "guard bytes of the map written"
    got = ibuf[ioff:ioff + B * h * w].view(B, h, w)
    # simt_class_mix_items on the widened bytes
    lab64 = torch.from_numpy(lab_np.astype(np.int64)).to(dev)
    _words, part64 = M._presence_launch(lab64, Cn, dev)
    xo, lo = torch.empty_like(x), torch.empty_like(lab64)
    want = torch.full((B, h, w), 0xEE, dtype=torch.uint8, device=dev)
    e = L.ClassMixDesc()
    e.x, e.lab, e.x_out, e.lab_out, e.part = x.data_ptr(), lab64.data_ptr(), xo.data_ptr(), lo.data_ptr(), part64.data_ptr()
    e.B, e.h, e.w, e.n_classes = B, h, w, Cn
    table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
    table[:B, :Cn] = rank
    C.memmove(e.rank, table.ctypes.data, table.nbytes)
    for i in range(B):
        e.partner[i], e.apply[i] = (i + 1) % B, 1 if apply[i] else 0
    L.call("simt_class_mix_items", C.byref(e), want.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes of the map differ from simt_class_mix_items"
    assert torch.equal(xo, x1) and torch.equal(lo, l1)
    masks = ref.paste_masks(lab_np.astype(np.int64), apply, rank, Cn)
    own = torch.arange(B, device=dev, dtype=torch.uint8).view(B, 1, 1).expand(B, h, w)
    assert torch.equal(got != own, torch.from_numpy(masks).to(dev)), "the map is not the paste mask"
    for i in range(B):
        if not apply[i]:
            assert bool((got[i] == i).all())
    d = M._u8_mix_desc(x, lab8, x1, l1, part, B, h, w, Cn, rows, apply, rank)
    for bad in (None, ibuf.data_ptr() + ioff + 1):
        with pytest.raises(L.SimtHipError):
            L.call("simt_class_mix_u8_items", C.byref(d), bad, ops.stream_ptr())


# ---- the weighted head -------------------------------------------------------------------------------------------------------------------------------
def _head(dev, case, half, single, pred1, pred2, lab, *, w=None, w_item=None, gscale=1.0, lambda_seg=0.1):
    """One pass-1 + pass-2 pair at CASES[case]: fp32 AND bf16 gradient outputs from the same launch, conf_out.  w None: the unweighted
    launches.  -> dict(hout[:16], dp1, dp2 (fp32 raw), dt1, dt2 (bf16 raw), conf, back)."""
    B, h, w_, H, W, Q, Cn = wr.CASES[case]
    lib = L.load()
    ldp = ops.round_up(Q, 4) + 4
    QP = ops.round_up(Q, 8)
    ld_t = QP + 8

    def low(p):
        t = torch.zeros(B * h * w_, ldp, device=dev)
        t[:, :Q] = p.to(dev).permute(0, 2, 3, 1).reshape(-1, Q)
        return t
    p2 = low(pred2)
    p1 = None if single else low(pred1)
    labd = lab.to(dev)
    part = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Cn), device=dev)
    keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
    hout = torch.zeros(lib.simt_head_hout_floats(Q, Cn), device=dev)
    g1 = torch.zeros(2, B, H, w_, QP, device=dev)
    dp = [torch.full((B * h * w_, ldp), 5.0, device=dev) for _ in range(2)]
    dt = [torch.full((B * h * w_, ld_t), SENTINEL, dtype=BF, device=dev) for _ in range(2)]
    conf = torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
    hd = L.HeadDesc()
    hd.pred1, hd.pred2, hd.fixp, hd.label, hd.T1, hd.T2 = (None if single else p1.data_ptr()), p2.data_ptr(), None, labd.data_ptr(), None, None
    hd.part, hd.keys, hd.hout, hd.g1 = part.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
    hd.dpred1_f32, hd.dpred2_f32 = (None if single else dp[0].data_ptr()), dp[1].data_ptr()
    hd.dpred1_t, hd.dpred2_t = (None if single else dt[0].data_ptr()), dt[1].data_ptr()
    hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w_, H, W, Cn, Q
    hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = ldp, ldp, QP, ldp, ld_t, L.SIMT_BF16
    hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, lambda_seg, 0.0, gscale
    hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1, int(single), int(half), 0
    hd.conf_out = conf.data_ptr()
    st = ops.stream_ptr()
    if w is None:
        L.call("simt_head_loss", C.byref(hd), st)
        L.call("simt_head_grad", C.byref(hd), st)
    else:
        wd = torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev)
        item = None if w_item is None else w_item.to(dev).contiguous()
        ip = None if item is None else item.data_ptr()
        L.call("simt_head_loss_weighted", C.byref(hd), wd.data_ptr(), ip, st)
        L.call("simt_head_grad_weighted", C.byref(hd), wd.data_ptr(), ip, st)
    torch.cuda.synchronize()
    back = lambda g: g.cpu()[:, :Q].reshape(B, h, w_, Q).permute(0, 3, 1, 2)          # noqa: E731
    return dict(hout=hout[:16].cpu(), dp1=dp[0].cpu(), dp2=dp[1].cpu(), dt1=dt[0].cpu(), dt2=dt[1].cpu(), conf=conf.cpu(), back=back, QP=QP, Q=Q,
                desc=hd, keep=(p1, p2, labd, part, keys, hout, g1, dp, dt, conf))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _normal(t, scale=1.0):
    """No non-zero value of t (times scale) is subnormal in its own format: fp32 and bf16 share the exponent range."""
    v = t.float().abs()
    v = v[v > 0]
    return v.numel() > 0 and float(v.min()) * scale >= 2.0 ** -126


HEADS = [("straddle", False, False), ("straddle", True, False), ("straddle", False, True), ("straddle", True, True), ("rows", False, False)]
_HID = lambda c: f"{c[0]}-{'half' if c[1] else 'align'}-{'one' if c[2] else 'two'}"          # noqa: E731
_BASE = {}


def _base(dev, c):
    """The unweighted launches at the case, and its inputs (shared by (a)-(d))."""
    if c not in _BASE:
        case, half, single = c
        p1, p2, lab, wt, item = wr.inputs(case, CD)
        _BASE[c] = (p1, p2, lab, wt, item, _head(dev, case, half, single, p1, p2, lab))
    return _BASE[c]


def _grads(r, single):
    """The written columns of the gradient outputs (the drivers pre-fill the rest)."""
    out = [("dp2", r["dp2"][:, :r["QP"]]), ("dt2", r["dt2"][:, :r["QP"]])]
    if not single:
        out += [("dp1", r["dp1"][:, :r["QP"]]), ("dt1", r["dt1"][:, :r["QP"]])]
    return out


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_weighted_head_exact_properties(dev, c):
    case, half, single = c
    B = wr.CASES[case][0]
    p1, p2, lab, _wt, _item, base = _base(dev, c)
    run = lambda **kw: _head(dev, case, half, single, p1, p2, lab, **kw)          # noqa: E731
    # (a) w = 1, no map: the unweighted launches, bit for bit
    one = run(w=np.ones(B, np.float32))
    assert torch.equal(_bits(one["hout"]), _bits(base["hout"])), (one["hout"].tolist(), base["hout"].tolist())
    assert torch.equal(one["conf"], base["conf"])
    for (n, a), (_n, b) in zip(_grads(one, single), _grads(base, single)):
        assert torch.equal(_bits(a), _bits(b)), f"(a) {n}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ from the unweighted launch"
        assert _normal(b, 0.25), f"{n}: a compared value (or its quarter) is subnormal"
        assert bool((b[:, :base["Q"]] != 0).any())
    assert bool((one["dt2"][:, one["QP"]:] == SENTINEL).all()), "pad columns [QP, ld_t) of the bf16 gradient were written"
    assert int(base["hout"][15]) == 2 and int(base["hout"][6]) == int(((lab >= 0) & (lab < wr.CASES[case][6])).sum())
    assert _normal(base["hout"][[1, 14]], 0.5) and (single or _normal(base["hout"][[0]], 0.5))
    # (b) w = 0.5: exactly half
    hf = run(w=np.full(B, 0.5, np.float32))
    for i in ((1, 14) if single else (0, 1, 14)):
        assert float(hf["hout"][i]) == 0.5 * float(base["hout"][i]), (i, float(hf["hout"][i]), float(base["hout"][i]))
    assert float(hf["hout"][6]) == float(base["hout"][6]) and float(hf["hout"][15]) == float(base["hout"][15])
    assert torch.equal(hf["conf"], base["conf"])
    for (n, a), (_n, b) in zip(_grads(hf, single), _grads(base, single)):
        assert bool((a.float() == 0.5 * b.float()).all()), f"(b) {n}: {int((a.float() != 0.5 * b.float()).sum())} elements are not half of (a)"
    # (c) per-item powers of two: the gradient rows of item b are w_b times (a)'s
    wc = np.array([1.0, 0.5, 0.25], np.float32)
    pc = run(w=wc)
    rows = base["dp2"].shape[0] // B
    scale = torch.from_numpy(wc).repeat_interleave(rows)[:, None]
    for (n, a), (_n, b) in zip(_grads(pc, single), _grads(base, single)):
        assert bool((a.float() == scale * b.float()).all()), f"(c) {n}: {int((a.float() != scale * b.float()).sum())} elements are not w_b times (a)"
    assert float(pc["hout"][6]) == float(base["hout"][6])
    # (d) a constant map per item with a permuted table == the map-less launch on the gathered table
    table = np.array([0.3, 0.9, 0.55], np.float32)
    perm = [2, 0, 1]
    H, W = lab.shape[1:]
    const = torch.tensor(perm, dtype=torch.uint8).view(B, 1, 1).expand(B, H, W).contiguous()
    via_map, gathered = run(w=table, w_item=const), run(w=table[perm])
    assert torch.equal(_bits(via_map["hout"]), _bits(gathered["hout"]))
    for (n, a), (_n, b) in zip(_grads(via_map, single), _grads(gathered, single)):
        assert torch.equal(_bits(a), _bits(b)), f"(d) {n}: the constant map differs from the gathered table"
    assert not torch.equal(_bits(gathered["dp2"]), _bits(base["dp2"]))


@pytest.mark.parametrize("c", HEADS, ids=_HID)
def test_weighted_head_vs_float64(dev, c):
    """(e) general weights and a random map (one block of bytes >= B: clamped) against tests/_weighted_ref.py: losses within
    1e-4 * (1 + |ref|), gradients under tests/_head_bar.py as it stands (tau from the fp32 and float64 references, CAP 0.1 %, bf16 within one
    ulp and bit for bit the rounding of the fp32 output of the same launch)."""
    case, half, single = c
    B, h, w_, H, W, Q, Cn = wr.CASES[case]
    p1, p2, lab, wt, item, _b = _base(dev, c)
    got = _head(dev, case, half, single, p1, p2, lab, w=wt, w_item=item)
    r64, r32 = hb.ref_pair(("weighted refs", c), lambda dt: wr.weighted_ref(None if single else p1, p2, lab, wt, item, 0.1, half, dt, Cn))
    for i, k in ((1, "l2"), (14, "total")) + (() if single else ((0, "l1"),)):
        want = float(r64[k])
        print(f"[weighted] {_HID(c)} hout[{i}] = {float(got['hout'][i])!r}, float64 {want!r}")
        assert abs(float(got["hout"][i]) - want) <= 1e-4 * (1 + abs(want)), (k, float(got["hout"][i]), want)
    assert int(got["hout"][6]) == r64["N"] and int(got["hout"][15]) == 2
    for hd_, f32, bf in (("dpred2", got["dp2"], got["dt2"]),) + (() if single else (("dpred1", got["dp1"], got["dt1"]),)):
        hb.trainer_form(_HID(c), hd_, f32, bf, got["back"], Q, got["QP"], r64[hd_], r32[hd_], 1.0)
    # NULL map: the item's own weight
    own = _head(dev, case, half, single, p1, p2, lab, w=wt)
    o64 = hb.cached(("weighted refs own", c), lambda: wr.weighted_ref(None if single else p1, p2, lab, wt, None, 0.1, half, torch.float64, Cn))
    assert abs(float(own["hout"][14]) - float(o64["total"])) <= 1e-4 * (1 + abs(float(o64["total"])))
    assert abs(float(o64["total"]) - float(r64["total"])) > 1e-4 * (1 + abs(float(r64["total"]))), "the map changes nothing: the case shows nothing"


def test_weighted_head_refusals_write_nothing(dev):
    c = HEADS[0]
    case, half, single = c
    p1, p2, lab, wt, item, base = _base(dev, c)
    hd = base["desc"]
    hout = base["keep"][5]
    hout.fill_(-3.0)
    wd = torch.from_numpy(wt).to(dev)
    st = ops.stream_ptr()
    for name in ("simt_head_loss_weighted", "simt_head_grad_weighted"):
        with pytest.raises(L.SimtHipError):
            L.call(name, C.byref(hd), None, None, st)                          # no table
        with pytest.raises(L.SimtHipError):
            L.call(name, C.byref(hd), wd.data_ptr() + 2, None, st)             # misaligned
        with pytest.raises(L.SimtHipError):
            L.call(name, None, wd.data_ptr(), None, st)
        hd.mode = 0                                                            # the SimT loss block takes no weights
        try:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(hd), wd.data_ptr(), None, st)
        finally:
            hd.mode = 1
    torch.cuda.synchronize()
    assert bool((hout == -3.0).all())
