"""ClassMix behind the teacher on the GPU (simt_online_label_u8 / simt_online_label_cb_u8 in csrc/label_sweep.hip,
simt_class_mix_u8 in csrc/class_mix.hip, the keyword online_mix of the warm-up trainers, --online-mix of trainV1_warmup).  Every comparison
is between two executions of the same arithmetic or selection and therefore BITWISE.  The yardsticks are the launches that existed before the
keyword and tests/_class_mix_ref.py, never the code under test:

  (a) the label launches: lab8 / counts against simt_pseudo_label_u8 / simt_pseudo_label2_u8 mode 1 (cb: against simt_online_label_cb,
      hist included); the OR of `part` per item against numpy on those labels and against simt_label_presence on the widened labels;
      every word of a garbage-filled `part` overwritten; refusals;
  (b) simt_class_mix_u8 against simt_label_presence + simt_class_mix on the widened labels and against _class_mix_ref; refusals;
  (c) the trainers with online_mix against a trainer WITHOUT online_labels that is fed the image and label pair the existing launches make
      from a separate teacher plan with the same draws; resume; the keyword-less trainer calls none of the new symbols;
  (d) the tool."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as ref
import test_gpu_online_labels as OL
import test_gpu_resume as R
from simt_amd import _lib as L
from simt_amd import ops
from simt_amd import train_state as tsf
from simt_amd.ema_teacher import refresh_due
from test_gpu_online_labels_cb import BalancedComposition, _cb_desc, _thr_vector
from test_gpu_step_coherence import one_rank_group

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
NEW = ("simt_online_label_parts", "simt_online_label_u8", "simt_online_label_cb_u8", "simt_class_mix_u8")
SENTINEL = 0x5A


# ---- (a) the label launches ------------------------------------------------------------------------------------------------------------------------
# (family, B, h, w, H, W, C, ld)
GEOMETRIES = [(0, 3, 2, 2, 3, 5, 19, 24),              # 45 pixels: ONE wave spans three items
              (1, 3, 2, 2, 3, 5, 19, 24),
              (0, 2, 3, 4, 7, 9, 19, 24),              # H * W % 4 != 0
              (1, 2, 3, 4, 7, 9, 19, 19),              # (the scalar gathers of family 1)
              (0, 2, 9, 17, 33, 65, 19, 24),           # W = 65; more than one block
              (1, 2, 9, 17, 33, 65, 19, 24),
              (0, 2, 2, 3, 33, 65, 1, 4),              # C = 1
              (1, 2, 2, 3, 33, 65, 1, 4),
              (0, 3, 9, 9, 64, 64, 32, 32),            # C = 32: every bit of the presence word
              (1, 3, 9, 9, 64, 64, 32, 32),
              (0, 2, 17, 17, 520, 520, 19, 24),        # B*H*W = 540800 > 512 * 1024: the stride loop runs twice
              (1, 2, 17, 17, 520, 520, 19, 24)]        # ... > 1024 * 512 likewise
TAUS = [0.0, 0.5, 0.968, float("nan")]
_ID = lambda g: "fam{}-{}x{}x{}to{}x{}-C{}-ld{}".format(*g)          # noqa: E731


def _u8_desc(view, lab8, counts, part, family, B, h, w, ld, H, W, Cn, thr):
    d = L.OnlineLabelU8Desc()
    d.fix, d.lab8, d.counts, d.part = view.data_ptr(), lab8.data_ptr(), counts.data_ptr(), (part.data_ptr() if part is not None else None)
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, ld, H, W, Cn, family, thr
    return d


def _rows(family, B, H, W):
    """The workgroups of the sweep, from its documented launch shape: 1024 pixels per workgroup and at most 512 (family 0), 512 and 1024."""
    block, most = (1024, 512) if family == 0 else (512, 1024)
    return min(-(-B * H * W // block), most)


def _presence_np(lab, Cn):
    """[B] words: the OR of 1 << l over the labels l < Cn of every item, in numpy."""
    out = []
    for item in lab.reshape(lab.shape[0], -1):
        word = 0
        for v in np.unique(item):
            if int(v) < Cn:
                word |= 1 << int(v)
        out.append(word)
    return np.array(out, dtype=np.uint32)


def _presence_launch(lab64, Cn, dev):
    """The words of the EXISTING presence launch for int64 labels, OR-ed per item."""
    B = lab64.shape[0]
    part = torch.zeros(B, L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)
    L.call("simt_label_presence", ops._p(lab64), B, lab64[0].numel(), Cn, ops._p(part), ops.stream_ptr())
    torch.cuda.synchronize()
    return np.bitwise_or.reduce(part.cpu().numpy().view(np.uint32), axis=1), part


def _aligned_u8(n, dev, fill):
    """n bytes at a 16-byte aligned base, with 16 guard bytes on either side -> (buffer, view)."""
    buf = torch.full((n + 32,), fill, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 16 + 16
    return buf, buf[off:off + n], off


def _check_part(part_buf, rows, B, lab_np, Cn, dev, what):
    words = part_buf[:rows * B].cpu().numpy().view(np.uint32).reshape(B, rows).T          # -> [workgroup][item]
    got = np.bitwise_or.reduce(words, axis=0)
    want = _presence_np(lab_np, Cn)
    assert (got == want).all(), f"{what}: presence {[hex(int(v)) for v in got]}, numpy {[hex(int(v)) for v in want]}"
    launch, _ = _presence_launch(torch.from_numpy(lab_np.astype(np.int64)).to(dev), Cn, dev)
    assert (got == launch).all(), f"{what}: presence differs from simt_label_presence"
    return words


@pytest.mark.parametrize("geo", GEOMETRIES, ids=_ID)
def test_u8_label_launch_equals_the_export_and_its_presence_words_are_exact(dev, geo):
    family, B, h, w, H, W, Cn, ld = geo
    buf, view = OL._input(family, B, h, w, Cn, ld, dev, seed=sum(geo))
    if B == 3:          # item 1: NaN everywhere -- every label 255, presence 0
        view.view(B, h * w * ld)[1].fill_(float("nan"))
    before = buf.clone()
    P = B * H * W
    rows = _rows(family, B, H, W)
    some_kept = False
    for thr in TAUS:
        lbuf, lab8, off = _aligned_u8(P, dev, 77)
        counts = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
        words = []
        for garbage in (-1, 0x12345678):          # every word is written whatever lay there: two prefills, the same words
            part = torch.full((rows * B + 8,), garbage, dtype=torch.int32, device=dev)
            d = _u8_desc(view, lab8, counts, part, family, B, h, w, ld, H, W, Cn, thr)
            assert L.load().simt_online_label_parts(C.byref(d)) == rows
            L.call("simt_online_label_u8", C.byref(d), ops.stream_ptr())
            torch.cuda.synchronize()
            assert bool((part[rows * B:] == garbage).all()), "words behind part written"
            words.append(part[:rows * B].clone())
        assert torch.equal(words[0], words[1]), "a word of part kept its prefill"
        out, cnt = OL._yardstick(view, family, B, h, w, ld, H, W, Cn, thr, dev)
        torch.cuda.synchronize()
        assert torch.equal(lab8.view(B, H, W), out), f"threshold {thr}: {int((lab8.view(B, H, W) != out).sum())} of {P} labels differ"
        assert torch.equal(counts, 2 * cnt) and int(cnt.sum()) == P          # two calls: the counts accumulate
        assert bool((lbuf[:off] == 77).all()) and bool((lbuf[off + P:] == 77).all()), "guard bytes of the labels written"
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the input was written"
        lab_np = out.cpu().numpy()
        per_block = _check_part(words[0], rows, B, lab_np, Cn, dev, f"threshold {thr}")
        if thr != thr:
            assert (lab_np == 255).all() and not per_block.any(), "a NaN threshold keeps nothing and sets no bit"
        if B == 3:
            assert (lab_np[1] == 255).all() and not per_block[:, 1].any(), "the all-NaN item has a label or a bit"
        some_kept = some_kept or bool((lab_np != 255).any())
        if rows > 1 and thr == 0.0:          # block g of the sweep sees pixels [g * block, (g + 1) * block) + k * rows * block: zero elsewhere
            block = 1024 if family == 0 else 512
            flat = lab_np.reshape(-1)
            for g in (0, rows - 1):
                mine = np.concatenate([flat[s:s + block] for s in range(g * block, P, rows * block)])
                item = np.concatenate([np.arange(s, min(s + block, P)) // (H * W) for s in range(g * block, P, rows * block)])
                for b in range(B):
                    want = 0
                    for v in np.unique(mine[item == b]):
                        want |= (1 << int(v)) if int(v) < Cn else 0
                    assert int(per_block[g, b]) == want, (g, b)
    assert some_kept


@pytest.mark.parametrize("geo", [g for g in GEOMETRIES if g[6] > 1 and g[4] < 520] + [GEOMETRIES[-2]], ids=_ID)
def test_cb_u8_label_launch_equals_the_int64_launch(dev, geo):
    family, B, h, w, H, W, Cn, ld = geo
    buf, view = OL._input(family, B, h, w, Cn, ld, dev, seed=sum(geo) + 1)
    P = B * H * W
    rows = _rows(family, B, H, W)
    thr = torch.from_numpy(_thr_vector(Cn)).to(dev)          # NaN, -1, 0.5, 0.968, 1 in turn
    lab64 = torch.full((P,), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
    hist = torch.zeros(Cn, L.CONF_BINS, dtype=torch.int64, device=dev)
    L.call("simt_online_label_cb", C.byref(_cb_desc(view, lab64, cnt, hist, thr, family, B, h, w, ld, H, W, Cn)), ops.stream_ptr())
    lbuf, lab8, off = _aligned_u8(P, dev, 77)
    counts = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
    hist8 = torch.zeros(Cn, L.CONF_BINS, dtype=torch.int64, device=dev)
    part = torch.full((rows * B + 8,), -1, dtype=torch.int32, device=dev)
    d = L.OnlineLabelCbU8Desc()
    d.fix, d.lab8, d.counts, d.hist, d.thr, d.part = view.data_ptr(), lab8.data_ptr(), counts.data_ptr(), hist8.data_ptr(), thr.data_ptr(), part.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family = B, h, w, ld, H, W, Cn, family
    L.call("simt_online_label_cb_u8", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(lab8.long(), lab64 & 255) and bool(((lab64 >= 0) & (lab64 < 256)).all())          # the low byte of the int64 word
    assert torch.equal(counts, cnt) and torch.equal(hist8, hist) and int(hist.sum()) == P
    assert bool((lbuf[:off] == 77).all()) and bool((lbuf[off + P:] == 77).all()) and bool((part[rows * B:] == -1).all())
    _check_part(part, rows, B, lab8.view(B, H, W).cpu().numpy(), Cn, dev, "class-balanced")
    if h > 2:          # the tie band belongs to class 1 (threshold -1: kept), the NaN pixel's neighbourhood is 255
        assert bool((lab8 == 255).any()) and bool((lab8 != 255).any())
    # refusals of the cb flavour's own pointers
    for field, value in (("hist", None), ("thr", None), ("hist", hist8.data_ptr() + 4), ("thr", thr.data_ptr() + 2), ("part", None)):
        keep = getattr(d, field)
        setattr(d, field, value)
        with pytest.raises(L.SimtHipError):
            L.call("simt_online_label_cb_u8", C.byref(d), ops.stream_ptr())
        setattr(d, field, keep)
    torch.cuda.synchronize()
    assert torch.equal(counts, cnt), "a refused call counted"


def test_u8_label_launch_refusals_write_nothing(dev):
    family, B, h, w, H, W, Cn, ld = GEOMETRIES[4]
    buf, view = OL._input(family, B, h, w, Cn, ld, dev, seed=1)
    P = B * H * W
    lbuf, lab8, off = _aligned_u8(P, dev, SENTINEL)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    part = torch.full((1024 * 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    good = dict(family=family, B=B, h=h, w=w, ld=ld, H=H, W=W, C=Cn, thr=0.5)

    def desc(**kw):
        a = dict(good, **kw)
        d = _u8_desc(view, lab8, counts, part, a["family"], a["B"], a["h"], a["w"], a["ld"], a["H"], a["W"], a["C"], a["thr"])
        for k in ("fix", "lab8", "counts", "part"):
            if k in kw:
                setattr(d, k, kw[k])
        return d
    bad = [desc(fix=None), desc(lab8=None), desc(counts=None), desc(part=None), desc(C=25), desc(C=33, ld=36), desc(B=33), desc(family=2),
           desc(family=-1), desc(lab8=lab8.data_ptr() + 4), desc(lab8=lab8.data_ptr() + 8), desc(part=part.data_ptr() + 2), desc(B=0),
           desc(H=0), desc(w=0), desc(C=0), desc(H=65536, W=32768),
           desc(family=1, B=1, h=32768, w=32768, ld=4, C=3)]                  # B*h*w*ld = 2^32: the 32-bit tap offsets of family 1
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_online_label_u8", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_online_label_u8", None, ops.stream_ptr())
    assert L.load().simt_online_label_parts(None) < 0 and L.load().simt_online_label_parts(C.byref(desc(B=0))) < 0
    assert L.load().simt_online_label_parts(C.byref(desc(family=3))) < 0
    torch.cuda.synchronize()
    assert bool((lbuf == SENTINEL).all()) and int(counts.sum()) == 0 and bool((part == 0x5A5A5A5A).all())
    L.call("simt_online_label_u8", C.byref(desc()), ops.stream_ptr())          # the descriptor itself is sound
    torch.cuda.synchronize()
    assert int(counts.sum()) == P and bool((lbuf[:off] == SENTINEL).all())


# ---- (b) simt_class_mix_u8 -------------------------------------------------------------------------------------------------------------------------
def _mix_batch(B, h, w, Cn, seed, blank=None):
    """x: every bit pattern (NaN payloads, -0.0, infinities among them) as int32; lab: block-wise classes with 255s sprinkled, item `blank` all
    255."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2 ** 31, 2 ** 31, (B, 3, h, w), dtype=np.int64).astype(np.int32)
    special = np.array([0x7FC00001, -0x3FFFFF, -0x80000000, 0x7F800000, -0x800000, 0x7F812345], dtype=np.int64).astype(np.int32)
    x.reshape(-1)[::7] = special[np.arange(x.size)[::7] % len(special)]
    blocks = rng.integers(0, Cn, (B, -(-h // 3), -(-w // 5)))
    lab = np.kron(blocks, np.ones((3, 5), dtype=np.int64))[:, :h, :w].astype(np.uint8)
    lab[rng.random((B, h, w)) < 0.1] = 255
    if blank is not None:
        lab[blank] = 255
    return x, np.ascontiguousarray(lab)


def _spread_part(lab, Cn, rows):
    """Presence words spread over `rows` rows by hand: the bit of class c of item b lies in row (c + b) % rows alone."""
    B = lab.shape[0]
    part = np.zeros((B, rows), dtype=np.uint32)
    for b in range(B):
        for v in np.unique(lab[b]):
            if int(v) < Cn:
                part[b, (int(v) + b) % rows] |= np.uint32(1 << int(v))
    return part


def _u8_mix_desc(x, lab8, x_out, lab_out, part, B, h, w, Cn, rows, apply, rank):
    d = L.ClassMixU8Desc()
    d.x, d.lab8, d.x_out, d.lab_out, d.part = x.data_ptr(), lab8.data_ptr(), x_out.data_ptr(), lab_out.data_ptr(), part.data_ptr()
    d.B, d.h, d.w, d.n_classes, d.rows = B, h, w, Cn, rows
    table = np.full((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), 0xEE, dtype=np.uint8)          # garbage beyond B and beyond C
    table[:B, :Cn] = rank
    C.memmove(d.rank, table.ctypes.data, table.nbytes)
    for i in range(L.CLASS_MIX_MAX):
        d.partner[i] = (i + 1) % B if i < B else 0xEE
        d.apply[i] = (1 if apply[i] else 0) if i < B else 0xEE
    return d


def _existing_mix(x, lab64, apply, rank, Cn, dev):
    """simt_label_presence + simt_class_mix on int64 labels -> (x_out, lab_out) device tensors."""
    B, _c, h, w = x.shape
    _words, part = _presence_launch(lab64, Cn, dev)
    x_out, lab_out = torch.empty_like(x), torch.empty_like(lab64)
    d = L.ClassMixDesc()
    d.x, d.lab, d.x_out, d.lab_out, d.part = x.data_ptr(), lab64.data_ptr(), x_out.data_ptr(), lab_out.data_ptr(), part.data_ptr()
    d.B, d.h, d.w, d.n_classes = B, h, w, Cn
    table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
    table[:B, :Cn] = rank
    C.memmove(d.rank, table.ctypes.data, table.nbytes)
    for i in range(B):
        d.partner[i], d.apply[i] = (i + 1) % B, 1 if apply[i] else 0
    L.call("simt_class_mix", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    return x_out, lab_out


# (B, h, w, C, rows, apply: "none" | "all" | "mixed")
MIX_CASES = [(2, 8, 12, 19, 1, "all"), (2, 8, 12, 19, 3, "none"), (3, 8, 12, 19, 70, "mixed"),          # h * w % 4 == 0: the 16-byte flavour
             (2, 7, 9, 19, 5, "all"), (3, 7, 9, 19, 64, "mixed"), (2, 7, 9, 1, 2, "all"),                # h * w % 4 == 3: the scalar flavour and its tail
             (32, 6, 10, 32, 1024, "mixed"), (32, 5, 5, 32, 65, "mixed"),                                # B = 32, C = 32, the most rows
             (2, 72, 64, 19, 512, "all"), (4, 67, 65, 7, 9, "mixed"),                                    # more than one workgroup per item
             (3, 33, 37, 19, 7, "mixed")]                                                                # 305 quads + 1 pixel: the tail lane in a lane's SECOND quad round


@pytest.mark.parametrize("case", MIX_CASES, ids=lambda c: "B{}-{}x{}-C{}-rows{}-{}".format(*c))
def test_class_mix_u8_equals_the_existing_launches_and_the_restatement(dev, case):
    B, h, w, Cn, rows, how = case
    x_np, lab_np = _mix_batch(B, h, w, Cn, seed=sum(case[:5]), blank=1 if B > 2 else None)
    rng = ref.generator(5, 0)
    apply, rank = ref.draws(rng, B, Cn, 0.5)
    apply = {"none": np.zeros(B, bool), "all": np.ones(B, bool), "mixed": apply}[how]
    if how == "mixed":
        apply[0], apply[1], apply[-1] = True, False, True          # item 0 receives from the blank item 1 (B > 2): nothing may be pasted
    x = torch.from_numpy(x_np).to(dev)
    lbuf, lab8, _off = _aligned_u8(B * h * w, dev, 0)
    lab8.copy_(torch.from_numpy(lab_np).reshape(-1))
    part = torch.from_numpy(_spread_part(lab_np, Cn, rows).view(np.int32)).to(dev)
    x_out = torch.full_like(x, 0x5A5A5A5A)
    lab_out = torch.full((B, h, w), -3, dtype=torch.int64, device=dev)
    before = (x.clone(), lbuf.clone(), part.clone())
    d = _u8_mix_desc(x, lab8, x_out, lab_out, part, B, h, w, Cn, rows, apply, rank)
    L.call("simt_class_mix_u8", C.byref(d), ops.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(x, before[0]) and torch.equal(lbuf, before[1]) and torch.equal(part, before[2]), "an input was written"
    want_x, want_lab = ref.mix(x_np, lab_np.astype(np.int64), apply, rank, Cn)
    assert (lab_out.cpu().numpy() == want_lab).all(), f"{int((lab_out.cpu().numpy() != want_lab).sum())} labels differ from the restatement"
    assert (x_out.cpu().numpy() == want_x).all(), "the image differs from the restatement"
    ex_x, ex_lab = _existing_mix(x, torch.from_numpy(lab_np.astype(np.int64)).to(dev), apply, rank, Cn, dev)
    assert torch.equal(lab_out, ex_lab) and torch.equal(x_out, ex_x), "differs from simt_label_presence + simt_class_mix"
    masks = ref.paste_masks(lab_np.astype(np.int64), apply, rank, Cn)
    if how == "none":
        assert not masks.any() and torch.equal(x_out, x) and (lab_out.cpu().numpy() == lab_np).all()
    else:
        assert masks.any() and not masks.all(), "the case pastes nothing or everything"
    if B > 2 and how == "mixed":
        assert not masks[0].any(), "something was pasted from the all-255 item"


def test_class_mix_u8_refusals_leave_the_outputs_untouched(dev):
    B, h, w, Cn, rows = 2, 8, 12, 19, 3
    x_np, lab_np = _mix_batch(B, h, w, Cn, seed=3)
    apply, rank = ref.draws(ref.generator(1, 0), B, Cn, 1.0)
    x = torch.from_numpy(np.concatenate([x_np.reshape(-1), x_np.reshape(-1)])).to(dev)          # room for an overlapping x_out
    _lbuf, lab8, _off = _aligned_u8(B * h * w, dev, 0)
    lab8.copy_(torch.from_numpy(lab_np).reshape(-1))
    part = torch.from_numpy(_spread_part(lab_np, Cn, rows).view(np.int32)).to(dev)
    x_out = torch.full((B * 3 * h * w + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    lab_out = torch.full((B * h * w + 2,), -3, dtype=torch.int64, device=dev)
    x_before = x.clone()

    def desc(**kw):
        d = _u8_mix_desc(x, lab8, x_out, lab_out, part, B, h, w, Cn, rows, apply, rank)
        for k, v in kw.items():
            if k in ("partner0", "rank00"):
                continue
            setattr(d, k, v)
        if "partner0" in kw:
            d.partner[0] = kw["partner0"]
        if "rank00" in kw:
            d.rank[0][0] = kw["rank00"]
        return d
    n = B * 3 * h * w * 4
    bad = [desc(x=None), desc(lab8=None), desc(x_out=None), desc(lab_out=None), desc(part=None),
           desc(x=x.data_ptr() + 4), desc(lab8=lab8.data_ptr() + 4), desc(x_out=x_out.data_ptr() + 8), desc(lab_out=lab_out.data_ptr() + 8),
           desc(part=part.data_ptr() + 2), desc(B=1), desc(B=33), desc(n_classes=0), desc(n_classes=33), desc(h=0), desc(w=-1),
           desc(h=65536, w=32768), desc(rows=0), desc(rows=1025),
           desc(x_out=x.data_ptr()), desc(x_out=x.data_ptr() + 16), desc(x_out=x.data_ptr() + n - 16),          # x_out overlapping x
           desc(partner0=2), desc(rank00=19)]
    for d in bad:
        with pytest.raises(L.SimtHipError):
            L.call("simt_class_mix_u8", C.byref(d), ops.stream_ptr())
    with pytest.raises(L.SimtHipError):
        L.call("simt_class_mix_u8", None, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool((x_out == 0x5A5A5A5A).all()) and bool((lab_out == -3).all()) and torch.equal(x, x_before)
    L.call("simt_class_mix_u8", C.byref(desc()), ops.stream_ptr())          # the descriptor itself is sound; the words behind the outputs stay
    L.call("simt_class_mix_u8", C.byref(desc(x_out=x.data_ptr() + n)), ops.stream_ptr())          # adjacent is not overlapping
    torch.cuda.synchronize()
    assert bool((x_out[:-4] != 0x5A5A5A5A).any()) and bool((x_out[-4:] == 0x5A5A5A5A).all()) and bool((lab_out[-2:] == -3).all())
    assert torch.equal(x[n // 4:], x_out[:-4])


# ---- (c) trainers ----------------------------------------------------------------------------------------------------------------------------------
SIZE = OL.SIZE
MODELS = OL.MODELS
PORT = 29593
MIX_P, MIX_SEED = 0.5, 11
PORTION, MOMENTUM = 0.5, 0.5


def _mixed_pair(strong, lab64, rng, dev):
    """What the EXISTING launches make of (student's image, teacher's labels) with the next draws of `rng`."""
    apply, rank = ref.draws(rng, SIZE[0], 19, MIX_P)
    return _existing_mix(strong.contiguous(), lab64.contiguous(), apply, rank, 19, dev) + (bool(apply.any()),)


_RUNS = {}


def _run(model, dev, dtype, mode, every=None, steps=3, its=1, dp=False, balanced=False, pass_weak=True, scale=1.0):
    """One memoised run.  mode "mix": the trainer with online_labels and online_mix.  mode "composition": the trainer WITHOUT online_labels,
    fed the mixed image and label the existing launches make from a separate teacher plan (refreshed by hand where refresh_due says so) with
    the same draws.  -> dict(tau, labels, inputs, scalars, state, shares, mixed)."""
    key = (model, dtype, mode, every, steps, its, dp, balanced, pass_weak, scale)
    if key in _RUNS:
        return _RUNS[key]
    data = OL._views(dev, steps, its)
    probe = OL.Composition(model, dev, dtype)
    tau = probe.threshold(data[0][0][1] if pass_weak else data[0][0][0], scale=scale)
    del probe
    comp = BalancedComposition(model, dev, dtype, tau, PORTION, MOMENTUM) if balanced else OL.Composition(model, dev, dtype)
    label_of = (lambda img: comp.label_balanced(img)) if balanced else (lambda img: comp.label(img, tau))
    ema = {} if every is None else {"ema_decay": 0.9}
    bal = dict(online_labels_balanced=PORTION, online_labels_momentum=MOMENTUM) if balanced else {}
    res = dict(tau=tau, labels=[], inputs=[], scalars=[], shares=[], mixed=[], refreshes=0)
    rng = ref.generator(MIX_SEED, 0)
    with (one_rank_group(dev, PORT) if dp else contextlib.nullcontext()) as pg:
        if mode == "mix":
            kw = dict(ema, online_labels=tau, online_mix=MIX_P, online_mix_seed=MIX_SEED, **bal)
            if every is not None:
                kw["online_labels_every"] = every
            tr = OL._trainer(model, dev, dtype, pg, its, **kw)
        else:
            tr = OL._trainer(model, dev, dtype, pg, its, **ema)
            assert not hasattr(tr, "fixed") and not hasattr(tr, "lab8") and tr.online_mix is None
        for mb in data:
            strong = [m[0] for m in mb] if its > 1 else mb[0][0]
            weak = [m[1] for m in mb] if its > 1 else mb[0][1]
            if mode == "mix":
                tr.step(strong, None, teacher_image=weak) if pass_weak else tr.step(strong)
            else:
                pairs = []
                for m in mb:
                    lab = label_of(m[1] if pass_weak else m[0]).clone()
                    res["shares"].append(float((lab != 255).float().mean()))
                    pairs.append(_mixed_pair(m[0], lab, rng, dev))
                    res["mixed"].append(pairs[-1][2] and not torch.equal(pairs[-1][1], lab))
                tr.step([p[0] for p in pairs] if its > 1 else pairs[0][0], [p[1] for p in pairs] if its > 1 else pairs[0][1])
                if every is not None and refresh_due(tr.ema_updates, every):
                    comp.follow(tr.ema_params)
                    res["refreshes"] += 1
            torch.cuda.synchronize()
            res["labels"].append(tr.label.clone())                         # (iter_size > 1: the last micro-batch's)
            res["inputs"].append(tr.plan.x_in.clone())
            res["scalars"].append(R.scalars(tr))
        res["losses"] = R.finite_losses(tr, f"{model} {mode}") if not balanced else tr.losses()
        res["state"] = OL._state(tr)
        if mode == "mix" and every is not None:
            res["refreshes"] = tr.teacher_refreshes
        del tr
    del comp
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


def _assert_same(a, b, what):
    for i in range(len(a["scalars"])):
        assert torch.equal(a["labels"][i], b["labels"][i]), f"{what}: {int((a['labels'][i] != b['labels'][i]).sum())} labels of step {i + 1} differ"
        assert torch.equal(a["inputs"][i].view(torch.int32), b["inputs"][i].view(torch.int32)), f"{what}: the student's input of step {i + 1} differs"
        assert torch.equal(a["scalars"][i], b["scalars"][i]), f"{what}: the scalars of step {i + 1} differ"
    sa, sb = a["state"], b["state"]
    assert sa.keys() == sb.keys()
    diff = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
    assert not diff, f"{what}: {len(diff)} of {len(sa)} tensors differ: {diff[:8]}"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("model", MODELS)
def test_mixing_trainer_equals_the_composition(dev, model, dtype):
    """3 steps, a weak view for the teacher, P = 0.5: the student's input, the labels, the loss scalars and every tensor of the state."""
    comp = _run(model, dev, dtype, "composition")
    print(f"{model}: tau = {comp['tau']!r}, kept shares {comp['shares']}, mixed {comp['mixed']}")
    assert all(0.1 < s < 0.9 for s in comp["shares"]), comp["shares"]
    assert any(comp["mixed"]), "no step of the composition pasted anything: the draws never applied"
    got = _run(model, dev, dtype, "mix")
    _assert_same(got, comp, f"{model} online mix")
    # `labelled` stays the share of the teacher's labels BEFORE the mix (read once, after 3 steps)
    assert abs(got["losses"]["labelled"] - sum(comp["shares"]) / 3) < 1e-6 and "labelled" not in comp["losses"]


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_mixing_trainer_iter_size_2(dev, model):
    comp = _run(model, dev, BF, "composition", its=2)
    assert any(comp["mixed"])
    _assert_same(_run(model, dev, BF, "mix", its=2), comp, f"{model} iter_size 2")


@pytest.mark.parametrize("model", MODELS)
def test_mixing_trainer_with_a_moving_teacher(dev, model):
    sc = OL.MOVING_SCALE[model]
    comp = _run(model, dev, BF, "composition", every=1, steps=4, scale=sc)
    got = _run(model, dev, BF, "mix", every=1, steps=4, scale=sc)
    assert got["refreshes"] == comp["refreshes"] == 4
    _assert_same(got, comp, f"{model} moving teacher")


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_mixing_trainer_with_balanced_thresholds(dev, model):
    comp = _run(model, dev, BF, "composition", balanced=True)
    got = _run(model, dev, BF, "mix", balanced=True)
    _assert_same(got, comp, f"{model} class-balanced")
    assert len(got["losses"]["label_thresholds"]) == 19


def test_mixing_trainer_without_a_weak_view(dev):
    """teacher_image=None: the teacher labels the student's image, and the mix selects from that same image."""
    _assert_same(_run("v2", dev, BF, "mix", pass_weak=False), _run("v2", dev, BF, "composition", pass_weak=False), "no weak view")


def test_mixing_trainer_one_rank_rccl_group(dev):
    _assert_same(_run("v2", dev, BF, "mix", dp=True), _run("v2", dev, BF, "mix"), "one-rank RCCL group")


def test_image_that_the_launch_cannot_read_goes_through_the_staging_buffer(dev):
    """A non-contiguous view, a misaligned base and a host tensor give what the contiguous device tensor gives."""
    data = OL._views(dev, 1)
    strong, weak = data[0][0]
    tau = OL.Composition("v2", dev, BF).threshold(weak)
    kw = dict(online_labels=tau, online_mix=1.0, online_mix_seed=3)
    B, H, W = SIZE
    wide = torch.zeros(B, 3, H, W + 3, device=dev)
    wide[..., :W] = strong
    flat = torch.zeros(strong.numel() + 1, device=dev)
    flat[1:] = strong.reshape(-1)
    outs = []
    for img in (strong, wide[..., :W], flat[1:].view(B, 3, H, W), strong.cpu()):
        tr = OL._trainer("v2", dev, **kw)
        assert tr._mix_stage is None
        tr.step(img, None, teacher_image=weak)
        torch.cuda.synchronize()
        outs.append((tr.plan.x_in.clone(), tr.label.clone(), R.scalars(tr), tr._mix_stage is not None))
        del tr
    assert [o[3] for o in outs] == [False, True, True, True]
    for o in outs[1:]:
        assert torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])
    assert not torch.equal(outs[0][0], strong), "online_mix = 1 pasted nothing"
    with pytest.raises(ValueError, match="image of shape"):
        OL._trainer("v2", dev, **kw).step(strong[:, :, :-1], None)


def test_labelled_is_the_teachers_share_and_the_plain_trainers_call_no_new_symbol(dev, monkeypatch):
    data = OL._views(dev, 1)
    strong, weak = data[0][0]
    tau = OL.Composition("v2", dev, BF).threshold(weak)
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    online = OL._trainer("v2", dev, online_labels=tau)
    plain = OL._trainer("v2", dev)
    online.step(strong, None, teacher_image=weak)
    plain.step(strong, online.label.clone())
    torch.cuda.synchronize()
    assert not set(calls) & set(NEW), "a trainer without the keyword launched a new symbol"
    for tr in (online, plain):
        assert tr.online_mix is None and not any(hasattr(tr, a) for a in ("lab8", "mix_part", "mix_desc", "_mix_rng", "online_u8_desc", "_mix_stage"))
    mixing = OL._trainer("v2", dev, online_labels=tau, online_mix=1.0)
    mixing.step(strong, None, teacher_image=weak)
    torch.cuda.synchronize()
    assert calls.count("simt_online_label_u8") == 1 and calls.count("simt_class_mix_u8") == 1
    assert calls.count("simt_online_label") == 1          # (the online trainer's, before)
    share_mix, share_online = mixing.losses()["labelled"], online.losses()["labelled"]
    assert share_mix == share_online and 0.0 < share_online < 1.0, (share_mix, share_online)
    assert not torch.equal(mixing.label, online.label), "online_mix = 1 changed no label"
    for kw, named in [(dict(online_mix=0.5), "^online_mix needs online_labels"), (dict(online_labels=tau, online_mix=0.0), "^online_mix 0.0"),
                      (dict(online_labels=tau, online_mix=float("nan")), "^online_mix nan"),
                      (dict(online_labels=tau, online_mix_seed=4), "^online_mix_seed needs online_mix"),
                      (dict(online_labels=tau, online_mix=0.5, online_mix_seed=1.5), "^online_mix_seed 1.5")]:
        with pytest.raises(ValueError, match=named):
            OL._trainer("v2", dev, **kw)


@pytest.mark.parametrize("model", MODELS)
def test_resume(dev, tmp_path, model):
    """3 steps + save + a new trainer + load + 3 steps == 6 steps, draws included; the refusals of the train state."""
    data = OL._views(dev, 6)
    tau = OL.Composition(model, dev, BF).threshold(data[0][0][1])
    kw = dict(online_labels=tau, online_mix=MIX_P, online_mix_seed=MIX_SEED)

    def steps(tr, part, out):
        for mb in part:
            tr.step(mb[0][0], None, teacher_image=mb[0][1])
            out["scalars"].append(R.scalars(tr))
            out["labelled"].append(tr.losses()["labelled"])
            out["labels"].append(tr.label.clone())
            out["inputs"].append(tr.plan.x_in.clone())

    a = dict(scalars=[], labelled=[], labels=[], inputs=[])
    tr = OL._trainer(model, dev, **kw)
    steps(tr, data, a)
    a["state"] = OL._state(tr)
    del tr
    b = dict(scalars=[], labelled=[], labels=[], inputs=[])
    tr = OL._trainer(model, dev, **kw)
    steps(tr, data[:3], b)
    ts = tr.training_state()
    assert ts["hyper"]["online_mix"] == MIX_P and ts["hyper"]["online_mix_seed"] == MIX_SEED and "mix_rng" in ts
    path = str(tmp_path / "run.state")
    tsf.save(path, ts, None, {"world": 1})
    del tr, ts
    ts, _k, _l = tsf.load(path)
    tr = OL._trainer(model, dev, **kw)
    tr.load_training_state(ts)
    steps(tr, data[3:], b)
    b["state"] = OL._state(tr)
    assert b["labelled"] == a["labelled"]
    _assert_same(a, b, f"{model} resumed after step 3")
    if model != "v2":
        return
    online = OL._trainer(model, dev, online_labels=tau)
    with pytest.raises(ValueError, match=r"online_mix \(state: 0\.5, this trainer: None\)"):
        online.load_training_state(ts)
    with pytest.raises(ValueError, match=r"online_mix \(state: None, this trainer: 0\.5\)"):
        tr.load_training_state(online.training_state())
    for other, named in [(dict(kw, online_mix=0.25), r"online_mix \(state: 0\.5, this trainer: 0\.25\)"),
                         (dict(kw, online_mix_seed=12), r"online_mix_seed \(state: 11, this trainer: 12\)")]:
        with pytest.raises(ValueError, match=named):
            OL._trainer(model, dev, **other).load_training_state(ts)
    ots = online.training_state()
    assert "mix_rng" not in ots and not any(k.startswith("online_mix") for k in ots["hyper"])


# ---- (d) the tool ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool_model", ["DeepLab", "DeepLabv3", "DeepLabVGG"])
def test_tool_mixes_online_and_resumes(dev, tmp_path, capsys, monkeypatch, tool_model):
    """trainV1_warmup --synthetic --online-labels 0 --online-mix 0.5, B = 2, 129,65: 2 + 2 == 4 through --train-state in the loss lines and in
    every tensor of the final snapshot; one label launch and one mix per iteration; the flag-off run launches none of the new symbols; a resume
    with the flag dropped or changed is refused.  (T = 0 keeps every pixel with a confidence: the constructor init labels something.)"""
    from simt_amd.tools import trainV1_warmup as tool
    common = ["--learning-rate", "2.5e-4", "--model", tool_model, "--input-size-target", "129,65", "--batch-size", "2", "--num-steps", "50",
              "--save-pred-every", "100", "--print-every", "1", "--from-scratch", "--restore-from", "", "--synthetic", "--online-labels", "0"]
    flags = ["--online-mix", "0.5"]
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run(tag, stop, *more):
        del calls[:]
        snap = str(tmp_path / tag)
        tool.main(common + ["--snapshot-dir", snap, "--num-steps-stop", str(stop)] + list(more))
        return capsys.readouterr().out, os.path.join(snap, "GTA5_4.pth")

    state = str(tmp_path / "run.state")
    out_a, snap_a = run("a", 4, *flags)
    lines = R._loss_lines(out_a)
    assert len(lines) == 4 and not re.search(r"loss_seg\w* = nan", out_a), out_a
    assert calls.count("simt_online_label_u8") == 4 and calls.count("simt_class_mix_u8") == 4 and "simt_online_label" not in calls
    assert "; online mix: with probability 0.5 an item receives" in out_a
    out_b1, _ = run("b", 2, *flags, "--train-state", state)
    assert R._loss_lines(out_b1) == lines[:2]
    out_b2, snap_b = run("b", 4, *flags, "--train-state", state)
    assert re.search(r"resumed \w+ from .* at iteration 2\b", out_b2), out_b2
    assert R._loss_lines(out_b2) == lines[2:], (out_a, out_b2)
    R._same_snapshot(snap_a, snap_b)
    for other in ([], ["--online-mix", "0.25"]):
        with pytest.raises(SystemExit, match="online_mix"):
            tool.main(common + other + ["--snapshot-dir", str(tmp_path / "b"), "--num-steps-stop", "6", "--train-state", state])
    capsys.readouterr()
    out_o, _ = run("o", 2)          # the flag-off run: the int64 launch, none of the new symbols
    assert not set(calls) & set(NEW) and calls.count("simt_online_label") == 2 and "online mix" not in out_o
