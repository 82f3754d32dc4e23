"""simt_adamw_multi (csrc/optim.hip) element by element against the float64 restatement of tests/_adamw_ref.py: EVERY element of
p, m and v within twice its carried bound (derived there, not measured) over three chained launches; the dword path and the 16-byte path
bit for bit the same; guards, the guard word, every refusal, a red case; and the tie to simt_adam_step's restatement at its sizes.

The float64 reference of a (wd) case is computed once and shared by every pointer-offset case; nothing writes to it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _adamw_ref as ref
from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu
CHUNK = 65536
# chunk edges (chunk = 65536 elements), float4 tails, a sub-wave and a sub-block segment
NS = [1, 3, 4, 5, 255, 1023, 65535, 65536, 65537, 2 * 65536 + 9]
SEGS = [(n, (i + k) & 3) for k in range(3) for i, n in enumerate(NS)]      # 30 x (n, group): every n in three of the four groups
NTOT = sum(n for n, _g in SEGS)
LRS = (1e-3, 1e-2, 3e-3, 3e-2)
WDS = {"wd": (0.01, 0.05, 0.1, 0.02), "wd0": (0.0, 0.0, 0.0, 0.0)}
BETAS, EPS = (0.9, 0.999), 1e-8
# bytes past a 16-byte boundary of (p, g, m, v): the SGD test's tuples with a fourth pointer -- all four different, one pointer off alone
# (each of the four), all off alike
OFFS = [(4, 8, 12, 0), (8, 12, 0, 4), (12, 0, 4, 8), (0, 4, 8, 12), (4, 0, 0, 0), (0, 12, 0, 0), (0, 0, 8, 0), (0, 0, 0, 4), (4, 4, 4, 4)]
SEG_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("pad", "<i4")])


def _layout(off_bytes):
    """Element offsets of the segments inside one buffer: every segment starts `off_bytes` past a 16-byte boundary, with at least four guard
    elements before it and one after.  -> (starts, total)."""
    starts, cur = [], 0
    for (n, _g) in SEGS:
        s = (cur + 3) // 4 * 4 + 4 + off_bytes // 4
        starts.append(s)
        cur = s + n + 1
    return starts, (cur + 3) // 4 * 4 + 4


def _constants(step, wds):
    return ref.constants([lr * 0.7 ** step for lr in LRS], wds, BETAS, step + 1)


@functools.lru_cache(maxsize=None)
def _reference(wd_key):
    """(p0, [g per step], [(p, m, v) of the restatement per step]) of three chained launches: first_step 1, 0, 0, the learning rates changing."""
    gen = torch.Generator().manual_seed(2300 + len(wd_key))
    p0 = torch.randn(NTOT, generator=gen)
    group = torch.cat([torch.full((n,), g_, dtype=torch.int64) for n, g_ in SEGS])
    grads, out = [], []
    p, m, v = ref.exact(p0), None, None
    for step in range(3):
        g = torch.randn(NTOT, generator=gen) * 10.0 ** float(-step)
        g[::7] *= 1e-19      # second moments among the subnormals (the eta of the restatement): a trunk's far corners hold such gradients
        c = _constants(step, WDS[wd_key])
        p, m, v = ref.adamw_ref(p, ref.exact(g), m, v, ref.per_element(c["step_size"], group), ref.per_element(c["decay"], group),
                                c["beta2"], c["omb1"], c["omb2"], c["bc2s"], EPS, step == 0)
        grads.append(g)
        out.append((p, m, v))
    return p0, grads, out


def fill_desc(d, c, eps, first_step):
    for i in range(4):
        d.step_size[i], d.decay[i] = c["step_size"][i], c["decay"][i]
    d.beta1, d.beta2, d.omb1, d.omb2, d.bc2s, d.eps, d.first_step = c["beta1"], c["beta2"], c["omb1"], c["omb2"], c["bc2s"], eps, first_step


class _Run:
    """One set of device buffers (p, g, m, v as views into four NaN-filled buffers at the given byte offsets) and the launch descriptor.
    m and v stay NaN until the first launch: first_step = 1 must not read them."""

    def __init__(self, dev, offs, p0):
        self.dev = dev
        self.lay = [_layout(o) for o in offs]
        self.bufs = [torch.full((tot,), float("nan"), device=dev) for (_s, tot) in self.lay]
        self.seg_mask = []
        for b, (starts, tot) in zip(self.bufs, self.lay):
            assert b.data_ptr() % 16 == 0
            m = torch.zeros(tot, dtype=torch.bool)
            for s, (n, _g) in zip(starts, SEGS):
                assert s >= 4 and s + n + 1 <= tot      # inside the buffer, guards on both sides
                m[s:s + n] = True
            self.seg_mask.append(m.to(dev))
        self.put(0, p0)
        recs = []
        for i, (n, group) in enumerate(SEGS):
            ptrs = [self.bufs[k].data_ptr() + 4 * self.lay[k][0][i] for k in range(4)]
            assert [q % 16 for q in ptrs] == list(offs)
            recs.append((*ptrs, n, group, 0))
        self.segs = torch.from_numpy(np.array(recs, dtype=SEG_DT).view(np.uint8).copy()).to(dev)
        chunks = [(si, ci) for si, r in enumerate(recs) for ci in range((r[4] + CHUNK - 1) // CHUNK)]
        self.chunks = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self.skip = torch.zeros(1, dtype=torch.int64, device=dev)
        d = L.AdamwDesc()
        d.segs, d.chunks, d.nchunks, d.chunk = self.segs.data_ptr(), self.chunks.data_ptr(), len(chunks), CHUNK
        d.skip_if = self.skip.data_ptr()
        self.d = d

    def put(self, k, flat):
        self.bufs[k][self.seg_mask[k]] = flat.to(self.dev)

    def get(self, k):
        return self.bufs[k][self.seg_mask[k]].cpu()

    def guards_intact(self):
        return all(bool(torch.isnan(b[~m]).all()) for b, m in zip(self.bufs, self.seg_mask))

    def launch(self, c, first_step, eps=EPS):
        fill_desc(self.d, c, eps, first_step)
        rc = L.load().simt_adamw_multi(C.byref(self.d), ops.stream_ptr())
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("wd_key", ["wd", "wd0"])
@pytest.mark.parametrize("offs", OFFS, ids=lambda o: "p%d_g%d_m%d_v%d" % o)
def test_adamw_multi_every_element_vs_float64(dev, offs, wd_key):
    p0, grads, want = _reference(wd_key)
    runs = [_Run(dev, offs, p0), _Run(dev, (0, 0, 0, 0), p0)]
    worst = 0.0
    for step in range(3):
        c = _constants(step, WDS[wd_key])
        for run in runs:
            run.put(1, grads[step])
            assert run.launch(c, 1 if step == 0 else 0) == 0
            assert run.guards_intact(), f"step {step}: a guard element next to a segment was written"
        for k, name in ((0, "p"), (2, "m"), (3, "v")):
            got = runs[0].get(k)
            assert not bool(torch.isnan(got).any()), f"step {step}: NaN in {name} (first_step = 1 must not read the NaN-filled moments)"
            assert torch.equal(got.view(torch.int32), runs[1].get(k).view(torch.int32)), \
                f"step {step}: {name} differs between the unaligned (dword) and the aligned (16-byte) run"
            worst = max(worst, ref.ratio(got, want[step][(0, None, 1, 2)[k]], f"step {step} {name}"))
    print(f"simt_adamw_multi offs {offs} {wd_key}: worst |stored - float64| / bound = {worst:.3f} (allowed {ref.SLACK})")
    # ---- red: one element 4x its own bound away must fail, by name
    p = want[2][0]
    gp = runs[0].get(0).clone()
    idx = 3 * 65536 + 7
    gp[idx] = float(p.v[idx] + 4.0 * p.e[idx])
    with pytest.raises(AssertionError, match=f"element {idx} "):
        ref.ratio(gp, p, "red p")


def _bits(run):
    return [b.clone().view(torch.int32) for b in run.bufs]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_adamw_multi_guard_word_and_refusals(dev):
    p0, grads, _want = _reference("wd")
    run = _Run(dev, (4, 8, 12, 0), p0)
    run.put(1, grads[0])
    c = _constants(0, WDS["wd"])
    assert run.launch(c, 1) == 0
    # ---- guard word: non-zero -> all four buffers keep their bits; zero again -> they move
    before = _bits(run)
    run.skip.fill_(1)
    assert run.launch(_constants(1, WDS["wd"]), 0) == 0
    assert _same(before, _bits(run)), "skip_if non-zero: something moved"
    run.skip.zero_()
    assert run.launch(_constants(1, WDS["wd"]), 0) == 0
    after = _bits(run)
    for k, name in ((0, "p"), (2, "m"), (3, "v")):
        moved = (after[k] != before[k])[run.seg_mask[k]]
        assert float(moved.double().mean()) > 0.99, f"skip_if zero again: {name} did not move"
    assert torch.equal(after[1], before[1]), "the gradient is read only"
    # ---- refusals: SIMT_ERR_INVALID (1), nothing launched, every buffer keeps its bits
    before = _bits(run)
    good = _constants(2, WDS["wd"])
    inf, nan = np.float32("inf"), np.float32("nan")

    def refused(what, consts=good, eps=EPS, **fields):
        d = run.d
        saved = {f: getattr(d, f) for f in fields}
        for f, val in fields.items():
            setattr(d, f, val)
        try:
            rc = run.launch(consts, 0, eps)
        finally:
            for f, val in saved.items():
                setattr(d, f, val)
        assert rc == 1, f"{what}: returned {rc}, expected SIMT_ERR_INVALID"
        assert _same(before, _bits(run)), f"{what}: refused, yet something moved"

    refused("NULL segs", segs=None)
    refused("NULL chunks", chunks=None)
    refused("nchunks 0", nchunks=0)
    refused("nchunks -1", nchunks=-1)
    refused("chunk 0", chunk=0)
    refused("beta1 = 1", dict(good, beta1=np.float32(1.0)))
    refused("beta1 < 0", dict(good, beta1=np.float32(-0.1)))
    refused("beta2 = 1", dict(good, beta2=np.float32(1.0)))
    refused("beta2 NaN", dict(good, beta2=nan))
    refused("eps 0", eps=0.0)
    refused("eps < 0", eps=-1e-8)
    for i in range(4):
        ss, dc = list(good["step_size"]), list(good["decay"])
        ss[i], dc[i] = inf, nan
        refused(f"step_size[{i}] inf", dict(good, step_size=ss))
        refused(f"decay[{i}] NaN", dict(good, decay=dc))
    assert L.load().simt_adamw_multi(None, ops.stream_ptr()) == 1
    assert run.launch(good, 0) == 0 and not _same(before, _bits(run)), "the good descriptor still launches"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tie to simt_adam_step: one segment, one group, decay = 1, at that test's sizes -- within the same bar of ITS restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _adam_step_ref(p, g, m, v, lr, beta1, beta2, eps, step):
    """adam_step_kernel (csrc/ntm.hip) in float64 with the carried bound, in ITS order: no decay, m and v read on every step."""
    f32 = np.float32
    bc1, bc2 = 1.0 - float(f32(beta1)) ** step, 1.0 - float(f32(beta2)) ** step
    step_size, bc2s = f32(float(f32(lr)) / bc1), f32(np.sqrt(bc2))
    omb1, omb2 = f32(1.0) - f32(beta1), f32(1.0) - f32(beta2)
    mi = ref.add(m, ref.mul(ref.sub(g, m), ref.const(omb1, p)))
    vi = ref.add(ref.mul(v, ref.const(beta2, p)), ref.mul(ref.mul(ref.const(omb2, p), g), g))
    den = ref.add(ref.div(ref.sqrt(vi), ref.const(bc2s, p)), ref.const(eps, p))
    return ref.sub(p, ref.mul(ref.const(step_size, p), ref.div(mi, den))), mi, vi


@pytest.mark.parametrize("Q,Cn", [(22, 19), (25, 19), (34, 19)])
def test_adamw_multi_one_segment_sits_on_adam_step(dev, Q, Cn):
    gen = torch.Generator().manual_seed(Q * 100 + 1)
    n = Q * Cn
    lr, eps = float(np.float32(6e-3)), 1e-8      # (an fp32 learning rate: simt_adam_step receives it as a float)
    p0 = torch.randn(n, generator=gen) * 2.0
    pd, gd = p0.clone().to(dev), torch.zeros(n, device=dev)
    md, vd = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
    pa, ma, va = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)      # simt_adam_step itself, beside it
    segs = torch.from_numpy(np.array([(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, 0, 0)], dtype=SEG_DT).view(np.uint8).copy()).to(dev)
    chunks = torch.tensor([(0, 0)], dtype=torch.int32).to(dev)
    d = L.AdamwDesc()
    d.segs, d.chunks, d.nchunks, d.chunk = segs.data_ptr(), chunks.data_ptr(), 1, CHUNK
    p, m, v = ref.exact(p0), ref.V(torch.zeros(n, dtype=ref.F64)), ref.V(torch.zeros(n, dtype=ref.F64))
    worst = 0.0
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen) * 1e-2
        gd.copy_(g)
        c = ref.constants([lr] * 4, [0.0] * 4, BETAS, step)
        assert all(float(x) == 1.0 for x in c["decay"])
        fill_desc(d, c, eps, 1 if step == 1 else 0)
        L.call("simt_adamw_multi", C.byref(d), ops.stream_ptr())
        L.call("simt_adam_step", pa.data_ptr(), gd.data_ptr(), ma.data_ptr(), va.data_ptr(), n, lr, BETAS[0], BETAS[1], eps, step, ops.stream_ptr())
        torch.cuda.synchronize()
        p, m, v = _adam_step_ref(p, ref.exact(g), m, v, lr, BETAS[0], BETAS[1], eps, step)
        for name, got, want in (("p", pd, p), ("m", md, m), ("v", vd, v)):
            worst = max(worst, ref.ratio(got, want, f"Q{Q} step {step} {name}"))
        for name, got, want in (("p", pa, p), ("m", ma, m), ("v", va, v)):      # the single-tensor launch meets the same bar on the same data
            ref.ratio(got, want, f"simt_adam_step Q{Q} step {step} {name}")
    print(f"simt_adamw_multi as simt_adam_step, {Q} x {Cn}: worst |stored - float64| / bound = {worst:.3f} (allowed {ref.SLACK})")
