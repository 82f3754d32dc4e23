"""The chunk size of a multi-tensor launch changes no bit (csrc/multi_sweep.h; simt_sgd_multi, simt_adamw_multi, simt_ema_multi,
simt_bn_fold_multi).  Per-element arithmetic does not depend on which workgroup serves an element or at which width it is loaded, so the
same seeded data launched with different `chunk` values must leave identical 32-bit words in every output -- no tolerance.  The other kernel
tests launch at chunk = 65536 only; here chunk = 1024 puts chunk starts inside segments, and chunk = 1022 (4088 bytes = 8 mod 16) makes
every second chunk start off 16-byte alignment, so one segment mixes the 16-byte and the dword path.  Segments of 1028 and 2052 elements
are 257 and 513 quads: the edges of the EMA's pair loop.  The last segment's pointers all start 4 bytes past a 16-byte boundary.  The
tables are built by hand: they pin the C ABI independently of simt_amd/multi_tensor.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from simt_amd import _lib as L
from simt_amd import optimizer as opt

pytestmark = pytest.mark.gpu
NS = [1, 3, 4, 5, 1021, 1022, 1023, 1028, 2048, 2052, 3 * 1022 + 1, 2052]
OFFS = [0] * (len(NS) - 1) + [1]          # elements past a 16-byte boundary
GUARD = 8                                 # sentinel words on either side of every segment
SENTINEL = 0x5EADBEEF
CHUNKS = (65536, 1024, 1022)


class _Arena:
    """One int32 device buffer of sentinels per name with the segments NS planted in it, seeded: two arenas of one seed hold the same words."""

    def __init__(self, dev, names, seed, positive=()):
        rng = np.random.default_rng(seed)
        self.starts, cur = [], GUARD
        for n, off in zip(NS, OFFS):
            self.starts.append(cur + off)
            cur = (cur + off + n + GUARD + 3) // 4 * 4
        self.mask = np.zeros(cur, dtype=bool)
        for s, n in zip(self.starts, NS):
            self.mask[s:s + n] = True
        self.init, self.buf = {}, {}
        for name in names:
            x = rng.standard_normal(int(self.mask.sum())).astype(np.float32)
            host = np.full(cur, SENTINEL, dtype=np.uint32)
            host[self.mask] = (np.abs(x) + np.float32(0.5) if name in positive else x).view(np.uint32)
            self.init[name] = host
            self.buf[name] = torch.from_numpy(host.view(np.int32)).to(dev)
            assert self.buf[name].data_ptr() % 16 == 0
        assert [self.ptr(names[0], i) % 16 for i in range(len(NS))] == [4 * o for o in OFFS]

    def ptr(self, name, i):
        return self.buf[name].data_ptr() + 4 * self.starts[i]

    def words(self, name):
        return self.buf[name].cpu().numpy().view(np.uint32)


def _pairs(dev, chunk):
    pairs = [(si, ci) for si, n in enumerate(NS) for ci in range((n + chunk - 1) // chunk)]
    return torch.tensor(pairs, dtype=torch.int32, device=dev)


def _table(dev, recs, dtype, d, chunk):
    """Upload the records and the pairs for `chunk`, fill the table fields of d; -> what must stay alive."""
    segs = torch.from_numpy(np.array(recs, dtype=dtype).view(np.uint8).copy()).to(dev)
    pairs = _pairs(dev, chunk)
    d.segs, d.chunks, d.nchunks, d.chunk = segs.data_ptr(), pairs.data_ptr(), pairs.shape[0], chunk
    return segs, pairs


def _launch(name, d):
    L.call(name, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _same_everywhere(runs, outputs, inputs, what):
    """runs: one arena per chunk size, in the order of the chunk sizes given."""
    base = runs[0]
    for a in runs:
        for name in outputs:
            w = a.words(name)
            assert bool((w[~a.mask] == SENTINEL).all()), f"{what}: a guard band of {name} was written"
            assert np.array_equal(w, base.words(name)), f"{what}: {name} differs between chunk sizes in {int((w != base.words(name)).sum())} words"
        for name in inputs:
            assert np.array_equal(a.words(name), a.init[name]), f"{what}: the input {name} was written"


SGD_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("mult", "<i4"), ("group", "<i4")])
ADAMW_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("pad", "<i4")])
EMA_DT = np.dtype([("w", "<u8"), ("e", "<u8"), ("n", "<i8")])


def test_sgd_multi_chunk_size_changes_no_bit(dev):
    """p and buf at mult 1 and 3, first_step 1 then 0, weight decay and momentum on."""
    runs, descs, keep = [], [], []
    for chunk in CHUNKS:
        a = _Arena(dev, ("p", "g", "buf"), seed=11)
        d = L.SgdDesc()
        keep.append(_table(dev, [(a.ptr("p", i), a.ptr("g", i), a.ptr("buf", i), n, (1, 3)[i & 1], (i >> 1) & 1) for i, n in enumerate(NS)],
                           SGD_DT, d, chunk))
        d.lr[0], d.lr[1], d.wd[0], d.wd[1], d.momentum, d.dampening = 0.1, 1.0, 5e-4, 5e-4, 0.9, 0.0
        runs.append(a), descs.append(d)
    for first in (1, 0):
        for d in descs:
            d.first_step = first
            _launch("simt_sgd_multi", d)
        _same_everywhere(runs, ("p", "buf"), ("g",), f"first_step {first}")
        for name in ("p", "buf"):
            assert (runs[0].words(name) != runs[0].init[name])[runs[0].mask].mean() > 0.99, f"{name} did not move"


def test_adamw_multi_chunk_size_changes_no_bit(dev):
    """p, m and v, first_step 1 then 0 (the first creates the moments from whatever the buffers hold)."""
    runs, descs, keep = [], [], []
    for chunk in CHUNKS:
        a = _Arena(dev, ("p", "g", "m", "v"), seed=12)
        d = L.AdamwDesc()
        keep.append(_table(dev, [(a.ptr("p", i), a.ptr("g", i), a.ptr("m", i), a.ptr("v", i), n, i & 3, 0) for i, n in enumerate(NS)],
                           ADAMW_DT, d, chunk))
        d.eps = 1e-8
        runs.append(a), descs.append(d)
    for t in (1, 2):
        step_size, decay, b1, b2, omb1, omb2, bc2s = opt.adamw_constants((6e-5, 6e-4, 6e-5, 6e-4), (0.01, 0.01, 0.0, 0.0), (0.9, 0.999), t)
        for d in descs:
            for i in range(4):
                d.step_size[i], d.decay[i] = step_size[i], decay[i]
            d.beta1, d.beta2, d.omb1, d.omb2, d.bc2s, d.first_step = b1, b2, omb1, omb2, bc2s, int(t == 1)
            _launch("simt_adamw_multi", d)
        _same_everywhere(runs, ("p", "m", "v"), ("g",), f"step {t}")
        for name in ("p", "m", "v"):
            assert (runs[0].words(name) != runs[0].init[name])[runs[0].mask].mean() > 0.99, f"{name} did not move"


@pytest.mark.parametrize("omd", [1.0, 0.5], ids=["copy", "half"])
def test_ema_multi_chunk_size_changes_no_bit(dev, omd):
    runs, keep = [], []
    for chunk in CHUNKS:
        a = _Arena(dev, ("w", "e"), seed=13)
        d = L.EmaDesc()
        keep.append(_table(dev, [(a.ptr("w", i), a.ptr("e", i), n) for i, n in enumerate(NS)], EMA_DT, d, chunk))
        d.omd = omd
        _launch("simt_ema_multi", d)
        runs.append(a)
    _same_everywhere(runs, ("e",), ("w",), f"omd {omd}")
    assert (runs[0].words("e") != runs[0].init["e"])[runs[0].mask].mean() > 0.99, "e did not move"
    if omd == 1.0:
        assert np.array_equal(runs[0].words("e")[runs[0].mask], runs[0].init["w"][runs[0].mask])


def test_bn_fold_multi_chunk_size_changes_no_bit(dev):
    """scale and shift at 256 and 100 channels per workgroup."""
    runs, keep = [], []
    for chunk in (256, 100):
        a = _Arena(dev, ("gamma", "beta", "rm", "rv", "scale", "shift"), seed=14, positive=("rv",))
        host = (L.BnFoldSeg * len(NS))()
        for i, (s, n) in enumerate(zip(host, NS)):
            s.gamma, s.beta, s.running_mean, s.running_var = a.ptr("gamma", i), a.ptr("beta", i), a.ptr("rm", i), a.ptr("rv", i)
            s.scale, s.shift, s.C = a.ptr("scale", i), a.ptr("shift", i), n
        segs = torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).copy()).to(dev)
        pairs = _pairs(dev, chunk)
        d = L.BnFoldDesc()
        d.segs, d.segs_host, d.chunks = segs.data_ptr(), host, pairs.data_ptr()
        d.nsegs, d.nchunks, d.chunk, d.eps = len(NS), pairs.shape[0], chunk, 1e-5
        keep.append((host, segs, pairs))
        _launch("simt_bn_fold_multi", d)
        runs.append(a)
    _same_everywhere(runs, ("scale", "shift"), ("gamma", "beta", "rm", "rv"), "fold")
    for name in ("scale", "shift"):
        assert (runs[0].words(name) != runs[0].init[name])[runs[0].mask].mean() > 0.99, f"{name} did not move"
