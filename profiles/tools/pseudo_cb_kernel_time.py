"""Kernel times of the class-balanced pseudo-label launches (simt_pseudo_conf_u8 / simt_pseudo_conf2_u8) at 1 x 1024 x 2048, C = 19,
against the confidence-mode launch of another build of the library (the parent commit's):

    python profiles/tools/pseudo_cb_kernel_time.py <parent tree>/simt_amd/libsimt_hip.so [OUT_DIR]

Inputs: low-res maps of the export's geometry (65 x 129 probabilities; 64 x 128 logits, in-model size 512 x 1024) -- `spread`: softmax of
random logits; `hot60`: 60 % of the low-res pixels of the upper half are class 0 at exactly 1.0; `allhot`: all of them.  Device events
around 40 launches, the variants alternating, 7 rounds after a warm-up; median (min, max) per launch."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from simt_amd import _lib as L    # noqa: E402
from simt_amd import ops          # noqa: E402

OUT = sys.argv[2] if len(sys.argv) > 2 else "."
os.makedirs(OUT, exist_ok=True)
dev = torch.device("cuda:0")
new = L.load()
parent = C.CDLL(sys.argv[1])
for name in ("simt_pseudo_label_u8", "simt_pseudo_label2_u8"):
    getattr(parent, name).restype, getattr(parent, name).argtypes = L.SIGNATURES[name]
Cn, H, W = 19, 1024, 2048
P = H * W
N, ROUNDS = 40, 7
stream = ops.stream_ptr()
out = torch.zeros(P, device=dev, dtype=torch.uint8)
counts = torch.zeros(Cn + 1, device=dev, dtype=torch.int64)
hist = torch.zeros(Cn, 256, device=dev, dtype=torch.int64)
thr = np.full(Cn, 0.8, np.float32)
thr_cb = np.array([((37 * c) % 256) / 256 for c in range(Cn)], np.float32)


def inputs(family, kind):
    g = torch.Generator().manual_seed(3)
    h, w, ld = (65, 129, 22) if family == 1 else (64, 128, 24)
    lg = torch.zeros(1, h, w, ld)
    lg[..., :Cn] = torch.randn(1, h, w, Cn, generator=g) * 2.5
    if kind != "spread":
        hot = torch.rand(h, w, generator=g) < (0.6 if kind == "hot60" else 2.0)
        if kind == "hot60":
            hot[h // 2:] = False
        row = torch.zeros(ld)
        row[0] = 60.0                                   # softmax: class 0 at exactly 1.0
        lg[0][hot] = row
    lg = lg.to(dev)
    if family == 2:
        return lg.reshape(-1, ld).contiguous(), (h, w, ld, 512, 1024)
    prob = torch.zeros_like(lg)
    ops.softmax_rows(lg, ld, prob, ld, h * w, Cn)
    return prob, (h, w, ld)


def check(rc):
    if rc != 0:
        raise RuntimeError(f"call failed: {rc}")


def variants(family, src, geo):
    p = src.data_ptr()
    if family == 1:
        old = lambda lib: check(lib.simt_pseudo_label_u8(p, *geo, None, 0, 0, 0, 1, H, W, Cn, 1, 0.8, out.data_ptr(), counts.data_ptr(), stream))   # noqa: E731
        cb = lambda t, o, c, hh: check(new.simt_pseudo_conf_u8(p, *geo, 1, H, W, Cn, t, o, c, hh, stream))   # noqa: E731
    else:
        old = lambda lib: check(lib.simt_pseudo_label2_u8(p, *geo, None, 0, 0, 0, 0, 0, 1, H, W, Cn, 1, 0.8, out.data_ptr(), counts.data_ptr(), stream))   # noqa: E731
        cb = lambda t, o, c, hh: check(new.simt_pseudo_conf2_u8(p, *geo, 1, H, W, Cn, t, o, c, hh, stream))   # noqa: E731
    return {
        "parent mode 1": lambda: old(parent),
        "this mode 1": lambda: old(new),
        "statistics": lambda: cb(None, None, None, hist.data_ptr()),
        "labels thr 0.8": lambda: cb(thr.ctypes.data, out.data_ptr(), counts.data_ptr(), None),
        "labels per class": lambda: cb(thr_cb.ctypes.data, out.data_ptr(), counts.data_ptr(), None),
        "combined": lambda: cb(thr_cb.ctypes.data, out.data_ptr(), counts.data_ptr(), hist.data_ptr()),
    }


def time_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / N


res = {}
lines = []
for family in (1, 2):
    for kind in ("spread", "hot60", "allhot"):
        src, geo = inputs(family, kind)
        vs = variants(family, src, geo)
        hist.zero_()
        vs["statistics"]()
        torch.cuda.synchronize()
        hh = hist.cpu().numpy()
        assert hh.sum() == P
        top = float(hh.max()) / P
        nz = int((hh > 0).sum())
        # the mode-1 labels of the parent's library and of this one agree byte for byte
        vs["parent mode 1"]()
        ref = out.clone()
        vs["this mode 1"]()
        assert torch.equal(ref, out)
        vs["labels thr 0.8"]()                         # conf >= 0.8 against conf > 0.8: equal unless a conf is exactly 0.8f
        same = float((ref == out).float().mean())
        for _ in range(3):
            for fn in vs.values():
                for _ in range(5):
                    fn()
        torch.cuda.synchronize()
        t = {k: [] for k in vs}
        for _ in range(ROUNDS):
            for k, fn in vs.items():
                t[k].append(time_us(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
        res[f"family{family}/{kind}"] = {"median_us": med, "min_max_us": spread, "largest_word_share": top, "nonzero_bins": nz, "labels_equal_share": same}
        lines.append(f"family {family} ({'simt_pseudo_conf_u8' if family == 1 else 'simt_pseudo_conf2_u8'}), input {kind}: "
                     f"largest histogram word holds {100 * top:.1f} % of the pixels, {nz} non-zero bins")
        for k in vs:
            lines.append(f"    {k:18s} {med[k]:8.1f} us   (min {spread[k][0]:.1f}, max {spread[k][1]:.1f})   x{med[k] / med['parent mode 1']:.3f} of the parent's mode 1")
        print("\n".join(lines[-7:]), flush=True)
json.dump(res, open(os.path.join(OUT, "cb_kernel_time.json"), "w"), indent=1)
open(os.path.join(OUT, "cb_kernel_time.txt"), "w").write("\n".join(lines) + "\n")
