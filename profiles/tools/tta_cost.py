#!/usr/bin/env python3
"""Cost of test-time augmentation (simt_tta_label and the forwards it needs) -> profiles/tta.txt.

    python profiles/tools/tta_cost.py [--out FILE] [--pairs 3] [--reps 100] [--frames 10] [--no-eval]

Label size 1 x 1024 x 2048, C = 19, fp32.  Low-res maps of one synthetic scene (a coarse field resampled to each size + noise, so that
labels form regions and confidences spread): 65 x 129 and 81 x 161 (DeepLab-v2 at 1024 x 512 and 1280 x 640; a third scale 97 x 193),
row pitch 24; for the two-resample family 64 x 128 / 80 x 160 / 96 x 192 through virtual maps 512 x 1024 / 640 x 1280 / 768 x 1536.
  1. kernel time: every launch timed with device events over `--reps` back-to-back launches after a warm-up, the candidates of a group
     in alternating order (a b c ..., then ... c b a) `--pairs` times; microseconds per launch, every round listed.
  2. evaluation: full-depth DeepLab-v2 Evaluator at the reference's two scales, predict() of `--frames` resident frames, with and
     without flip, alternating, wall time between synchronisations; ms per image.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from simt_amd import _lib as L  # noqa: E402
from simt_amd import ops  # noqa: E402

B, H, W, C, LD = 1, 1024, 2048, 19, 24
ONE = ((65, 129), (81, 161), (97, 193))
TWO = (((64, 128), (512, 1024)), ((80, 160), (640, 1280)), ((96, 192), (768, 1536)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--no-eval", action="store_true")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    coarse = torch.randn(B, C, 9, 17, device=dev, generator=g) * 4.0

    def scene(h, w, flip):
        m = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True) + 0.7 * torch.randn(B, C, h, w, device=dev, generator=g)
        if flip:
            m = m.flip(3)
        t = torch.zeros(B, h, w, LD, device=dev)
        t[..., :C] = m.permute(0, 2, 3, 1)
        return t

    def terms(n, two=False, prob=False):
        """n terms: the scales in turn, plain then mirrored (the order of ops.tta_terms)."""
        maps = []
        for i in range(n):
            k, f = (i // 2, i % 2 == 1) if n > 3 else (i, False)
            (h, w), (hi, wi) = (TWO[k] if two else (ONE[k], (0, 0)))
            t = scene(h, w, f)
            if prob:
                ops.softmax_rows(t, LD, t, LD, B * h * w, C)
            maps.append((t, h, w, LD, hi, wi, f))
        return maps

    pred = torch.zeros(B, H, W, device=dev, dtype=torch.int32)
    lab = torch.zeros(B, H, W, device=dev, dtype=torch.uint8)
    counts = torch.zeros(C + 1, device=dev, dtype=torch.int64)
    hist = torch.zeros(C, L.CONF_BINS, device=dev, dtype=torch.int64)
    thr = np.full(C, 0.8, np.float32)
    sp = ops.stream_ptr

    def timed(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    def group(title, cands):
        say(f"\n{title}")
        res = {name: [] for name, _ in cands}
        for p in range(a.pairs):
            for name, fn in (cands if p % 2 == 0 else cands[::-1]):
                res[name].append(timed(fn))
        for name, _ in cands:
            v = res[name]
            say(f"  {name:<58s} " + "  ".join(f"{x:7.1f}" for x in v) + f"   mean {sum(v) / len(v):7.1f} us")
        return {k: sum(v) / len(v) for k, v in res.items()}

    say(f"label {B} x {H} x {W}, C = {C}, fp32, row pitch {LD}; {a.reps} launches per timing, {a.pairs} rounds in alternating order; us per launch")
    m2, m4, m6 = terms(2), terms(4), terms(6)
    (la, ha, wa, *_r), (lb, hb, wb, *_r2) = m2
    r = group("1a. one-resample family, mode 0 (logits summed, arg-max)", [
        ("simt_upsample_sum_argmax, 2 maps (int32)", lambda: L.call("simt_upsample_sum_argmax", ops._p(la), ha, wa, LD, ops._p(lb), hb, wb, LD, B, H, W, C, ops._p(pred), sp())),
        ("simt_pseudo_label_u8 mode 0, 2 maps (uint8 + counts)", lambda: L.call("simt_pseudo_label_u8", ops._p(la), ha, wa, LD, ops._p(lb), hb, wb, LD, B, H, W, C, 0, 0.0, ops._p(lab), ops._p(counts), sp())),
        ("simt_tta_label, the same 2 terms -> pred", lambda: ops.tta_label(m2, B=B, H=H, W=W, Cn=C, mode=0, pred=pred)),
        ("simt_tta_label, the same 2 terms -> out + counts", lambda: ops.tta_label(m2, B=B, H=H, W=W, Cn=C, mode=0, out=lab, counts=counts)),
        ("simt_tta_label, 4 terms (2 scales x flip) -> pred", lambda: ops.tta_label(m4, B=B, H=H, W=W, Cn=C, mode=0, pred=pred)),
        ("simt_tta_label, 6 terms (3 scales x flip) -> pred", lambda: ops.tta_label(m6, B=B, H=H, W=W, Cn=C, mode=0, pred=pred)),
    ])
    old, new = r["simt_upsample_sum_argmax, 2 maps (int32)"], r["simt_tta_label, the same 2 terms -> pred"]
    say(f"  simt_tta_label on the old kernel's two terms: {100 * (new / old - 1):+.1f} % against simt_upsample_sum_argmax")
    t2, t4, t6 = terms(2, two=True), terms(4, two=True), terms(6, two=True)
    (la2, ha2, wa2, _l, hia, wia, _f), (lb2, hb2, wb2, _l2, hib, wib, _f2) = t2
    r = group("1b. two-resample family (DeepLabv3), mode 0", [
        ("simt_upsample2_sum_argmax, 2 maps", lambda: L.call("simt_upsample2_sum_argmax", ops._p(la2), ha2, wa2, LD, hia, wia, ops._p(lb2), hb2, wb2, LD, hib, wib, B, H, W, C, ops._p(pred), sp())),
        ("simt_tta_label, the same 2 terms -> pred", lambda: ops.tta_label(t2, B=B, H=H, W=W, Cn=C, mode=0, pred=pred)),
        ("simt_tta_label, 4 terms -> pred", lambda: ops.tta_label(t4, B=B, H=H, W=W, Cn=C, mode=0, pred=pred)),
        ("simt_tta_label, 6 terms -> pred", lambda: ops.tta_label(t6, B=B, H=H, W=W, Cn=C, mode=0, pred=pred)),
    ])
    old, new = r["simt_upsample2_sum_argmax, 2 maps"], r["simt_tta_label, the same 2 terms -> pred"]
    say(f"  simt_tta_label on the old kernel's two terms: {100 * (new / old - 1):+.1f} % against simt_upsample2_sum_argmax")
    p1, p2, p4 = terms(1, prob=True), terms(2, prob=True), terms(4, prob=True)
    (pa, pha, pwa, *_r3), = p1
    group("1c. mode 1 (probabilities averaged), labels with per-class thresholds 0.8 + counts", [
        ("simt_pseudo_conf_u8, 1 map, labels", lambda: L.call("simt_pseudo_conf_u8", ops._p(pa), pha, pwa, LD, B, H, W, C, thr.ctypes.data, ops._p(lab), ops._p(counts), None, sp())),
        ("simt_tta_label mode 1, 1 term, labels", lambda: ops.tta_label(p1, B=B, H=H, W=W, Cn=C, mode=1, thr=thr, out=lab, counts=counts)),
        ("simt_tta_label mode 1, 2 terms, labels", lambda: ops.tta_label(p2, B=B, H=H, W=W, Cn=C, mode=1, thr=thr, out=lab, counts=counts)),
        ("simt_tta_label mode 1, 4 terms, labels", lambda: ops.tta_label(p4, B=B, H=H, W=W, Cn=C, mode=1, thr=thr, out=lab, counts=counts)),
    ])
    group("1d. mode 1, confidence histogram only", [
        ("simt_pseudo_conf_u8, 1 map, histogram", lambda: L.call("simt_pseudo_conf_u8", ops._p(pa), pha, pwa, LD, B, H, W, C, None, None, None, ops._p(hist), sp())),
        ("simt_tta_label mode 1, 1 term, histogram", lambda: ops.tta_label(p1, B=B, H=H, W=W, Cn=C, mode=1, hist=hist)),
        ("simt_tta_label mode 1, 2 terms, histogram", lambda: ops.tta_label(p2, B=B, H=H, W=W, Cn=C, mode=1, hist=hist)),
        ("simt_tta_label mode 1, 4 terms, histogram", lambda: ops.tta_label(p4, B=B, H=H, W=W, Cn=C, mode=1, hist=hist)),
    ])
    if a.no_eval:
        return

    from simt_amd import model_spec as ms
    from simt_amd.tools.evaluate_cityscapes import Evaluator
    st = ms.trained_like_init(ms.state_shapes(19, 3, True), seed=1234)
    xs = [torch.randn(1, 3, h, w, device=dev, generator=g) * 50 for (h, w) in ((512, 1024), (640, 1280))]
    evs = {"two scales": Evaluator(st, num_classes=19, open_classes=3, device=dev), "two scales x flip": Evaluator(st, num_classes=19, open_classes=3, device=dev, flip=True)}

    def frames(ev):
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.frames):
            ev.predict(*xs)
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3 / a.frames
    say(f"\n2. DeepLab-v2 (ResNet-101, fp32) Evaluator.predict at 1024 x 512 + 1280 x 640, {a.frames} resident frames per timing; ms per image "
        "(forwards + label launch; no decoding, no resize)")
    for ev in evs.values():
        frames(ev)
    res = {k: [] for k in evs}
    for p in range(a.pairs):
        for k in (list(evs) if p % 2 == 0 else list(evs)[::-1]):
            res[k].append(frames(evs[k]))
    for k, v in res.items():
        say(f"  {k:<20s} " + "  ".join(f"{x:7.2f}" for x in v) + f"   mean {sum(v) / len(v):7.2f} ms")


if __name__ == "__main__":
    main()
