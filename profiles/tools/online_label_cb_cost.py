#!/usr/bin/env python3
"""Cost of class-balanced online labels (simt_online_label_cb / simt_class_thresholds) -> profiles/online_labels_cb.txt.
MEASUREMENT ONLY.

    python profiles/tools/online_label_cb_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/online_label_cb_cost.py step --model v2|vgg [--online-labels T] [--balanced P] [--steps 30] [--warmup 8] [--repo TREE]

kernel  The fused label launch beside (a) simt_online_label alone and (b) the two launches that yield the same labels and the same
        histogram without it: simt_online_label, then simt_pseudo_conf_u8 / simt_pseudo_conf2_u8 statistics only (hist, no out) -- the gather
        runs twice there.  Then simt_class_thresholds alone, on the histogram the label launch left (it zeroes it: every timed launch after the
        first reads zeros, the same 2 KB per class).  Sizes, input, buffers, events and the alternating rounds: those of
        profiles/tools/online_label_cost.py, and a second, confident input (randn * 12: most pixels in the top bins, as a trained teacher's --
        the histogram's flush issues one global atomic per OCCUPIED bin and block); the device thresholds are 0.968 for every class, so (a), (b) and the fused launch write the same
        labels up to the one pixel in 2^24 whose confidence EQUALS the threshold.
step    As online_label_cost.py step; --balanced P adds online_labels_balanced (momentum: the default).  --repo TREE imports another
        checkout (the parent commit's).  One process per run; the driver alternates parent / --online-labels / --online-labels --balanced.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("DeepLab-v2, B = 4, 97 x 97 -> 768 x 768", 0, 4, 97, 97, 768, 768),
         ("DeepLab-VGG16, B = 8, 65 x 65 -> 512 x 512", 0, 8, 65, 65, 512, 512),
         ("DeepLabv3, B = 4, 32 x 64 -> 512 x 1024", 1, 4, 32, 64, 512, 1024)]
CN, LD, THR, NBUF = 19, 24, 0.968, 6


def kernel(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    from simt_amd import ops
    dev = torch.device("cuda:0")
    print(f"C = {CN}, ld = {LD}, threshold {THR} for every class; {a.reps} launches per timing over {NBUF} rotating label buffers, {a.rounds} "
          "rounds in alternating order; us per launch")
    for name, fam, B, h, w, H, W, scale in [c + (s,) for s in a.scales for c in CASES]:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B * h * w, LD, generator=g) * scale
        if fam == 0:
            x[:, :CN] = torch.softmax(x[:, :CN], 1)
        x = x.to(dev)
        lab = [torch.zeros(B, H, W, dtype=torch.int64, device=dev) for _ in range(NBUF)]
        counts = torch.zeros(CN + 1, dtype=torch.int64, device=dev)
        hist = torch.zeros(CN, L.CONF_BINS, dtype=torch.int64, device=dev)
        thr = torch.full((CN,), THR, device=dev)
        one, cb = [], []
        for t in lab:
            d = L.OnlineLabelDesc()
            d.fix, d.label, d.counts = x.data_ptr(), t.data_ptr(), counts.data_ptr()
            d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, LD, H, W, CN, fam, THR
            one.append(d)
            d = L.OnlineLabelCbDesc()
            d.fix, d.label, d.counts, d.hist, d.thr = x.data_ptr(), t.data_ptr(), counts.data_ptr(), hist.data_ptr(), thr.data_ptr()
            d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family = B, h, w, LD, H, W, CN, fam
            cb.append(d)
        td = L.ClassThresholdsDesc()
        td.hist, td.thr, td.t_out, td.drop, td.C, td.cap, td.omd = hist.data_ptr(), thr.data_ptr(), None, 0.5, CN, THR, 0.1

        def fused(i):
            L.call("simt_online_label_cb", C.byref(cb[i % NBUF]), ops.stream_ptr())

        def alone(i):
            L.call("simt_online_label", C.byref(one[i % NBUF]), ops.stream_ptr())

        def stats(i):
            if fam == 0:
                L.call("simt_pseudo_conf_u8", ops._p(x), h, w, LD, B, H, W, CN, None, None, None, ops._p(hist), ops.stream_ptr())
            else:
                L.call("simt_pseudo_conf2_u8", ops._p(x), h, w, LD, H, W, B, H, W, CN, None, None, None, ops._p(hist), ops.stream_ptr())

        def both(i):
            alone(i)
            stats(i)

        def thresholds(i):
            L.call("simt_class_thresholds", C.byref(td), ops.stream_ptr())
        fns = [("simt_online_label_cb", fused), ("(a) simt_online_label", alone), ("statistics only", stats), ("(b) label + statistics", both),
               ("simt_class_thresholds", thresholds)]

        def timed(fn):
            for i in range(NBUF):
                fn(i)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.reps):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.reps
        res = {n: [] for n, _f in fns}
        for r in range(a.rounds):
            for n, f in (fns if r % 2 == 0 else fns[::-1]):
                res[n].append(timed(f))
        thr.fill_(THR)
        hist.zero_()
        fused(0)
        torch.cuda.synchronize()
        h_fused, l_fused = hist.clone(), lab[0].clone()
        hist.zero_()
        both(0)
        torch.cuda.synchronize()
        differ = int((l_fused != lab[0]).sum())
        kept = float((l_fused != 255).float().mean())
        bins = int((h_fused != 0).sum())
        print(f"\n{name}, input randn * {scale:g}: {bins} of {CN * L.CONF_BINS} bins occupied, {B * H * W * 8 / 1e6:.1f} MB of labels, {kept:.3f} of the pixels kept, histogram equal to the statistics launch's: "
              f"{bool(torch.equal(h_fused, hist))}, labels that differ from simt_online_label's (conf == threshold): {differ}")
        print(f"{'launch':>24}  " + " ".join(f"{'':>7}" for _ in range(a.rounds - 1)) + f"{'rounds':>7} {'mean':>8}")
        for n, _f in fns:
            print(f"{n:>24}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f" {sum(res[n]) / len(res[n]):8.1f}")
        del lab


def step(a):
    tree = os.path.abspath(a.repo) if a.repo else ROOT
    sys.path.insert(0, tree)
    import torch

    import simt_amd
    from simt_amd import model_spec as ms
    from simt_amd.step import Hyper, WarmupTrainer
    assert os.path.dirname(os.path.dirname(os.path.abspath(simt_amd.__file__))) == tree
    dev = torch.device("cuda:0")
    cd = ms.load_class_dist("bapa")
    kw = {} if a.online_labels is None else {"online_labels": a.online_labels}
    if a.balanced is not None:
        kw["online_labels_balanced"] = a.balanced
    hp = Hyper(num_classes=19, open_classes=0, lr=2.5e-4)
    if a.model == "v2":
        B, H, W = 4, 768, 768
        tr = WarmupTrainer(ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), hp, B, H, W, device=dev, **kw)
    else:
        from simt_amd.step_single import WarmupSingleTrainer
        from simt_amd.tools.trainV2_simt import single_model_state
        B, H, W = 8, 512, 512
        tr = WarmupSingleTrainer("vgg", single_model_state("DeepLabVGG", 19), hp, B, H, W, device=dev, **kw)
    img, lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    args = (img, lab) if a.online_labels is None else (img,)
    for _ in range(a.warmup):
        tr.step(*args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(*args)
    torch.cuda.synchronize()
    out = {"model": a.model, "tree": "parent" if a.repo else "this", "online_labels": a.online_labels, "balanced": a.balanced, "steps": a.steps,
           "ms_per_step": (time.perf_counter() - t0) * 1e3 / a.steps, "images_per_s": B * a.steps / (time.perf_counter() - t0)}
    losses = tr.losses()
    if "labelled" in losses:
        out["labelled"] = losses["labelled"]
    if "label_thresholds" in losses:
        out["thr_min"], out["thr_max"] = min(losses["label_thresholds"]), max(losses["label_thresholds"])
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    k.add_argument("--scales", type=float, nargs="+", default=[3.0, 12.0],
                   help="the input is randn * scale (family 0: softmaxed): 3 spreads the confidence over every bin, 12 is a confident teacher")
    s = sub.add_parser("step")
    s.add_argument("--model", choices=["v2", "vgg"], required=True)
    s.add_argument("--online-labels", type=float, default=None)
    s.add_argument("--balanced", type=float, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=8)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
