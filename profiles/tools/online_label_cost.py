#!/usr/bin/env python3
"""Cost of online labels (simt_amd/online_labels.py, simt_online_label) -> profiles/online_labels.txt.  MEASUREMENT ONLY.

    python profiles/tools/online_label_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/online_label_cost.py step --model v2|vgg [--online-labels T] [--steps 30] [--warmup 8] [--repo TREE]

kernel  simt_online_label beside the composition that yields the same bytes from the launches that existed before it -- simt_pseudo_label_u8
        mode 1 (DeepLabv3: simt_pseudo_label2_u8 mode 1 at hia = H, wia = W), then the uint8 -> int64 widening copy (torch's copy_) -- at
        B = 4, 97 x 97 -> 768 x 768 (DeepLab-v2), B = 8, 65 x 65 -> 512 x 512 (VGG16) and B = 4, 32 x 64 -> 512 x 1024 (DeepLabv3), C = 19,
        ld = 24, threshold 0.968.  Device events over `--reps` back-to-back launches after a warm-up, six rotating output buffers (the label
        map of a training step is rewritten with a whole step's traffic in between), `--rounds` rounds in alternating order; microseconds per
        launch.  The input is softmax(randn * 3) / randn * 3: the low-res map stays in the on-die cache, as behind the teacher's forward.
step    The warm-up trainer of DeepLab-v2 R-101 (B = 4, 768 x 768) or DeepLab-VGG16 (B = 8, 512 x 512), bf16, constructor init, on a resident
        synthetic batch: `--steps` steps after `--warmup`, wall-clock milliseconds per step around a device synchronise, one JSON line.
        --online-labels T passes the keyword (a fixed teacher) and also times the teacher's eval-mode forward alone, serially (the plan the
        SimT step's frozen forward runs at that geometry); --repo TREE imports another checkout (the parent commit's, which has no such
        keyword).  One process per run; the driver alternates parent / flag off / flag on.
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
    print(f"C = {CN}, ld = {LD}, threshold {THR}; {a.reps} launches per timing over {NBUF} rotating output buffers, {a.rounds} rounds in "
          "alternating order; us per launch")
    for name, fam, B, h, w, H, W in CASES:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B * h * w, LD, generator=g) * 3
        if fam == 0:
            x[:, :CN] = torch.softmax(x[:, :CN], 1)
        x = x.to(dev)
        lab64 = [torch.zeros(B, H, W, dtype=torch.int64, device=dev) for _ in range(NBUF)]
        lab8 = [torch.zeros(B, H, W, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
        counts = torch.zeros(CN + 1, dtype=torch.int64, device=dev)
        descs = []
        for t in lab64:
            d = L.OnlineLabelDesc()
            d.fix, d.label, d.counts = x.data_ptr(), t.data_ptr(), counts.data_ptr()
            d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, LD, H, W, CN, fam, THR
            descs.append(d)

        def online(i):
            L.call("simt_online_label", C.byref(descs[i % NBUF]), ops.stream_ptr())

        def export(i):
            o = lab8[i % NBUF]
            if fam == 0:
                L.call("simt_pseudo_label_u8", ops._p(x), h, w, LD, None, 0, 0, 0, B, H, W, CN, 1, THR, ops._p(o), ops._p(counts), ops.stream_ptr())
            else:
                L.call("simt_pseudo_label2_u8", ops._p(x), h, w, LD, H, W, None, 0, 0, 0, 0, 0, B, H, W, CN, 1, THR, ops._p(o), ops._p(counts),
                       ops.stream_ptr())

        def widen(i):
            lab64[i % NBUF].copy_(lab8[i % NBUF])

        def both(i):
            export(i)
            widen(i)
        fns = [("simt_online_label", online), ("export kernel (uint8)", export), ("widening copy", widen), ("composition (both)", both)]

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
        online(0)
        both(0)
        torch.cuda.synchronize()
        same = bool(torch.equal(lab64[0], lab8[0].long()))
        kept = float((lab64[0] != 255).float().mean())
        print(f"\n{name}: {B * H * W * 8 / 1e6:.1f} MB of labels, {kept:.3f} of the pixels kept, equal to the composition's bytes: {same}")
        print(f"{'launch':>24}  " + " ".join(f"{'':>7}" for _ in range(a.rounds - 1)) + f"{'rounds':>7} {'mean':>8}")
        for n, _f in fns:
            print(f"{n:>24}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f" {sum(res[n]) / len(res[n]):8.1f}")
        del lab64, lab8


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
    out = {"model": a.model, "tree": "parent" if a.repo else "this", "online_labels": a.online_labels, "steps": a.steps,
           "ms_per_step": (time.perf_counter() - t0) * 1e3 / a.steps, "images_per_s": B * a.steps / (time.perf_counter() - t0)}
    losses = tr.losses()
    if "labelled" in losses:
        out["labelled"] = losses["labelled"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _pass in range(2):          # the first pass warms up
            e0.record()
            for _ in range(10):
                tr._fix_fwd.run()
            e1.record()
            torch.cuda.synchronize()
        out["teacher_forward_ms"] = e0.elapsed_time(e1) / 10
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    s = sub.add_parser("step")
    s.add_argument("--model", choices=["v2", "vgg"], required=True)
    s.add_argument("--online-labels", type=float, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=8)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
