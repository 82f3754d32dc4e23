#!/usr/bin/env python3
"""Cost of the mix behind the teacher (online_mix) -> profiles/online_mix.txt.  MEASUREMENT ONLY.

    python profiles/tools/online_mix_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/online_mix_cost.py step --model v2|vgg [--online-mix P] [--steps 20] [--warmup 6] [--repo TREE]

kernel  At B = 4, 97 x 97 -> 768 x 768 (DeepLab-v2) and B = 8, 65 x 65 -> 512 x 512 (VGG16), C = 19, ld = 24, threshold 0.5, in ONE run:
        (1) simt_online_label_u8 beside simt_online_label + simt_label_presence (the composition that yields the same labels and presence),
        (2) simt_class_mix_u8 beside simt_class_mix into a staging pair + the device copies of image and labels into the buffers the trainer
            reads (torch's copy_).
        Device events over `--reps` back-to-back launches after a warm-up, `--rounds` rounds in alternating order; microseconds per launch.
        The teacher's map is softmax(randn * 3) at low resolution: the labels come in patches of the resampling factor; 0.18 of the
        pixels pass the threshold, the rest are 255.
step    The warm-up trainer of DeepLab-v2 R-101 (B = 4, 768 x 768) or DeepLab-VGG16 (B = 8, 512 x 512), bf16, constructor init, with
        online_labels = 0 (the untrained teacher is confident nowhere; above 0 keeps every pixel, so the mix has classes to paste) on a resident
        synthetic batch: `--steps` steps after `--warmup`, wall-clock milliseconds per step around a device
        synchronise, one JSON line.  --online-mix P passes the keyword; --repo TREE imports another checkout (the parent commit's, which has
        no such keyword).  One process per run; the driver rotates the order of parent / keyword off / keyword on from round to round.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("DeepLab-v2, B = 4, 97 x 97 -> 768 x 768", 0, 4, 97, 97, 768, 768),
         ("DeepLab-VGG16, B = 8, 65 x 65 -> 512 x 512", 0, 8, 65, 65, 512, 512)]
CN, LD, THR = 19, 24, 0.5


def _timed(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _table(fns, rounds, timed):
    res = {n: [] for n, _f in fns}
    for r in range(rounds):
        for n, f in (fns if r % 2 == 0 else fns[::-1]):
            res[n].append(timed(f))
    print(f"{'launch':>44}  " + " ".join(f"{'':>7}" for _ in range(rounds - 1)) + f"{'rounds':>7} {'mean':>8}")
    for n, _f in fns:
        print(f"{n:>44}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f" {sum(res[n]) / len(res[n]):8.1f}")


def kernel(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd import ops
    from simt_amd.data import class_mix
    dev = torch.device("cuda:0")
    lib = L.load()
    print(f"C = {CN}, ld = {LD}, threshold {THR}; {a.reps} launches per timing, {a.rounds} rounds in alternating order; us per launch")
    for name, fam, B, h, w, H, W in CASES:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B * h * w, LD, generator=g) * 3
        x[:, :CN] = torch.softmax(x[:, :CN], 1)
        x = x.to(dev)
        st = ops.stream_ptr()
        lab64, lab8 = torch.zeros(B, H, W, dtype=torch.int64, device=dev), torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        counts = torch.zeros(CN + 1, dtype=torch.int64, device=dev)
        part64 = torch.zeros(B, L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)
        d = L.OnlineLabelDesc()
        d.fix, d.label, d.counts = x.data_ptr(), lab64.data_ptr(), counts.data_ptr()
        d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, h, w, LD, H, W, CN, fam, THR
        u = L.OnlineLabelU8Desc()
        u.fix, u.lab8, u.counts = x.data_ptr(), lab8.data_ptr(), counts.data_ptr()
        u.B, u.h, u.w, u.ld, u.H, u.W, u.C, u.family, u.threshold = B, h, w, LD, H, W, CN, fam, THR
        rows = lib.simt_online_label_parts(C.byref(u))
        part8 = torch.zeros(B, rows, dtype=torch.int32, device=dev)
        u.part = part8.data_ptr()

        def label_u8():
            L.call("simt_online_label_u8", C.byref(u), st)

        def label_i64():
            L.call("simt_online_label", C.byref(d), st)

        def presence():
            L.call("simt_label_presence", ops._p(lab64), B, H * W, CN, ops._p(part64), st)

        def label_both():
            label_i64()
            presence()
        label_u8()
        label_both()
        torch.cuda.synchronize()
        same = bool(torch.equal(lab64, lab8.long()))
        words8 = np.bitwise_or.reduce(part8.cpu().numpy().view(np.uint32), axis=1)
        words64 = np.bitwise_or.reduce(part64.cpu().numpy().view(np.uint32), axis=1)
        kept = float((lab8 != 255).float().mean())
        print(f"\n{name}: {B * H * W / 1e6:.2f} Mpx, {kept:.3f} of the pixels kept, {rows} rows of presence words; labels equal: {same}, "
              f"presence equal: {bool((words8 == words64).all())}")
        _table([("simt_online_label_u8", label_u8), ("simt_online_label", label_i64), ("simt_label_presence", presence),
                ("simt_online_label + simt_label_presence", label_both)], a.rounds, lambda f: _timed(torch, f, a.reps))

        img = torch.randn(B, 3, H, W, generator=g).to(dev)
        x_in, label = torch.zeros_like(img), torch.zeros_like(lab64)
        sx, sl = torch.zeros_like(img), torch.zeros_like(lab64)
        apply, rank = class_mix.draw_batch(class_mix.generator(0, 0), B, CN, 1.0)
        table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
        table[:B, :CN] = rank
        m8, m64 = L.ClassMixU8Desc(), L.ClassMixDesc()
        m8.x, m8.lab8, m8.x_out, m8.lab_out, m8.part = img.data_ptr(), lab8.data_ptr(), x_in.data_ptr(), label.data_ptr(), part8.data_ptr()
        m8.B, m8.h, m8.w, m8.n_classes, m8.rows = B, H, W, CN, rows
        m64.x, m64.lab, m64.x_out, m64.lab_out, m64.part = img.data_ptr(), lab64.data_ptr(), sx.data_ptr(), sl.data_ptr(), part64.data_ptr()
        m64.B, m64.h, m64.w, m64.n_classes = B, H, W, CN
        for m in (m8, m64):
            C.memmove(m.rank, table.ctypes.data, table.nbytes)
            for i in range(B):
                m.partner[i], m.apply[i] = (i + 1) % B, 1

        def mix_u8():
            L.call("simt_class_mix_u8", C.byref(m8), st)

        def mix_i64():
            L.call("simt_class_mix", C.byref(m64), st)

        def copies():
            x_in.copy_(sx)
            label.copy_(sl)

        def mix_both():
            mix_i64()
            copies()
        mix_u8()
        torch.cuda.synchronize()
        got = (x_in.clone(), label.clone())
        mix_both()
        torch.cuda.synchronize()
        same = bool(torch.equal(got[0].view(torch.int32), x_in.view(torch.int32)) and torch.equal(got[1], label))
        pasted = float((label != lab64).float().mean())
        print(f"mix: apply = 1 for every item, {pasted:.3f} of the labels changed; equal to the composition's bytes: {same}")
        _table([("simt_class_mix_u8", mix_u8), ("simt_class_mix (staging pair)", mix_i64), ("copies into x_in and label", copies),
                ("simt_class_mix + copies", mix_both)], a.rounds, lambda f: _timed(torch, f, a.reps))
        del img, x_in, label, sx, sl, lab64, lab8


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
    kw = {"online_labels": 0.0}
    if a.online_mix is not None:
        kw["online_mix"] = a.online_mix
    hp = Hyper(num_classes=19, open_classes=0, lr=2.5e-4)
    if a.model == "v2":
        B, H, W = 4, 768, 768
        tr = WarmupTrainer(ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), hp, B, H, W, device=dev, **kw)
    else:
        from simt_amd.step_single import WarmupSingleTrainer
        from simt_amd.tools.trainV2_simt import single_model_state
        B, H, W = 8, 512, 512
        tr = WarmupSingleTrainer("vgg", single_model_state("DeepLabVGG", 19), hp, B, H, W, device=dev, **kw)
    img, _lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    for _ in range(a.warmup):
        tr.step(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(img)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"model": a.model, "tree": "parent" if a.repo else "this", "online_mix": a.online_mix, "steps": a.steps,
           "ms_per_step": dt * 1e3 / a.steps, "images_per_s": B * a.steps / dt, "labelled": tr.losses()["labelled"]}
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
    s.add_argument("--online-mix", type=float, default=None)
    s.add_argument("--steps", type=int, default=20)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
