#!/usr/bin/env python3
"""Cost of the labelled source batch (online_source) -> profiles/online_source.txt.  MEASUREMENT ONLY.

    python profiles/tools/online_source_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/online_source_cost.py step --model v2|vgg [--source] [--online-mix P] [--weighted batch|item] [--steps 30] [--warmup 6] [--repo TREE]

kernel  At B = 4, 768 x 768 and B = 8, 512 x 512, C = 19, in ONE run: simt_source_mix and simt_source_mix_items (and the presence launch over
        the B source items that runs in front of them) beside the composition that yields the same bytes with the launches that existed --
        the four copies into a 2B-item batch (the widening of the byte labels among them), simt_label_presence over 2B items and
        simt_class_mix_items -- and beside the kernel's byte floor at the copy rate a device-to-device copy of the image batch reaches in the
        same run.  Then the head passes with the [2B] table (simt_head_*_weighted_n) beside the existing weighted passes (nw = B), with a map.
        Device events over `--reps` back-to-back launches after a warm-up, `--rounds` rounds in alternating order; microseconds per launch.
step    The warm-up trainer at those sizes (DeepLab-v2 B = 4 768 x 768, VGG16 B = 8 512 x 512), bf16, constructor init, online_labels = 0 on a
        resident synthetic batch (and, with --source, a resident synthetic source pair): `--steps` steps after `--warmup`, wall-clock
        milliseconds per step around a device synchronise, one JSON line.  --repo TREE imports another checkout (the parent commit's, which
        has no such keyword).  One process per run; the driver rotates the order of parent / keyword off / keyword on from round to round.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, single, B, h, w, H, W)
CASES = [("B = 4, 768 x 768 (DeepLab-v2: 97 x 97 logits, two heads)", 0, 4, 97, 97, 768, 768),
         ("B = 8, 512 x 512 (DeepLab-VGG16: 65 x 65 logits, one head)", 1, 8, 65, 65, 512, 512)]
CN, LD = 19, 24


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
    print(f"{'launch':>52}  " + " ".join(f"{'':>7}" for _ in range(rounds - 1)) + f"{'rounds':>7} {'mean':>8}")
    for n, _f in fns:
        print(f"{n:>52}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f" {sum(res[n]) / len(res[n]):8.1f}")
    return {n: sum(v) / len(v) for n, v in res.items()}


def kernel(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd import model_spec as ms
    from simt_amd import ops
    from simt_amd.data import class_mix
    dev = torch.device("cuda:0")
    lib = L.load()
    cd = ms.load_class_dist("bapa")
    timed = lambda f: _timed(torch, f, a.reps)          # noqa: E731
    print(f"C = {CN}; {a.reps} launches per timing, {a.rounds} rounds in alternating order; us per launch")
    for name, single, B, h, w, H, W in CASES:
        st = ops.stream_ptr()
        xt, lab_t = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
        xs, labs = ms.synthetic_batch(B, H, W, cd, seed=2, device=dev)
        xt, xs, labs = xt.contiguous(), xs.contiguous(), labs.contiguous()
        lab8 = lab_t.to(torch.uint8).contiguous()
        x_out, lab_out = torch.zeros_like(xt), torch.zeros_like(labs)
        items = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        part_s = torch.zeros(B, L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)
        apply, rank = class_mix.draw_batch(class_mix.generator(0, 0), B, CN, 1.0)
        table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
        table[:B, :CN] = rank
        m = L.SourceMixDesc()
        m.xs, m.labs, m.part_s, m.xt, m.lab8 = xs.data_ptr(), labs.data_ptr(), part_s.data_ptr(), xt.data_ptr(), lab8.data_ptr()
        m.x_out, m.lab_out = x_out.data_ptr(), lab_out.data_ptr()
        m.B, m.h, m.w, m.n_classes = B, H, W, CN
        C.memmove(m.rank, table.ctypes.data, table.nbytes)
        for i in range(B):
            m.apply[i] = 1
        call = lambda n, *args: (lambda: L.call(n, *args, st))          # noqa: E731
        presence_b = call("simt_label_presence", labs.data_ptr(), B, H * W, CN, part_s.data_ptr())
        presence_b()
        call("simt_source_mix_items", C.byref(m), items.data_ptr())()
        torch.cuda.synchronize()
        own = torch.arange(B, device=dev, dtype=torch.uint8).view(B, 1, 1)
        share = float((items != own).float().mean())
        # the composition with the launches that existed
        x2, lab2 = torch.zeros(2 * B, 3, H, W, device=dev), torch.zeros(2 * B, H, W, dtype=torch.int64, device=dev)
        xo2, lo2 = torch.zeros_like(x2), torch.zeros_like(lab2)
        items2 = torch.zeros(2 * B, H, W, dtype=torch.uint8, device=dev)
        part2 = torch.zeros(2 * B, L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)
        e = L.ClassMixDesc()
        e.x, e.lab, e.x_out, e.lab_out, e.part = x2.data_ptr(), lab2.data_ptr(), xo2.data_ptr(), lo2.data_ptr(), part2.data_ptr()
        e.B, e.h, e.w, e.n_classes = 2 * B, H, W, CN
        C.memmove(e.rank, table.ctypes.data, table.nbytes)
        for i in range(2 * B):
            e.partner[i], e.apply[i] = (B + i if i < B else i), (1 if i < B else 0)

        def copies():
            x2[:B].copy_(xt)
            x2[B:].copy_(xs)
            lab2[:B].copy_(lab8)          # the widening
            lab2[B:].copy_(labs)
        presence_2b = call("simt_label_presence", lab2.data_ptr(), 2 * B, H * W, CN, part2.data_ptr())
        mix_2b = call("simt_class_mix_items", C.byref(e), items2.data_ptr())

        def composition():
            copies()
            presence_2b()
            mix_2b()
        composition()
        torch.cuda.synchronize()
        assert torch.equal(xo2[:B], x_out) and torch.equal(lo2[:B], lab_out) and torch.equal(items2[:B], items)
        print(f"\n{name}: {B * H * W / 1e6:.2f} Mpx, {share:.3f} of the pixels pasted")
        t = _table([("device-to-device copy of the image batch", lambda: x_out.copy_(xt)),
                    ("simt_label_presence (B source items)", presence_b),
                    ("simt_source_mix", call("simt_source_mix", C.byref(m))),
                    ("simt_source_mix_items", call("simt_source_mix_items", C.byref(m), items.data_ptr())),
                    ("composition: the four copies", copies),
                    ("composition: simt_label_presence (2B items)", presence_2b),
                    ("composition: simt_class_mix_items (2B items)", mix_2b),
                    ("composition: all of it", composition)], a.rounds, timed)
        px = B * H * W
        rate = 2 * xt.numel() * 4 / t["device-to-device copy of the image batch"]          # bytes per microsecond, read + write
        floor = px * (12 + 8 + 12 + 8 + (1 - share))
        print(f"copy rate {rate / 1e6:.2f} TB/s (read + write); byte floor of simt_source_mix {floor / 1e6:.1f} MB = {floor / rate:.1f} us, "
              f"of simt_source_mix_items {(floor + px) / 1e6:.1f} MB = {(floor + px) / rate:.1f} us")

        # the head passes, mode 1, bf16 gradient output as the trainers ask for it, with the source mix's map
        g = torch.Generator().manual_seed(1)
        Q, QP = CN, ops.round_up(CN, 8)
        p1, p2 = (torch.randn(B * h * w, LD, generator=g).to(dev) * 3 for _ in range(2))
        hp = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Q), device=dev)
        keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
        hout = torch.zeros(lib.simt_head_hout_floats(Q, Q), device=dev)
        g1 = torch.zeros(2, B, H, w, QP, device=dev)
        dt = [torch.zeros(B * h * w, QP, dtype=torch.bfloat16, device=dev) for _ in range(2)]
        hd = L.HeadDesc()
        hd.pred1, hd.pred2, hd.label = (None if single else p1.data_ptr()), p2.data_ptr(), lab_out.data_ptr()
        hd.part, hd.keys, hd.hout, hd.g1 = hp.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
        hd.dpred1_t, hd.dpred2_t = (None if single else dt[0].data_ptr()), dt[1].data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, CN, Q
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = LD, LD, QP, 0, QP, L.SIMT_BF16
        hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, 0.1, 0.0, 1.0
        hd.mode, hd.single, hd.up_half_pixel = 1, single, 0
        q = torch.cat([torch.rand(B, generator=g) * 0.9 + 0.1, torch.ones(B)]).to(dev)
        qp, ip = q.data_ptr(), items.data_ptr()
        _table([("simt_head_loss_weighted, map (nw = B)", call("simt_head_loss_weighted", C.byref(hd), qp, ip)),
                ("simt_head_loss_weighted_n, map, nw = B", call("simt_head_loss_weighted_n", C.byref(hd), qp, B, ip)),
                ("simt_head_loss_weighted_n, map, nw = 2B", call("simt_head_loss_weighted_n", C.byref(hd), qp, 2 * B, ip)),
                ("simt_head_grad_weighted, map (nw = B)", call("simt_head_grad_weighted", C.byref(hd), qp, ip)),
                ("simt_head_grad_weighted_n, map, nw = B", call("simt_head_grad_weighted_n", C.byref(hd), qp, B, ip)),
                ("simt_head_grad_weighted_n, map, nw = 2B", call("simt_head_grad_weighted_n", C.byref(hd), qp, 2 * B, ip))], a.rounds, timed)
        del x2, lab2, xo2, lo2, items2, g1


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
    if a.weighted is not None:
        kw["online_labels_weighted"] = a.weighted
    if a.source:
        kw["online_source"] = True
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
    skw = {}
    if a.source:
        sx, sl = ms.synthetic_batch(B, H, W, cd, seed=2, device=dev)
        skw = dict(source_image=sx, source_label=sl)
    for _ in range(a.warmup):
        tr.step(img, **skw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(img, **skw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    print(json.dumps({"model": a.model, "tree": "parent" if a.repo else "this", "source": a.source, "weighted": a.weighted, "online_mix": a.online_mix,
                      "steps": a.steps, "ms_per_step": round(dt * 1e3 / a.steps, 3), "images_per_s": round(B * a.steps / dt, 2),
                      "labelled": l["labelled"], "source_seg2": l.get("source_seg2")}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    s = sub.add_parser("step")
    s.add_argument("--model", choices=["v2", "vgg"], required=True)
    s.add_argument("--source", action="store_true")
    s.add_argument("--weighted", choices=["batch", "item"], default=None)
    s.add_argument("--online-mix", type=float, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
