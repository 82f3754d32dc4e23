#!/usr/bin/env python3
"""Cost of the quality weights (online_labels_weighted) -> profiles/online_labels_weighted.txt.  MEASUREMENT ONLY.

    python profiles/tools/online_weighted_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/online_weighted_cost.py step --model v2|vgg|v3 [--weighted batch|item] [--online-mix P] [--steps 30] [--warmup 6] [--repo TREE]

kernel  At B = 4, 97 x 97 -> 768 x 768 (DeepLab-v2, two heads), B = 8, 65 x 65 -> 512 x 512 (VGG16, one head) and B = 4, 64 x 128 -> 512 x 1024
        (DeepLabv3, one head, half-pixel, family 1), C = 19, threshold 0.5, in ONE run: the `_w` label launches beside the launches they
        replace, simt_label_quality, the weighted head passes (no map / with a map) beside the unweighted mode-1 passes, and
        simt_class_mix_u8_items beside simt_class_mix_u8.  Device events over `--reps` back-to-back launches after a warm-up, `--rounds`
        rounds in alternating order; microseconds per launch.
step    The warm-up trainer at those three sizes, bf16, constructor init, online_labels = 0 on a resident synthetic batch: `--steps` steps
        after `--warmup`, wall-clock milliseconds per step around a device synchronise, one JSON line.  --weighted passes the keyword;
        --repo TREE imports another checkout (the parent commit's, which has no such keyword).  One process per run; the driver rotates
        the order of parent / keyword off / keyword on from round to round.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, family, single, half, B, h, w, H, W)
CASES = [("DeepLab-v2, B = 4, 97 x 97 -> 768 x 768, two heads", 0, 0, 0, 4, 97, 97, 768, 768),
         ("DeepLab-VGG16, B = 8, 65 x 65 -> 512 x 512, one head", 0, 1, 0, 8, 65, 65, 512, 512),
         ("DeepLabv3, B = 4, 64 x 128 -> 512 x 1024, one head", 1, 1, 1, 4, 64, 128, 512, 1024)]
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
    timed = lambda f: _timed(torch, f, a.reps)          # noqa: E731
    print(f"C = {CN}, ld = {LD}, threshold {THR}; {a.reps} launches per timing, {a.rounds} rounds in alternating order; us per launch")
    for name, fam, single, half, B, h, w, H, W in CASES:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B * h * w, LD, generator=g) * 3
        if fam == 0:
            x[:, :CN] = torch.softmax(x[:, :CN], 1)
        x = x.to(dev)
        st = ops.stream_ptr()
        lab64, lab8 = torch.zeros(B, H, W, dtype=torch.int64, device=dev), torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        counts = torch.zeros(CN + 1, dtype=torch.int64, device=dev)
        geo = dict(B=B, h=h, w=w, ld=LD, H=H, W=W, C=CN, family=fam, threshold=THR)

        def fill(d, **ptrs):
            for k, v in dict(geo, fix=x.data_ptr(), counts=counts.data_ptr(), **ptrs).items():
                setattr(d, k, v)
            return d
        u = fill(L.OnlineLabelU8Desc(), lab8=lab8.data_ptr())
        rows = lib.simt_online_label_parts(C.byref(u))
        part, conf_part = (torch.zeros(B, rows, dtype=torch.int32, device=dev) for _ in range(2))
        u.part = part.data_ptr()
        d = fill(L.OnlineLabelDesc(), label=lab64.data_ptr())
        dw = fill(L.OnlineLabelWDesc(), label=lab64.data_ptr(), conf_part=conf_part.data_ptr())
        uw = fill(L.OnlineLabelWU8Desc(), lab8=lab8.data_ptr(), part=part.data_ptr(), conf_part=conf_part.data_ptr())
        q = torch.zeros(B, device=dev)
        lq = L.LabelQualityDesc()
        lq.conf_part, lq.q, lq.B, lq.rows, lq.H, lq.W, lq.mode = conf_part.data_ptr(), q.data_ptr(), B, rows, H, W, 0
        call = lambda n, *args: (lambda: L.call(n, *args, st))          # noqa: E731
        call("simt_online_label_w_u8", C.byref(uw))()
        call("simt_label_quality", C.byref(lq))()
        torch.cuda.synchronize()
        print(f"\n{name}: {B * H * W / 1e6:.2f} Mpx, {rows} workgroups; q = {[round(v, 3) for v in q.tolist()]}")
        _table([("simt_online_label", call("simt_online_label", C.byref(d))), ("simt_online_label_w", call("simt_online_label_w", C.byref(dw))),
                ("simt_online_label_u8", call("simt_online_label_u8", C.byref(u))),
                ("simt_online_label_w_u8", call("simt_online_label_w_u8", C.byref(uw))),
                ("simt_label_quality", call("simt_label_quality", C.byref(lq)))], a.rounds, timed)

        # the mix and its item map
        img = torch.randn(B, 3, H, W, generator=g).to(dev)
        x_in, label = torch.zeros_like(img), torch.zeros_like(lab64)
        items = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        apply, rank = class_mix.draw_batch(class_mix.generator(0, 0), B, CN, 1.0)
        table = np.zeros((L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES), dtype=np.uint8)
        table[:B, :CN] = rank
        m = L.ClassMixU8Desc()
        m.x, m.lab8, m.x_out, m.lab_out, m.part = img.data_ptr(), lab8.data_ptr(), x_in.data_ptr(), label.data_ptr(), part.data_ptr()
        m.B, m.h, m.w, m.n_classes, m.rows = B, H, W, CN, rows
        C.memmove(m.rank, table.ctypes.data, table.nbytes)
        for i in range(B):
            m.partner[i], m.apply[i] = (i + 1) % B, 1
        call("simt_class_mix_u8_items", C.byref(m), items.data_ptr())()
        torch.cuda.synchronize()
        print(f"mix: {float((items != torch.arange(B, device=dev, dtype=torch.uint8).view(B, 1, 1)).float().mean()):.3f} of the pixels pasted")
        _table([("simt_class_mix_u8", call("simt_class_mix_u8", C.byref(m))),
                ("simt_class_mix_u8_items", call("simt_class_mix_u8_items", C.byref(m), items.data_ptr()))], a.rounds, timed)

        # the head passes, mode 1, bf16 gradient output as the trainers ask for it
        Q, QP = CN, ops.round_up(CN, 8)
        p1, p2 = (torch.randn(B * h * w, LD, generator=g).to(dev) * 3 for _ in range(2))
        hp = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Q), device=dev)
        keys = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
        hout = torch.zeros(lib.simt_head_hout_floats(Q, Q), device=dev)
        g1 = torch.zeros(2, B, H, w, QP, device=dev)
        dt = [torch.zeros(B * h * w, QP, dtype=torch.bfloat16, device=dev) for _ in range(2)]
        hd = L.HeadDesc()
        hd.pred1, hd.pred2, hd.label = (None if single else p1.data_ptr()), p2.data_ptr(), label.data_ptr()
        hd.part, hd.keys, hd.hout, hd.g1 = hp.data_ptr(), keys.data_ptr(), hout.data_ptr(), g1.data_ptr()
        hd.dpred1_t, hd.dpred2_t = (None if single else dt[0].data_ptr()), dt[1].data_ptr()
        hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, CN, Q
        hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = LD, LD, QP, 0, QP, L.SIMT_BF16
        hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, 0.1, 0.0, 1.0
        hd.mode, hd.single, hd.up_half_pixel = 1, single, half
        qp, ip = q.data_ptr(), items.data_ptr()
        _table([("simt_head_loss (pass 1)", call("simt_head_loss", C.byref(hd))),
                ("simt_head_loss_weighted, no map", call("simt_head_loss_weighted", C.byref(hd), qp, None)),
                ("simt_head_loss_weighted, map", call("simt_head_loss_weighted", C.byref(hd), qp, ip)),
                ("simt_head_grad (pass 2)", call("simt_head_grad", C.byref(hd))),
                ("simt_head_grad_weighted, no map", call("simt_head_grad_weighted", C.byref(hd), qp, None)),
                ("simt_head_grad_weighted, map", call("simt_head_grad_weighted", C.byref(hd), qp, ip))], a.rounds, timed)
        del img, x_in, label, lab64, lab8, items, g1


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
    hp = Hyper(num_classes=19, open_classes=0, lr=2.5e-4)
    if a.model == "v2":
        B, H, W = 4, 768, 768
        tr = WarmupTrainer(ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), hp, B, H, W, device=dev, **kw)
    else:
        from simt_amd.step_single import WarmupSingleTrainer
        from simt_amd.tools.trainV2_simt import single_model_state
        B, H, W = (8, 512, 512) if a.model == "vgg" else (4, 512, 1024)
        tr = WarmupSingleTrainer(a.model, single_model_state("DeepLabVGG" if a.model == "vgg" else "DeepLabv3", 19), hp, B, H, W, device=dev, **kw)
    img, _lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    for _ in range(a.warmup):
        tr.step(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(img)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    print(json.dumps({"model": a.model, "tree": "parent" if a.repo else "this", "weighted": a.weighted, "online_mix": a.online_mix,
                      "steps": a.steps, "ms_per_step": round(dt * 1e3 / a.steps, 3), "images_per_s": round(B * a.steps / dt, 2),
                      "labelled": l["labelled"], "label_quality": l.get("label_quality")}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    s = sub.add_parser("step")
    s.add_argument("--model", choices=["v2", "vgg", "v3"], required=True)
    s.add_argument("--weighted", choices=["batch", "item"], default=None)
    s.add_argument("--online-mix", type=float, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
