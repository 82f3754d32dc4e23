#!/usr/bin/env python3
"""Cost of the ImageNet feature distance (feat_dist) -> profiles/feat_dist.txt.  MEASUREMENT ONLY.

    python profiles/tools/feat_dist_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/feat_dist_cost.py step [--feat-dist L] [--steps 20] [--warmup 6] [--repo TREE]

kernel  At the DeepLab-v2 production geometry (B = 4, 768 x 768 labels, a 97 x 97 x 2048 layer-4 map, bf16), in ONE run: a plain device copy
        of the seed's size (the rate the byte floors are taken at), then simt_feat_dist_mask, simt_feat_dist and simt_feat_dist_finalize for
        three label sets -- `synthetic_batch`, nothing kept (all 255), everything kept (all class 13) -- each beside its byte floor (mask: the
        label bytes; main pass: the seed bytes written plus the two feature rows of the kept cells), and the layer-4 head's input-gradient
        launch of a production train plan with `res` = the seed and with `res` = NULL.  Device events over `--reps` back-to-back launches after
        a warm-up, `--rounds` rounds in alternating order; microseconds per launch.
step    The warm-up trainer of DeepLab-v2 R-101 (B = 4, 768 x 768), bf16, constructor init, online_labels = 0 and online_source on a resident
        synthetic target image and source pair: `--steps` steps after `--warmup`, wall-clock milliseconds per step around a device
        synchronise, one JSON line.  --feat-dist L passes the keyword (the frozen trunk: another constructor init); then the line also
        carries the ImageNet trunk's eval forward alone and the three launches alone (device events).  --repo TREE imports another checkout
        (the parent commit's, which has no such keyword).  One process per run; the driver rotates parent / keyword off / keyword on.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, H, W = 4, 768, 768
THINGS = (6, 7, 11, 12, 13, 14, 15, 16, 17, 18)


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


def _rounds(fns, rounds, timed):
    res = {n: [] for n, _f in fns}
    for r in range(rounds):
        for n, f in (fns if r % 2 == 0 else fns[::-1]):
            res[n].append(timed(f))
    return res


def kernel(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    from simt_amd import model_spec as ms
    from simt_amd import ops
    from simt_amd.engine import TrunkPlan, multi_heads
    dev = torch.device("cuda:0")
    lib = L.load()
    cd = ms.load_class_dist("bapa")
    plan = TrunkPlan({k: v.to(dev) for k, v in ms.reference_init(ms.state_shapes(19, 0, False), seed=1234).items()}, B, H, W,
                     multi_heads(19, 0, False), dtype=torch.bfloat16, train=True, feat_grad_seed=True)
    h, w = plan.feat_hw
    M, Cf = plan.feat_seed.shape
    img, lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    plan.forward(img)
    for t in plan.dlogits.values():
        t.normal_(0, 1e-3)
        t[:, 19:] = 0
    plan.backward()
    torch.cuda.synchronize()
    st = ops.stream_ptr()
    fs = plan.block_io[-1]["z"]
    fi = (fs.float() + torch.randn(M, Cf, device=dev) * 0.5).to(torch.bfloat16)
    label = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    mask = torch.zeros(M, dtype=torch.uint8, device=dev)
    kept = torch.zeros(lib.simt_feat_dist_mask_parts(B, h, w), dtype=torch.int32, device=dev)
    dist, part, out = torch.zeros(M, device=dev), torch.zeros(lib.simt_feat_dist_parts(M), device=dev), torch.zeros(3, device=dev)
    md = L.FeatDistMaskDesc()
    md.label, md.mask, md.part, md.classes = label.data_ptr(), mask.data_ptr(), kept.data_ptr(), sum(1 << c for c in THINGS)
    md.B, md.H, md.W, md.h, md.w, md.min_ratio = B, H, W, h, w, 0.75
    d = L.FeatDistDesc()
    d.fs, d.fi, d.mask, d.kept_part = fs.data_ptr(), fi.data_ptr(), mask.data_ptr(), kept.data_ptr()
    d.seed, d.d, d.part, d.out = plan.feat_seed.data_ptr(), dist.data_ptr(), part.data_ptr(), out.data_ptr()
    d.lam, d.M, d.C, d.ld, d.dtype, d.n_kept_part, d.lam_g = 0.005, M, Cf, Cf, ops.dt_code(torch.bfloat16), kept.numel(), 0.005
    print(f"B = {B}, {H} x {W} labels, {h} x {w} x {Cf} bf16 (M = {M}); {a.reps} launches per timing, {a.rounds} rounds in alternating order; us per launch")
    twin = torch.empty_like(plan.feat_seed)
    copy = _rounds([("copy", lambda: twin.copy_(plan.feat_seed))], a.rounds, lambda f: _timed(torch, f, a.reps))["copy"]
    seed_bytes = M * Cf * 2
    rate = 2 * seed_bytes / (sum(copy) / len(copy) * 1e-6)          # bytes read + bytes written per second
    print(f"plain copy of {seed_bytes / 1e6:.1f} MB (read + write): " + " ".join(f"{v:.1f}" for v in copy) + f" us -> {rate / 1e12:.2f} TB/s moved")
    sets = [("synthetic_batch", lab), ("nothing kept (all 255)", torch.full_like(lab, 255)), ("everything kept (all 13)", torch.full_like(lab, 13))]
    for name, l in sets:
        label.copy_(l)
        fns = [("simt_feat_dist_mask", lambda: L.call("simt_feat_dist_mask", C.byref(md), st)),
               ("simt_feat_dist", lambda: L.call("simt_feat_dist", C.byref(d), st)),
               ("simt_feat_dist_finalize", lambda: L.call("simt_feat_dist_finalize", C.byref(d), st))]
        for _n, f in fns:
            f()
        torch.cuda.synchronize()
        N = int(out[2].item())
        floors = {"simt_feat_dist_mask": B * H * W * 8, "simt_feat_dist": seed_bytes + N * 2 * Cf * 2, "simt_feat_dist_finalize": 0}
        res = _rounds(fns, a.rounds, lambda f: _timed(torch, f, a.reps))
        print(f"\nlabels: {name}; N = {N} of {M} cells, mean distance {float(out[1]):.3f}")
        for n, _f in fns:
            mean = sum(res[n]) / len(res[n])
            fl = floors[n] / rate * 1e6
            print(f"{n:>26}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f"  mean {mean:7.1f} us; floor {floors[n] / 1e6:7.1f} MB = {fl:6.1f} us"
                  + (f"; {mean / fl:.2f} x the floor" if fl > 0 else ""))
    # the head's input-gradient launch with and without the seed
    it = next(i for i in plan.bwd_list.items if i.keep is plan.feat_seed_desc)

    def dgrad(on):
        def f():
            plan.use_feat_seed(on)
            rc = it.fn(*it.args, st)
            assert rc == 0
        return f
    res = _rounds([("res = the seed", dgrad(True)), ("res = NULL", dgrad(False))], a.rounds, lambda f: _timed(torch, f, a.reps))
    print(f"\nthe layer-4 head's input-gradient launch ({it.tag}, {it.shape}):")
    for n, v in res.items():
        print(f"{n:>26}  " + " ".join(f"{x:7.1f}" for x in v) + f"  mean {sum(v) / len(v):7.1f} us")
    print(f"the seed read costs {seed_bytes / 1e6:.1f} MB = {seed_bytes / (rate / 2) * 1e6:.1f} us at the copy's one-way rate")


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
    kw = {"online_labels": 0.0, "online_source": True}
    shapes = ms.state_shapes(19, 0, False)
    if a.feat_dist is not None:
        im = ms.reference_init(shapes, seed=7)
        kw.update(feat_dist=a.feat_dist, feat_dist_state={k: v for k, v in im.items() if not k.startswith(("layer5", "layer6"))})
    hp = Hyper(num_classes=19, open_classes=0, lr=2.5e-4)
    tr = WarmupTrainer(ms.reference_init(shapes, seed=1234), hp, B, H, W, device=dev, **kw)
    img, _lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    sx, sl = ms.synthetic_batch(B, H, W, cd, seed=2, device=dev)
    run = lambda: tr.step(img, source_image=sx, source_label=sl)
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    out = {"tree": "parent" if a.repo else "this", "feat_dist": a.feat_dist, "steps": a.steps, "ms_per_step": dt * 1e3 / a.steps,
           "images_per_s": B * a.steps / dt, "source_seg2": l["source_seg2"]}
    if a.feat_dist is not None:
        from simt_amd import ops
        out.update(feat_dist_loss=l["feat_dist"], cells=l["feat_dist_cells"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for name, fn in (("imagenet_forward_ms", tr.imnet.fwd_list.run), ("three_launches_ms", lambda: tr._fd_launches(ops.stream_ptr()))):
            for _pass in range(2):          # the first pass warms up
                e0.record()
                for _ in range(10):
                    fn()
                e1.record()
                torch.cuda.synchronize()
            out[name] = e0.elapsed_time(e1) / 10
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    s = sub.add_parser("step")
    s.add_argument("--feat-dist", type=float, default=None)
    s.add_argument("--steps", type=int, default=20)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
