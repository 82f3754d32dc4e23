#!/usr/bin/env python3
"""Cost of the weight EMA (simt_ema_multi, and a training step with ema_decay) -> profiles/ema.txt.  MEASUREMENT ONLY.

    python profiles/tools/ema_cost.py launch [--out FILE] [--rounds 3] [--reps 60]
    python profiles/tools/ema_cost.py step --model v2|vgg [--ema 0.999] [--steps 40] [--warmup 10] [--repo TREE]

launch  the production segment tables -- every floating tensor of the trainable model's state -- of DeepLab-v2 R-101 (19 + 15 classes),
        DeepLabv3 R-50 and DeepLab-VGG16; three rotating sets of (w, e, g, buf) buffers (a set is past the caches, operands come from HBM);
        `--rounds` rounds in alternating order, microseconds per launch over `--reps` launches between two device events after a warm-up:
          ema      simt_ema_multi, omd = float32(1 - 0.999)                     12 bytes per element (w and e read, e written)
          ema copy simt_ema_multi, omd = 1 (update 0)                            8 bytes per element
          sgd      simt_sgd_multi over the SAME segment table and chunk size    20 bytes per element (p, buf read and written, g read)
          copy     torch's device-to-device copy of one flat tensor of the same element count: the chip's plain-copy rate, 8 bytes per element
        The bar: `ema` takes no longer than `sgd` on any table (it moves 0.6 x the bytes with the same access pattern).
step    one trainer on a resident synthetic batch (DeepLab-v2 SimT B = 4 at 768 x 768, or DeepLab-VGG16 warm-up B = 8 at 512 x 512), `--steps`
        steps after `--warmup`: median milliseconds per step from device events and wall-clock milliseconds per step, one JSON line.
        --ema D passes ema_decay; --repo TREE imports another checkout (the parent commit's, which has no such keyword: then --ema is an error).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time


def _tables(torch):
    from simt_amd import model_spec as ms
    from simt_amd.engine_v3 import v3_state_shapes
    from simt_amd.engine_vgg import vgg_state_shapes
    shapes = {"DeepLab-v2 R-101": ms.state_shapes(19, 15, True), "DeepLabv3 R-50": v3_state_shapes(19, 15, True),
              "DeepLab-VGG16": vgg_state_shapes(19 + 15)}
    return {name: {k: tuple(v) for k, v in sh.items() if "num_batches_tracked" not in k} for name, sh in shapes.items()}


def launch(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd.ema import CHUNK, WeightEma
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    SETS = 3

    def timed(fn):
        for k in range(SETS):
            fn(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(a.reps):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    say(f"{a.reps} launches per timing over {SETS} rotating buffer sets, {a.rounds} rounds in alternating order; us per launch")
    for name, shapes in _tables(torch).items():
        g = torch.Generator(device=dev).manual_seed(1)
        sets = []
        for k in range(SETS):
            w = {n: torch.randn(s, device=dev, generator=g) * 0.05 for n, s in shapes.items()}
            ema = WeightEma(w, 0.999)
            for e in ema.shadow.values():
                e.add_(torch.randn(e.shape, device=dev, generator=g) * 0.01)
            grads = {n: torch.randn(s, device=dev, generator=g) * 1e-3 for n, s in shapes.items()}
            bufs = {n: torch.zeros(s, device=dev) for n, s in shapes.items()}
            # simt_sgd_multi over the same segments, in the same order, with the same chunk table
            names = [n for n, e in ema.shadow.items() if e.numel() > 0]
            recs = np.array([(w[n].data_ptr(), grads[n].data_ptr(), bufs[n].data_ptr(), w[n].numel(), 1, 0) for n in names],
                            dtype=[("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("mult", "<i4"), ("group", "<i4")])
            segs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
            sd = L.SgdDesc()
            sd.segs, sd.chunks, sd.nchunks, sd.chunk = segs.data_ptr(), ema.chunks.data_ptr(), ema.chunks.shape[0], CHUNK
            sd.lr[0], sd.wd[0], sd.momentum, sd.dampening, sd.first_step = 1e-6, 5e-4, 0.9, 0.0, 0
            flat = (torch.empty(ema.elements, device=dev), torch.empty(ema.elements, device=dev))
            sets.append(dict(w=w, ema=ema, grads=grads, bufs=bufs, segs=segs, sgd=sd, flat=flat))
        n_el, n_seg, n_chunks = sets[0]["ema"].elements, len(names), sets[0]["ema"].chunks.shape[0]
        small = sum(1 for n in names if shapes[n] and int(np.prod(shapes[n])) < 4096)

        def run_ema(k, omd):
            d = sets[k % SETS]["ema"].desc
            d.omd = omd
            L.call("simt_ema_multi", C.byref(d), st)

        omd = float(np.float32(1 - 0.999))
        fns = {"ema": lambda k: run_ema(k, omd), "ema copy": lambda k: run_ema(k, 1.0),
               "sgd": lambda k: L.call("simt_sgd_multi", C.byref(sets[k % SETS]["sgd"]), st),
               "copy": lambda k: sets[k % SETS]["flat"][1].copy_(sets[k % SETS]["flat"][0])}
        nbytes = {"ema": 12, "ema copy": 8, "sgd": 20, "copy": 8}
        res = {n: [] for n in fns}
        for r in range(a.rounds):
            for n in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
                res[n].append(timed(fns[n]))
        say(f"\n{name}: {n_el / 1e6:.2f} M elements in {n_seg} segments ({small} below 4096 elements), {n_chunks} workgroups of {CHUNK} elements")
        say(f"{'launch':>9s}  {'rounds':>{8 * a.rounds}s}  {'mean':>7s}  {'B/elem':>6s}  {'MB':>7s}  {'GB/s':>7s}  {'x sgd':>6s}  {'x copy rate':>11s}")
        mean = {n: sum(v) / len(v) for n, v in res.items()}
        copy_rate = 8 * n_el / mean["copy"]
        for n in fns:
            rate = nbytes[n] * n_el / mean[n]
            say(f"{n:>9s}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f"  {mean[n]:7.1f}  {nbytes[n]:6d}  {nbytes[n] * n_el / 1e6:7.1f}  "
                f"{rate / 1e3:7.0f}  {mean[n] / mean['sgd']:6.2f}  {rate / copy_rate:11.2f}")
        say(f"bar (ema <= sgd in every round's pair and in the mean): {'HOLDS' if mean['ema'] <= mean['sgd'] else 'MISSED'}")
        del sets
        torch.cuda.empty_cache()


def step(a):
    root = os.path.abspath(a.repo or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    sys.path.insert(0, root)
    import torch

    from simt_amd import model_spec as ms
    from simt_amd.engine import reserve_streams
    from simt_amd.step import Hyper
    dev = torch.device("cuda:0")
    reserve_streams(dev)
    cd = ms.load_class_dist("bapa")
    kw = {} if a.ema is None else {"ema_decay": a.ema}
    if a.model == "v2":
        from simt_amd.step import SimTTrainer
        B, H, W, K = 4, 768, 768, 3
        hp = Hyper(open_classes=K, lr=6e-4, lr_T=6e-3)
        tr = SimTTrainer(ms.reference_init(ms.state_shapes(19, K, True), seed=1234), ms.reference_init(ms.state_shapes(19, 0, False), seed=1234),
                         ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), hp, cd, B, H, W, device=dev, **kw)
    else:
        from simt_amd.engine_vgg import vgg_state_shapes
        from simt_amd.step_single import WarmupSingleTrainer
        B, H, W = 8, 512, 512
        hp = Hyper(open_classes=0, lr=2.5e-4)
        tr = WarmupSingleTrainer("vgg", ms.kaiming_init(vgg_state_shapes(19), seed=1234), hp, B, H, W, device=dev, **kw)
    img, lab = ms.synthetic_batch(B, H, W, cd, seed=1234, device=dev)
    for _ in range(a.warmup):
        tr.step(img, lab)
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(a.steps):
        tr.step(img, lab)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
    tr.losses()
    print(json.dumps({"mode": "step", "tree": os.path.relpath(root), "model": a.model, "B": B, "size": [H, W], "ema": a.ema, "steps": a.steps,
                      "median_ms": round(per[len(per) // 2], 3), "wall_ms_per_step": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["launch", "step"])
    p.add_argument("--out", default=None)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=60)
    p.add_argument("--model", choices=["v2", "vgg"], default="v2")
    p.add_argument("--ema", type=float, default=None)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    a = p.parse_args()
    {"launch": launch, "step": step}[a.mode](a)
