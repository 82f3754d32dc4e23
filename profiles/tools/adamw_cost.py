#!/usr/bin/env python3
"""Cost of the AdamW launch (simt_adamw_multi, and a training step with optimizer="adamw") -> profiles/adamw.txt.  MEASUREMENT ONLY.

    python profiles/tools/adamw_cost.py launch [--out FILE] [--rounds 3] [--reps 60]
    python profiles/tools/adamw_cost.py step --model v2|vgg [--optimizer sgd|adamw] [--late] [--steps 40] [--warmup 10] [--repo TREE]

launch  the applied tensors of the three models as the trainers list them -- DeepLab-v2 R-101 SimT stage (layer3, layer4, heads; 19 + 15
        classes), DeepLabv3 R-50 (layer3, ASPP, classifiers, with their BatchNorm gamma / beta) and DeepLab-VGG16 (everything) -- each tensor
        ONCE, gradients in one flat buffer with every entry on a 16-byte boundary (engine.layout_flat_grads); three rotating sets of
        (p, g, m, v) buffers (a set is past the caches: operands come from HBM); `--rounds` rounds in alternating order, microseconds per launch
        over `--reps` launches between two device events after a warm-up:
          adamw    simt_adamw_multi, first_step = 0                                  28 bytes per element (p, g, m, v read; p, m, v written)
          sgd      simt_sgd_multi over the SAME tensors, mult = 1, momentum 0.9       20 bytes per element (p, buf read and written, g read)
          copy     torch's device-to-device copy of 3.5 x the element count in fp32: 28 bytes per element, the chip's plain-copy rate
        The expectation: adamw / sgd = 28 / 20 = 1.4 at a comparable fraction of the copy rate.
step    one trainer on a resident synthetic batch (DeepLab-v2 SimT B = 4 at 768 x 768, or DeepLab-VGG16 warm-up B = 8 at 512 x 512), `--steps`
        steps after `--warmup`: median milliseconds per step from device events and wall-clock milliseconds per step, one JSON line.
        --optimizer adamw passes the keyword (DAFormer's lr 6e-5, weight decay 0.01); --late sets SIMT_EARLY_SGD=0 (the launch behind the
        backward instead of on the side stream); --repo TREE imports another checkout (the parent commit's, which has no such keyword).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time


def _tables():
    from simt_amd import model_spec as ms
    from simt_amd.engine_v3 import v3_state_shapes
    from simt_amd.engine_vgg import vgg_state_shapes
    from simt_amd.step import optim_listing
    stats = ("running_mean", "running_var", "num_batches_tracked")
    v2 = {k: tuple(v) for k, v in ms.state_shapes(19, 15, True).items()}
    g0, g1 = optim_listing([k for k, s in v2.items() if len(s) == 4 or k.split(".")[0].startswith(("layer5", "layer6"))])
    v3 = {k: tuple(v) for k, v in v3_state_shapes(19, 15, True).items() if not k.endswith(stats)}
    v3_0 = [k for k in v3 if k.startswith("resnet.resnet_50.layer3.")]
    v3_1 = [k for k in v3 if k.startswith(("assp.", "conv.", "conv_1."))]
    vgg = {k: tuple(v) for k, v in vgg_state_shapes(19 + 15).items() if not k.endswith(stats)}
    norm = lambda shapes, n: (n.rsplit(".", 1)[0] + ".running_mean") in shapes
    v3_all = {k: tuple(v) for k, v in v3_state_shapes(19, 15, True).items()}
    return {"DeepLab-v2 R-101 (SimT stage)": [(n, v2[n], g) for g, names in ((0, g0), (1, g1)) for n in names],
            "DeepLabv3 R-50": [(n, v3[n], g + (2 if norm(v3_all, n) else 0)) for g, names in ((0, v3_0), (1, v3_1)) for n in names],
            "DeepLab-VGG16": [(n, s, 0) for n, s in vgg.items()]}


def launch(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd.optimizer import adamw_constants, adamw_table
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    SETS, CHUNK = 3, 65536

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
    for name, table in _tables().items():
        g = torch.Generator(device=dev).manual_seed(1)
        n_el = sum(int(np.prod(s)) for _n, s, _g in table)
        sets = []
        for k in range(SETS):
            p = [torch.randn(s, device=dev, generator=g) * 0.05 for _n, s, _g in table]
            m = [torch.randn(s, device=dev, generator=g) * 1e-3 for _n, s, _g in table]
            v = [torch.rand(s, device=dev, generator=g) * 1e-6 for _n, s, _g in table]
            spans = [(t.numel() + 3) // 4 * 4 for t in p]
            flat = torch.randn(sum(spans), device=dev, generator=g) * 1e-3
            offs = np.concatenate([[0], np.cumsum(spans)[:-1]])
            grads = [flat[o:o + t.numel()] for o, t in zip(offs, p)]
            segs, chunks = adamw_table([(t.data_ptr(), gr.data_ptr(), mm.data_ptr(), vv.data_ptr(), t.numel(), grp)
                                        for t, gr, mm, vv, (_n, _s, grp) in zip(p, grads, m, v, table)], CHUNK)
            segs_d, chunks_d = torch.from_numpy(segs).to(dev), torch.tensor(chunks, dtype=torch.int32).to(dev)
            ad = L.AdamwDesc()
            ad.segs, ad.chunks, ad.nchunks, ad.chunk = segs_d.data_ptr(), chunks_d.data_ptr(), len(chunks), CHUNK
            ss, dc, b1, b2, o1, o2, bc = adamw_constants((6e-5, 6e-4, 6e-5, 6e-4), (0.01, 0.01, 0.0, 0.0), (0.9, 0.999), 100)
            for i in range(4):
                ad.step_size[i], ad.decay[i] = ss[i], dc[i]
            ad.beta1, ad.beta2, ad.omb1, ad.omb2, ad.bc2s, ad.eps, ad.first_step = b1, b2, o1, o2, bc, 1e-8, 0
            recs = np.array([(t.data_ptr(), gr.data_ptr(), mm.data_ptr(), t.numel(), 1, grp & 1) for t, gr, mm, (_n, _s, grp) in zip(p, grads, m, table)],
                            dtype=[("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("mult", "<i4"), ("group", "<i4")])
            ssegs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
            sd = L.SgdDesc()
            sd.segs, sd.chunks, sd.nchunks, sd.chunk = ssegs.data_ptr(), chunks_d.data_ptr(), len(chunks), CHUNK
            sd.lr[0], sd.lr[1], sd.wd[0], sd.wd[1], sd.momentum, sd.dampening, sd.first_step = 1e-6, 1e-5, 5e-4, 5e-4, 0.9, 0.0, 0
            n_copy = n_el * 7 // 2
            copy = (torch.empty(n_copy, device=dev), torch.empty(n_copy, device=dev))
            sets.append(dict(keep=(p, m, v, flat, segs_d, chunks_d, ssegs), adamw=ad, sgd=sd, copy=copy))
        fns = {"adamw": lambda k: L.call("simt_adamw_multi", C.byref(sets[k % SETS]["adamw"]), st),
               "sgd": lambda k: L.call("simt_sgd_multi", C.byref(sets[k % SETS]["sgd"]), st),
               "copy": lambda k: sets[k % SETS]["copy"][1].copy_(sets[k % SETS]["copy"][0])}
        nbytes = {"adamw": 28, "sgd": 20, "copy": 28}
        res = {n: [] for n in fns}
        for r in range(a.rounds):
            for n in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
                res[n].append(timed(fns[n]))
        small = sum(1 for _n, s, _g in table if int(np.prod(s)) < 4096)
        say(f"\n{name}: {n_el / 1e6:.2f} M elements in {len(table)} segments ({small} below 4096 elements), {len(chunks)} workgroups of {CHUNK} elements; "
            f"AdamW state {8 * n_el / 1e6:.0f} MB (m and v; v is the copy SGD does not have: {4 * n_el / 1e6:.0f} MB)")
        say(f"{'launch':>9s}  {'rounds':>{8 * a.rounds}s}  {'mean':>7s}  {'range':>15s}  {'B/elem':>6s}  {'MB':>7s}  {'TB/s':>6s}  {'x sgd':>6s}  {'x copy rate':>11s}")
        mean = {n: sum(v) / len(v) for n, v in res.items()}
        copy_rate = 28 * n_el / mean["copy"]
        for n in fns:
            rate = nbytes[n] * n_el / mean[n]
            say(f"{n:>9s}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f"  {mean[n]:7.1f}  {min(res[n]):7.1f}-{max(res[n]):<7.1f}  {nbytes[n]:6d}  "
                f"{nbytes[n] * n_el / 1e6:7.1f}  {rate / 1e6:6.2f}  {mean[n] / mean['sgd']:6.2f}  {rate / copy_rate:11.2f}")
        ratio = mean["adamw"] / mean["sgd"]
        say(f"expectation (adamw / sgd = 28 / 20 = 1.40 at a comparable fraction of the copy rate): measured {ratio:.2f}, "
            f"fractions of the copy rate {28 * n_el / mean['adamw'] / copy_rate:.2f} (adamw) and {20 * n_el / mean['sgd'] / copy_rate:.2f} (sgd)")
        del sets
        torch.cuda.empty_cache()


def step(a):
    root = os.path.abspath(a.repo or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    sys.path.insert(0, root)
    if a.late:
        os.environ["SIMT_EARLY_SGD"] = "0"
    import torch

    from simt_amd import model_spec as ms
    from simt_amd.engine import reserve_streams
    from simt_amd.step import Hyper
    dev = torch.device("cuda:0")
    reserve_streams(dev)
    cd = ms.load_class_dist("bapa")
    kw, hkw = ({}, {}) if a.optimizer is None else ({"optimizer": a.optimizer}, {"weight_decay": 0.01, "power": 1.0} if a.optimizer == "adamw" else {})
    adam = a.optimizer == "adamw"
    if a.model == "v2":
        from simt_amd.step import SimTTrainer
        B, H, W, K = 4, 768, 768, 3
        hp = Hyper(open_classes=K, lr=6e-5 if adam else 6e-4, lr_T=6e-3, **hkw)
        tr = SimTTrainer(ms.reference_init(ms.state_shapes(19, K, True), seed=1234), ms.reference_init(ms.state_shapes(19, 0, False), seed=1234),
                         ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), hp, cd, B, H, W, device=dev, **kw)
        assert tr._early_sgd == (not a.late)
    else:
        from simt_amd.engine_vgg import vgg_state_shapes
        from simt_amd.step_single import WarmupSingleTrainer
        B, H, W = 8, 512, 512
        hp = Hyper(open_classes=0, lr=6e-5 if adam else 2.5e-4, **hkw)
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
    print(json.dumps({"mode": "step", "tree": os.path.relpath(root), "model": a.model, "B": B, "size": [H, W], "optimizer": a.optimizer,
                      "late": bool(a.late), "steps": a.steps, "median_ms": round(per[len(per) // 2], 3), "wall_ms_per_step": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["launch", "step"])
    p.add_argument("--out", default=None)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=60)
    p.add_argument("--model", choices=["v2", "vgg"], default="v2")
    p.add_argument("--optimizer", choices=["sgd", "adamw"], default=None, help="default: no keyword (what the parent commit's trainers accept)")
    p.add_argument("--late", action="store_true", help="SIMT_EARLY_SGD=0: the optimiser launch behind the backward, not on the side stream")
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    a = p.parse_args()
    {"launch": launch, "step": step}[a.mode](a)
