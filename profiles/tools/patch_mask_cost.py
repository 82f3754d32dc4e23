#!/usr/bin/env python3
"""Cost of --mask-patches (simt_patch_mask, and the training tools with the flag) -> profiles/patch_mask.txt.  MEASUREMENT ONLY.

    python profiles/tools/patch_mask_cost.py launch [--out FILE] [--pairs 3] [--reps 60]
    python profiles/tools/patch_mask_cost.py tool DIR --tool trainV2_simt --model DeepLab --crop 768,768 --batch 4 [--mask-patches [R]] [--repo TREE]

launch  B = 4 at 768 x 768 and B = 8 at 512 x 512, P = 64, R = 0.7 (the draws of patch_mask.generator(1, 0), a fresh mask per buffer set),
        random fp32 images; six rotating sets of input and output buffers (0.34 GB at either size: past the caches, operands come from
        HBM); per size, in alternating order `--pairs` times, microseconds per launch over `--reps` launches between two device events
        after a warm-up: the mask in place, the mask out of place, a plain device copy of the batch (the chip's copy rate in this run) and
        simt_class_mix with apply all on (labels of 64 x 64 blocks).  Beside each mask time its byte floor -- R' * 12*B*h*w in place,
        (2 - R') * 12*B*h*w out of place, R' the share of the pixels the drawn masks blank -- and the rate that makes of the time.
        In place the launch blanks the same patches again on every pass over a set: the stores are the same.
tool    a training tool on the files of DIR (profiles/tools/loader_bench.py make DIR) with --cache-dataset device --random-mirror, with or
        without --mask-patches, for 5 epochs of the list; epochs 2-5 timed as loader_bench.py's `tool` mode times them (--repo TREE imports
        another checkout, e.g. the parent commit's, which has no such flag).  One JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time


def launch(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd.data import class_mix as cm
    from simt_amd.data import patch_mask as pm
    from simt_amd.data.pipeline import InputPrep
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    Cn, SETS, P, R = 19, 6, 64, 0.7

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

    say(f"P = {P}, R = {R}; {a.reps} launches per timing over {SETS} rotating buffer sets, {a.pairs} rounds in alternating order; us per launch")
    for B, h, w in ((4, 768, 768), (8, 512, 512)):
        rng = np.random.default_rng(B)
        prep = InputPrep(B, (h, w), (w, h), dev, class_mix=(Cn, 1.0), patch_mask=(P, R))
        gh, gw = prep.pm[2:]
        g = pm.generator(1, 0)
        xs, xo, labs, lo, words = [], [], [], [], []
        for k in range(SETS):
            xs.append(torch.randn(B, 3, h, w, device=dev))
            xo.append(torch.empty(B, 3, h, w, device=dev))
            blocks = rng.integers(0, Cn, (B, h // 64, w // 64)).astype(np.int64)
            blocks[rng.random(blocks.shape) < 0.03] = 255
            labs.append(torch.from_numpy(np.repeat(np.repeat(blocks, 64, 1), 64, 2)).to(dev))
            lo.append(torch.empty(B, h, w, dtype=torch.int64, device=dev))
            words.append(pm.draw_batch(g, B, gh, gw, R))
        share = float(np.mean([pm.blanked_share(wd, h, w, P).mean() for wd in words]))
        batch_bytes = 12 * B * h * w

        def desc(k, in_place):
            d = L.PatchMaskDesc()
            d.x, d.x_out = xs[k].data_ptr(), (xs[k] if in_place else xo[k]).data_ptr()
            d.B, d.h, d.w, d.patch = B, h, w, P
            C.memmove(d.rows, np.ascontiguousarray(words[k]).ctypes.data, B * L.PATCH_MASK_GRID * 4)
            return d

        apply_on, rank = cm.draw_batch(cm.generator(1, 0), B, Cn, 1.0)

        def mix_desc(k):
            d = L.ClassMixDesc()
            d.x, d.lab, d.x_out, d.lab_out, d.part = xs[k].data_ptr(), labs[k].data_ptr(), xo[k].data_ptr(), lo[k].data_ptr(), prep.part.data_ptr()
            d.B, d.h, d.w, d.n_classes = B, h, w, Cn
            for i in range(B):
                d.partner[i], d.apply[i] = (i + 1) % B, 1
                for c in range(Cn):
                    d.rank[i][c] = int(rank[i][c])
            return d

        descs = {"in place": [desc(k, True) for k in range(SETS)], "out of place": [desc(k, False) for k in range(SETS)],
                 "class mix": [mix_desc(k) for k in range(SETS)]}
        L.call("simt_label_presence", labs[0].data_ptr(), B, h * w, Cn, prep.part.data_ptr(), st)     # the mix reads these words
        fns = {"out of place": lambda k: L.call("simt_patch_mask", C.byref(descs["out of place"][k % SETS]), st),
               "plain copy": lambda k: xo[k % SETS].copy_(xs[k % SETS]),
               "class mix": lambda k: L.call("simt_class_mix", C.byref(descs["class mix"][k % SETS]), st),
               "in place": lambda k: L.call("simt_patch_mask", C.byref(descs["in place"][k % SETS]), st)}      # last: it changes xs
        floors = {"in place": share * batch_bytes, "out of place": (2 - share) * batch_bytes, "plain copy": 2 * batch_bytes, "class mix": None}
        res = {n: [] for n in fns}
        for p in range(a.pairs):                     # "in place" stays last in either order: the other three read the images it blanks
            names = [n for n in fns if n != "in place"]
            for n in (names if p % 2 == 0 else names[::-1]) + ["in place"]:
                res[n].append(timed(fns[n]))
        say(f"\nB = {B}, {w} x {h}: the drawn masks blank {share:.3f} of the pixels; the batch is {batch_bytes / 1e6:.1f} MB")
        say(f"{'launch':>13s}  {'rounds':>{8 * a.pairs - 1}s}  {'mean':>7s}  {'floor MB':>8s}  {'floor TB/s':>10s}")
        for n in ("in place", "out of place", "plain copy", "class mix"):
            m = sum(res[n]) / a.pairs
            f = floors[n]
            say(f"{n:>13s}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f"  {m:7.1f}  " +
                (f"{f / 1e6:8.1f}  {f / m / 1e6:10.2f}" if f is not None else f"{'-':>8s}  {'-':>10s}"))
        del xs, xo, labs, lo, descs


def tool(a):
    root = os.path.abspath(a.repo or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    sys.path.insert(0, root)
    import torch

    from simt_amd.tools import trainV1_warmup, trainV2_simt
    mod = {"trainV1_warmup": trainV1_warmup, "trainV2_simt": trainV2_simt}[a.tool]
    n = len(open(os.path.join(a.dir, "list.lst")).read().split("\n")) - 1
    per_epoch = n // a.batch
    marks = {}
    real = trainV2_simt.batches

    def timed(*args, **kw):
        it = real(*args, **kw)
        k = 0
        while True:
            if k in (per_epoch, 5 * per_epoch):            # the first pull of epoch 2, the pull after epoch 5's last step
                torch.cuda.synchronize()
                marks[k] = time.perf_counter()
            yield next(it)
            k += 1
    trainV2_simt.batches = trainV1_warmup.batches = timed
    argv = ["--model", a.model, "--input-size-target", a.crop, "--batch-size", str(a.batch), "--num-steps", "250000",
            "--num-steps-stop", str(5 * per_epoch + 1), "--save-pred-every", "1000000", "--print-every", "1000000", "--from-scratch",
            "--restore-from", "", "--snapshot-dir", tempfile.mkdtemp(), "--num-workers", str(a.workers), "--random-mirror",
            "--data-dir-target", a.dir, "--data-list-target", os.path.join(a.dir, "list.lst"), "--cache-dataset", "device"]
    if a.mask_patches is not None:
        argv += ["--mask-patches", a.mask_patches]
    mod.main(argv)
    dt = marks[5 * per_epoch] - marks[per_epoch]
    print(json.dumps({"mode": "tool", "tree": os.path.relpath(root), "tool": a.tool, "model": a.model, "crop": a.crop, "batch": a.batch,
                      "workers": a.workers, "mask_patches": a.mask_patches if a.mask_patches is not None else False, "steps": 4 * per_epoch,
                      "ms_per_step": round(dt / (4 * per_epoch) * 1e3, 3), "img_s_epochs2to5": round(4 * per_epoch * a.batch / dt, 1)}))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["launch", "tool"])
    p.add_argument("dir", nargs="?", default="")
    p.add_argument("--out", default=None)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--reps", type=int, default=60)
    p.add_argument("--crop", default="768,768")
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--tool", choices=["trainV1_warmup", "trainV2_simt"], default="trainV2_simt")
    p.add_argument("--model", default="DeepLab")
    p.add_argument("--mask-patches", type=str, nargs="?", const="0.7", default=None)
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    a = p.parse_args()
    {"launch": launch, "tool": tool}[a.mode](a)
