#!/usr/bin/env python3
"""Cost of --colour-jitter / --gaussian-blur (simt_grey_mean_parts + simt_photometric, and the training tools with the flags)
-> profiles/photometric.txt.  MEASUREMENT ONLY.

    python profiles/tools/photometric_cost.py launch [--out FILE] [--pairs 3] [--reps 60]
    python profiles/tools/photometric_cost.py tool DIR --tool trainV2_simt --model DeepLab --crop 768,768 --batch 4 [--photometric] [--repo TREE]

launch  B = 4 at 768 x 768 and B = 8 at 512 x 512, uint8 colours minus the mean; six rotating sets of input and output buffers (past the
        caches, operands come from HBM); per size, in alternating order (a b ..., then ... b a) `--pairs` times, microseconds per launch
        over `--reps` launches between two device events after a warm-up: the grey-mean launch alone (all items jittered) and the
        photometric launch in its four flavours (every item of the batch the same: copy, jitter only, blur only, both).  Beside each the
        byte floor of 24 bytes per pixel (12 read + 12 written; the grey mean: 12 read) and the rate that makes of the time; and, re-measured
        in the same run as the chip's plain-copy yardsticks, simt_class_mix with apply all off (40 bytes per pixel, a pure copy) and with
        apply all on.
tool    a training tool on the files of DIR (profiles/tools/loader_bench.py make DIR) with --cache-dataset device --random-mirror, with or
        without --colour-jitter --gaussian-blur (their default values), for 5 epochs of the list; epochs 2-5 timed as loader_bench.py's
        `tool` mode times them (--repo TREE imports another checkout, e.g. the parent commit's, which has no such flags).  One JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

COPY_TB_S = (5.2, 5.9)      # plain streaming copy on this chip, read + write


def launch(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd.data import class_mix as cm
    from simt_amd.data import photometric as ph
    from simt_amd.data.pipeline import IMG_MEAN, InputPrep
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    Cn, SETS = 19, 6

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

    say(f"{a.reps} launches per timing over {SETS} rotating buffer sets, {a.pairs} rounds in alternating order; us per launch; "
        f"floor = bytes / time at {COPY_TB_S[0]}-{COPY_TB_S[1]} TB/s (the chip's plain copy)")
    for B, h, w in ((4, 768, 768), (8, 512, 512)):
        rng = np.random.default_rng(B)
        prep = InputPrep(B, (h, w), (w, h), dev, class_mix=(Cn, 1.0), photometric=(0.2, 0.5))
        mean = torch.tensor(IMG_MEAN, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
        xs, labs, xo, lo = [], [], [], []
        for k in range(SETS):
            blocks = rng.integers(0, Cn, (B, h // 64, w // 64)).astype(np.int64)
            labs.append(torch.from_numpy(np.repeat(np.repeat(blocks, 64, 1), 64, 2)).to(dev))
            xs.append(torch.randint(0, 256, (B, 3, h, w), device=dev).float() - mean)
            xo.append(torch.empty(B, 3, h, w, device=dev))
            lo.append(torch.empty(B, h, w, dtype=torch.int64, device=dev))
        px = B * h * w
        draws = ph.draw_batch(ph.generator(1, 0), B, (0.2, 0.5))
        apply_on, rank = cm.draw_batch(cm.generator(1, 0), B, Cn, 1.0)

        def pdesc(k, jit, blur):
            d = L.PhotometricDesc()
            d.x, d.x_out, d.part = xs[k].data_ptr(), xo[k].data_ptr(), prep.grey_part.data_ptr()
            d.inv, d.B, d.h, d.w = ph.inv_pixels(h, w), B, h, w
            d.mean[0], d.mean[1], d.mean[2] = prep.mean
            for i in range(B):
                fb, fc, omfc, A, wk = ph.item_params(draws["fb"][i], draws["fc"][i], draws["fs"][i], draws["theta"][i], draws["sigma"][i])
                d.jit[i], d.blur[i], d.fb[i], d.fc[i], d.omfc[i] = jit, blur, float(fb), float(fc), float(omfc)
                C.memmove(d.A[i], np.ascontiguousarray(A, dtype=np.float32).ctypes.data, 36)
                C.memmove(d.wk[i], np.ascontiguousarray(wk, dtype=np.float32).ctypes.data, 24)
            return d

        def mdesc(k, apply):
            d = L.ClassMixDesc()
            d.x, d.lab, d.x_out, d.lab_out, d.part = xs[k].data_ptr(), labs[k].data_ptr(), xo[k].data_ptr(), lo[k].data_ptr(), prep.part.data_ptr()
            d.B, d.h, d.w, d.n_classes = B, h, w, Cn
            for i in range(B):
                d.partner[i], d.apply[i] = (i + 1) % B, 1 if apply[i] else 0
                for c in range(Cn):
                    d.rank[i][c] = int(rank[i][c])
            return d

        flavours = {"copy": (0, 0), "jitter": (1, 0), "blur": (0, 1), "both": (1, 1)}
        descs = {n: [pdesc(k, *f) for k in range(SETS)] for n, f in flavours.items()}
        descs["mix off"] = [mdesc(k, np.zeros(B, bool)) for k in range(SETS)]
        descs["mix on"] = [mdesc(k, apply_on) for k in range(SETS)]
        fns = {"grey mean": lambda k: L.call("simt_grey_mean_parts", C.byref(descs["both"][k % SETS]), st)}
        for n in flavours:
            fns[n] = lambda k, n=n: L.call("simt_photometric", C.byref(descs[n][k % SETS]), st)
        for n in ("mix off", "mix on"):
            fns[n] = lambda k, n=n: L.call("simt_class_mix", C.byref(descs[n][k % SETS]), st)
        L.call("simt_label_presence", labs[0].data_ptr(), B, h * w, Cn, prep.part.data_ptr(), st)      # the mix reads these words
        fns["grey mean"](0)                                                                             # the jitter reads these
        floors = {"grey mean": 12 * px, "copy": 24 * px, "jitter": 24 * px, "blur": 24 * px, "both": 24 * px, "mix off": 40 * px,
                  "mix on": 44 * px}                    # (mix on: 40-48 by the paste mask; about half of the pixels are not pasted)
        res = {n: [] for n in fns}
        for p in range(a.pairs):
            for n in (list(fns) if p % 2 == 0 else list(fns)[::-1]):
                res[n].append(timed(fns[n]))
        say(f"\nB = {B}, {w} x {h}")
        say(f"{'launch':>9s}  {'rounds':>{8 * a.pairs}s}  {'mean':>7s}  {'MB':>7s}  {'floor us':>13s}  {'TB/s':>5s}  {'x floor':>11s}  {'x mix on':>8s}")
        mix_on = sum(res["mix on"]) / a.pairs
        for n in fns:
            m = sum(res[n]) / a.pairs
            f_lo, f_hi = floors[n] / COPY_TB_S[1] / 1e6, floors[n] / COPY_TB_S[0] / 1e6
            say(f"{n:>9s}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f"  {m:7.1f}  {floors[n] / 1e6:7.1f}  {f_lo:6.1f}-{f_hi:<6.1f}  "
                f"{floors[n] / m / 1e6:5.2f}  {m / f_hi:5.2f}-{m / f_lo:<5.2f}  {m / mix_on:8.2f}")
        del xs, labs, xo, lo, descs


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
    if a.photometric:
        argv += ["--colour-jitter", "--gaussian-blur"]
    mod.main(argv)
    dt = marks[5 * per_epoch] - marks[per_epoch]
    print(json.dumps({"mode": "tool", "tree": os.path.relpath(root), "tool": a.tool, "model": a.model, "crop": a.crop, "batch": a.batch,
                      "workers": a.workers, "photometric": bool(a.photometric), "steps": 4 * per_epoch,
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
    p.add_argument("--photometric", action="store_true", help="pass --colour-jitter --gaussian-blur (their default values)")
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    a = p.parse_args()
    {"launch": launch, "tool": tool}[a.mode](a)
