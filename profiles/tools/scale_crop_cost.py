#!/usr/bin/env python3
"""Cost of --scale-crop (simt_scale_crop and the training tools with it) -> profiles/scale_crop.txt.  MEASUREMENT ONLY.

    python profiles/tools/scale_crop_cost.py launch [--out FILE] [--pairs 3] [--reps 50]
    python profiles/tools/scale_crop_cost.py tool DIR --tool trainV1_warmup --model DeepLabVGG --crop 512,512 --batch 8 [--scale-crop [S ...]]

launch  B = 4 frames of 1024 x 2048 -> crop (1024, 512), mirror flags mixed, every item at the same choice, origins in the middle of their
        ranges; per default choice, in alternating order (a b, then b a) `--pairs` times, microseconds per launch over `--reps` launches
        between two device events after a warm-up:
          scale_crop    ONE simt_scale_crop launch
          composition   the existing launches that yield the same bytes: two full-frame simt_resample_u8 (x, then y), the window copy of
                        image and label (device-to-device slice copies), simt_image_to_input at the crop and simt_label_nearest at the
                        scaled size
        and, once, the parent's simt_cache_gather on a B = 4 batch of that crop: the floor an unscaled cached batch pays.
tool    a training tool on the files of DIR (profiles/tools/loader_bench.py make DIR) with --cache-dataset device --random-mirror, with or
        without --scale-crop, for 5 epochs of the list; epochs 2-5 timed as loader_bench.py's `tool` mode times them.  One JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def launch(a):
    import torch

    from simt_amd import _lib as L
    from simt_amd.data import scale_crop as sc
    from simt_amd.data.cache import DatasetCache
    from simt_amd.data.pipeline import IMG_MEAN, InputPrep
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    B, Hs, Ws, w, h = 4, 1024, 2048, 1024, 512
    st = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator().manual_seed(1)
    rgb = torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 19, (B, Hs, Ws), dtype=torch.uint8, generator=g).to(dev)
    x = torch.empty(B, 3, h, w, device=dev)
    lo = torch.empty(B, h, w, dtype=torch.int64, device=dev)
    mirror = [False, True, False, True]
    choices = sc.DEFAULT_CHOICES
    prep = InputPrep(B, (Hs, Ws), (w, h), dev, mean=IMG_MEAN, scale_crop=choices)
    say(f"B = {B}, {Ws} x {Hs} -> crop {w} x {h}; {a.reps} launches per timing, {a.pairs} rounds in alternating order; us per launch")
    say(f"simt_scale_crop: {prep.sc.max_rows} source rows per tile at most, {prep.sc.lds_bytes()} bytes of LDS per workgroup")

    def timed(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    # the floor: the parent's gather of a cached batch at the crop
    cache = DatasetCache((w, h), slab_slots=8, device=dev)
    slots = [cache.reserve((str(i), "l")) for i in range(B)]
    for s in cache.slabs:
        s[0].random_(0, 256)
        s[1].random_(0, 19)
    plain = InputPrep(B, (h, w), (w, h), dev, mean=IMG_MEAN)
    ip, lp = [cache.img_ptr(s) for s in slots], [cache.lab_ptr(s) for s in slots]
    gather = [timed(lambda: plain.gather(ip, lp, mirror, x, lo, st)) for _ in range(a.pairs)]
    floor = sum(gather) / len(gather)
    say(f"\nsimt_cache_gather, B = {B}, crop {w} x {h}: " + "  ".join(f"{v:7.1f}" for v in gather) + f"   mean {floor:7.1f} us")
    say(f"\n{'choice':>6s} {'scaled':>11s}  {'scale_crop':>30s}  {'composition':>30s}  {'ratio':>6s} {'x gather':>8s}")
    img_ptrs, lab_ptrs = [rgb[b].data_ptr() for b in range(B)], [lab[b].data_ptr() for b in range(B)]
    worst = 0.0
    for ci, c in enumerate(choices):
        e = prep.sc.entries[ci]
        ws, hs = e["ws"], e["hs"]
        ox = sum(sc.origin_range(ws, w)) // 2
        oy = sum(sc.origin_range(hs, h)) // 2
        draws = (mirror, [ci] * B, [ox] * B, [oy] * B)
        full = InputPrep(B, (Hs, Ws), (ws, hs), dev, mean=IMG_MEAN)          # the whole frame at the scaled size: the existing launches
        S = torch.empty(B, hs, ws, 3, dtype=torch.uint8, device=dev)
        Ln = torch.empty(B, hs, ws, dtype=torch.int64, device=dev)
        win = torch.zeros(B, h, w, 3, dtype=torch.uint8, device=dev)
        ya, yb, xa, xb = max(0, -oy), min(h, hs - oy), max(0, -ox), min(w, ws - ox)

        def composition():
            cur = rgb
            if full.need_x:
                L.call("simt_resample_u8", cur.data_ptr(), full.tmp_x.data_ptr(), B, Hs, Ws, 3, ws, 1, full.bx.data_ptr(), full.cx.data_ptr(),
                       full.kx, st)
                cur = full.tmp_x
            if full.need_y:
                L.call("simt_resample_u8", cur.data_ptr(), S.data_ptr(), B, Hs, ws, 3, hs, 0, full.by.data_ptr(), full.cy.data_ptr(), full.ky, st)
                cur = S
            win[:, ya:yb, xa:xb].copy_(cur[:, ya + oy:yb + oy, xa + ox:xb + ox])
            L.call("simt_image_to_input", win.data_ptr(), x.data_ptr(), B, h, w, *plain.mean, 0, st)
            L.call("simt_label_nearest", lab.data_ptr(), Ln.data_ptr(), B, Hs, Ws, hs, ws, full.ytab.data_ptr(), full.xtab.data_ptr(), 0, st)
            lo[:, ya:yb, xa:xb].copy_(Ln[:, ya + oy:yb + oy, xa + ox:xb + ox])

        def one():
            prep.scale_crop_batch(img_ptrs, lab_ptrs, draws, x, lo, st)

        res = {"one": [], "comp": []}
        for p in range(a.pairs):
            for name, fn in ((("one", one), ("comp", composition)) if p % 2 == 0 else (("comp", composition), ("one", one))):
                res[name].append(timed(fn))
        m1, m2 = sum(res["one"]) / a.pairs, sum(res["comp"]) / a.pairs
        worst = max(worst, m1 / m2)
        say(f"{c:>6s} {ws:5d}x{hs:<5d}  " + " ".join(f"{v:7.1f}" for v in res["one"]) + f" = {m1:7.1f}  " +
            " ".join(f"{v:7.1f}" for v in res["comp"]) + f" = {m2:7.1f}  {m1 / m2:6.2f} {m1 / floor:8.2f}")
        del full, S, Ln, win
    say(f"\nworst scale_crop / composition over the choices: {worst:.2f}")


def tool(a):
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
    if a.scale_crop is not None:
        argv += ["--scale-crop"] + a.scale_crop
    mod.main(argv)
    dt = marks[5 * per_epoch] - marks[per_epoch]
    print(json.dumps({"mode": "tool", "tool": a.tool, "model": a.model, "crop": a.crop, "batch": a.batch, "workers": a.workers,
                      "scale_crop": a.scale_crop if a.scale_crop is not None else False, "steps": 4 * per_epoch,
                      "ms_per_step": round(dt / (4 * per_epoch) * 1e3, 3), "img_s_epochs2to5": round(4 * per_epoch * a.batch / dt, 1)}))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["launch", "tool"])
    p.add_argument("dir", nargs="?", default="")
    p.add_argument("--out", default=None)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--crop", default="512,512")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--tool", choices=["trainV1_warmup", "trainV2_simt"], default="trainV1_warmup")
    p.add_argument("--model", default="DeepLabVGG")
    p.add_argument("--scale-crop", type=str, nargs="*", default=None)
    a = p.parse_args()
    {"launch": launch, "tool": tool}[a.mode](a)
