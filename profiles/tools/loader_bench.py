"""The input pipeline on real files, with and without the device-resident dataset cache.  MEASUREMENT ONLY (profiles/dataset_cache.txt).

    python profiles/tools/loader_bench.py make   DIR [--n 64]
    python profiles/tools/loader_bench.py loader DIR --crop 1024,512 --batch 4 --workers 4 --epochs 5 [--cache device] [--repo TREE]
    python profiles/tools/loader_bench.py gather                      (under rocprofv3 --kernel-trace --stats for the kernel's own time)
    python profiles/tools/loader_bench.py tool   DIR --tool trainV1_warmup --model DeepLabVGG --crop 512,512 --batch 8 --feed synthetic|resident|off|device

make    writes N frames of 1024 x 2048 blurred noise (PNG, Pillow's default compression) and block-constant 19-class labels, plus the
        list file, once; prints the mean file sizes.
loader  drives the public GpuLoader alone (so that it also runs on a tree without the cache: --repo names the tree to import
        simt_amd from): images/s per epoch, device synchronised at each epoch's end.
gather  launches simt_cache_gather 50 times at B=4 1024x512, B=4 768x768, B=8 512x512 on slots spread over a cache of 64 items.
tool    runs a training tool on the files (or --synthetic) for 5 epochs of the list and times epochs 2-5: the tool's `batches` iterator
        is wrapped, the device is synchronised at the first pull of epoch 2 and at the pull after epoch 5, nothing else is touched.
        --feed resident hands out ONE synthetic batch again and again (the tools' --synthetic generates a new batch per step, which
        costs more than the step of the fast models): the step rate with no input work at all.
Each prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time


def _repo(path):
    root = os.path.abspath(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    sys.path.insert(0, root)
    return root


def _one_frame(job):
    root, i = job
    import numpy as np
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(i)
    img = Image.fromarray(rng.integers(0, 256, (1024, 2048, 3), dtype=np.uint8)).filter(ImageFilter.GaussianBlur(2.4))
    img.save(os.path.join(root, "img", f"f{i:03d}.png"))
    lab = np.repeat(np.repeat(rng.integers(0, 19, (16, 32), dtype=np.uint8), 64, 0), 64, 1)
    Image.fromarray(lab).save(os.path.join(root, "lab", f"f{i:03d}.png"))
    return os.path.getsize(os.path.join(root, "img", f"f{i:03d}.png")), os.path.getsize(os.path.join(root, "lab", f"f{i:03d}.png"))


def make(a):
    from concurrent.futures import ProcessPoolExecutor
    for d in ("img", "lab"):
        os.makedirs(os.path.join(a.dir, d), exist_ok=True)
    with ProcessPoolExecutor(min(16, a.n)) as pool:
        sizes = list(pool.map(_one_frame, [(a.dir, i) for i in range(a.n)]))
    with open(os.path.join(a.dir, "list.lst"), "w") as f:
        f.write("".join(f"img/f{i:03d}.png lab/f{i:03d}.png\n" for i in range(a.n)))
    print(json.dumps({"mode": "make", "n": a.n, "mean_image_png_bytes": sum(s[0] for s in sizes) // a.n,
                      "mean_label_png_bytes": sum(s[1] for s in sizes) // a.n}))


def loader(a):
    root = _repo(a.repo)
    import torch
    from simt_amd.data.pipeline import IMG_MEAN, GpuLoader
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    dev = torch.device("cuda:0")
    w, h = (int(v) for v in a.crop.split(","))
    ds = cityscapesPseudo(a.dir, os.path.join(a.dir, "list.lst"), crop_size=(w, h), scale=False, mirror=True, mean=IMG_MEAN)
    kw = {}
    if a.cache == "device":
        from simt_amd.data.cache import DatasetCache
        kw["cache"] = DatasetCache((w, h), device=dev)
    nb = len(ds) // a.batch
    torch.cuda.synchronize()
    rates, k, t0 = [], 0, time.perf_counter()
    sink = torch.zeros((), device=dev)
    for x, lab, _s, _n in GpuLoader(ds, a.batch, shuffle=True, num_workers=a.workers, device=dev, seed=1234, epochs=a.epochs, **kw):
        sink += x[0, 0, 0, 0] + lab[0, 0, 0]                # a consumer on the current stream, like a step's first kernel
        k += 1
        if k % nb == 0:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rates.append(round(nb * a.batch / (t1 - t0), 1))
            t0 = t1
    later = rates[1:]
    print(json.dumps({"mode": "loader", "tree": os.path.relpath(root), "cache": a.cache, "crop": a.crop, "batch": a.batch, "workers": a.workers,
                      "epoch1_img_s": rates[0], "epochs2plus_img_s": round(len(later) * nb * a.batch / sum(nb * a.batch / r for r in later), 1),
                      "per_epoch_img_s": rates}))


def gather(a):
    _repo(a.repo)
    import torch
    from simt_amd.data.cache import DatasetCache
    from simt_amd.data.pipeline import IMG_MEAN, InputPrep
    dev = torch.device("cuda:0")
    out = []
    for B, (w, h) in ((4, (1024, 512)), (4, (768, 768)), (8, (512, 512))):
        cache = DatasetCache((w, h), slab_slots=16, device=dev)
        slots = [cache.reserve((str(i), "l")) for i in range(64)]
        for s in cache.slabs:
            s[0].random_(0, 256)
            s[1].random_(0, 19)
        prep = InputPrep(B, (h, w), (w, h), dev, mean=IMG_MEAN)
        xs = [torch.empty(B, 3, h, w, device=dev) for _ in range(4)]                 # rotating outputs, like the prefetcher's slots
        ls = [torch.empty(B, h, w, dtype=torch.int64, device=dev) for _ in range(4)]
        st = torch.cuda.current_stream(dev).cuda_stream
        g = torch.Generator().manual_seed(B)
        picks = [torch.randperm(64, generator=g)[:B].tolist() for _ in range(60)]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it, pick in enumerate(picks):
            if it == 10:
                ev0.record()
            prep.gather([cache.img_ptr(slots[p]) for p in pick], [cache.lab_ptr(slots[p]) for p in pick], [p % 2 == 0 for p in pick],
                        xs[it % 4], ls[it % 4], st)
        ev1.record()
        torch.cuda.synchronize()
        us = ev0.elapsed_time(ev1) * 1000 / 50
        out.append({"B": B, "crop": f"{w},{h}", "bytes": 24 * h * w * B, "us_per_launch_back_to_back": round(us, 1),
                    "TB_s": round(24 * h * w * B / us / 1e6, 2)})
    print(json.dumps({"mode": "gather", "cases": out}))


def tool(a):
    _repo(a.repo)
    import torch
    from simt_amd.tools import trainV1_warmup, trainV2_simt
    mod = {"trainV1_warmup": trainV1_warmup, "trainV2_simt": trainV2_simt}[a.tool]
    w, h = (int(v) for v in a.crop.split(","))
    n = len(open(os.path.join(a.dir, "list.lst")).read().split("\n")) - 1
    per_epoch = n // a.batch
    marks = {}
    real = trainV2_simt.batches

    def timed(*args, **kw):
        it = real(*args, **kw)
        k, first = 0, None
        while True:
            if k in (per_epoch, 5 * per_epoch):            # the first pull of epoch 2, the pull after epoch 5's last step
                torch.cuda.synchronize()
                marks[k] = time.perf_counter()
            if a.feed == "resident":                       # one synthetic batch, handed out again and again: the step alone
                first = next(it) if first is None else first
                yield first
            else:
                yield next(it)
            k += 1
    trainV2_simt.batches = trainV1_warmup.batches = timed
    snap = tempfile.mkdtemp()
    argv = ["--model", a.model, "--input-size-target", a.crop, "--batch-size", str(a.batch), "--num-steps", "250000",
            "--num-steps-stop", str(5 * per_epoch + 1), "--save-pred-every", "1000000", "--print-every", "1000000", "--from-scratch",
            "--restore-from", "", "--snapshot-dir", snap, "--num-workers", str(a.workers), "--random-mirror"]
    if a.feed in ("synthetic", "resident"):
        argv += ["--synthetic"]
    else:
        argv += ["--data-dir-target", a.dir, "--data-list-target", os.path.join(a.dir, "list.lst")]
        if a.feed == "device":
            argv += ["--cache-dataset", "device"]
    mod.main(argv)
    dt = marks[5 * per_epoch] - marks[per_epoch]
    print(json.dumps({"mode": "tool", "tool": a.tool, "model": a.model, "crop": a.crop, "batch": a.batch, "workers": a.workers, "feed": a.feed,
                      "steps": 4 * per_epoch, "ms_per_step": round(dt / (4 * per_epoch) * 1e3, 3),
                      "img_s_epochs2to5": round(4 * per_epoch * a.batch / dt, 1)}))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["make", "loader", "gather", "tool"])
    p.add_argument("dir", nargs="?", default="")
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--crop", default="1024,512")
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--cache", choices=["off", "device"], default="off")
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    p.add_argument("--tool", choices=["trainV1_warmup", "trainV2_simt"], default="trainV1_warmup")
    p.add_argument("--model", default="DeepLabVGG")
    p.add_argument("--feed", choices=["synthetic", "resident", "off", "device"], default="device")
    a = p.parse_args()
    {"make": make, "loader": loader, "gather": gather, "tool": tool}[a.mode](a)
