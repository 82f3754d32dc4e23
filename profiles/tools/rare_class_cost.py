#!/usr/bin/env python3
"""Cost of rare-class sampling (--rare-class-sampling) -> profiles/rare_class.txt.  MEASUREMENT ONLY.

    python profiles/tools/rare_class_cost.py make DIR [--frames 12]
    python profiles/tools/rare_class_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/rare_class_cost.py step DIR --model v2|vgg [--rcs] [--steps 30] [--warmup 6] [--repo TREE]

make    A GTA5-shaped source set of 1052 x 1914 frames (images/, labels/ with GTA5 ids, train.txt) made from a seed: blocky labels, a
        rectangle of a rare class in some frames; and stats.json, what simt_amd.tools.compute_class_stats writes for it.
kernel  At B = 4, 1052 x 1914 -> 768 x 768 and B = 8 -> 512 x 512, the default scale choices, K = 10 candidates per item drawn as the
        loader draws them, mirror flags mixed, in ONE run: simt_rare_crop_counts, simt_rare_crop_pick, simt_scale_crop_win and the three
        together, beside simt_scale_crop (the launch they replace) on the windows the pick chose, and simt_scale_crop without labels (the
        difference is the label half of that launch; the counts gather K windows of labels).  Device events over `--reps` back-to-back
        launches after a warm-up, `--rounds` rounds in alternating order; microseconds per launch.
step    The warm-up trainer (DeepLab-v2 B = 4 768 x 768, VGG16 B = 8 512 x 512), bf16, constructor init, online_labels = 0 and
        online_source on a resident synthetic target batch, the source pair from the REAL loader over DIR (GTA5DataSet, --scale-crop's
        default choices, mirror on, the original frames held in a device cache so that PNG decoding is not what is timed): `--steps` steps
        after `--warmup`, wall-clock milliseconds per step around a device synchronise, one JSON line.  --rcs: the dataset carries
        rare_class (T = 0.01, 3000 pixels, ratio 0.5, K = 10).  --repo TREE imports another checkout (the parent commit's, which has no
        such argument).  One process per run; the driver rotates the order of parent / off / on from round to round.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HS, WS = 1052, 1914
CASES = [("B = 4, 1052 x 1914 -> 768 x 768", 4, 768, 768), ("B = 8, 1052 x 1914 -> 512 x 512", 8, 512, 512)]
K, MIN_COUNT = 10, 1500


def make(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    from PIL import Image

    from simt_amd.dataset.gta5_dataset import GTA5DataSet
    from simt_amd.tools import compute_class_stats as stats
    g = np.random.default_rng(7)
    common = np.array([7, 8, 11, 21, 23, 26, 1], dtype=np.uint8)          # road, sidewalk, building, vegetation, sky, car, an unmapped id
    rare = [19, 25, 31, 32, 33]                                           # traffic light, rider, train, motorcycle, bicycle
    for sub in ("images", "labels"):
        os.makedirs(os.path.join(a.dir, sub), exist_ok=True)
    names = [f"{n:05d}.png" for n in range(a.frames)]
    for n, name in enumerate(names):
        blocks = common[g.integers(0, len(common), (9, 15))]
        lab = np.kron(blocks, np.ones((117, 128), dtype=np.uint8))[:HS, :WS].copy()
        if n % 2 == 0:                                                    # a 120 x 160 rectangle of a rare class somewhere
            y, x = int(g.integers(0, HS - 120)), int(g.integers(0, WS - 160))
            lab[y:y + 120, x:x + 160] = rare[(n // 2) % len(rare)]
        colour = (lab[..., None].astype(np.int64) * np.array([37, 91, 53]) % 256).astype(np.uint8)
        Image.fromarray(lab).save(os.path.join(a.dir, "labels", name))
        Image.fromarray(colour // 2 + g.integers(0, 8, (HS, WS, 3), dtype=np.uint8)).save(os.path.join(a.dir, "images", name))
    lst = os.path.join(a.dir, "train.txt")
    open(lst, "w").write("".join(n + "\n" for n in names))
    stats.main(["--data-dir", a.dir, "--data-list", lst, "--out", os.path.join(a.dir, "stats.json"), "--num-workers", "8"])
    assert len(GTA5DataSet(a.dir, lst)) == a.frames


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
    print(f"{'launch':>58}  " + " ".join(f"{'':>7}" for _ in range(rounds - 1)) + f"{'rounds':>7} {'mean':>8} {'spread':>7}")
    for n, _f in fns:
        print(f"{n:>58}  " + " ".join(f"{v:7.1f}" for v in res[n]) + f" {sum(res[n]) / len(res[n]):8.1f} {max(res[n]) - min(res[n]):7.1f}")
    return {n: sum(v) / len(v) for n, v in res.items()}


def kernel(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from simt_amd import _lib as L
    from simt_amd.data import scale_crop as sc
    from simt_amd.data.pipeline import IMG_MEAN, InputPrep
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    timed = lambda f: _timed(torch, f, a.reps)
    print(f"{a.reps} launches per timing, {a.rounds} rounds in alternating order; us per launch; K = {K} candidates, min_count = {MIN_COUNT}, "
          f"choices {' '.join(sc.DEFAULT_CHOICES)}")
    for name, B, w, h in CASES:
        g = torch.Generator().manual_seed(1)
        rgb = torch.randint(0, 256, (B, HS, WS, 3), dtype=torch.uint8, generator=g).to(dev)
        blocks = torch.randint(0, 19, (B, 9, 15), dtype=torch.uint8, generator=g)
        lab = blocks.repeat_interleave(117, 1).repeat_interleave(128, 2)[:, :HS, :WS].contiguous().to(dev)
        x = torch.empty(B, 3, h, w, device=dev)
        lo = torch.empty(B, h, w, dtype=torch.int64, device=dev)
        parts = torch.empty(B, K, L.RARE_CROP_PARTS, dtype=torch.int32, device=dev)
        win = torch.empty(B, 4, dtype=torch.int32, device=dev)
        prep = InputPrep(B, (HS, WS), (w, h), dev, mean=IMG_MEAN, scale_crop=sc.DEFAULT_CHOICES)
        bare = InputPrep(B, (HS, WS), (w, h), dev, mean=IMG_MEAN, with_label=False, scale_crop=sc.DEFAULT_CHOICES)
        draws = sc.draw_batch_candidates(np.random.default_rng(3), B, K, sc.DEFAULT_CHOICES, (w, h), True)
        cls = [int(blocks[b, 4, 7]) for b in range(B)]
        ip, lp = [rgb[b].data_ptr() for b in range(B)], [lab[b].data_ptr() for b in range(B)]
        (d,) = prep.rare_crop_descs(ip, lp, draws, cls, MIN_COUNT, x, lo, parts, win)
        prep.rare_crop_batch(ip, lp, draws, cls, MIN_COUNT, x, lo, parts, win, st)
        torch.cuda.synchronize()
        wn = win.cpu().tolist()
        chosen = (draws[0], [r[0] for r in wn], [r[1] for r in wn], [r[2] for r in wn])
        x_win, lo_win = x.clone(), lo.clone()
        prep.scale_crop_batch(ip, lp, chosen, x, lo, st)
        torch.cuda.synchronize()
        same = torch.equal(x_win.view(torch.int32), x.view(torch.int32)) and torch.equal(lo_win, lo)
        print(f"\n{name}: LDS {prep.sc.lds_bytes()} bytes, {prep.sc.max_rows} source rows per tile; picks (choice, ox, oy, count) {wn}; "
              f"simt_scale_crop_win == simt_scale_crop on those windows, bit for bit: {same}")
        call = lambda fn: (lambda: L.call(fn, C.byref(d), st))
        m = _table([("simt_rare_crop_counts", call("simt_rare_crop_counts")),
                    ("simt_rare_crop_pick", call("simt_rare_crop_pick")),
                    ("simt_scale_crop_win", call("simt_scale_crop_win")),
                    ("counts + pick + simt_scale_crop_win", lambda: prep.rare_crop_batch(ip, lp, draws, cls, MIN_COUNT, x, lo, parts, win, st)),
                    ("simt_scale_crop on the picked windows (the parent's launch)", lambda: prep.scale_crop_batch(ip, lp, chosen, x, lo, st)),
                    ("simt_scale_crop, images only (lab_out NULL)", lambda: bare.scale_crop_batch(ip, [None] * B, chosen, x, None, st))],
                   a.rounds, timed)
        half = m["simt_scale_crop on the picked windows (the parent's launch)"] - m["simt_scale_crop, images only (lab_out NULL)"]
        print(f"label half of simt_scale_crop: {half:.1f} us; K x that: {K * half:.1f} us; simt_rare_crop_counts: {m['simt_rare_crop_counts']:.1f} us")
        del rgb, lab, x, lo, prep, bare


def step(a):
    tree = os.path.abspath(a.repo) if a.repo else ROOT
    sys.path.insert(0, tree)
    import torch

    import simt_amd
    from simt_amd import model_spec as ms
    from simt_amd.data.cache import DatasetCache
    from simt_amd.data.pipeline import IMG_MEAN, GpuLoader
    from simt_amd.data.scale_crop import DEFAULT_CHOICES
    from simt_amd.dataset.gta5_dataset import GTA5DataSet
    from simt_amd.step import Hyper, WarmupTrainer
    assert os.path.dirname(os.path.dirname(os.path.abspath(simt_amd.__file__))) == tree
    dev = torch.device("cuda:0")
    cd = ms.load_class_dist("bapa")
    kw = {"online_labels": 0.0, "online_source": True}
    hp = Hyper(num_classes=19, open_classes=0, lr=2.5e-4)
    if a.model == "v2":
        B, H, W = 4, 768, 768
        tr = WarmupTrainer(ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), hp, B, H, W, device=dev, **kw)
    else:
        from simt_amd.step_single import WarmupSingleTrainer
        from simt_amd.tools.trainV2_simt import single_model_state
        B, H, W = 8, 512, 512
        tr = WarmupSingleTrainer("vgg", single_model_state("DeepLabVGG", 19), hp, B, H, W, device=dev, **kw)
    dkw = {}
    if a.rcs:
        from simt_amd.data import rare_class
        probe = GTA5DataSet(a.dir, os.path.join(a.dir, "train.txt"))
        dkw["rare_class"] = rare_class.RareClass(rare_class.load_stats(os.path.join(a.dir, "stats.json"), probe), 0.01, 3000, "0.5", K)
    ds = GTA5DataSet(a.dir, os.path.join(a.dir, "train.txt"), crop_size=(W, H), scale=False, mirror=True, mean=IMG_MEAN, scale_crop=DEFAULT_CHOICES,
                     **dkw)
    cache = DatasetCache((WS, HS), with_label=True, budget_bytes=int(2e9), device=dev)
    loader = GpuLoader(ds, B, shuffle=True, num_workers=8, device=dev, seed=1234 + 0x5372, cache=cache)
    src = iter(loader)
    img, _lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    met, n = torch.zeros((), dtype=torch.int64, device=dev), 0

    def one():
        nonlocal n
        sx, sl = next(src)[:2]
        if a.rcs:
            met.add_((loader.last_windows()[:, 3] > ds.rare_class.min_count).sum())
            n += B
        tr.step(img, source_image=sx, source_label=sl)
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    print(json.dumps({"model": a.model, "tree": "parent" if a.repo else "this", "rcs": a.rcs, "steps": a.steps,
                      "ms_per_step": round(dt * 1e3 / a.steps, 3), "images_per_s": round(B * a.steps / dt, 2), "source_seg2": l.get("source_seg2"),
                      "rcs_share": round(int(met.item()) / n, 3) if n else None, "cache_hits": cache.hits, "cache_misses": cache.misses}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    m = sub.add_parser("make")
    m.add_argument("dir")
    m.add_argument("--frames", type=int, default=12)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    s = sub.add_parser("step")
    s.add_argument("dir")
    s.add_argument("--model", choices=["v2", "vgg"], required=True)
    s.add_argument("--rcs", action="store_true")
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    {"make": make, "kernel": kernel, "step": step}[a.mode](a)


if __name__ == "__main__":
    main()
