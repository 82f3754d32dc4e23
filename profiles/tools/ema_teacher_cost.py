#!/usr/bin/env python3
"""Cost of the EMA teacher's refresh (simt_amd/ema_teacher.py) and of a training step with it -> profiles/ema_teacher.txt.  MEASUREMENT ONLY.

    python profiles/tools/ema_teacher_cost.py refresh [--out FILE] [--rounds 3] [--reps 40]
    python profiles/tools/ema_teacher_cost.py step [--ema 0.999] [--ema-teacher 1] [--steps 40] [--warmup 10] [--repo TREE]

refresh the frozen plans of DeepLab-v2 R-101 (B = 4, 768 x 768), DeepLabv3 R-50 (B = 4, 512 x 1024) and DeepLab-VGG16 (B = 8, 512 x 512), bf16,
        each inside its SimT trainer built with ema_decay and ema_teacher_every = 1; `--rounds` rounds in alternating order.  Per entry two
        figures, microseconds per replay: GPU time (`--reps` replays between two device events after a warm-up) and the HOST time to enqueue
        (a host clock around the same replays on an idle stream, before the synchronise that ends the timing):
          copy        simt_ema_multi, omd = 1, shadow -> fixed_params
          fold multi  simt_bn_fold_multi over every BatchNorm of the plan, one launch          (absent for VGG16: nothing to fold)
          fold chain  the plan's own simt_bn_fold launches, one per BatchNorm: what `fold multi` replaces
          rest        the pack list without its folds: simt_pack_weight_multi, simt_stem7_pack, simt_vec_acc
          refresh     the whole launch list (copy + fold multi + rest), as TeacherRefresh.run replays it
          repack      fixed.repack(): fold chain + rest, the launches of the parent commit
        The bar: `fold multi` takes no longer than `fold chain`, on the GPU and on the host, in every round.
step    DeepLab-v2 SimT B = 4 at 768 x 768, bf16, on a resident synthetic batch, `--steps` steps after `--warmup`: median milliseconds per step
        from device events and wall-clock milliseconds per step, one JSON line.  --ema D passes ema_decay, --ema-teacher N ema_teacher_every;
        --repo TREE imports another checkout (the parent commit's, which has no ema_teacher_every: then --ema-teacher is an error).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _trainers(torch, dev):
    """name -> constructor of the SimT trainer whose frozen plan is measured (built one at a time: each is released before the next)."""
    from simt_amd import model_spec as ms
    from simt_amd.step import Hyper, SimTTrainer
    from simt_amd.step_single import SimTSingleTrainer
    from simt_amd.tools.trainV2_simt import single_model_states
    cd = ms.load_class_dist("bapa")
    K = 15
    hp = lambda: Hyper(open_classes=K, lr=6e-4, lr_T=6e-3)
    kw = dict(device=dev, ema_decay=0.999, ema_teacher_every=1)

    def v2():
        return SimTTrainer(ms.reference_init(ms.state_shapes(19, K, True), seed=1234), ms.trained_like_init(ms.state_shapes(19, 0, False), seed=7),
                           ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), hp(), cd, 4, 768, 768, **kw)

    def single(model, name, B, H, W):
        def make():
            st, fst = single_model_states(name, 19, K)
            return SimTSingleTrainer(model, st, fst, ms.ntm_init(19, K, 1), hp(), cd, B, H, W, **kw)
        return make
    return {"DeepLab-v2 R-101, B = 4, 768 x 768": v2, "DeepLabv3 R-50, B = 4, 512 x 1024": single("v3", "DeepLabv3", 4, 512, 1024),
            "DeepLab-VGG16, B = 8, 512 x 512": single("vgg", "DeepLabVGG", 8, 512, 512)}


def refresh(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    lib = L.load()
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream

    def replay(launches):
        for fn, args in launches:
            rc = fn(*args, st)
            if rc != 0:
                L.check(rc)

    def timed(launches):
        """(GPU us per replay, host us to enqueue one replay)."""
        for _ in range(3):
            replay(launches)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            replay(launches)
        host = (time.perf_counter() - t0) * 1e6 / a.reps
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps, host

    say(f"{a.reps} replays per timing, {a.rounds} rounds in alternating order; per replay: GPU us (device events) / host us to enqueue")
    for name, make in _trainers(torch, dev).items():
        tr = make()
        t = tr.teacher
        raw = tr.fixed._pack_items_raw
        chain = [(it.fn, it.args) for it in raw if it.fn is lib.simt_bn_fold]
        multi = [(fn, args) for fn, args in t.launches if fn is lib.simt_bn_fold_multi]
        copy = [(fn, args) for fn, args in t.launches if fn is lib.simt_ema_multi]
        rest = [(fn, args) for fn, args in t.launches if fn not in (lib.simt_bn_fold_multi, lib.simt_ema_multi)]
        repack = [(it.fn, it.args) for it in tr.fixed.pack_list.items]
        sets = {"copy": copy, "fold multi": multi, "fold chain": chain, "rest": rest, "refresh": list(t.launches), "repack": repack}
        sets = {k: v for k, v in sets.items() if v}
        res = {k: [] for k in sets}
        for r in range(a.rounds):
            for k in (list(sets) if r % 2 == 0 else list(sets)[::-1]):
                res[k].append(timed(sets[k]))
        channels = sum(it.args[7] for it in raw if it.fn is lib.simt_bn_fold)
        say(f"\n{name}: {t.elements / 1e6:.2f} M elements copied in {t.copy_desc.nchunks} workgroups; {len(chain)} BatchNorm folds, {channels} channels, "
            f"{t.fold_desc.nchunks if t.fold_desc is not None else 0} workgroups of simt_bn_fold_multi; {len(rest)} other pack-list launches")
        say(f"{'entry':>11s}  {'launches':>8s}  {'GPU us by round':>{8 * a.rounds}s}  {'mean':>7s}  {'host us by round':>{8 * a.rounds}s}  {'mean':>7s}")
        for k, v in res.items():
            g, h = [x[0] for x in v], [x[1] for x in v]
            say(f"{k:>11s}  {len(sets[k]):8d}  " + " ".join(f"{x:7.1f}" for x in g) + f"  {sum(g) / len(g):7.1f}  " +
                " ".join(f"{x:7.1f}" for x in h) + f"  {sum(h) / len(h):7.1f}")
        if multi:
            ok = all(m[0] <= c[0] and m[1] <= c[1] for m, c in zip(res["fold multi"], res["fold chain"]))
            say(f"bar (fold multi <= fold chain, GPU and host, in every round): {'HOLDS' if ok else 'MISSED'}")
        del tr, t, sets
        torch.cuda.empty_cache()


def step(a):
    root = os.path.abspath(a.repo or ROOT)
    sys.path.insert(0, root)
    import torch

    from simt_amd import model_spec as ms
    from simt_amd.engine import reserve_streams
    from simt_amd.step import Hyper, SimTTrainer
    dev = torch.device("cuda:0")
    reserve_streams(dev)
    cd = ms.load_class_dist("bapa")
    kw = {} if a.ema is None else {"ema_decay": a.ema}
    if a.ema_teacher is not None:
        kw["ema_teacher_every"] = a.ema_teacher
    B, H, W, K = 4, 768, 768, 3
    hp = Hyper(open_classes=K, lr=6e-4, lr_T=6e-3)
    tr = SimTTrainer(ms.reference_init(ms.state_shapes(19, K, True), seed=1234), ms.reference_init(ms.state_shapes(19, 0, False), seed=1234),
                     ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), hp, cd, B, H, W, device=dev, **kw)
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
    print(json.dumps({"mode": "step", "tree": os.path.relpath(root), "B": B, "size": [H, W], "ema": a.ema, "ema_teacher": a.ema_teacher,
                      "refreshes": getattr(getattr(tr, "teacher", None), "refreshes", 0), "steps": a.steps,
                      "median_ms": round(per[len(per) // 2], 3), "wall_ms_per_step": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["refresh", "step"])
    p.add_argument("--out", default=None)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--ema", type=float, default=None)
    p.add_argument("--ema-teacher", type=int, default=None)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    a = p.parse_args()
    {"refresh": refresh, "step": step}[a.mode](a)
