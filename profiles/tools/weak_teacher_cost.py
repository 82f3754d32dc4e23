#!/usr/bin/env python3
"""Cost of the weak-view teacher -> profiles/weak_teacher.txt.  MEASUREMENT ONLY.

    python profiles/tools/weak_teacher_cost.py head [--repo TREE] [--reps 40]
    python profiles/tools/weak_teacher_cost.py step [--repo TREE] [--weak] [--steps 40] [--warmup 10]
    python profiles/tools/weak_teacher_cost.py mix [--reps 40]

head  the fused head's launches on the head descriptors of the three SimT trainers (DeepLab-v2 B = 4 768 x 768 K = 3; DeepLabv3 B = 4
      512 x 1024 K = 15; DeepLab-VGG16 B = 8 512 x 512 K = 15: trunks of reduced depth -- the head's geometry does not depend on it), after
      one step on a synthetic batch, bf16: `loss` = simt_head_loss (key memset + pass 1 + reduction + finalize), `grad` = simt_head_grad
      (pass 2 + y-reduction), microseconds per call from device events over `--reps` calls.  In a tree that has them, also the _views
      symbols with a blocky item map.  --repo TREE imports another checkout (the parent commit's).  One JSON line per geometry.
step  DeepLab-v2 SimT B = 4 at 768 x 768, bf16, K = 3, on a resident synthetic batch: median milliseconds per step from device events, and the
      stem launch(es) alone.  --weak: teacher_view=True with a second resident batch as the weak view and a blocky item map (two one-set
      stem launches instead of one two-set launch).  One JSON line.
mix   simt_class_mix against simt_class_mix_items at B = 4, 768 x 768, 19 classes, blocky labels: microseconds per launch.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def _blocky_map(torch, B, H, W, dev):
    g = torch.Generator().manual_seed(3)
    sel = torch.randint(0, 2, (B, (H + 7) // 8, (W + 7) // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    own = torch.arange(B)[:, None, None]
    return torch.where(sel.bool(), (own + 1) % B, own).to(torch.uint8).to(dev)


def head(a):
    root = os.path.abspath(a.repo or ROOT)
    sys.path.insert(0, root)
    import torch

    from simt_amd import _lib as L
    from simt_amd import model_spec as ms
    from simt_amd import ops
    from simt_amd.step import Hyper, SimTTrainer
    from simt_amd.step_single import SimTSingleTrainer
    from simt_amd.tools.trainV2_simt import single_model_states
    dev = torch.device("cuda:0")
    cd = ms.load_class_dist("bapa")
    views = "simt_head_loss_views" in L.SIGNATURES

    def v2():
        lay, K = (1, 1, 1, 1), 3
        return SimTTrainer(ms.reference_init(ms.state_shapes(19, K, True, layers=lay), seed=1234),
                           ms.trained_like_init(ms.state_shapes(19, 0, False, layers=lay), seed=7), ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2),
                           Hyper(open_classes=K, lr=6e-4, lr_T=6e-3), cd, 4, 768, 768, device=dev, layers=lay), (4, 768, 768)

    def single(model, name, B, H, W):
        def make():
            K, lay = 15, (1, 1, 1)
            st, fst = single_model_states(name, 19, K, lay)
            arch = {"layers": lay} if model == "v3" else None
            return SimTSingleTrainer(model, st, fst, ms.ntm_init(19, K, 1), Hyper(open_classes=K, lr=6e-4, lr_T=6e-3), cd, B, H, W, device=dev,
                                     arch=arch), (B, H, W)
        return make
    for name, make in (("DeepLab-v2 B=4 768x768 K=3", v2), ("DeepLabv3 B=4 512x1024 K=15", single("v3", "DeepLabv3", 4, 512, 1024)),
                       ("DeepLab-VGG16 B=8 512x512 K=15", single("vgg", "DeepLabVGG", 8, 512, 512))):
        tr, (B, H, W) = make()
        img, lab = ms.synthetic_batch(B, H, W, cd, seed=1234, device=dev)
        tr.step(img, lab)
        torch.cuda.synchronize()
        st = ops.stream_ptr()
        hd = C.byref(tr.head_desc)
        res = {"mode": "head", "tree": os.path.relpath(root), "geometry": name, "h": tr.h, "w": tr.w, "reps": a.reps,
               "loss_us": _timed(torch, lambda: L.call("simt_head_loss", hd, st), a.reps),
               "grad_us": _timed(torch, lambda: L.call("simt_head_grad", hd, st), a.reps)}
        if views:
            m = _blocky_map(torch, B, H, W, dev)
            res["loss_null_views_us"] = _timed(torch, lambda: L.call("simt_head_loss_views", hd, None, st), a.reps)
            res["loss_map_us"] = _timed(torch, lambda: L.call("simt_head_loss_views", hd, m.data_ptr(), st), a.reps)
            res["grad_map_us"] = _timed(torch, lambda: L.call("simt_head_grad_views", hd, m.data_ptr(), st), a.reps)
            conf, lws = tr.head_desc.conf_out, tr.head_desc.label_ws          # pass 2 deciding the labels again: the form that reads fixp
            tr.head_desc.conf_out, tr.head_desc.label_ws = None, None
            res["grad_decide_us"] = _timed(torch, lambda: L.call("simt_head_grad", hd, st), a.reps)
            res["grad_decide_map_us"] = _timed(torch, lambda: L.call("simt_head_grad_views", hd, m.data_ptr(), st), a.reps)
            tr.head_desc.conf_out, tr.head_desc.label_ws = conf, lws
        print(json.dumps(res), flush=True)
        del tr
        torch.cuda.empty_cache()


def step(a):
    root = os.path.abspath(a.repo or ROOT)
    sys.path.insert(0, root)
    import torch

    from simt_amd import _lib as L
    from simt_amd import model_spec as ms
    from simt_amd.engine import reserve_streams
    from simt_amd.step import Hyper, SimTTrainer
    dev = torch.device("cuda:0")
    reserve_streams(dev)
    cd = ms.load_class_dist("bapa")
    B, H, W, K = 4, 768, 768, 3
    hp = Hyper(open_classes=K, lr=6e-4, lr_T=6e-3)
    kw = {"teacher_view": True} if a.weak else {}
    tr = SimTTrainer(ms.reference_init(ms.state_shapes(19, K, True), seed=1234), ms.reference_init(ms.state_shapes(19, 0, False), seed=1234),
                     ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), hp, cd, B, H, W, device=dev, **kw)
    img, lab = ms.synthetic_batch(B, H, W, cd, seed=1234, device=dev)
    skw = {}
    if a.weak:
        skw = {"teacher_image": ms.synthetic_batch(B, H, W, cd, seed=4321, device=dev)[0], "fix_item": _blocky_map(torch, B, H, W, dev)}
    for _ in range(a.warmup):
        tr.step(img, lab, **skw)
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(a.steps):
        tr.step(img, lab, **skw)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
    tr.losses()
    stems = [tr.plan.fwd_list.items[0]] + ([tr.fixed.fwd_list.items[0]] if a.weak else [])
    st = torch.cuda.current_stream(dev).cuda_stream

    def run_stems():
        for it in stems:
            rc = it.fn(*it.args, st)
            if rc != 0:
                L.check(rc)
    print(json.dumps({"mode": "step", "tree": os.path.relpath(root), "weak": bool(a.weak), "B": B, "size": [H, W], "steps": a.steps,
                      "median_ms": round(per[len(per) // 2], 3), "wall_ms_per_step": round(wall, 3), "stem_launches": len(stems),
                      "stem_us": _timed(torch, run_stems, 40)}), flush=True)


def mix(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    from simt_amd.data.pipeline import InputPrep
    dev = torch.device("cuda:0")
    B, H, W, Cn = 4, 768, 768, 19
    prep = InputPrep(B, (H, W), (W, H), dev, class_mix=(Cn, 1.0))
    g = torch.Generator().manual_seed(1)
    lab = torch.randint(0, Cn, (B, H // 16, W // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).to(dev)
    x = torch.randn(B, 3, H, W, generator=g).to(dev)
    xo, lo, item = torch.empty_like(x), torch.empty_like(lab), torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    import numpy as np
    rng = np.random.default_rng(1)
    draws = (np.ones(B, bool), rng.permuted(np.tile(np.arange(Cn, dtype=np.uint8), (B, 1)), axis=1))
    st = torch.cuda.current_stream(dev).cuda_stream
    res = {"mode": "mix", "B": B, "size": [H, W], "reps": a.reps}
    for _ in range(2):      # both orders
        res.setdefault("mix_us", []).append(_timed(torch, lambda: prep.class_mix_batch(x, lab, draws, xo, lo, st), a.reps))
        res.setdefault("mix_items_us", []).append(_timed(torch, lambda: prep.class_mix_batch(x, lab, draws, xo, lo, st, item_out=item), a.reps))
    res["note"] = "each figure: simt_label_presence + the mix launch, as class_mix_batch issues them"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["head", "step", "mix"])
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--weak", action="store_true")
    p.add_argument("--repo", default=None, help="tree to import simt_amd from (default: the one this file is in)")
    a = p.parse_args()
    {"head": head, "step": step, "mix": mix}[a.mode](a)
