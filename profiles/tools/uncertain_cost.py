#!/usr/bin/env python3
"""Cost of --uncertainty-rectify (simt_head_loss_uncertain / simt_head_grad_uncertain) -> profiles/uncertainty.txt.  MEASUREMENT ONLY.

    python profiles/tools/uncertain_cost.py resources
    python profiles/tools/uncertain_cost.py launch [--rounds 3] [--reps 40]
    python profiles/tools/uncertain_cost.py dump --out FILE [--lib LIBSIMT_HIP_SO]
    python profiles/tools/uncertain_cost.py compare A B
    python profiles/tools/uncertain_cost.py step --mode warmup|source [--uncertainty LAMBDA_KL] [--steps 30] [--warmup 6] [--repo TREE]

resources  entropy_cost.py's table (no GPU): VGPRs, SGPRs, scratch bytes and waves per SIMD of every head_pass kernel of the shipped library; the
           uncertainty flavours carry five trailing flags (false, false, true, false, true).
launch     The uncertainty loss and gradient launches beside simt_head_loss_weighted / simt_head_grad_weighted AND the entropy pair on the same
           inputs (weights 0.7, no map), B = 4, 768 x 768, two heads, at Q = C = 19 (the QM = 24 builds) and at Q = C = 27 (QM = 40).  Device events
           over `--reps` back-to-back calls after a warm-up, `--rounds` rounds in alternating order; microseconds per call.
dump / compare   entropy_cost.py's: every word the EXISTING head entry points write, from the library at --lib (a library from before the feature
           exports no uncertainty entry points: they are not bound).
step       The DeepLab-v2 warm-up trainer, B = 4, 768 x 768, bf16, constructor init, on resident synthetic batches.  --mode warmup: labels given,
           no teacher (the plain warm-up step);  --mode source: online_labels = 0, online_labels_weighted = "batch", online_source, online_mix =
           0.5 (entropy_cost.py's step).  --uncertainty LAMBDA_KL adds the keyword.  Wall-clock milliseconds per step around a device synchronise,
           one JSON line.  --repo TREE imports another checkout (the parent commit's, which has no such keyword).  One process per run; the driver
           rotates parent / flag off / flag on from round to round.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import entropy_cost as ec          # noqa: E402

NEW = ("simt_head_loss_uncertain", "simt_head_grad_uncertain")
LAUNCH_CASES = [("B = 4, 768 x 768, two heads, Q = C = 19 (QM = 24)", (4, 97, 97, 768, 768, 19, 19)),
                ("B = 4, 768 x 768, two heads, Q = C = 27 (QM = 40)", (4, 97, 97, 768, 768, 27, 27))]


def launch(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    from simt_amd import ops
    dev = torch.device("cuda:0")
    print(f"{a.reps} calls per timing, {a.rounds} rounds in alternating order; us per call; weights 0.7 for every item, no map; lambda_kl 1; "
          "lambda_ent 0.005, eta 2")
    for name, geo in LAUNCH_CASES:
        B = geo[0]
        k = ec._desc(torch, L, ops, dev, geo, False, False)
        k["w"].fill_(0.7)
        st, hd, wp = ops.stream_ptr(), C.byref(k["hd"]), k["w"].data_ptr()
        unc, ent = C.byref(L.HeadUncertainty(1.0)), C.byref(L.HeadEntropy(0.005, 2.0))
        fns = [("simt_head_loss_weighted", lambda: L.call("simt_head_loss_weighted", hd, wp, None, st)),
               ("simt_head_loss_entropy", lambda: L.call("simt_head_loss_entropy", hd, wp, B, None, ent, st)),
               ("simt_head_loss_uncertain", lambda: L.call("simt_head_loss_uncertain", hd, wp, B, None, unc, st)),
               ("simt_head_grad_weighted", lambda: L.call("simt_head_grad_weighted", hd, wp, None, st)),
               ("simt_head_grad_entropy", lambda: L.call("simt_head_grad_entropy", hd, wp, B, None, ent, st)),
               ("simt_head_grad_uncertain", lambda: L.call("simt_head_grad_uncertain", hd, wp, B, None, unc, st))]
        res = {n: [] for n, _f in fns}
        for r in range(a.rounds):
            for n, fn in (fns if r % 2 == 0 else fns[::-1]):
                res[n].append(ec._timed(torch, fn, a.reps))
        mean = {n: sum(v) / len(v) for n, v in res.items()}
        print(f"\n{name} (low-res {geo[1]} x {geo[2]})")
        for n, _f in fns:
            print(f"{n:>26}  " + " ".join(f"{v:8.1f}" for v in res[n]) + f"  mean {mean[n]:8.1f}  min {min(res[n]):8.1f}")
        both = lambda s: mean[f"simt_head_loss_{s}"] + mean[f"simt_head_grad_{s}"]          # noqa: E731
        for s in ("uncertain", "entropy"):
            print(f"{s} / weighted: loss {mean[f'simt_head_loss_{s}'] / mean['simt_head_loss_weighted']:.3f}, "
                  f"grad {mean[f'simt_head_grad_{s}'] / mean['simt_head_grad_weighted']:.3f}, both {both(s) / both('weighted'):.3f}")
        del k


def dump(a):
    if a.lib:
        sys.path.insert(0, ROOT)
        from simt_amd import _lib as L
        for name in NEW:
            L.SIGNATURES.pop(name, None)
    ec.dump(a)


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
    kw = {}
    if a.mode == "source":
        kw = {"online_labels": 0.0, "online_labels_weighted": "batch", "online_source": True, "online_mix": 0.5, "online_mix_seed": 1234}
    if a.uncertainty is not None:
        kw["uncertainty_rectify"] = a.uncertainty
    B, H, W = 4, 768, 768
    tr = WarmupTrainer(ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), Hyper(num_classes=19, open_classes=0, lr=2.5e-4), B, H, W,
                       device=dev, **kw)
    img, lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    sx, sl = ms.synthetic_batch(B, H, W, cd, seed=2, device=dev)
    one = (lambda: tr.step(img, source_image=sx, source_label=sl)) if a.mode == "source" else (lambda: tr.step(img, lab))
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    print(json.dumps({"mode": a.mode, "tree": "parent" if a.repo else "this", "uncertainty": a.uncertainty, "steps": a.steps,
                      "ms_per_step": round(dt * 1e3 / a.steps, 3), "images_per_s": round(B * a.steps / dt, 2),
                      "uncertainty2": l.get("uncertainty2"), "rectify2": l.get("rectify2")}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)
    sub.add_parser("resources")
    k = sub.add_parser("launch")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    d = sub.add_parser("dump")
    d.add_argument("--out", required=True)
    d.add_argument("--lib", default=None)
    c = sub.add_parser("compare")
    c.add_argument("A")
    c.add_argument("B")
    s = sub.add_parser("step")
    s.add_argument("--mode", choices=["warmup", "source"], required=True)
    s.add_argument("--uncertainty", type=float, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    {"resources": ec.resources, "launch": launch, "dump": dump, "compare": ec.compare, "step": step}[a.cmd](a)


if __name__ == "__main__":
    main()
