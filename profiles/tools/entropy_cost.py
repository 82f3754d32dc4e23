#!/usr/bin/env python3
"""Cost of --entropy-min (simt_head_loss_entropy / simt_head_grad_entropy) -> profiles/entropy_min.txt.  MEASUREMENT ONLY.

    python profiles/tools/entropy_cost.py resources
    python profiles/tools/entropy_cost.py launch [--rounds 3] [--reps 40]
    python profiles/tools/entropy_cost.py dump --out FILE [--lib LIBSIMT_HIP_SO]
    python profiles/tools/entropy_cost.py compare A B
    python profiles/tools/entropy_cost.py step --model v2|vgg [--entropy LAMBDA] [--steps 30] [--warmup 6] [--repo TREE]

resources  No GPU: VGPRs, SGPRs, scratch bytes and waves per SIMD (512 VGPRs per lane and SIMD, blocks of 8) of every head_pass kernel of the
           shipped library, read from the code objects' notes; the entropy flavours (four trailing flags) stand beside their weighted neighbours.
launch     The entropy loss and gradient launches beside simt_head_loss_weighted / simt_head_grad_weighted on the same inputs (weights 0.7, no
           map) at B = 4 768 x 768 C = 19 two heads, B = 8 512 x 512 one head, B = 4 512 x 1024 one head half-pixel.  Device events over
           `--reps` back-to-back calls after a warm-up, `--rounds` rounds in alternating order; microseconds per call (a "loss" call is pass
           1 + reduce + finalize, a "grad" call pass 2 + y-reduction).
dump       Every word the EXISTING head entry points write (hout[:16], both gradients in fp32 and bf16, conf_out) at the geometries of the weighted
           head tests, plain / weighted with a map / weighted_n, from the library at --lib (default: the tree's) -> FILE.  One process per library.
compare    Two such files word for word.
step       The warm-up trainer (DeepLab-v2 B = 4 768 x 768, VGG16 B = 8 512 x 512), bf16, constructor init, online_labels = 0,
           online_labels_weighted = "batch", online_source, online_mix = 0.5 on resident synthetic batches; --entropy LAMBDA adds entropy_min.
           `--steps` steps after `--warmup`, wall-clock milliseconds per step around a device synchronise, one JSON line.  --repo TREE imports
           another checkout (the parent commit's, which has no such keyword: --entropy is refused with it).  One process per run; the driver
           rotates the order of parent / flag off / flag on from round to round.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LAUNCH_CASES = [("B = 4, 768 x 768, two heads", 4, 97, 97, 768, 768, False, False),
                ("B = 8, 512 x 512, one head", 8, 65, 65, 512, 512, True, False),
                ("B = 4, 512 x 1024, one head, half-pixel", 4, 64, 128, 512, 1024, True, True)]
# (B, h, w, H, W, Q, C) of tests/_weighted_ref.py's CASES, x (half, single) of tests/test_gpu_online_weighted.py's HEADS
DUMP_CASES = [((3, 9, 33, 65, 260, 19, 19), False, False), ((3, 9, 33, 65, 260, 19, 19), True, False), ((3, 9, 33, 65, 260, 19, 19), False, True),
              ((3, 9, 33, 65, 260, 19, 19), True, True), ((3, 65, 5, 516, 20, 22, 19), False, False)]


def resources(_a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import _codeobj
    from simt_amd import _lib
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(_codeobj.code_objects(_lib.LIB_PATH)):
            f = os.path.join(td, f"co{i}.o")
            open(f, "wb").write(co)
            notes = subprocess.check_output([os.path.join(_codeobj.LLVM, "llvm-readelf"), "--notes", f]).decode(errors="replace")
            if "head_pass" not in notes:
                continue
            for blk in notes.split("  - .agpr_count")[1:]:
                g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)          # noqa: E731
                name = subprocess.check_output(["c++filt", g("name")]).decode().strip()
                if "head_pass" in name:
                    v = int(g("vgpr_count"))
                    rows.append((name.replace("void ", "").replace("(HeadArgs)", ""), v, int(g("sgpr_count")), int(g("private_segment_fixed_size")),
                                 int(g("group_segment_fixed_size")), min(8, 512 // ((v + 7) // 8 * 8))))
    print(f"{'kernel':62s} {'VGPR':>5s} {'SGPR':>5s} {'scratch B':>9s} {'static LDS B':>12s} {'waves/SIMD by VGPRs':>20s}")
    for r in sorted(rows):
        print(f"{r[0]:62s} {r[1]:5d} {r[2]:5d} {r[3]:9d} {r[4]:12d} {r[5]:20d}")


def _desc(torch, L, ops, dev, geo, half, single, seed=0):
    """A mode-1 descriptor over random logits and labels (a band of 255s), every buffer kept alive in the returned dict."""
    B, h, w, H, W, Q, Cn = geo
    lib = L.load()
    g = torch.Generator().manual_seed(100 + seed + H)
    ldp, QP = ops.round_up(Q, 4) + 4, ops.round_up(Q, 8)
    ld_t = QP + 8

    def low():
        t = torch.zeros(B * h * w, ldp)
        t[:, :Q] = torch.randn(B * h * w, Q, generator=g) * 3
        return t.to(dev)
    k = dict(p1=None if single else low(), p2=low())
    lab = torch.randint(0, Cn, (B, (H + 7) // 8, (W + 7) // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()
    lab[B - 1, H // 2:H // 2 + 5] = 255
    k["lab"] = lab.to(dev)
    k["part"] = torch.zeros(lib.simt_head_nblk(B, H, W), lib.simt_head_part_floats(Q, Cn), device=dev)
    k["keys"] = torch.zeros(lib.simt_head_keys_count(), device=dev, dtype=torch.int64)
    k["hout"] = torch.zeros(lib.simt_head_hout_floats(Q, Cn), device=dev)
    k["g1"] = torch.zeros(2, B, H, w, QP, device=dev)
    k["dp"] = [torch.zeros(B * h * w, ldp, device=dev) for _ in range(2)]
    k["dt"] = [torch.zeros(B * h * w, ld_t, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    k["conf"] = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
    k["item"] = torch.randint(0, B, (B, (H + 12) // 13, (W + 6) // 7), generator=g).repeat_interleave(13, 1).repeat_interleave(7, 2)[:, :H, :W] \
        .to(torch.uint8).contiguous().to(dev)
    k["w"] = (torch.rand(2 * B, generator=g) * 0.9 + 0.1).to(dev)
    hd = L.HeadDesc()
    hd.pred1, hd.pred2, hd.label = (None if single else k["p1"].data_ptr()), k["p2"].data_ptr(), k["lab"].data_ptr()
    hd.part, hd.keys, hd.hout, hd.g1 = k["part"].data_ptr(), k["keys"].data_ptr(), k["hout"].data_ptr(), k["g1"].data_ptr()
    hd.dpred1_f32, hd.dpred2_f32 = (None if single else k["dp"][0].data_ptr()), k["dp"][1].data_ptr()
    hd.dpred1_t, hd.dpred2_t = (None if single else k["dt"][0].data_ptr()), k["dt"][1].data_ptr()
    hd.B, hd.h, hd.w, hd.H, hd.W, hd.C, hd.Q = B, h, w, H, W, Cn, Q
    hd.ldp, hd.ldf, hd.QP, hd.ld_f32, hd.ld_t, hd.grad_dtype = ldp, ldp, QP, ldp, ld_t, L.SIMT_BF16
    hd.th_high, hd.th_low, hd.lambda_seg, hd.lambda_place, hd.gscale = 2.0, -1.0, 0.1, 0.0, 1.0
    hd.mode, hd.single, hd.up_half_pixel, hd.fix_logits = 1, int(single), int(half), 0
    hd.conf_out = k["conf"].data_ptr()
    k["hd"] = hd
    return k


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


def launch(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    from simt_amd import ops
    dev = torch.device("cuda:0")
    print(f"{a.reps} calls per timing, {a.rounds} rounds in alternating order; us per call; weights 0.7 for every item, no map; lambda_ent 0.005, eta 2")
    for name, B, h, w, H, W, single, half in LAUNCH_CASES:
        k = _desc(torch, L, ops, dev, (B, h, w, H, W, 19, 19), half, single)
        k["w"].fill_(0.7)
        st, hd, wp = ops.stream_ptr(), C.byref(k["hd"]), k["w"].data_ptr()
        rec = C.byref(L.HeadEntropy(0.005, 2.0))
        fns = [("simt_head_loss_weighted", lambda: L.call("simt_head_loss_weighted", hd, wp, None, st)),
               ("simt_head_loss_entropy", lambda: L.call("simt_head_loss_entropy", hd, wp, B, None, rec, st)),
               ("simt_head_grad_weighted", lambda: L.call("simt_head_grad_weighted", hd, wp, None, st)),
               ("simt_head_grad_entropy", lambda: L.call("simt_head_grad_entropy", hd, wp, B, None, rec, st))]
        res = {n: [] for n, _f in fns}
        for r in range(a.rounds):
            for n, fn in (fns if r % 2 == 0 else fns[::-1]):
                res[n].append(_timed(torch, fn, a.reps))
        mean = {n: sum(v) / len(v) for n, v in res.items()}
        print(f"\n{name} (low-res {h} x {w}, C = Q = 19)")
        for n, _f in fns:
            print(f"{n:>26}  " + " ".join(f"{v:8.1f}" for v in res[n]) + f"  mean {mean[n]:8.1f}")
        print(f"entropy / weighted: loss {mean['simt_head_loss_entropy'] / mean['simt_head_loss_weighted']:.3f}, "
              f"grad {mean['simt_head_grad_entropy'] / mean['simt_head_grad_weighted']:.3f}, "
              f"both {(mean['simt_head_loss_entropy'] + mean['simt_head_grad_entropy']) / (mean['simt_head_loss_weighted'] + mean['simt_head_grad_weighted']):.3f}")
        del k


def dump(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import _lib as L
    if a.lib:          # (a library from before the feature exports no entropy entry points: they are not bound, nor called here)
        L.LIB_PATH = os.path.abspath(a.lib)
        for name in ("simt_head_loss_entropy", "simt_head_grad_entropy"):
            L.SIGNATURES.pop(name, None)
    from simt_amd import ops
    dev = torch.device("cuda:0")
    out = {}
    for ci, (geo, half, single) in enumerate(DUMP_CASES):
        B = geo[0]
        for form in ("plain", "weighted", "weighted_n"):
            k = _desc(torch, L, ops, dev, geo, half, single, seed=ci)
            st, hd = ops.stream_ptr(), C.byref(k["hd"])
            if form == "plain":
                L.call("simt_head_loss", hd, st)
                L.call("simt_head_grad", hd, st)
            elif form == "weighted":
                L.call("simt_head_loss_weighted", hd, k["w"].data_ptr(), k["item"].data_ptr(), st)
                L.call("simt_head_grad_weighted", hd, k["w"].data_ptr(), k["item"].data_ptr(), st)
            else:
                item = (k["item"] + B * (k["item"] % 2)).contiguous()          # half of the bytes name the entries behind the batch
                L.call("simt_head_loss_weighted_n", hd, k["w"].data_ptr(), 2 * B, item.data_ptr(), st)
                L.call("simt_head_grad_weighted_n", hd, k["w"].data_ptr(), 2 * B, item.data_ptr(), st)
            torch.cuda.synchronize()
            heads = [1] if single else [0, 1]
            out[f"{ci} {form}"] = [k["hout"][:16].cpu().view(torch.int32), k["conf"].cpu()] + [k["dp"][i].cpu().view(torch.int32) for i in heads] + \
                [k["dt"][i].cpu().view(torch.int16) for i in heads]
    torch.save(out, a.out)
    print(f"{a.out}: {len(out)} launch pairs, {sum(t.numel() for v in out.values() for t in v)} words, library {L.LIB_PATH}")


def compare(a):
    import torch
    x, y = torch.load(a.A), torch.load(a.B)
    assert set(x) == set(y)
    words = diff = 0
    for k in sorted(x):
        for s, t in zip(x[k], y[k]):
            words += s.numel()
            diff += int((s != t).sum())
    print(f"{len(x)} launch pairs, {words} words compared, {diff} differ")
    sys.exit(1 if diff else 0)


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
    kw = {"online_labels": 0.0, "online_labels_weighted": "batch", "online_source": True, "online_mix": 0.5, "online_mix_seed": 1234}
    if a.entropy is not None:
        kw["entropy_min"] = a.entropy
    hp = Hyper(num_classes=19, open_classes=0, lr=2.5e-4)
    if a.model == "v2":
        B, H, W = 4, 768, 768
        tr = WarmupTrainer(ms.reference_init(ms.state_shapes(19, 0, False), seed=1234), hp, B, H, W, device=dev, **kw)
    else:
        from simt_amd.step_single import WarmupSingleTrainer
        from simt_amd.tools.trainV2_simt import single_model_state
        B, H, W = 8, 512, 512
        tr = WarmupSingleTrainer("vgg", single_model_state("DeepLabVGG", 19), hp, B, H, W, device=dev, **kw)
    img, _lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    sx, sl = ms.synthetic_batch(B, H, W, cd, seed=2, device=dev)
    for _ in range(a.warmup):
        tr.step(img, source_image=sx, source_label=sl)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(img, source_image=sx, source_label=sl)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    print(json.dumps({"model": a.model, "tree": "parent" if a.repo else "this", "entropy": a.entropy, "steps": a.steps,
                      "ms_per_step": round(dt * 1e3 / a.steps, 3), "images_per_s": round(B * a.steps / dt, 2), "entropy2": l.get("entropy2")}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
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
    s.add_argument("--model", choices=["v2", "vgg"], required=True)
    s.add_argument("--entropy", type=float, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    {"resources": resources, "launch": launch, "dump": dump, "compare": compare, "step": step}[a.mode](a)


if __name__ == "__main__":
    main()
