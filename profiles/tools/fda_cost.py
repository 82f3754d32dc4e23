#!/usr/bin/env python3
"""Cost of --fda (simt_fda_transfer) -> profiles/fda.txt.  MEASUREMENT ONLY.

    python profiles/tools/fda_cost.py kernel [--rounds 3] [--reps 40]
    python profiles/tools/fda_cost.py step --model v2|vgg [--fda BETA] [--steps 30] [--warmup 6] [--repo TREE]

kernel  At B = 4, 768 x 768 and B = 8, 512 x 512, per beta, in ONE run: the four launches of simt_fda_transfer (one call) beside a
        device-to-device copy of the image batch, the byte floor at that copy's rate -- 4 x 12 bytes per pixel: xs read twice, xt once, x_out
        written once -- and the eager torch.fft.fft2 / ifft2 composition that yields the same batch (with its largest difference from the
        launch; reported as not available where this torch build's FFT does not run on the device).  Device events over `--reps`
        back-to-back calls after a warm-up, `--rounds` rounds in alternating order; microseconds per call.
step    The warm-up trainer at those sizes (DeepLab-v2 B = 4 768 x 768, VGG16 B = 8 512 x 512), bf16, constructor init, online_labels = 0 and
        online_source on resident synthetic batches; with --fda the source batch goes through FdaTransfer in front of every step, as the
        tool's loop does it.  `--steps` steps after `--warmup`, wall-clock milliseconds per step around a device synchronise, one JSON line.
        --repo TREE imports another checkout (the parent commit's, which has no such module: --fda is refused with it).  One process per
        run; the driver rotates the order of parent / flag off / flag on from round to round.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = [(4, 768, 768, ("0.01", "0.08")),       # 0.09 at 768 is b = 69: above SIMT_FDA_MAX_BAND, refused; 0.08 (b = 61) stands in
         (8, 512, 512, ("0.01", "0.09"))]


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


def torch_fda(torch, xs, xt, mean, b):
    """The published composition, eager: fft2 of both batches, the centre square of the shifted amplitude swapped, ifft2."""
    m = torch.tensor(mean, device=xs.device, dtype=xs.dtype).view(1, 3, 1, 1)
    fs, ft = torch.fft.fft2(xs + m), torch.fft.fft2(xt + m)
    amp, pha = torch.fft.fftshift(fs.abs(), dim=(-2, -1)), fs.angle()
    amp_t = torch.fft.fftshift(ft.abs(), dim=(-2, -1))
    h, w = xs.shape[-2:]
    ch, cw = h // 2, w // 2
    amp[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = amp_t[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    return torch.fft.ifft2(torch.polar(torch.fft.ifftshift(amp, dim=(-2, -1)), pha)).real - m


def kernel(a):
    sys.path.insert(0, ROOT)
    import torch

    from simt_amd import model_spec as ms
    from simt_amd.data.fda import FdaTransfer, parse
    from simt_amd.data.pipeline import IMG_MEAN
    dev = torch.device("cuda:0")
    cd = ms.load_class_dist("bapa")
    print(f"{a.reps} calls per timing, {a.rounds} rounds in alternating order; us per call")
    for B, h, w, betas in CASES:
        xt = ms.synthetic_batch(B, h, w, cd, seed=1, device=dev)[0].contiguous()
        xs = ms.synthetic_batch(B, h, w, cd, seed=2, device=dev)[0].contiguous()
        spare = torch.empty_like(xs)
        px = B * 3 * h * w
        try:
            parse("0.09", (w, h))
        except ValueError as e:
            print(f"\nB = {B}, {w} x {h}: {e}")
        for beta in betas:
            f = FdaTransfer(B, h, w, beta, dev)
            fns = [("device-to-device copy of the image batch", lambda: spare.copy_(xt)), ("simt_fda_transfer (four launches)", lambda: f(xs, xt))]
            try:
                ref = torch_fda(torch, xs, xt, IMG_MEAN, f.b)
                torch.cuda.synchronize()
                diff = float((ref - f(xs, xt)).abs().max())
                fns.append(("eager torch.fft composition", lambda: torch_fda(torch, xs, xt, IMG_MEAN, f.b)))
                note = f"largest difference between the two: {diff:.2e} grey levels"
            except RuntimeError as e:
                note = f"torch.fft does not run on this device build: {str(e).splitlines()[0]}"
            res = {n: [] for n, _f in fns}
            for r in range(a.rounds):
                for n, fn in (fns if r % 2 == 0 else fns[::-1]):
                    res[n].append(_timed(torch, fn, a.reps))
            print(f"\nB = {B}, {w} x {h}, beta = {beta}: b = {f.b}, {(f.b + 8) // 8} pass(es) of 8 frequencies, workspace {f.work.numel() / 1e6:.1f} MB; {note}")
            for n, _f in fns:
                print(f"{n:>44}  " + " ".join(f"{v:8.1f}" for v in res[n]) + f"  mean {sum(res[n]) / len(res[n]):8.1f}")
            copy = sum(res[fns[0][0]]) / a.rounds
            rate = 2 * px * 4 / copy                        # bytes per microsecond, read + write
            mine = sum(res[fns[1][0]]) / a.rounds
            print(f"copy rate {rate / 1e6:.2f} TB/s (read + write); byte floor 4 x 12 bytes per pixel = {16 * px / 1e6:.1f} MB = {16 * px / rate:.1f} us; "
                  f"simt_fda_transfer takes {mine / (16 * px / rate):.2f} x the floor")
            del f


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
    img, _lab = ms.synthetic_batch(B, H, W, cd, seed=1, device=dev)
    sx, sl = ms.synthetic_batch(B, H, W, cd, seed=2, device=dev)
    fda = None
    if a.fda is not None:
        from simt_amd.data.fda import FdaTransfer
        fda = FdaTransfer(B, H, W, a.fda, dev)

    def one():
        tr.step(img, source_image=sx if fda is None else fda(sx, img), source_label=sl)
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = tr.losses()
    print(json.dumps({"model": a.model, "tree": "parent" if a.repo else "this", "fda": a.fda, "b": None if fda is None else fda.b, "steps": a.steps,
                      "ms_per_step": round(dt * 1e3 / a.steps, 3), "images_per_s": round(B * a.steps / dt, 2), "source_seg2": l.get("source_seg2")}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=3)
    k.add_argument("--reps", type=int, default=40)
    s = sub.add_parser("step")
    s.add_argument("--model", choices=["v2", "vgg"], required=True)
    s.add_argument("--fda", type=str, default=None)
    s.add_argument("--steps", type=int, default=30)
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--repo", type=str, default=None)
    a = p.parse_args()
    (kernel if a.mode == "kernel" else step)(a)


if __name__ == "__main__":
    main()
