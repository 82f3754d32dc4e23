"""proto_contrast_cost.py [launch] [step [--root DIR]]: what --proto-contrast costs (results in profiles/proto_contrast.txt).

launch: the kernels' registers / LDS / scratch (code-object metadata), then simt_cell_labels / simt_proto_contrast_prep / simt_proto_contrast /
  simt_proto_contrast_finalize on synthetic inputs at the production geometry -- B = 4 768 x 768 DeepLab-v2 (M = 37 636, D = 2048, C = 19) in bf16 --
  beside simt_proto_rectify and simt_feat_dist on the same features and a device copy of the same run (its rate prices the byte floor: fs read
  twice and the seed written once), three alternating rounds of 40 launches each.
step: the warm-up step of the reduced DeepLab-v2 with online_labels = 0 and proto_denoise, keyword off / keyword on, three alternating rounds.
  --root DIR imports the package of another checkout (the parent commit's, built there): it has no keyword, so only `off` runs -- the parent's
  column, to be run in the same session between the rounds of this one."""
import ctypes as C
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from simt_amd import _lib as L      # noqa: E402
from simt_amd import ops, proto      # noqa: E402

B, HW, h, D, Cn = 4, 768, 97, 2048, 19
M = B * h * h


def timed(fn, n=40):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us


def launch():
    sys.path.insert(0, HERE)
    from kres import kernel_resources      # noqa: E402  (profiles/tools)
    from simt_amd import proto_contrast as PC
    for name, r in kernel_resources(L.LIB_PATH).items():
        if "proto_contrast" in name or "cell_labels" in name:
            print(f"  {name[:90]:90s} vgpr {r['vgpr']:3d} agpr {r['agpr']:2d} sgpr {r['sgpr']:3d} lds {r['lds']:5d} scratch {r['scratch']}")
    dev, st, bf = torch.device("cuda:0"), ops.stream_ptr(), torch.bfloat16
    lib = L.load()
    g = torch.Generator(device="cpu").manual_seed(M)
    eta = torch.randn(Cn, D, generator=g).abs()
    truth = torch.randint(0, Cn, (M,), generator=g)
    F = (eta[truth] + 0.5 * torch.randn(M, D, generator=g)).clamp_(min=0).to(dev, bf)
    Fi = (F.float() + 0.3).to(bf)
    eta_d, n = eta.to(dev), torch.ones(Cn, device=dev, dtype=torch.int32)
    # labels: blocks of 8 x 8 pixels of the cell's class, a tenth of the cells 255
    cells = truth.view(B, h, h).clone()
    cells[torch.rand(B, h, h, generator=g) < 0.1] = 255
    label = torch.nn.functional.interpolate(cells[:, None].float(), size=(HW, HW), mode="nearest")[:, 0].long().to(dev).contiguous()
    lab, lab_part = torch.zeros(M, device=dev, dtype=torch.uint8), torch.zeros(lib.simt_cell_labels_parts(B, h, h), device=dev, dtype=torch.int32)
    phat, hdr = torch.zeros(lib.simt_proto_contrast_phat_floats(Cn, D), device=dev), torch.zeros(4, device=dev, dtype=torch.int32)
    seed, dd = torch.zeros(M, D, device=dev, dtype=bf), torch.zeros(M, device=dev)
    part, out = torch.zeros(lib.simt_proto_contrast_parts(M), device=dev), torch.zeros(3, device=dev)
    cl = PC.fill_cell_labels(label, lab, lab_part, n, B, HW, HW, h, h, Cn, 0.75)
    pc = PC.fill_contrast(F, lab, eta_d, n, phat, hdr, seed, dd, part, out, M, D, Cn, bf, 0.1, 0.1, 1.0)
    # the neighbours on the same features: 7.26's rectify and 7.22's distance (every cell kept)
    ldp = 32
    P = torch.cat([torch.softmax(torch.randn(M, Cn, generator=g) * 2, 1), torch.zeros(M, ldp - Cn)], 1).contiguous().to(dev)
    rmap, rlab = torch.zeros(M, ldp, device=dev), torch.zeros(M, device=dev, dtype=torch.uint8)
    ch = torch.zeros(lib.simt_proto_parts(M), device=dev, dtype=torch.int32)
    r = proto.fill_rectify(F, D, D, P, rmap, ldp, eta_d, n, rlab, ch, M, Cn, bf, 0, 1.0, 0.5)
    mask, kept = torch.ones(M, device=dev, dtype=torch.uint8), torch.tensor([M], device=dev, dtype=torch.int32)
    fseed, fd_d, fd_part, fd_out = torch.zeros(M, D, device=dev, dtype=bf), torch.zeros(M, device=dev), torch.zeros(lib.simt_feat_dist_parts(M), device=dev), torch.zeros(3, device=dev)
    f = L.FeatDistDesc()
    f.fs, f.fi, f.mask, f.kept_part = F.data_ptr(), Fi.data_ptr(), mask.data_ptr(), kept.data_ptr()
    f.seed, f.d, f.part, f.out = fseed.data_ptr(), fd_d.data_ptr(), fd_part.data_ptr(), fd_out.data_ptr()
    f.lam, f.M, f.C, f.ld, f.dtype, f.n_kept_part, f.lam_g = 0.005, M, D, D, ops.dt_code(bf), 1, 0.005
    src, dst = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    fbytes = M * D * 2
    for rnd in range(3):
        t = {name: timed(lambda name=name, d=d: L.call(name, C.byref(d), st)) for name, d in
             (("simt_cell_labels", cl), ("simt_proto_contrast_prep", pc), ("simt_proto_contrast", pc), ("simt_proto_contrast_finalize", pc),
              ("simt_proto_rectify", r), ("simt_feat_dist", f))}
        t_c = timed(lambda: dst.copy_(src))
        rate = 2 * src.numel() * 4 / t_c          # bytes per us moved by the copy (read + write)
        four = sum(v for k, v in t.items() if "contrast" in k or "cell" in k)
        print(f"  round {rnd}: cell_labels {t['simt_cell_labels']:6.1f} us  prep {t['simt_proto_contrast_prep']:6.1f}  contrast {t['simt_proto_contrast']:7.1f}  "
              f"finalize {t['simt_proto_contrast_finalize']:5.1f}  sum {four:7.1f}   |  proto_rectify {t['simt_proto_rectify']:7.1f}  feat_dist {t['simt_feat_dist']:6.1f}   |  "
              f"copy {rate / 1e6:.2f} TB/s, byte floor {3 * fbytes / rate:6.1f} us (fs {fbytes / 1e6:.0f} MB x 2 + seed x 1)")
    torch.cuda.synchronize()
    print(f"  valid cells {int(hdr[2])} of {M}, seen {int(hdr[3])}, loss {float(out[1]):.4f}")


def step():
    import test_gpu_online_labels as O
    dev = torch.device("cuda:0")
    data = O._views(dev, 12)
    base = dict(online_labels=0.0, proto_denoise=1.0)
    trainers = {"off": O._trainer("v2", dev, **base)}
    if "--root" not in sys.argv:
        trainers["on"] = O._trainer("v2", dev, proto_contrast=0.1, **base)
    for rnd in range(3):
        for name, tr in trainers.items():
            for mb in data[:2]:
                tr.step(mb[0][0], None, it=1, teacher_image=mb[0][1])      # (a fixed iteration: the test settings' schedule ends at 20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for mb in data[2:]:
                tr.step(mb[0][0], None, it=1, teacher_image=mb[0][1])      # (a fixed iteration: the test settings' schedule ends at 20)
            torch.cuda.synchronize()
            print(f"  reduced v2 2x65x129 round {rnd} keyword {name:3s} ({'the --root checkout' if '--root' in sys.argv else 'this checkout'}):{(time.perf_counter() - t0) / 10 * 1e3:.3f} ms / step")


if __name__ == "__main__":
    what = [a for a in sys.argv[1:] if a in ("launch", "step")] or ["launch", "step"]
    for w in what:
        print(w + ":")
        {"launch": launch, "step": step}[w]()
