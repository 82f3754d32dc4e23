"""proto_cost.py [launch] [step]: what --proto-denoise costs (results in profiles/proto_denoise.txt).

launch: simt_proto_rectify / simt_proto_accumulate / simt_proto_update on synthetic inputs at the three production geometries -- B = 4
  768 x 768 DeepLab-v2 (M = 37 636, D = 2048), B = 8 512 x 512 DeepLab-VGG16 (D = 1024) and B = 4 512 x 1024 DeepLabv3 (D = 2048, logits) -- in
  bf16, three alternating rounds of 40 launches each, beside a device copy of the same run (its rate prices the byte floor: F read twice, P
  read and the map written once, the workspace written and read once) and the kernels' registers / LDS / scratch (code-object metadata).
step: the warm-up step of the reduced DeepLab-v2 with online_labels, keyword off / keyword on, three alternating rounds (the parent commit's
  library is a checkout of its own: run this file there for the third column)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from simt_amd import _lib as L      # noqa: E402
from simt_amd import ops, proto      # noqa: E402

GEOS = [("v2  B=4 768x768", 4 * 97 * 97, 2048, 19, 32, 0), ("vgg B=8 512x512", 8 * 65 * 65, 1024, 19, 32, 0), ("v3  B=4 512x1024", 4 * 33 * 65, 2048, 19, 32, 1)]


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
    from kres import kernel_resources      # noqa: E402  (profiles/tools)
    for name, r in kernel_resources(L.LIB_PATH).items():
        if "proto_" in name:
            print(f"  {name[:90]:90s} vgpr {r['vgpr']:3d} agpr {r['agpr']:2d} sgpr {r['sgpr']:3d} lds {r['lds']:5d} scratch {r['scratch']}")
    dev, st = torch.device("cuda:0"), ops.stream_ptr()
    lib = L.load()
    for tag, M, D, Cn, ldp, family in GEOS:
        g = torch.Generator(device="cpu").manual_seed(M)
        eta = torch.randn(Cn, D, generator=g)
        truth = torch.randint(0, Cn, (M,), generator=g)
        F = (eta[truth] + 0.5 * torch.randn(M, D, generator=g)).to(dev, torch.bfloat16)
        v = torch.randn(M, ldp, generator=g) * 2
        P = (v if family else torch.softmax(v[:, :Cn], 1).contiguous()).to(dev)
        if not family:
            P = torch.cat([P, torch.zeros(M, ldp - Cn, device=dev)], 1).contiguous()
        eta_d, n = eta.to(dev), torch.ones(Cn, device=dev, dtype=torch.int32)
        out, lab = torch.zeros(M, ldp, device=dev), torch.zeros(M, device=dev, dtype=torch.uint8)
        ch = torch.zeros(lib.simt_proto_parts(M), device=dev, dtype=torch.int32)
        words = lib.simt_proto_ws_floats(M, Cn, D)
        ws = torch.zeros(words, device=dev)
        r = proto.fill_rectify(F, D, D, P, out, ldp, eta_d, n, lab, ch, M, Cn, torch.bfloat16, family, 1.0, 0.5)
        a = proto.fill_accumulate(F, D, D, lab, ws, M, Cn, torch.bfloat16)
        u = proto.fill_update(ws, eta_d, n, M, D, Cn, 0.9999)
        src, dst = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
        fbytes, pbytes, wbytes = M * D * 2, M * ldp * 4, words * 4
        for rnd in range(3):
            t_r = timed(lambda: L.call("simt_proto_rectify", C.byref(r), st))
            t_a = timed(lambda: L.call("simt_proto_accumulate", C.byref(a), st))
            t_u = timed(lambda: L.call("simt_proto_update", C.byref(u), st))
            t_c = timed(lambda: dst.copy_(src))
            rate = 2 * src.numel() * 4 / t_c          # bytes per us moved by the copy (read + write)
            floor = (2 * fbytes + 2 * pbytes + 2 * wbytes) / rate
            print(f"  {tag} round {rnd}: rectify {t_r:7.1f} us  accumulate {t_a:7.1f}  update {t_u:6.1f}  sum {t_r + t_a + t_u:7.1f}   copy {rate / 1e6:.2f} TB/s, "
                  f"byte floor {floor:6.1f} us (F {fbytes / 1e6:.0f} MB x 2, maps {pbytes / 1e6:.1f} MB x 2, workspace {wbytes / 1e6:.1f} MB x 2)")


def step():
    import test_gpu_online_labels as O
    dev = torch.device("cuda:0")
    data = O._views(dev, 12)
    trainers = {"off": O._trainer("v2", dev, online_labels=0.3), "on": O._trainer("v2", dev, online_labels=0.3, proto_denoise=1.0)}
    for rnd in range(3):
        for name, tr in trainers.items():
            for mb in data[:2]:
                tr.step(mb[0][0], None, teacher_image=mb[0][1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for mb in data[2:]:
                tr.step(mb[0][0], None, teacher_image=mb[0][1])
            torch.cuda.synchronize()
            print(f"  reduced v2 2x65x129 round {rnd} keyword {name:3s}: {(time.perf_counter() - t0) / 10 * 1e3:.3f} ms / step")


if __name__ == "__main__":
    what = sys.argv[1:] or ["launch", "step"]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for w in what:
        print(w + ":")
        {"launch": launch, "step": step}[w]()
