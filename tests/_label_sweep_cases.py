"""The cases of tests/test_gpu_label_sweep.py: every entry point of csrc/label_sweep.hip on seeded inputs, through the C ABI alone, so that the
same code runs against any build of the library (SIMT_LIB_PATH).

    SIMT_LIB_PATH=<library of the parent commit> python tests/_label_sweep_cases.py --parent <commit hash> --hipcc "$(hipcc --version)" [--out FILE]

writes tests/golden/g17_label_sweep.npz (or FILE): every output array of every case (identical arrays stored once), the SHA-256 of every generated
input, the commit whose library made the recording and the compiler's version string.  For the cases marked `digest` the maps are stored
as the SHA-256 of their bytes; counts, histograms and thresholds are stored whole.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_label_sweep.npz")

# (family, B, h, w, H, W, C, ld): GEOMETRIES and THRESHOLDS of tests/test_gpu_online_labels.py (family 0: one resample, 1: two resamples)
GEOMETRIES = [(0, 2, 9, 17, 65, 129, 19, 24), (0, 3, 9, 9, 64, 64, 19, 24), (0, 1, 5, 5, 33, 33, 3, 8), (0, 1, 1, 1, 7, 5, 19, 24),
              (1, 2, 9, 17, 65, 129, 19, 24), (1, 2, 8, 16, 64, 128, 19, 24), (1, 2, 9, 17, 65, 129, 19, 19), (1, 2, 8, 16, 64, 128, 19, 19)]
THRESHOLDS = [-1.0, 0.5, 0.968, 1.0, float("nan")]
# name -> (geometry, digest)
CASES = {"fam{}-{}x{}x{}to{}x{}-C{}-ld{}".format(*g): (g, False) for g in GEOMETRIES}
CASES.update({"tail-fam0": ((0, 1, 2, 2, 1, 3, 19, 24), False),          # P = 3: the byte-store tail of the uint8 store
              "tail-fam1": ((1, 1, 2, 2, 1, 3, 19, 24), False),
              # P = 525 825 > 1024 * 512 = 512 * 1024: the grid-stride loop takes a second trip in both launch shapes; W % 4 == 1
              "second-trip-fam0": ((0, 1, 9, 17, 513, 1025, 19, 24), True),
              "second-trip-fam1": ((1, 1, 9, 17, 513, 1025, 19, 24), True)})
TERMS = (1, 3, 8)             # terms of a test-time-augmentation launch; the odd ones belong to the mirrored frame
GARBAGE = 0x5EADBEEF5EADBEEF


def _map(rs, B, h, w, Cn, ld, prob):
    """[B][h][w][ld] float32: randn * 3 (prob: its softmax); in item 0 two low-res rows whose two largest channels are exactly equal, one
    low-res pixel of NaNs; pad columns C..ld-1 = 1e30 (must be ignored)."""
    x = (rs.standard_normal((B, h, w, Cn)) * 3).astype(np.float32)
    if h > 2:
        x[0, :2, :, 1] = x[0, :2].max(-1) + 1.0
        x[0, :2, :, min(4, Cn - 1)] = x[0, :2, :, 1]
    if prob:
        e = np.exp(x.astype(np.float64) - x.max(-1, keepdims=True))
        x = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    if h > 2:
        x[-1, h - 1, w // 2, :] = np.nan
    full = np.full((B, h, w, ld), 1e30, np.float32)
    full[..., :Cn] = x
    return full


def inputs(name):
    """-> {"logit<i>" / "prob<i>": (array, h, w)} for the 8 terms i (sizes in turn: the geometry's, ~5/4 and ~3/2 of it), and "thr"."""
    (fam, B, h, w, H, W, Cn, ld), _digest = CASES[name]
    sizes = [(h, w), (h + h // 4 + 1, w + w // 4 + 1), (h + h // 2 + 1, w + w // 2 + 1)]
    out = {}
    for i in range(max(TERMS)):
        hh, ww = sizes[i % 3]
        seed = 1000 * sorted(CASES).index(name) + i
        out[f"logit{i}"] = (_map(np.random.RandomState(seed), B, hh, ww, Cn, ld, False), hh, ww)
        if fam == 0:
            out[f"prob{i}"] = (_map(np.random.RandomState(seed), B, hh, ww, Cn, ld, True), hh, ww)
    thr = np.linspace(0.3, 0.95, Cn).astype(np.float32)
    thr[0], thr[-1] = 0.0, np.nan
    out["thr"] = (thr, 0, 0)
    return out


def input_digests(name):
    return {k: hashlib.sha256(v[0].tobytes()).hexdigest() for k, v in inputs(name).items()}


def run(name, dev):
    """Every entry point that accepts the case's family -> {key: numpy array}."""
    import torch

    from simt_amd import _lib as L
    from simt_amd import ops
    (fam, B, h, w, H, W, Cn, ld), _digest = CASES[name]
    BINS = L.CONF_BINS
    host = inputs(name)
    thr = host.pop("thr")[0]
    gpu = {k: (torch.from_numpy(a).to(dev), hh, ww) for k, (a, hh, ww) in host.items()}
    assert all(t.data_ptr() % 16 == 0 for t, _h, _w in gpu.values())
    st = ops.stream_ptr()
    res = {}

    def new(kind):
        if kind == "u8":
            return torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
        if kind == "i32":
            return torch.full((B, H, W), -7, dtype=torch.int32, device=dev)
        if kind == "i64":
            return torch.full((B, H, W), GARBAGE, dtype=torch.int64, device=dev)
        return torch.zeros({"counts": (Cn + 1,), "hist": (Cn, BINS)}[kind], dtype=torch.int64, device=dev)

    def keep(key, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            res[f"{key}/{k}"] = t.cpu().numpy()

    def term(kind, i, two):
        t, hh, ww = gpu[f"{kind}{i}"]
        return (t, hh, ww, ld, 4 * hh if two else 0, 4 * ww if two else 0, i % 2 == 1)

    la, ha, wa = gpu["logit0"]
    lb, hb, wb = gpu["logit1"]
    combos = [("hist+out", True, True), ("hist", True, False), ("out", False, True)]
    if fam == 0:
        pa = gpu["prob0"][0]
        for tag, b in (("1scale", (None, 0, 0, 0)), ("2scales", (ops._p(lb), hb, wb, ld))):
            pred, out, cnt = new("i32"), new("u8"), new("counts")
            L.call("simt_upsample_sum_argmax", ops._p(la), ha, wa, ld, *b, B, H, W, Cn, ops._p(pred), st)
            L.call("simt_pseudo_label_u8", ops._p(la), ha, wa, ld, *b, B, H, W, Cn, 0, 0.0, ops._p(out), ops._p(cnt), st)
            keep(f"upsample_sum_argmax/{tag}", pred=pred)
            keep(f"pseudo_label_u8/mode0-{tag}", out=out, counts=cnt)
        for t in THRESHOLDS:
            out, cnt = new("u8"), new("counts")
            L.call("simt_pseudo_label_u8", ops._p(pa), ha, wa, ld, None, 0, 0, 0, B, H, W, Cn, 1, t, ops._p(out), ops._p(cnt), st)
            keep(f"pseudo_label_u8/mode1-{t}", out=out, counts=cnt)
        for tag, with_hist, with_out in combos:
            out, cnt, hist = new("u8"), new("counts"), new("hist")
            L.call("simt_pseudo_conf_u8", ops._p(pa), ha, wa, ld, B, H, W, Cn, thr.ctypes.data if with_out else None,
                   ops._p(out) if with_out else None, ops._p(cnt) if with_out else None, ops._p(hist) if with_hist else None, st)
            keep(f"pseudo_conf_u8/{tag}", out=out, counts=cnt, hist=hist)
    else:
        hia, wia, hib, wib = 4 * ha, 4 * wa, 4 * hb, 4 * wb
        for tag, b in (("1scale", (None, 0, 0, 0, 0, 0)), ("2scales", (ops._p(lb), hb, wb, ld, hib, wib))):
            pred, out, cnt = new("i32"), new("u8"), new("counts")
            L.call("simt_upsample2_sum_argmax", ops._p(la), ha, wa, ld, hia, wia, *b, B, H, W, Cn, ops._p(pred), st)
            L.call("simt_pseudo_label2_u8", ops._p(la), ha, wa, ld, hia, wia, *b, B, H, W, Cn, 0, 0.0, ops._p(out), ops._p(cnt), st)
            keep(f"upsample2_sum_argmax/{tag}", pred=pred)
            keep(f"pseudo_label2_u8/mode0-{tag}", out=out, counts=cnt)
        for t in THRESHOLDS:
            out, cnt = new("u8"), new("counts")
            L.call("simt_pseudo_label2_u8", ops._p(la), ha, wa, ld, hia, wia, None, 0, 0, 0, 0, 0, B, H, W, Cn, 1, t, ops._p(out), ops._p(cnt), st)
            keep(f"pseudo_label2_u8/mode1-{t}", out=out, counts=cnt)
        for tag, with_hist, with_out in combos:
            out, cnt, hist = new("u8"), new("counts"), new("hist")
            L.call("simt_pseudo_conf2_u8", ops._p(la), ha, wa, ld, hia, wia, B, H, W, Cn, thr.ctypes.data if with_out else None,
                   ops._p(out) if with_out else None, ops._p(cnt) if with_out else None, ops._p(hist) if with_hist else None, st)
            keep(f"pseudo_conf2_u8/{tag}", out=out, counts=cnt, hist=hist)

    # online labels: the teacher's map is probabilities (family 0) or logits (family 1, virtual map of the label's size)
    fix = gpu["prob0" if fam == 0 else "logit0"][0]
    for t in THRESHOLDS:
        lab, cnt = new("i64"), new("counts")
        d = L.OnlineLabelDesc()
        d.fix, d.label, d.counts = fix.data_ptr(), lab.data_ptr(), cnt.data_ptr()
        d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family, d.threshold = B, ha, wa, ld, H, W, Cn, fam, t
        L.call("simt_online_label", C.byref(d), st)
        keep(f"online_label/{t}", label=lab, counts=cnt)
    lab, cnt, hist = new("i64"), new("counts"), new("hist")
    dthr = torch.from_numpy(thr).to(dev)
    t_out = torch.full((Cn,), -3.0, device=dev)
    d = L.OnlineLabelCbDesc()
    d.fix, d.label, d.counts, d.hist, d.thr = fix.data_ptr(), lab.data_ptr(), cnt.data_ptr(), hist.data_ptr(), dthr.data_ptr()
    d.B, d.h, d.w, d.ld, d.H, d.W, d.C, d.family = B, ha, wa, ld, H, W, Cn, fam
    L.call("simt_online_label_cb", C.byref(d), st)
    keep("online_label_cb", label=lab, counts=cnt, hist=hist)
    ct = L.ClassThresholdsDesc()
    ct.hist, ct.thr, ct.t_out = hist.data_ptr(), dthr.data_ptr(), t_out.data_ptr()
    ct.drop, ct.C, ct.cap, ct.omd = 0.2, Cn, 0.9, 0.5
    L.call("simt_class_thresholds", C.byref(ct), st)
    keep("class_thresholds", hist=hist, thr=dthr, t_out=t_out)

    # test-time augmentation: kind 0 of both families (pred, out, both), kinds 1-3 of the one-resample family
    for n in TERMS:
        two = fam == 1
        maps = [term("logit", i, two) for i in range(n)]
        for tag, with_pred, with_out in (("pred", True, False), ("out", False, True), ("pred+out", True, True)):
            pred, out, cnt = new("i32"), new("u8"), new("counts")
            ops.tta_label(maps, B=B, H=H, W=W, Cn=Cn, mode=0, pred=pred if with_pred else None, out=out if with_out else None,
                          counts=cnt if with_out else None)
            keep(f"tta_label/{n}terms-kind0-{tag}", pred=pred, out=out, counts=cnt)
        if two:
            continue
        maps = [term("prob", i, False) for i in range(n)]
        for tag, kw in (("kind1-strict", dict(threshold=0.5, out=True)), ("kind1-perclass", dict(thr=thr, out=True)), ("kind2", dict(hist=True)),
                        ("kind3-strict", dict(threshold=0.5, out=True, hist=True)), ("kind3-perclass", dict(thr=thr, out=True, hist=True))):
            out, cnt, hist = new("u8"), new("counts"), new("hist")
            ops.tta_label(maps, B=B, H=H, W=W, Cn=Cn, mode=1, threshold=kw.get("threshold", 0.0), thr=kw.get("thr"),
                          out=out if kw.get("out") else None, counts=cnt if kw.get("out") else None, hist=hist if kw.get("hist") else None)
            keep(f"tta_label/{n}terms-{tag}", out=out, counts=cnt, hist=hist)
    return res


def is_map(name, arr):
    (_f, B, _h, _w, H, W, _C, _ld), _d = CASES[name]
    return arr.shape == (B, H, W)


def stored(name, key, arr):
    """What the fixture holds for one output: the array, or (digest cases, maps only) the SHA-256 of its bytes."""
    if CASES[name][1] and is_map(name, arr):
        return np.array(hashlib.sha256(arr.tobytes()).hexdigest())
    return arr


def record(parent, hipcc, path):
    import torch
    dev = torch.device("cuda:0")
    index = {"parent_commit": parent, "hipcc_version": hipcc, "inputs": {}, "outputs": {}}
    blobs = {}
    for name in CASES:
        index["inputs"][name] = input_digests(name)
        for key, arr in run(name, dev).items():
            a = stored(name, key, arr)
            sha = hashlib.sha256(a.tobytes() + str((a.dtype, a.shape)).encode()).hexdigest()[:20]
            blobs["blob_" + sha] = a
            index["outputs"][f"{name}/{key}"] = sha
    np.savez_compressed(path, index=np.array(json.dumps(index)), **blobs)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(index['outputs'])} outputs in {len(blobs)} distinct arrays")


if __name__ == "__main__":
    import argparse
    sys.path.insert(0, ROOT)
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--hipcc", required=True)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    record(a.parent, a.hipcc.strip(), a.out)
