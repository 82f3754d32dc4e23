#!/usr/bin/env python3
"""Pseudo-label export on MI355X: a source ("black-box") checkpoint -> the label PNGs, the `.lst` file `cityscapesPseudo` reads and the
`ClassDist_<name>.npy` prior `sig_NTM` multiplies into T -- everything the SimT stage (tools/trainV2_simt.py) takes as input.

The reference made its lists from its evaluation loop: the commented-out save lines of tools/evaluate_cityscapes.py:150-156
(evaluate_simt: main head at two input scales, upsampled to 1024 x 2048 with align_corners=True, summed, arg-maxed) and :214-219
(evaluate_warmup: one scale), and compute_ClassDistribution.py:66-92 for the prior.  `--threshold T` instead applies the SimT confidence
rule of trainV2_simt.py:353-359 (high threshold only): softmax at low resolution, upsampled, arg-max where max > T, 255 elsewhere.
`--class-balanced P` is the class-balanced rule of CBST / the label generator of BDL: the same confidence, but one threshold per class,
the confidence at the rank that keeps the share P of that class's own predictions (BDL: the median, P = 0.5), capped at
`--threshold-cap` (0.9); a pixel is kept iff conf >= thres[class].  It takes two passes over the list: statistics, then labels.

    python -m simt_amd.tools.make_pseudo_labels --restore-from src.pth --arch single --data-dir $CS --data-list train.txt \
        --out-name pseudo_mine --list-out pseudo_mine.lst [--threshold 0.8 | --class-balanced 0.5 [--threshold-cap 0.9]]
        [--thresholds-from pseudo_subset_thresholds.json] [--save-color --devkit-dir dataset/cityscapes_list] [--tta | --tta-flip]

`--tta` is test-time augmentation: every `--input-size` counts in every mode (the confidence modes otherwise use the first only), and
`--tta-flip` adds the horizontally mirrored frame of every scale.  One forward per term, then ONE simt_tta_label launch: the logits are
summed (plain arg-max) or the per-term softmax probabilities averaged (confidence rules); a mirrored term is read at mirrored column
indices of its low-res map.  Not built: the confidence rules of --arch v3 with --tta (the softmax of a model that upsamples inside).

--arch: multi (DeeplabMulti, the SimT DeepLab-v2), single (Res_Deeplab), v3 (DeepLabv3 at --v3-layers) or vgg (DeeplabVGG).  A v3 / vgg
checkpoint is read like the warm-up stage reads it (the module's own keys; a torchvision ImageNet file is mapped, but its classifier is
not, so it is refused); with --open-classes K it is the SimT model, DeepLabv3(C, K, openset=True) / DeeplabVGG(C + K).  The labels
always come from the first C channels.  DeepLabv3 upsamples inside the model (align_corners=False, to the input size): its confidence
rule takes the softmax of that input-size map before the align_corners=True resample to the label size.

Device: both eval-mode forwards (engine.TrunkPlan / engine_v3.V3Plan / engine_vgg.VggPlan, BN folded), the resizes
(data.pipeline.InputPrep, Pillow-exact) and one fused upsample + arg-max kernel (simt_pseudo_label_u8; simt_pseudo_label2_u8 for v3,
both resamples per label pixel) that writes the uint8 label map and the class counts; for the class-balanced rule
simt_pseudo_conf_u8 / simt_pseudo_conf2_u8, which also count the confidence per class into 256 bins.  Host: the thresholds from that
histogram (class_thresholds), PNG decoding on a bounded thread pool,
pinned copies of the label maps (guarded by events), PNG encoding on a writer pool, atomic file writes."""
import argparse
import json
import os
import os.path as osp
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.engine import TrunkPlan, multi_heads, single_head
from simt_amd.tools.evaluate_cityscapes import tta_hold_buffers, tta_low_res_maps, v3_low_res_forward, v3_low_res_logits

MAX_WORKERS = 16
ARCHS = ("multi", "single", "v3", "vgg")
MODES = ("argmax", "confidence", "class_balanced")
CONF_BINS = L.CONF_BINS                                # confidence bins per class (SIMT_CONF_BINS)
MAX_CB_CLASSES = 64                                    # the histogram kernel's LDS holds 64 x 256 counters
DEFAULT_SCALES = ((512, 1024), (640, 1280))          # (h, w): the crop sizes (1024, 512) and (1280, 640) of evaluate_simt :103-106


class PseudoLabeller:
    """Eval-mode plans of the model at each input scale + the fused label kernel.

    arch "multi": DeeplabMulti(C, K, K > 0), head x2, first C channels (evaluate_simt :128, :133).  arch "single": Res_Deeplab(C)
    (model/deeplab.py), head x.  arch "v3": DeepLabv3(C, K, openset=K > 0), the plans trimmed before the in-model upsample
    (simt_pseudo_label2_u8 applies it).  arch "vgg": DeeplabVGG(C + K), head x.  layers: the plans' trunk depth, as for Evaluator.
    mode "argmax": up(logits) summed over the scales, arg-max (one scale = evaluate_warmup).
    mode "confidence": first scale only, softmax -> up -> arg-max where max > threshold, else 255 (v3: the softmax of the input-size map).
    mode "class_balanced": the confidence of mode "confidence"; accumulate(*images) adds its per-class histogram to `conf_hist` (int64
    [C, 256], device), set_thresholds(thr) installs per-class thresholds, label(*images) then keeps arg-max where conf >= thr[arg-max].
    label(*images) -> uint8 [B, H, W] on the device; `counts` accumulates int64 [C+1] (classes, then the 255s).
    tta=True (test-time augmentation): every scale counts in every mode and, with flip=True, so does each scale's mirrored frame -- the
    terms of ops.tta_terms(scales, flip), one forward each and one simt_tta_label launch.  "argmax": the logits summed (Evaluator's labels
    for the same scales / flip).  "confidence" / "class_balanced": softmax per term at low resolution, the upsampled probabilities
    averaged, then the same rules.  arch "v3" has no such confidence rule (ValueError)."""

    def __init__(self, state, *, num_classes=19, open_classes=0, arch="multi", scales=DEFAULT_SCALES, label_hw=(1024, 2048),
                 mode="argmax", threshold=0.8, dtype=torch.float32, device="cuda:0", layers=None, batch=1, tta=False, flip=False):
        if arch not in ARCHS:
            raise ValueError(f"arch must be one of {ARCHS}, not {arch!r}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, not {mode!r}")
        if arch == "single" and open_classes:
            raise ValueError("the single-head model has no open-set classes")
        if not 0 < num_classes <= 255:
            raise ValueError("uint8 labels hold at most 255 classes (255 = ignore)")
        if mode == "class_balanced" and num_classes > MAX_CB_CLASSES:
            raise ValueError(f"class-balanced labels take at most {MAX_CB_CLASSES} classes")
        if flip and not tta:
            raise ValueError("flip=True belongs to tta=True")
        if tta and arch == "v3" and mode != "argmax":
            raise ValueError(f"arch 'v3' with mode {mode!r} and tta=True: mode 1 (averaged probabilities) of the two-resample family of "
                             "simt_tta_label is not built")
        self.dev = torch.device(device)
        self.C, self.mode, self.threshold, self.dtype = num_classes, mode, float(threshold), dtype
        scales = tuple(tuple(s) for s in scales)
        if mode != "argmax" and not tta:
            scales = scales[:1]
        self.tta, self.flip = bool(tta), bool(flip)
        self.terms = ops.tta_terms(scales, self.flip) if self.tta else None      # ValueError above TTA_MAX terms, before any plan is built
        self.arch = arch
        params = {k: v.detach().to(self.dev, torch.float32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
        if arch == "v3":
            from simt_amd.engine_v3 import V3Plan
            kw = {"layers": tuple(layers)} if layers is not None else {}
            self.plans = [V3Plan(params, batch, h, w, num_classes, open_classes, open_classes > 0, dtype=dtype, train=False, **kw)
                          for (h, w) in scales]
            self._fwd = [v3_low_res_forward(plan) for plan in self.plans]
        elif arch == "vgg":
            from simt_amd.engine_vgg import VggPlan
            kw = {"vgg_layers": list(layers)} if layers is not None else {}
            self.plans = [VggPlan(params, batch, h, w, num_classes + open_classes, dtype=dtype, train=False, **kw) for (h, w) in scales]
            self.head = "x"
        else:
            if arch == "multi":
                heads, self.head = multi_heads(num_classes, open_classes, open_classes > 0), "x2"
            else:
                heads, self.head = single_head(num_classes), "x"
            kw = {"layers": layers} if layers is not None else {}
            self.plans = [TrunkPlan(params, batch, h, w, heads, dtype=dtype, train=False, **kw) for (h, w) in scales]
        self.scales = scales
        self.B, (self.H, self.W) = batch, tuple(label_hw)
        self.labels = torch.zeros(batch, self.H, self.W, device=self.dev, dtype=torch.uint8)
        self.counts = torch.zeros(num_classes + 1, device=self.dev, dtype=torch.int64)
        self.prob = torch.zeros_like(self.plans[0].out[self.head]) if mode != "argmax" and arch != "v3" and not tta else None
        if self.tta:         # per term: its low-res logits (arg-max) or their softmax (confidence rules)
            self._hold = tta_hold_buffers(self.plans, None if arch == "v3" else self.head, self.flip)
        self.conf_hist = torch.zeros(num_classes, CONF_BINS, device=self.dev, dtype=torch.int64) if mode == "class_balanced" else None
        self.thresholds = None

    def set_thresholds(self, thr):
        """Install the per-class thresholds of mode "class_balanced": C float32 values (kept iff conf >= thr[class])."""
        if self.mode != "class_balanced":
            raise ValueError("per-class thresholds belong to mode 'class_balanced'")
        thr = np.ascontiguousarray(np.asarray(thr, dtype=np.float32).reshape(-1))
        if thr.shape != (self.C,) or np.isnan(thr).any():
            raise ValueError(f"{self.C} thresholds expected (no NaN), got {thr!r}")
        self.thresholds = thr

    def _conf_launch(self, images, thr, out, counts, hist):
        """The forward of the first scale, then one class-balanced launch (labels, statistics or both)."""
        if len(images) != len(self.plans):
            raise ValueError(f"{len(self.plans)} input scale(s) expected, got {len(images)} image tensor(s)")
        if self.tta:
            self._tta_launch(images, 1, thr, out, counts, hist)
            return
        tail = (self.B, self.H, self.W, self.C, thr.ctypes.data if thr is not None else None, ops._p(out), ops._p(counts), ops._p(hist),
                ops.stream_ptr())
        if self.arch == "v3":
            (la, ha, wa, lda, hia, wia), = v3_low_res_logits(self.plans, self._fwd, images, self.scales, self.dev)
            L.call("simt_pseudo_conf2_u8", ops._p(la), ha, wa, lda, hia, wia, *tail)
            return
        o = self.plans[0].forward(images[0].to(self.dev))[self.head]
        B, h, w, ld = o.shape
        ops.softmax_rows(o, ld, self.prob, ld, B * h * w, self.C)
        L.call("simt_pseudo_conf_u8", ops._p(self.prob), h, w, ld, *tail)

    def _tta_launch(self, images, mode, thr, out, counts, hist):
        """One forward per term, then one simt_tta_label launch.  mode 1: the terms hold probabilities (one simt_softmax_rows each)."""
        maps = tta_low_res_maps(self.plans, self._fwd if self.arch == "v3" else None, None if self.arch == "v3" else self.head, images,
                                self.scales, self.flip, self._hold, self.dev, prob_classes=self.C if mode == 1 else None)
        ops.tta_label(maps, B=self.B, H=self.H, W=self.W, Cn=self.C, mode=mode, threshold=self.threshold, thr=thr, out=out, counts=counts,
                      hist=hist)

    def accumulate(self, *images):
        """Mode "class_balanced": add the frame's confidence histogram to `conf_hist` (no labels are written)."""
        if self.mode != "class_balanced":
            raise ValueError("accumulate() belongs to mode 'class_balanced'")
        self._conf_launch(images, None, None, None, self.conf_hist)

    def label(self, *images):
        """images: one [B,3,h,w] fp32 tensor (BGR - mean) per scale.  Returns the label map uint8 [B,H,W] (device, reused by the next
        call) and adds its class counts to `counts`."""
        if len(images) != len(self.plans):
            raise ValueError(f"{len(self.plans)} input scale(s) expected, got {len(images)} image tensor(s)")
        if self.mode == "class_balanced":
            if self.thresholds is None:
                raise RuntimeError("class-balanced labels need thresholds: accumulate() over the list, class_thresholds(), set_thresholds()")
            self._conf_launch(images, self.thresholds, self.labels, self.counts, None)
            return self.labels
        mode = 1 if self.mode == "confidence" else 0
        if self.tta:
            self._tta_launch(images, mode, None, self.labels, self.counts, None)
            return self.labels
        if self.arch == "v3":
            outs = v3_low_res_logits(self.plans, self._fwd, images, self.scales, self.dev)
            (la, ha, wa, lda, hia, wia) = outs[0]
            lb, hb, wb, ldb, hib, wib = (outs[1] if len(outs) > 1 else (None, 0, 0, 0, 0, 0))
            L.call("simt_pseudo_label2_u8", ops._p(la), ha, wa, lda, hia, wia, ops._p(lb), hb, wb, ldb, hib, wib, self.B, self.H, self.W,
                   self.C, mode, self.threshold, ops._p(self.labels), ops._p(self.counts), ops.stream_ptr())
            return self.labels
        outs = [plan.forward(img.to(self.dev))[self.head] for plan, img in zip(self.plans, images)]
        if self.mode == "confidence":
            o = outs[0]
            B, h, w, ld = o.shape
            ops.softmax_rows(o, ld, self.prob, ld, B * h * w, self.C)
            outs = [self.prob]
        la = outs[0]
        lb = outs[1] if len(outs) > 1 else None
        hb, wb, ldb = (lb.shape[1], lb.shape[2], lb.shape[3]) if lb is not None else (0, 0, 0)
        L.call("simt_pseudo_label_u8", ops._p(la), la.shape[1], la.shape[2], la.shape[3], ops._p(lb), hb, wb, ldb,
               self.B, self.H, self.W, self.C, mode, self.threshold, ops._p(self.labels), ops._p(self.counts), ops.stream_ptr())
        return self.labels


# ---- host side: names, files, palette, prior ----------------------------------------------------------------------------------------

def label_basename(name):
    """'aachen/aachen_000000_000019_leftImg8bit.png' -> 'aachen_000000_000019_leftImg8bit' (evaluate_simt :152, :156)."""
    return osp.splitext(name.split("/")[-1])[0]


def list_line(set_name, name, out_name):
    """One line of a pseudo-label list in the layout of pseudo_bapa.lst: '<set>/<name>\\t<out_name>/<basename>.png'."""
    return f"{set_name}/{name}\t{out_name}/{label_basename(name)}.png"


def output_paths(data_dir, out_name, name):
    """-> (label PNG, colour PNG) under <data_dir>/<out_name>/."""
    base = osp.join(data_dir, out_name, label_basename(name))
    return base + ".png", base + "_color.png"


def read_palette(devkit_dir):
    """The colour palette of <devkit_dir>/info.json ('palette': [[r, g, b], ...] or flat), zero-padded to 256 entries."""
    with open(osp.join(devkit_dir, "info.json"), "r") as fp:
        info = json.load(fp)
    if "palette" not in info:
        raise ValueError(f"{osp.join(devkit_dir, 'info.json')} has no 'palette' entry (needed by --save-color)")
    flat = [int(v) for v in np.asarray(info["palette"]).reshape(-1)]
    if len(flat) > 768:
        raise ValueError("palette has more than 256 colours")
    return flat + [0] * (768 - len(flat))


def colorize(label, palette):
    """uint8 label map -> mode 'P' image with the palette (colorize_mask of the reference's evaluation script)."""
    from PIL import Image
    img = Image.fromarray(np.asarray(label, dtype=np.uint8)).convert("P")
    img.putpalette(palette)
    return img


def class_dist(counts, num_classes):
    """Normalised prior of compute_ClassDistribution.py:92: counts[:C] / (sum + 10e-10), float64 [C]; 255s do not count."""
    c = np.asarray(counts, dtype=np.float64)[:num_classes]
    return c / (np.sum(c) + 10e-10)


def class_thresholds(hist, portion, cap=0.9):
    """Per-class confidence thresholds of the class-balanced rule from the binned confidences: float32 [C].

    hist: [C, bins] counts, bin = min(bins-1, floor(conf * bins)) (simt_pseudo_conf*_u8).  BDL sorts a class's confidences ascending and
    takes x[round(n * 0.5)], then caps at 0.9; with the share `portion` to keep that index is k = min(round(n * (1 - portion)), n - 1)
    (np.round: half to even).  Here the threshold is the LOWER EDGE of the bin holding x[k]: b = the smallest bin whose inclusive
    cumulative count exceeds k, t = min(float32(b / bins), float32(cap)).  So, uncapped, t <= x[k] < t + 1/bins (a resolution of 1/256),
    the pixels with conf >= t are exactly hist[c][b:].sum() -- at least the n - k asked for, never fewer -- and, t being a float,
    conf >= t is conf > nextafter(t, -inf): the strict rule of the confidence mode.  A class without pixels gets 0; portion = 1 (k = 0) gives the lower edge of the
    class's lowest occupied bin -- 0 for a class with a pixel below 1/bins -- and keeps every pixel."""
    hist = np.asarray(hist)
    if hist.ndim != 2 or not np.issubdtype(hist.dtype, np.integer) or (hist < 0).any():
        raise ValueError("hist must be a [C, bins] array of non-negative integer counts")
    if not 0 < portion <= 1:
        raise ValueError(f"portion must be in (0, 1], not {portion}")
    bins = hist.shape[1]
    thr = np.zeros(hist.shape[0], np.float32)
    for c, row in enumerate(hist.astype(np.int64)):
        n = int(row.sum())
        if n == 0:
            continue
        k = min(int(np.round(n * (1 - portion))), n - 1)
        b = int(np.searchsorted(np.cumsum(row), k, side="right"))
        thr[c] = min(np.float32(b / bins), np.float32(cap))
    return thr


def thresholds_path(list_out, out_name):
    """<out-name>_thresholds.json beside the list file."""
    return osp.join(osp.dirname(osp.abspath(list_out)), f"{out_name}_thresholds.json")


def thresholds_record(thr, counts, hist, *, portion, cap, data_list, source=None, terms=None):
    """The contents of <out-name>_thresholds.json.  Per class: the pixels predicted as it and their confidence histogram (null / absent
    when the thresholds were given, not computed from this list), the threshold, the pixels kept and their share.  terms: the
    test-time-augmentation term list [(h, w, mirrored)] the confidences were averaged over (absent without --tta)."""
    thr = np.asarray(thr, np.float32)
    C = len(thr)
    classes = []
    for c in range(C):
        n = int(hist[c].sum()) if hist is not None else None
        kept = int(counts[c])
        e = {"class": c, "pixels": n, "threshold": float(thr[c]), "kept": kept, "kept_share": kept / n if n else None}
        if hist is not None:
            e["hist"] = [int(v) for v in hist[c]]
        classes.append(e)
    rec = {"num_classes": C, "bins": CONF_BINS, "portion": portion, "cap": cap, "data_list": data_list, "thresholds_from": source,
           "classes": classes}
    if terms is not None:
        rec["tta_terms"] = [{"h": int(h), "w": int(w), "flip": bool(f)} for (h, w, f) in terms]
    return rec


def save_json_atomic(obj, path):
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        with open(tmp, "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")
        os.replace(tmp, path)
    finally:
        if osp.exists(tmp):
            os.remove(tmp)


def load_thresholds(path, num_classes):
    """The thresholds of a file written by an earlier class-balanced export (--thresholds-from): -> (float32 [C], the record).
    Raises ValueError naming the field when the file was made for another class count or binning."""
    with open(path, "r") as f:
        rec = json.load(f)
    for field, want in (("num_classes", num_classes), ("bins", CONF_BINS)):
        if rec.get(field) != want:
            raise ValueError(f"{path}: {field} is {rec.get(field)!r}, this export has {field} = {want}")
    classes = rec.get("classes")
    if not isinstance(classes, list) or len(classes) != num_classes:
        raise ValueError(f"{path}: 'classes' must list {num_classes} entries")
    thr = np.array([e["threshold"] for e in classes], dtype=np.float32)       # floats were written from float32: exact
    return thr, rec


def save_png_atomic(img, path):
    """Encode to a temporary name in the target directory, then os.replace: a reader never sees a partial file."""
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        img.save(tmp, format="PNG")
        os.replace(tmp, path)
    finally:
        if osp.exists(tmp):
            os.remove(tmp)


def save_npy_atomic(arr, path):
    tmp = f"{path}.{os.getpid()}.tmp"
    with open(tmp, "wb") as f:
        np.save(f, arr)
    os.replace(tmp, path)


def _bounded_map(pool, fn, items, depth):
    """pool.map(fn, items) in order, with at most `depth` results pending (pool.map would decode the whole list ahead of the GPU)."""
    pending = deque()
    it = iter(items)
    for x in it:
        pending.append(pool.submit(fn, x))
        if len(pending) >= depth:
            break
    while pending:
        fut = pending.popleft()
        for x in it:
            pending.append(pool.submit(fn, x))
            break
        yield fut.result()


def export(state, data_dir, data_list, out_name, list_out, *, set_name="train", save_color=False, devkit_dir=None, workers=8,
           class_dist_out=None, num_classes=19, open_classes=0, arch="multi", scales=DEFAULT_SCALES, label_hw=(1024, 2048),
           mode="argmax", threshold=0.8, dtype=torch.float32, device="cuda:0", layers=None, labeller=None, verbose=True,
           portion=0.5, cap=0.9, thresholds=None, thresholds_source=None, tta=False, flip=False):
    """Label every frame of cityscapesDataSet(data_dir, data_list, set=set_name) and write
    <data_dir>/<out_name>/<basename>.png (8-bit trainIds, 255 = ignore; with save_color also <basename>_color.png), the list file
    `list_out` and the prior `class_dist_out` (default: ClassDist_<out_name>.npy beside the list).  Returns the int64 counts [C+1].

    mode "class_balanced": a first pass over the whole list only accumulates the per-class confidence histogram (nothing is written),
    class_thresholds(hist, portion, cap) gives the thresholds, and the second pass labels with them; `thresholds` (C floats, e.g. of
    load_thresholds) skips the first pass.  Also writes <out_name>_thresholds.json beside the list; the prior is that of the kept
    pixels, as in confidence mode.
    tta / flip: test-time augmentation (PseudoLabeller); a class-balanced export records the term list in its thresholds file."""
    from PIL import Image

    from simt_amd.data.pipeline import IMG_MEAN, InputPrep
    from simt_amd.dataset.cityscapes_dataset import cityscapesDataSet
    workers = min(max(1, int(workers)), MAX_WORKERS)
    palette = None
    if save_color:
        if not devkit_dir:
            raise ValueError("save_color needs devkit_dir (the palette of info.json)")
        palette = read_palette(devkit_dir)
    if class_dist_out is None:
        class_dist_out = osp.join(osp.dirname(osp.abspath(list_out)), f"ClassDist_{out_name}.npy")
    dev = torch.device(device)
    lab = labeller or PseudoLabeller(state, num_classes=num_classes, open_classes=open_classes, arch=arch, scales=scales,
                                     label_hw=label_hw, mode=mode, threshold=threshold, dtype=dtype, device=dev, layers=layers,
                                     tta=tta, flip=flip)
    if lab.B != 1:
        raise ValueError("export labels one frame at a time (batch 1)")
    C = lab.C
    balanced = lab.mode == "class_balanced"
    if balanced and not 0 < portion <= 1:
        raise ValueError(f"portion must be in (0, 1], not {portion}")
    ds = cityscapesDataSet(data_dir, data_list, crop_size=(lab.scales[0][1], lab.scales[0][0]), mean=IMG_MEAN, scale=False, mirror=False,
                           set=set_name)
    os.makedirs(osp.join(data_dir, out_name), exist_ok=True)
    lab.counts.zero_()

    def write(slot, name):
        slot["ready"].synchronize()                     # the D2H copy into this pinned buffer has landed
        m = slot["host"][0].numpy()
        png, color = output_paths(data_dir, out_name, name)
        save_png_atomic(Image.fromarray(m), png)
        if palette is not None:
            save_png_atomic(colorize(m, palette), color)

    # pinned staging buffers, one per label map in flight: the GPU labels frame i+1 while the writers encode frame i
    slots = [{"host": torch.empty(1, lab.H, lab.W, dtype=torch.uint8).pin_memory(), "ready": torch.cuda.Event(), "job": None}
             for _ in range(workers + 2)]
    preps = {}
    xs = [torch.empty(1, 3, h, w, device=dev) for (h, w) in lab.scales]

    def frames(readers):
        """(index, name) of every frame of the list, in order, with its resized inputs in `xs`."""
        for i, (rgb, _, name) in enumerate(_bounded_map(readers, ds.decode, range(len(ds)), 2 * workers)):
            key = rgb.shape[:2]
            if key not in preps:
                preps[key] = [InputPrep(1, key, (w, h), dev, with_label=False) for (h, w) in lab.scales]
            rgb_d = torch.from_numpy(rgb[None]).to(dev)
            for prep, x in zip(preps[key], xs):
                prep.run(rgb_d, x)
            yield i, name

    hist = None
    if balanced:
        if thresholds is None:                           # pass 1: statistics only
            lab.conf_hist.zero_()
            with ThreadPoolExecutor(workers) as readers:
                for _ in frames(readers):
                    lab.accumulate(*xs)
            hist = lab.conf_hist.cpu().numpy()
            thresholds = class_thresholds(hist, portion, cap)
        lab.set_thresholds(thresholds)
    lines = []
    with ThreadPoolExecutor(workers) as readers, ThreadPoolExecutor(workers) as writers:
        for i, name in frames(readers):
            out = lab.label(*xs)
            slot = slots[i % len(slots)]
            if slot["job"] is not None:
                slot["job"].result()                    # the writer is done with this buffer (and re-raises its error, if any)
            slot["host"].copy_(out, non_blocking=True)
            slot["ready"].record()
            slot["job"] = writers.submit(write, slot, name)
            lines.append(list_line(set_name, name, out_name))
        for slot in slots:
            if slot["job"] is not None:
                slot["job"].result()
    counts = lab.counts.cpu().numpy()
    tmp = f"{list_out}.{os.getpid()}.tmp"
    with open(tmp, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    os.replace(tmp, list_out)
    save_npy_atomic(class_dist(counts, C), class_dist_out)
    if balanced:
        given = hist is None
        save_json_atomic(thresholds_record(lab.thresholds, counts, hist, portion=None if given else portion, cap=None if given else cap,
                                           data_list=data_list, source=thresholds_source, terms=lab.terms),
                         thresholds_path(list_out, out_name))
    if verbose:
        total = max(int(counts.sum()), 1)
        share = counts[:C] / max(int(counts[:C].sum()), 1)
        print(f"{len(lines)} label maps -> {osp.join(data_dir, out_name)}; list {list_out}; prior {class_dist_out}")
        for c in range(C):
            print(f"class {c:3d}: {100 * share[c]:6.2f} %" + (f"   threshold {lab.thresholds[c]:.6f}" if balanced else ""))
        print(f"ignored (255): {100 * counts[C] / total:.2f} % of the pixels")
    return counts


# ---- command line -------------------------------------------------------------------------------------------------------------------

def _wh(s):
    try:
        w, h = (int(v) for v in s.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected W,H, got {s!r}")
    if w <= 0 or h <= 0:
        raise argparse.ArgumentTypeError(f"expected positive W,H, got {s!r}")
    return w, h


def get_arguments(argv=None):
    from simt_amd.tools.trainV2_simt import add_v3_layers
    p = argparse.ArgumentParser(description="Export pseudo labels (PNG + list + class prior) from a DeepLab-v2, DeepLabv3 or DeepLab-VGG16 "
                                            "checkpoint on MI355X")
    p.add_argument("--restore-from", type=str, required=True, help="source checkpoint (the same key forms as the training tools)")
    p.add_argument("--arch", choices=list(ARCHS), default="multi",
                   help="multi: DeeplabMulti (head layer6, first C channels); single: Res_Deeplab of model/deeplab.py; "
                        "v3: DeepLabv3 (model/deeplabv3.py, trunk depth --v3-layers); vgg: DeeplabVGG (model/deeplab_vgg.py)")
    p.add_argument("--num-classes", type=int, default=19)
    p.add_argument("--open-classes", type=int, default=0,
                   help="open-set classes of a SimT checkpoint (--arch multi, v3 or vgg); 0 for a source model")
    p.add_argument("--data-dir", type=str, default="")
    p.add_argument("--data-list", type=str, default="../dataset/cityscapes_list/train.txt")
    p.add_argument("--set", type=str, default="train")
    p.add_argument("--input-size", type=_wh, action="append", default=None,
                   help="W,H of an input scale; repeat for several (default 1024,512 and 1280,640; --threshold uses the first)")
    p.add_argument("--label-size", type=_wh, default=(2048, 1024), help="W,H of the label maps")
    p.add_argument("--out-name", type=str, default="pseudo_labels", help="label directory under --data-dir, and the list's label prefix")
    p.add_argument("--list-out", type=str, default=None, help="list file to write (default <out-name>.lst)")
    p.add_argument("--class-dist-out", type=str, default=None, help="class prior .npy (default ClassDist_<out-name>.npy beside the list)")
    p.add_argument("--threshold", type=float, default=None,
                   help="confidence mode: softmax arg-max where max > T, 255 elsewhere (trainV2_simt.py:353-359); default: plain arg-max")
    p.add_argument("--class-balanced", type=float, default=None, metavar="P",
                   help="class-balanced mode (CBST / BDL): per class, keep the share P (0 < P <= 1) of its most confident predictions; "
                        "the threshold is the lower edge of the 1/256 confidence bin at that rank, capped at --threshold-cap")
    p.add_argument("--threshold-cap", type=float, default=0.9, metavar="T", help="upper limit of the class-balanced thresholds")
    p.add_argument("--thresholds-from", type=str, default=None, metavar="FILE",
                   help="class-balanced mode with the thresholds of <out-name>_thresholds.json of an earlier export (e.g. of a subset "
                        "list): no statistics pass")
    p.add_argument("--tta", action="store_true",
                   help="test-time augmentation: every --input-size counts in every mode (logits summed / probabilities averaged over the "
                        "scales, one label launch)")
    p.add_argument("--tta-flip", action="store_true", help="--tta, and the horizontally mirrored frame of every scale as well")
    p.add_argument("--save-color", action="store_true", help="also write <name>_color.png with the palette of <devkit-dir>/info.json")
    p.add_argument("--devkit-dir", type=str, default="../dataset/cityscapes_list")
    p.add_argument("--eval-dtype", choices=["f32", "bf16"], default="f32",
                   help="arithmetic of the forwards: fp32 like the reference; bf16 is a labelled opt-in")
    p.add_argument("--num-workers", type=int, default=8, help=f"decode / encode threads each (capped at {MAX_WORKERS})")
    p.add_argument("--gpu", type=int, default=0)
    add_v3_layers(p)
    args = p.parse_args(argv)
    args.tta = args.tta or args.tta_flip
    if args.tta:
        if args.arch == "v3" and (args.threshold is not None or args.class_balanced is not None or args.thresholds_from):
            p.error("--tta with the confidence rules of --arch v3 is not built (the averaged softmax of a model that upsamples inside)")
        try:
            ops.tta_terms([(h, w) for (w, h) in (args.input_size or [(1024, 512), (1280, 640)])], args.tta_flip)
        except ValueError as e:
            p.error(f"--tta: {e}")
    if args.arch == "single" and args.open_classes:
        p.error("--arch single: Res_Deeplab has no open-set classes (--open-classes must be 0)")
    if args.threshold is not None and (args.class_balanced is not None or args.thresholds_from):
        p.error("--threshold (one global threshold) and --class-balanced / --thresholds-from (one per class) exclude each other")
    if args.class_balanced is not None and not 0 < args.class_balanced <= 1:
        p.error(f"--class-balanced P: the share to keep must be in (0, 1], not {args.class_balanced}")
    if args.class_balanced is not None and args.thresholds_from:
        p.error("--thresholds-from takes the thresholds as they are: give it without --class-balanced P")
    if not 0 < args.threshold_cap <= 1:
        p.error(f"--threshold-cap must be in (0, 1], not {args.threshold_cap}")
    if (args.class_balanced is not None or args.thresholds_from) and args.num_classes > MAX_CB_CLASSES:
        p.error(f"class-balanced labels take at most {MAX_CB_CLASSES} classes")
    return args


SINGLE_MODELS = {"v3": "DeepLabv3", "vgg": "DeepLabVGG"}     # --arch -> the trainV2_simt --model name
HEAD_PREFIX = {"v3": "conv.", "vgg": "classifier."}         # the classifier producing the first C channels


def restore_single_model(arch, path, num_classes, open_classes, v3_layers):
    """The state of DeepLabv3 / DeeplabVGG (--arch v3 | vgg; the SimT model with open_classes > 0) with `path` loaded the way the warm-up
    stage loads it (trainV1_warmup.restore_single: the module's keys, or a torchvision ImageNet file mapped onto the trunk).  Raises
    FileNotFoundError / RuntimeError (no file, no tensor matched) and SystemExit when no classifier tensor was restored: labels from a
    head left at its init would look like results.  -> (state, tensors restored, layout name)."""
    from simt_amd.tools.trainV1_warmup import restore_single
    from simt_amd.tools.trainV2_simt import single_model_state, single_model_states
    name = SINGLE_MODELS[arch]
    if open_classes:
        state, _ = single_model_states(name, num_classes, open_classes, v3_layers)
    else:
        state = single_model_state(name, num_classes, v3_layers)
    init = {k: v for k, v in state.items() if k.startswith(HEAD_PREFIX[arch])}
    n, layout = restore_single(state, path, arch, required=True)
    if all(state[k] is v for k, v in init.items()):
        shapes = ", ".join(f"{k} {tuple(v.shape)}" for k, v in init.items() if k.endswith("weight"))
        raise SystemExit(f"--restore-from {path!r} ({layout} layout): no classifier tensor ({HEAD_PREFIX[arch]}*) matched {shapes}; "
                         f"check --num-classes {num_classes} / --open-classes {open_classes}"
                         + (f" / --v3-layers {' '.join(map(str, v3_layers))}" if arch == "v3" else "")
                         + " (an ImageNet trunk file has no classifier to export labels from)")
    return state, n, layout


def main(argv=None):
    args = get_arguments(argv)
    from simt_amd import model_spec as ms
    from simt_amd.tools.trainV2_simt import restore
    C, K = args.num_classes, args.open_classes
    thresholds = None
    if args.thresholds_from:                                         # checked before the GPU is touched, like everything below
        try:
            thresholds, _ = load_thresholds(args.thresholds_from, C)
        except (OSError, ValueError, KeyError, TypeError) as e:
            raise SystemExit(f"--thresholds-from: {e}")
    if args.arch in SINGLE_MODELS:                                   # checked before the GPU is touched
        state, n, _ = restore_single_model(args.arch, args.restore_from, C, K, tuple(args.v3_layers))
    if not torch.cuda.is_available():
        raise SystemExit("make_pseudo_labels needs a GPU: the forward and the label kernel have no CPU fallback")
    dev = torch.device("cuda", args.gpu)
    torch.cuda.set_device(dev)
    if args.arch not in SINGLE_MODELS:
        single = args.arch == "single"
        shapes = ms.state_shapes(C, single_head=True) if single else ms.state_shapes(C, K, K > 0)
        state = ms.reference_init(shapes)
        n = restore(state, args.restore_from, strip_prefix=6, required=True)
    layers = tuple(args.v3_layers) if args.arch == "v3" else None
    sizes = args.input_size or [(1024, 512), (1280, 640)]
    dtype = torch.bfloat16 if args.eval_dtype == "bf16" else torch.float32
    list_out = args.list_out or f"{args.out_name}.lst"
    balanced = args.class_balanced is not None or thresholds is not None
    mode = "class_balanced" if balanced else "argmax" if args.threshold is None else "confidence"
    print(f"restored {n} tensors from {args.restore_from}; arch {args.arch}, {mode}"
          + (f" (threshold {args.threshold})" if args.threshold is not None else "")
          + (f" (keep {args.class_balanced} per class, cap {args.threshold_cap})" if args.class_balanced is not None else "")
          + (f" (thresholds of {args.thresholds_from})" if thresholds is not None else "")
          + (f"; test-time augmentation over {len(sizes)} scale(s)" + (" x mirror" if args.tta_flip else "") if args.tta else "")
          + ("" if dtype == torch.float32 else "   (bf16 plans: not the reference's fp32 arithmetic)"))
    export(state, args.data_dir, args.data_list, args.out_name, list_out, set_name=args.set, save_color=args.save_color,
           devkit_dir=args.devkit_dir, workers=args.num_workers, class_dist_out=args.class_dist_out, num_classes=C, open_classes=K,
           arch=args.arch, scales=[(h, w) for (w, h) in sizes], label_hw=(args.label_size[1], args.label_size[0]), mode=mode,
           threshold=args.threshold if args.threshold is not None else 0.0, dtype=dtype, device=dev, layers=layers,
           portion=args.class_balanced if args.class_balanced is not None else 0.5, cap=args.threshold_cap, thresholds=thresholds,
           thresholds_source=args.thresholds_from, tta=args.tta, flip=args.tta_flip)


if __name__ == "__main__":
    main()
