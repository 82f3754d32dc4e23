"""Evaluation of a SimT / DeepLab-v2 model on MI355X: the reference's tools/evaluate_cityscapes.py (evaluate_simt
:96-162, fast_hist :81-83, per_class_iu :86-87, label_mapping :90-94) with the per-image CPU/numpy work moved to the GPU.

    ev = Evaluator(state_dict, num_classes=19, open_classes=K, label_hw=(1024, 2048), scales=((512, 1024), (640, 1280)))
    for image_a, image_b, gt in loader:            # the image at both input scales, ground-truth label ids [B,H,W] int64
        ev.add(image_a, image_b, gt)
    miou, per_class = ev.result()

Two eval-mode plans (BN folded) produce the main head's logits at both scales; one fused kernel upsamples both to the
label resolution (align_corners=True), sums, arg-maxes; the confusion histogram is accumulated on the device with
integer atomics.  Dataset IO (PIL decoding, file lists) stays outside: `add` takes tensors.

model: "v2" DeepLab-v2 (DeeplabMulti, the reference's), "v3" DeepLabv3(nc, openc, openset=True), "vgg" DeeplabVGG(nc + openc).
DeepLabv3 upsamples inside the model (model/deeplabv3.py:137, align_corners=False, to the input size); its plans stop at the
low-res logits and simt_upsample2_sum_argmax applies both resamples per label pixel without storing the input-size map.
DeeplabVGG returns low-res logits like DeepLab-v2: the same kernel as v2 over its first nc channels.

Test-time augmentation: Evaluator(..., scales=<any number of sizes>, flip=True) runs one forward per term of ops.tta_terms(scales, flip)
-- per scale the frame, then its horizontal mirror (the same plan on x.flip(3)) -- keeps every term's low-res logits and labels them
with ONE simt_tta_label launch, which reads a mirrored term at mirrored column indices.  Up to two scales without flip take the
reference's recipe and launches above, unchanged."""
import numpy as np
import torch

from simt_amd import _lib as L
from simt_amd import ops
from simt_amd.engine import TrunkPlan, multi_heads


def fast_hist(a, b, n):
    k = (a >= 0) & (a < n)
    return np.bincount(n * a[k].astype(int) + b[k], minlength=n ** 2).reshape(n, n)


def per_class_iu(hist):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


def label_mapping(inp, mapping):
    out = np.copy(inp)
    for ind in range(len(mapping)):
        out[inp == mapping[ind][0]] = mapping[ind][1]
    return np.array(out, dtype=np.int64)


def v3_low_res_forward(plan):
    """The forward of an eval-mode V3Plan without its last launch, the in-model upsample to the input size: the label kernels
    (simt_upsample2_sum_argmax, simt_pseudo_label2_u8) apply it per label pixel from the low-res logits, as step_single.SimTSingleTrainer
    trims its forward.  -> a LaunchList that stops at plan.logits."""
    from simt_amd.engine import LaunchList
    assert plan.fwd_list.items[-1].tag == "simt_upsample_nchw"
    lst = LaunchList()
    lst.items = plan.fwd_list.items[:-1]
    return lst


def tta_low_res_maps(plans, fwds, head, images, scales, flip, hold, dev, prob_classes=None):
    """One forward per term of ops.tta_terms(scales, flip), in its order: scale k's plan on images[k], then (flip) on images[k].flip(3) --
    the prepared input mirrored, no second resize.  A plan's output is reused by its next forward, so every term's low-res logits are
    copied into hold[term] (tensors shaped like the plan's output, owned by the caller) -- or, with prob_classes = C, their softmax over
    the first C channels is written there instead (simt_softmax_rows: the probabilities of simt_tta_label's mode 1).
    fwds: the trimmed V3Plan forwards (v3_low_res_forward), or None: plans whose forward returns {head: NHWC logits}.
    -> the `maps` of ops.tta_label: [(hold[term], h, w, ld, hi, wi, flipped)], (hi, wi) = the input size for v3, (0, 0) otherwise."""
    if len(images) != len(plans):
        raise ValueError(f"{len(plans)} input scale(s) expected, got {len(images)} image tensor(s)")
    maps = []
    for k, (plan, img) in enumerate(zip(plans, images)):
        x = img.to(dev)
        for f in ((False, True) if flip else (False,)):
            xin = x.flip(3) if f else x
            if fwds is not None:
                plan.x_in.copy_(xin)
                fwds[k].run()
                lg, (h, w), ld, (hi, wi) = plan.logits, plan.feat_hw, plan.ldq, scales[k]
            else:
                lg = plan.forward(xin)[head]
                (h, w, ld), (hi, wi) = lg.shape[1:], (0, 0)
            buf = hold[len(maps)]
            if prob_classes is None:
                buf.copy_(lg)
            else:
                ops.softmax_rows(lg, ld, buf, ld, buf.numel() // ld, prob_classes)
            maps.append((buf, h, w, ld, hi, wi, f))
    return maps


def tta_hold_buffers(plans, head, flip):
    """The holding buffers of tta_low_res_maps: per term a tensor like its plan's low-res output (head None: V3Plan.logits)."""
    return [torch.zeros_like(plan.logits if head is None else plan.out[head]) for plan in plans for _ in range(2 if flip else 1)]


def v3_low_res_logits(plans, fwds, images, scales, dev):
    """Run each trimmed V3Plan forward on its image.  -> [(logits [B*h*w, ld], h, w, ld, hi, wi)] per scale, (hi, wi) = the plan's input
    size (the in-model upsample's target)."""
    outs = []
    for plan, lst, img, (hi, wi) in zip(plans, fwds, images, scales):
        plan.x_in.copy_(img.to(dev))
        lst.run()
        (h, w) = plan.feat_hw
        outs.append((plan.logits, h, w, plan.ldq, hi, wi))
    return outs


class Evaluator:
    MODELS = ("v2", "v3", "vgg")

    def __init__(self, state, *, num_classes=19, open_classes=0, openset=None, batch=1, label_hw=(1024, 2048),
                 scales=((512, 1024), (640, 1280)), dtype=torch.float32, device="cuda:0", layers=None, model="v2", flip=False):
        # dtype: fp32 by default -- the reference evaluates in fp32 (evaluate_cityscapes.py:96-162) and the metric is defined "argmax bit-exact";
        # bf16 plans are an explicit, labelled opt-in (tools: --eval-dtype bf16; < 0.2 % of the arg-max positions differ)
        # layers: trunk depth of the plans -- v2: ResNet layers (4 entries), v3: layer1..layer3 of the ResNet, vgg: the VGG_LAYERS list
        # scales / flip: the terms of the label (ops.tta_terms).  Up to two scales, no flip: the reference's recipe on the two-map kernels;
        # anything else (more scales, the mirrored frames): one forward per term and one simt_tta_label launch
        if model not in self.MODELS:
            raise ValueError(f"model must be one of {self.MODELS}, got {model!r}")
        self.model = model
        self.dev = torch.device(device)
        self.dtype = dtype
        self.C = num_classes
        openset = (open_classes > 0) if openset is None else openset
        params = {k: v.detach().to(self.dev, torch.float32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}
        self.scales = [tuple(s) for s in scales]
        self.flip = bool(flip)
        self.terms = ops.tta_terms(self.scales, self.flip)                   # ValueError above TTA_MAX terms, before any plan is built
        self.tta = self.flip or len(self.scales) > 2
        if model == "v2":
            kw = {"layers": layers} if layers is not None else {}
            self.plans = [TrunkPlan(params, batch, h, w, multi_heads(num_classes, open_classes, openset), dtype=dtype, train=False, **kw)
                          for (h, w) in scales]
        elif model == "v3":
            from simt_amd.engine_v3 import V3Plan
            kw = {"layers": tuple(layers)} if layers is not None else {}
            self.plans = [V3Plan(params, batch, h, w, num_classes, open_classes, openset, dtype=dtype, train=False, **kw) for (h, w) in scales]
            self._fwd = [v3_low_res_forward(plan) for plan in self.plans]
        else:
            from simt_amd.engine_vgg import VggPlan
            kw = {"vgg_layers": list(layers)} if layers is not None else {}
            self.plans = [VggPlan(params, batch, h, w, num_classes + (open_classes if openset else 0), dtype=dtype, train=False, **kw)
                          for (h, w) in scales]
        self.B, (self.H, self.W) = batch, label_hw
        self._head = {"v2": "x2", "v3": None, "vgg": "x"}[model]
        self._hold = tta_hold_buffers(self.plans, self._head, self.flip) if self.tta else None
        self.pred = torch.zeros(batch, self.H, self.W, device=self.dev, dtype=torch.int32)
        self.hist = torch.zeros(num_classes * num_classes, device=self.dev, dtype=torch.int64)

    def load(self, state):
        """Refresh the weights from a (training) state dict and re-fold / re-pack both plans: the in-loop evaluation of
        tools/trainV2_simt.py:452-456 reuses one Evaluator for the whole run."""
        for plan in self.plans:
            for k, v in plan.p.items():
                if k in state and v.dtype != torch.long:
                    v.copy_(state[k])
        for plan in self.plans:                   # packed / folded operands are per plan (per input size), also when plans share `p`
            plan.repack()
        self.hist.zero_()

    def predict(self, *images):
        """images: one [B,3,h,w] fp32 tensor per scale.  Returns the arg-max label map [B,H,W] int32 (device)."""
        if self.tta:
            maps = tta_low_res_maps(self.plans, self._fwd if self.model == "v3" else None, self._head, images, self.scales, self.flip,
                                    self._hold, self.dev)
            ops.tta_label(maps, B=self.B, H=self.H, W=self.W, Cn=self.C, mode=0, pred=self.pred)
            return self.pred
        if self.model == "v3":
            outs = v3_low_res_logits(self.plans, self._fwd, images, self.scales, self.dev)
            (la, ha, wa, lda, hia, wia) = outs[0]
            lb, hb, wb, ldb, hib, wib = (outs[1] if len(outs) > 1 else (None, 0, 0, 0, 0, 0))
            L.call("simt_upsample2_sum_argmax", ops._p(la), ha, wa, lda, hia, wia, ops._p(lb), hb, wb, ldb, hib, wib, self.B, self.H, self.W,
                   self.C, ops._p(self.pred), ops.stream_ptr())
            return self.pred
        outs = []
        for plan, img in zip(self.plans, images):
            o = plan.forward(img.to(self.dev))["x2" if self.model == "v2" else "x"]
            outs.append((o, o.shape[1], o.shape[2], o.shape[3]))
        (la, ha, wa, lda) = outs[0]
        lb, hb, wb, ldb = (outs[1] if len(outs) > 1 else (None, 0, 0, 0))
        L.call("simt_upsample_sum_argmax", ops._p(la), ha, wa, lda, ops._p(lb), hb, wb, ldb, self.B, self.H, self.W, self.C,
               ops._p(self.pred), ops.stream_ptr())
        return self.pred

    def add(self, *images_and_gt):
        *images, gt = images_and_gt
        pred = self.predict(*images)
        gt = gt.to(self.dev).long().contiguous()
        L.call("simt_confusion_hist", ops._p(gt), ops._p(pred), gt.numel(), self.C, ops._p(self.hist), ops.stream_ptr())

    def result(self):
        hist = self.hist.cpu().numpy().reshape(self.C, self.C).astype(np.float64)
        ius = per_class_iu(hist)
        return round(float(np.nanmean(ius)) * 100, 2), ius


def evaluate_simt(state, data_dir, data_list, gt_dir, devkit_dir="../dataset/cityscapes_list", *, num_classes=19, open_classes=0, set_name="val",
                  device="cuda:0", dtype=torch.float32, evaluator=None, rank=0, world=1, process_group=None, verbose=True, workers=4,
                  model="v2", layers=None, scales=None, flip=False):
    """File-based evaluation loop of the reference (evaluate_cityscapes.py:96-162): every validation frame at crop sizes (1024, 512) and
    (1280, 640) -> logits[:, :num_classes] of the main head, upsampled to 1024 x 2048, summed, arg-maxed -> fast_hist against the
    ground-truth label ids mapped with info.json's label2train -> mIoU (round(nanmean * 100, 2)).
    dtype: fp32 like the reference; torch.bfloat16 is an opt-in whose mIoU is printed with a "(bf16 plans)" label.
    Host: file lists, PNG decoding (threads), the label LUT.  Device: both resizes (Pillow-exact), BGR - mean, both forwards, the fused
    upsample + sum + arg-max, the histogram.  Data parallel: ranks take strided shards of the list and the histogram is all-reduced.
    model / layers: see Evaluator ("v2", "v3" or "vgg"; the plans' trunk depth).
    scales: the input sizes (h, w), default the reference's pair; flip: also the mirrored frame of every scale (test-time augmentation,
    see Evaluator).  A given `evaluator` brings its own."""
    import json
    from concurrent.futures import ThreadPoolExecutor
    from os.path import join

    from simt_amd.data.pipeline import IMG_MEAN, InputPrep
    from simt_amd.dataset.cityscapes_dataset import cityscapesDataSet
    from simt_amd.tools.ntm_stats import mapping_lut
    dev = torch.device(device)
    with open(join(devkit_dir, "info.json"), "r") as fp:
        info = json.load(fp)
    name_classes = info.get("label", [str(i) for i in range(num_classes)])
    lut = mapping_lut(np.array(info["label2train"]))
    ds = cityscapesDataSet(data_dir, data_list, crop_size=(1024, 512), mean=IMG_MEAN, scale=False, mirror=False, set=set_name)
    scales = tuple(tuple(s) for s in scales) if scales is not None else ((512, 1024), (640, 1280))
    ev = evaluator or Evaluator(state, num_classes=num_classes, open_classes=open_classes, dtype=dtype, device=dev, model=model, layers=layers,
                                scales=scales, flip=flip)
    if evaluator is not None:
        ev.load(state)
    from PIL import Image

    def fetch(i):
        rgb, _, name = ds.decode(i)
        gt_path = "%s/%s" % (gt_dir, name.split("leftImg8bit")[0] + "gtFine_labelIds.png")
        return rgb, lut[np.array(Image.open(gt_path))], name
    idx = list(range(rank, len(ds), world))
    preps = {}
    xs = [torch.empty(1, 3, h, w, device=dev) for (h, w) in ev.scales]
    with ThreadPoolExecutor(max(1, workers)) as pool:
        for rgb, label, name in pool.map(fetch, idx):
            key = rgb.shape[:2]
            if key not in preps:
                preps[key] = [InputPrep(1, key, (w, h), dev, with_label=False) for (h, w) in ev.scales]
            if label.size != ev.H * ev.W:
                print("Skipping: len(gt) = {:d}, len(pred) = {:d}, {:s}".format(label.size, ev.H * ev.W, name))
                continue
            rgb_d = torch.from_numpy(rgb[None]).to(dev)
            for prep, x in zip(preps[key], xs):
                prep.run(rgb_d, x)
            ev.add(*xs, torch.from_numpy(label[None].astype(np.int64)))
    if process_group is not None and world > 1:
        import torch.distributed as dist
        dist.all_reduce(ev.hist, group=process_group)
    miou, ius = ev.result()
    if verbose and rank == 0:
        for ind_class in range(num_classes):
            print("===>" + str(name_classes[ind_class]) + ":\t" + str(round(ius[ind_class] * 100, 2)))
        print("===> mIoU: " + str(miou) + ("" if ev.dtype == torch.float32 else "   (bf16 plans: not the reference's fp32 arithmetic)"))
    return miou


def evaluate_warmup(state, *args, **kw):
    """evaluate_cityscapes.py:165-225: the same loop for a warm-up (no open-set heads) checkpoint."""
    kw["open_classes"] = 0
    return evaluate_simt(state, *args, **kw)
