#!/usr/bin/env python3
"""Warm-up stage on MI355X: the reference's tools/trainV1_warmup.py (plain CE on both heads, SGD over the whole net)
driven by `WarmupTrainer` (simt_amd/step.py).  EVERY flag of the reference (trainV1_warmup.py:60-150) is accepted, the periodic
`evaluate_warmup` + best-mIoU snapshot rotation of :241-256 keeps the reference's file names; data: `cityscapesPseudo` through the device input pipeline (simt_amd/data/pipeline.py) or, with
--synthetic, Cityscapes-shaped synthetic batches.  --restore-from must exist and match (the reference's `k[6:]` prefix strip of :177
is honoured) unless --from-scratch is given.
--cache-dataset device [--cache-gb G], --scale-crop [S ...], --class-mix [P], --colour-jitter [S], --gaussian-blur [P] and
--mask-patches [R] [--mask-patch-size P] as in trainV2_simt: the flags they share, `batches` and the snapshot and train-state keepers live there,
the device set-up and the outer loop of both tools in simt_amd/tools/train_loop.py; `main` below builds the trainer of --model
(`build_trainer`) and hands the loop its step arguments (`step_args`), its loss line (`loss_tail`) and its evaluation.
--train-state FILE [--train-state-every N] as in trainV2_simt: resume from FILE if it exists, keep it current (simt_amd/train_state.py).
--ema [D] as in trainV2_simt: a weight EMA beside the trained model (simt_amd/ema.py), evaluated beside it, kept as
GTA5_BAPA_warmup_ema_iter<i>_mIoU<m>.pth and written at the stop as GTA5_<stop>_ema.pth.
--online-labels [T] [--online-labels-every N]: self-training from a list of images alone (simt_amd/online_labels.py) -- a frozen
copy of the start model, the teacher, labels every batch on the device (one launch per micro-batch, beside the student's forward), pixels whose
confidence is not above T (no value: 0.968; 0 <= T < 1) are ignored and the model trains on those labels by the same cross-entropy.
--data-list-target may then have one column; no label file is opened.  With --colour-jitter, --gaussian-blur or --mask-patches the teacher
labels the batch BEFORE them and the student sees it after (FixMatch / MIC consistency); --class-mix is refused (it needs the labels in the
loader).  With --ema and --online-labels-every N the teacher follows the weight EMA behind every N-th update (the mean teacher); without N it
stays at the start weights.  The loss line gains ` labelled = <share of pixels that received a label>`; --train-state carries the teacher and
the counts and refuses a resume with either flag added, dropped or changed.  With --synthetic the labels are ignored too.  Default: off.
--online-mix [P] (needs --online-labels, --batch-size 2 ... 32, --num-classes <= 32): ClassMix by the teacher's labels, inside the
trainer -- behind the teacher's label launch and in front of the student's forward, with probability P (no value: 1) item i receives, image and
label, the pixels of half of the classes the teacher found in item i+1 (one launch, simt_class_mix_u8; draws seeded by --random-seed).  With
--colour-jitter, --gaussian-blur or --mask-patches the teacher labels the weak view and the mix selects from the students' strong views: a pasted
region carries its partner's jitter, blur and blanked patches.  ` labelled` stays the share of the teacher's labels before the mix.  --train-state
carries the draws' generator and refuses a resume with the flag added, dropped or changed.
--online-labels-weighted [batch|item] (needs --online-labels, --batch-size <= 32; not with --online-labels-balanced): the quality
weights of DACS / DAFormer / MIC -- the model trains on the teacher's arg-max at EVERY pixel and each pixel's cross-entropy is multiplied by q,
the share of pixels whose confidence is above T (T deletes nothing).  batch (no value): one q per batch, the published rule; item: one per image,
and with --online-mix a pasted pixel carries its partner's.  ` labelled` stays the share of confident pixels; the loss line gains
` q = <min>..<max>`.  --train-state refuses a resume with the flag added, dropped or changed.
--online-source (needs --online-labels): the published DACS step -- every optimiser step also trains, by the plain cross-entropy, on
a labelled SOURCE batch: --data-dir / --data-list (GTA5: `images/<name>`, `labels/<name>`, ids mapped to train ids; simt_amd/dataset/gta5_dataset.py)
through a second loader at --input-size-target with a seed of its own derived from --random-seed; it honours --random-mirror and --scale-crop, none of
the target-side augmentations, and is not cached.  With --online-mix the mix is the cross-domain one: half of the classes of source image i are
pasted, image and ground truth, onto target image i (simt_source_mix); with --online-labels-weighted a pasted pixel has weight 1.  The loss line
gains ` src = <loss_seg2 of the source pass>`; --train-state resumes both loaders at the same batch and refuses the flag added or dropped.
--rare-class-sampling [T] (needs --online-source and --rcs-stats FILE): DAFormer's sampler for the source batch -- a class is drawn
with probability softmax((1 - f) / T) of the class frequencies (no value: T = 0.01), then a frame with at least --rcs-min-pixels N (3000) pixels of
it; FILE comes from `python -m simt_amd.tools.compute_class_stats`.  With --scale-crop --rcs-crops K (10) candidate windows are drawn per item and
the first that shows more than floor(N * --rcs-min-crop-ratio R (0.5)) pixels of the class is taken, the last when none does: counted, picked and
cropped on the copy stream, nothing read back; the loss line gains ` rcs = <share of the source items whose window met the bar>`.  One start-up
line gives the class probabilities and the frames per class.  --train-state refuses the flag added, dropped or changed.
--feat-dist [LAMBDA] --feat-dist-from FILE [--feat-dist-classes C ...] [--feat-dist-min-ratio R] (--model DeepLab; with --online-labels it needs
--online-source): DAFormer's thing-class ImageNet feature distance -- the pass with ground-truth labels adds LAMBDA (no value: 0.005)
times the mean L2 distance between the model's layer-4 features and those of a frozen ImageNet trunk (FILE: a torchvision resnet101 state dict or a
file in DeeplabMulti's keys) over the feature cells a thing class fills to R (0.75) of their label window; mask, distance and gradient are three
launches on the device, the ImageNet forward runs beside the model's.  The loss line gains ` fd = <feat_dist> (<cells>)`; one start-up line names the
file, the classes and the memory of the second trunk.  --train-state refuses the flag added, dropped or changed, or another FILE.
--fda [BETA] (needs --online-source, --batch-size <= 32): Fourier Domain Adaptation (Yang & Soatto, CVPR'20) of the source batch, a
stage between the two loaders and the trainer's step -- the amplitude of the (2b+1)^2 lowest frequencies of source image i,
b = floor(min(h, w) * BETA) (no value: BETA = 0.01; b <= 64), is replaced by that of the same step's target image i (the weak view where the loader
hands one out), the phase and the labels stay: four launches on the device (simt_fda_transfer), no FFT, no random draw.  It applies to --synthetic
source batches too.  One start-up line gives BETA, b and the band; --train-state refuses the flag added, dropped or changed.
--entropy-min [LAMBDA] (needs --online-labels): FDA's robust entropy term on the TARGET pass, inside the fused head -- every pixel,
labelled or not, adds LAMBDA (no value: 0.005) * (e^2 + 1e-8)^ETA / (B H W), e its softmax entropy / ln(C); --entropy-eta ETA (2.0: FDA's
Charbonnier penalty; 0.5: ADVENT's MinEnt) and --entropy-after N (0: FDA's switch2entropy -- the term is on from iteration N).  From iteration N on
the loss line gains ` ent = <the main head's mean penalty>`; before it the line is the one without the flag.  One start-up line states the term
and its departures; --train-state refuses the flags added, dropped or changed.
--uncertainty-rectify [LAMBDA_KL] (--model DeepLab only): Zheng & Yang's rectification of noisy pseudo labels, inside the fused head --
at every pixel D_k, the KL divergence of head k from the other head, is the label's uncertainty: the cross-entropy is multiplied by exp(-D_k) and
LAMBDA_KL (no value: 1.0; 0 is allowed) * the mean D_k is added, for both heads.  It applies to every pass whose labels are not ground truth: the
list's pseudo labels, the teacher's labels of --online-labels, and with --online-source the target pass only.  The loss line gains
` unc = <the main head's mean KL> x<its mean weight exp(-D)>`; one start-up line states the rule and its departures; not beside --entropy-min;
--train-state refuses the flag added, dropped or changed.
--proto-denoise [TEMP] (needs --online-labels): ProDA's prototype weights -- in front of the label launch of every mode the teacher's
low-res posterior is weighed by softmax(-(d - d_min) / TEMP) (no value: 1.0), d the distance of the cell's feature (the input of the teacher's
main classifier) to running class prototypes kept on the device, momentum --proto-momentum M (0.9999).  A batch is labelled with the
prototypes of the batches before it; the first one with the teacher's output as it is.  The loss line gains ` proto = <seen>/<C> moved <share>`.
One start-up line states the rule and its departures; --train-state refuses the flags added, dropped or changed.  All three models.
--proto-contrast [LAMBDA] (needs --proto-denoise, not with --feat-dist, --model DeepLab only): the prototype contrastive term of
SePiCo / ProDA -- every pass adds LAMBDA (no value: 0.1) * the mean over the valid layer-4 cells of -log softmax_seen(cos(f, prototype_c) / T)[y], f
the STUDENT's layer-4 feature, the prototypes --proto-denoise's, y the class that fills --proto-contrast-min-ratio R (0.75) of the cell's window of
the pass's labels, T = --proto-contrast-temp (0.1); its gradient enters the backward at layer 4's output.  The loss line gains
` pc = <value> (<cells>)`.  --proto-denoise 1e30 leaves the labels all but untouched for a run that wants the contrast alone.

--model: DeepLab (the reference's DeeplabMulti, `WarmupTrainer`), DeepLabv3 (model/deeplabv3.py, trunk depth --v3-layers) or DeepLabVGG
(model/deeplab_vgg.py); the last two run `WarmupSingleTrainer` (simt_amd/step_single.py), the same loss on the model's one output, and
write the checkpoint `trainV2_simt --model DeepLabv3 | DeepLabVGG --restore-from` starts from.  Their --restore-from also takes the
torchvision ImageNet files the reference builds them from (resnet50 / resnet101, vgg16: simt_amd/pretrained.py).

    python -m simt_amd.tools.trainV1_warmup --learning-rate 2.5e-4 --input-size-target 1024,512 --num-steps-stop 40000
    python -m simt_amd.tools.trainV1_warmup --model DeepLabv3 --restore-from resnet50-imagenet.pth --snapshot-dir ../snapshots/v3/
"""
import argparse
import os
import os.path as osp
import time

import torch

from simt_amd import model_spec as ms
from simt_amd.step import Hyper, WarmupTrainer
from simt_amd.tools.train_loop import scorer, setup_devices, train
from simt_amd.tools.trainV2_simt import (ENGINE_MODEL, MODELS, add_cache_args, add_class_mix_args,
                                          add_ema_args, add_online_label_args, add_optimizer_args, add_patch_mask_args, add_photometric_args, add_scale_crop_args,
                                          add_train_state_args, add_v3_layers, batches, check_online_label_args, check_patch_mask_args,
                                          model_lr, online_label_line, optimizer_kwargs, optimizer_line, patch_mask_line, restore, save_atomic,
                                          single_model_state, source_batches)      # (save_atomic: for those who import it from here)


def get_arguments(argv=None):
    """Every flag of the reference (trainV1_warmup.py:60-150), same names / types / defaults; the ones the reference parses and never
    reads (--target, --data-dir and --data-list without --online-source, --ignore-label, --input-size, --is-training, --learning-rate-T, --not-restore-last,
    --open-classes, --random-scale, --set, --log-dir) are parsed and ignored here too.  --model picks the network (check_model)."""
    p = argparse.ArgumentParser(description="DeepLab-ResNet warm-up on MI355X")
    p.add_argument("--model", type=str, default="DeepLab")
    p.add_argument("--target", type=str, default="cityscapes")
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--iter-size", type=int, default=1)
    p.add_argument("--num-workers", type=int, default=4)
    p.add_argument("--data-dir", type=str, default="")
    p.add_argument("--data-list", type=str, default="../dataset/gta5_list/train.txt")
    p.add_argument("--ignore-label", type=int, default=255)
    p.add_argument("--input-size", type=str, default="1024,512")
    p.add_argument("--data-dir-target", type=str, default="")
    p.add_argument("--data-list-target", type=str, default="../dataset/cityscapes_list/pseudo_bapa.lst")
    p.add_argument("--input-size-target", type=str, default="1024,512")
    p.add_argument("--is-training", action="store_true")
    p.add_argument("--learning-rate", type=float, default=2.5e-4)
    p.add_argument("--learning-rate-T", type=float, default=2.5e-4)
    p.add_argument("--lambda-seg", type=float, default=0.1)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--not-restore-last", action="store_true")
    p.add_argument("--num-classes", type=int, default=19)
    p.add_argument("--open-classes", type=int, default=15)
    p.add_argument("--num-steps", type=int, default=250000)
    p.add_argument("--num-steps-stop", type=int, default=40000)
    p.add_argument("--power", type=float, default=0.9)
    p.add_argument("--random-mirror", action="store_true")
    p.add_argument("--random-scale", action="store_true")
    p.add_argument("--random-seed", type=int, default=1234)
    p.add_argument("--restore-from", type=str, default="../snapshots/resnet_pretrain.pth")
    p.add_argument("--save-pred-every", type=int, default=1000)
    p.add_argument("--snapshot-dir", type=str, default="../snapshots/")
    p.add_argument("--weight-decay", type=float, default=0.0005)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--set", type=str, default="train")
    p.add_argument("--log-dir", type=str, default="./log/")
    # additions (all optional)
    p.add_argument("--compute-dtype", choices=["bf16", "f32"], default="bf16")
    p.add_argument("--eval-dtype", choices=["f32", "bf16"], default="f32",
                   help="arithmetic of the periodic evaluation: fp32 like the reference (evaluate_cityscapes.py:96-162); bf16 is a labelled opt-in")
    p.add_argument("--print-every", type=int, default=100)
    p.add_argument("--synthetic", action="store_true", help="synthetic Cityscapes-shaped batches")
    p.add_argument("--from-scratch", action="store_true", help="allow training from the constructor init (no --restore-from)")
    p.add_argument("--data-dir-val", type=str, default="", help="Cityscapes root for the in-loop evaluation (evaluate_cityscapes.py:26)")
    p.add_argument("--data-list-val", type=str, default="../dataset/cityscapes_list/val.txt")
    p.add_argument("--gt-dir-val", type=str, default="", help="directory of *_gtFine_labelIds.png (evaluate_cityscapes.py:140)")
    p.add_argument("--devkit-dir", type=str, default="../dataset/cityscapes_list")
    add_v3_layers(p)
    add_cache_args(p)
    add_scale_crop_args(p)
    add_class_mix_args(p)
    add_photometric_args(p)
    add_patch_mask_args(p)
    add_train_state_args(p)
    add_ema_args(p)
    add_online_label_args(p)
    add_feat_dist_args(p)
    add_optimizer_args(p)
    add_fda_args(p)
    add_entropy_args(p)
    add_uncertainty_args(p)
    add_proto_args(p)
    add_proto_contrast_args(p)
    args = p.parse_args(argv)
    check_patch_mask_args(p, args)
    check_online_label_args(p, args)
    check_feat_dist_args(p, args)
    check_fda_args(p, args)
    check_entropy_args(p, args)
    check_uncertainty_args(p, args)
    check_proto_args(p, args)
    check_proto_contrast_args(p, args)
    optimizer_kwargs(p, args)
    return args


def _feat_dist_lambda(text):
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v < float("inf"):             # (a NaN fails both comparisons)
        raise argparse.ArgumentTypeError(f"{text!r}: expected the weight of the feature distance, a finite LAMBDA >= 0")
    return v


def _feat_dist_ratio(text):
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.5 < v <= 1.0:
        raise argparse.ArgumentTypeError(f"{text!r}: expected the share of a cell's label window one thing class must fill, 0.5 < R <= 1")
    return v


def add_feat_dist_args(p):
    """--feat-dist / --feat-dist-from / --feat-dist-classes / --feat-dist-min-ratio; `check_feat_dist_args` holds their refusals."""
    from simt_amd.feat_dist import DEFAULT_CLASSES, DEFAULT_LAMBDA, DEFAULT_MIN_RATIO
    p.add_argument("--feat-dist", type=_feat_dist_lambda, nargs="?", const=DEFAULT_LAMBDA, default=None, metavar="LAMBDA",
                   help="DAFormer's thing-class ImageNet feature distance (simt_amd/feat_dist.py; DESIGN 7.22): the pass with ground-truth labels "
                        "(the source pass of --online-source; without --online-labels the only pass) adds LAMBDA * the mean L2 distance between "
                        "the model's layer-4 features and those of a frozen ImageNet trunk (--feat-dist-from), over the feature cells a thing "
                        f"class fills (no value: LAMBDA = {DEFAULT_LAMBDA}).  --model DeepLab only; with --online-labels it needs --online-source.  "
                        "Default: off")
    p.add_argument("--feat-dist-from", type=str, default=None, metavar="FILE",
                   help="with --feat-dist (required): the ImageNet weights of the frozen trunk -- a torchvision resnet101 state dict (fc.* dropped) "
                        "or any file in DeeplabMulti's keys (head keys dropped); simt_amd/pretrained.py")
    p.add_argument("--feat-dist-classes", type=int, nargs="+", default=None, metavar="C",
                   help=f"with --feat-dist: the thing classes.  Default with 19 classes: {' '.join(map(str, DEFAULT_CLASSES))}")
    p.add_argument("--feat-dist-min-ratio", type=_feat_dist_ratio, default=None, metavar="R",
                   help=f"with --feat-dist: a cell is kept when one thing class fills at least R of its label window (0.5 < R <= 1).  Default: {DEFAULT_MIN_RATIO}")


def check_feat_dist_args(p, args):
    """argparse's error (exit status 2) naming the flag: a --feat-dist-* flag without --feat-dist, --feat-dist without --feat-dist-from, with
    --online-labels but without --online-source (no ground truth for the mask), or with a one-output model."""
    if args.feat_dist is None:
        for flag in ("feat_dist_from", "feat_dist_classes", "feat_dist_min_ratio"):
            if getattr(args, flag) is not None:
                p.error(f"--{flag.replace('_', '-')} needs --feat-dist: it sets the feature distance")
        return
    if args.model != "DeepLab":
        p.error(f"--feat-dist with --model {args.model}: the feature distance is built for --model DeepLab only (DESIGN 7.22, not built: "
                "DeepLabv3 and DeepLabVGG)")
    if not args.feat_dist_from:
        p.error("--feat-dist needs --feat-dist-from FILE: the ImageNet weights of the frozen trunk")
    if args.online_labels is not None and not args.online_source:
        p.error("--feat-dist with --online-labels needs --online-source: the mask is made of ground-truth labels, and a run that trains on a "
                "teacher's labels alone has none")
    from simt_amd.feat_dist import check_feat_dist
    try:
        check_feat_dist(args.feat_dist, {"file": args.feat_dist_from}, args.feat_dist_classes, args.feat_dist_min_ratio, args.online_labels,
                        args.online_source, args.num_classes)
    except ValueError as e:
        p.error(str(e))


def feat_dist_kwargs(args, shapes, rank=0):
    """The trainer's keywords of --feat-dist (none without it): the file is read, mapped and checked (simt_amd.pretrained.imagenet_trunk);
    rank 0 prints the start-up line."""
    if getattr(args, "feat_dist", None) is None:
        return {}
    from simt_amd.feat_dist import DEFAULT_CLASSES, DEFAULT_MIN_RATIO
    from simt_amd.pretrained import imagenet_trunk
    if not osp.exists(args.feat_dist_from):
        raise SystemExit(f"--feat-dist-from {args.feat_dist_from!r}: no such file")
    saved = torch.load(args.feat_dist_from, map_location="cpu")
    try:
        layout, trunk = imagenet_trunk(saved, shapes)
    except ValueError as e:
        raise SystemExit(f"--feat-dist-from {args.feat_dist_from!r}: {e}")
    classes = list(DEFAULT_CLASSES) if args.feat_dist_classes is None else sorted(args.feat_dist_classes)
    ratio = DEFAULT_MIN_RATIO if args.feat_dist_min_ratio is None else args.feat_dist_min_ratio
    if rank == 0:
        mb = sum(v.numel() * 4 for v in trunk.values() if v.dtype != torch.long) / 2 ** 20
        print(f"feature distance: lambda {args.feat_dist} over the layer-4 cells one of the classes {' '.join(map(str, classes))} fills to {ratio}; "
              f"the frozen trunk is {args.feat_dist_from} ({layout} layout, {len(trunk)} tensors), {mb:.0f} MB of fp32 masters beside the model's "
              "(plus its packed operands and eval-mode activations)")
    return dict(feat_dist=args.feat_dist, feat_dist_state=trunk, feat_dist_classes=args.feat_dist_classes, feat_dist_min_ratio=args.feat_dist_min_ratio)


def feat_dist_text(args, l):
    """` fd = <feat_dist> (<cells>)` of the loss line: only with --feat-dist."""
    if getattr(args, "feat_dist", None) is None:
        return ""
    return " fd = {0:.4f} ({1:d})".format(l["feat_dist"], l["feat_dist_cells"])


def add_fda_args(p):
    """--fda; `check_fda_args` holds its refusals."""
    from simt_amd.data.fda import DEFAULT_BETA
    p.add_argument("--fda", nargs="?", const=DEFAULT_BETA, default=None, metavar="BETA",
                   help="with --online-source: Fourier Domain Adaptation of the source batch on the device (simt_amd/data/fda.py; DESIGN 7.24) -- "
                        "the amplitude of the (2b+1)^2 lowest frequencies of source image i, b = floor(min(h, w) * BETA), is replaced by that of "
                        f"the same step's target image i, the phase and the labels are kept (no value: BETA = {DEFAULT_BETA}; BETA > 0, 2b + 1 <= min(h, w), "
                        "b <= 64).  Needs --batch-size <= 32.  Default: off")


def check_fda_args(p, args):
    """argparse's error (exit status 2) naming the flag: --fda without --online-source, a BETA outside (0, 1), a band that does not fit the
    crop or the launch, a batch the launch does not take."""
    if args.fda is None:
        return
    if not getattr(args, "online_source", False):
        p.error("--fda needs --online-source: it restyles the labelled source batch after the target batch of the same step")
    from simt_amd.data.fda import MAX_ITEMS, parse
    try:
        parse(args.fda, tuple(map(int, args.input_size_target.split(","))))
    except ValueError as e:
        p.error(str(e))
    if not 1 <= args.batch_size <= MAX_ITEMS:
        p.error(f"--fda with --batch-size {args.batch_size}: one launch takes 1 to {MAX_ITEMS} items")


def fda_transfer(args, B, h, w, dev, rank=0):
    """--fda: -> the FdaTransfer of the loop (None without the flag); rank 0 prints the start-up line."""
    if getattr(args, "fda", None) is None:
        return None
    from simt_amd.data.fda import FdaTransfer
    fda = FdaTransfer(B, h, w, args.fda, dev, hold=max(1, args.iter_size))
    if rank == 0:
        print(f"FDA: beta = {fda.beta}, b = {fda.b}: the amplitudes of the {2 * fda.b + 1} x {2 * fda.b + 1} lowest frequencies of every source "
              f"image are those of the same step's target image ({h}x{w}); the phase and the labels are the source's")
    return fda


def fda_source(fda, mb, sb):
    """The source micro-batches with their images restyled after the target micro-batches beside them: the weak view where the loader hands
    one out, else the image the student sees.  Labels are untouched."""
    return [(fda(s[0], m[0] if m[2] is None else m[2]), s[1]) for m, s in zip(mb, sb)]


def add_entropy_args(p):
    """--entropy-min / --entropy-eta / --entropy-after; `check_entropy_args` holds their refusals."""
    from simt_amd.online_labels import DEFAULT_ENTROPY_ETA, DEFAULT_ENTROPY_LAMBDA
    p.add_argument("--entropy-min", nargs="?", type=float, const=DEFAULT_ENTROPY_LAMBDA, default=None, metavar="LAMBDA",
                   help="with --online-labels: FDA's robust entropy term on the target pass, in the fused head (simt_head_loss_entropy; DESIGN "
                        f"7.25) -- LAMBDA * mean over ALL pixels of (e^2 + 1e-8)^ETA, e = softmax entropy / ln(C) (no value: LAMBDA = {DEFAULT_ENTROPY_LAMBDA})")
    p.add_argument("--entropy-eta", type=float, default=DEFAULT_ENTROPY_ETA, metavar="ETA",
                   help=f"the exponent of the penalty (default {DEFAULT_ENTROPY_ETA}: FDA's Charbonnier penalty; 0.5: ADVENT's MinEnt up to 1e-4)")
    p.add_argument("--entropy-after", type=int, default=0, metavar="N",
                   help="the first iteration that carries the term (FDA's switch2entropy; default 0: every iteration)")


def check_entropy_args(p, args):
    """argparse's error (exit status 2) naming the flag: --entropy-min without --online-labels, a LAMBDA or ETA that is not finite and > 0, a
    negative N, --entropy-eta / --entropy-after without --entropy-min."""
    from simt_amd.online_labels import check_entropy
    if args.entropy_min is not None and args.online_labels is None:
        p.error("--entropy-min needs --online-labels: the term is a loss on an unlabelled target pass, and without a teacher the only pass "
                "has ground truth")
    try:
        check_entropy(args.entropy_min, args.entropy_eta, args.entropy_after, args.online_labels)
    except ValueError as e:
        msg = str(e)
        for k in ("entropy_min", "entropy_eta", "entropy_after"):      # the keywords' names -> the flags'
            msg = msg.replace(k, "--" + k.replace("_", "-"))
        p.error(msg)


def entropy_kwargs(args):
    """The trainers' keywords of --entropy-min / --entropy-eta / --entropy-after: nothing without the flag."""
    if getattr(args, "entropy_min", None) is None:
        return {}
    return {"entropy_min": args.entropy_min, "entropy_eta": args.entropy_eta, "entropy_after": args.entropy_after}


def entropy_line(args):
    """The start-up line of --entropy-min: the term and its departures from FDA's code."""
    if getattr(args, "entropy_min", None) is None:
        return
    when = "every iteration" if args.entropy_after == 0 else f"iteration {args.entropy_after} on"
    print(f"entropy term: lambda {args.entropy_min} * mean of (e^2 + 1e-8)^{args.entropy_eta} over the target pass, e = entropy / ln({args.num_classes}), "
          f"from {when}, inside the fused head; departures: EVERY pixel counts (unlabelled and pasted source pixels included), eps = 1e-8 on the "
          "normalised entropy, one lambda for both heads (the auxiliary head's share times --lambda-seg), no multi-band ensemble")


def entropy_text(l):
    """` ent = <hout[3]>` of the loss line: only at iterations that carry the term (losses() has `entropy2` exactly then)."""
    return " ent = {0:.3f}".format(l["entropy2"]) if "entropy2" in l else ""


def add_proto_args(p):
    """--proto-denoise / --proto-momentum; `check_proto_args` holds their refusals."""
    from simt_amd.proto import DEFAULT_MOMENTUM, DEFAULT_TEMP
    p.add_argument("--proto-denoise", nargs="?", type=float, const=DEFAULT_TEMP, default=None, metavar="TEMP",
                   help="with --online-labels: ProDA's prototype weights on the teacher's posterior, in front of the label launch (simt_proto_rectify / "
                        f"_accumulate / _update; DESIGN 7.26) -- softmax(-(d - d_min) / TEMP) over the distances to running class prototypes (no value: TEMP = {DEFAULT_TEMP})")
    p.add_argument("--proto-momentum", type=float, default=None, metavar="M",
                   help=f"the prototypes' momentum, 0 <= M < 1 (default {DEFAULT_MOMENTUM}: ProDA's)")


def check_proto_args(p, args):
    """argparse's error (exit status 2) naming the flag: --proto-denoise without --online-labels, a TEMP that is not finite and > 0, an M outside
    [0, 1), --proto-momentum without --proto-denoise."""
    from simt_amd.proto import check_proto
    if args.proto_denoise is not None and args.online_labels is None:
        p.error("--proto-denoise needs --online-labels: it weighs the teacher's posterior, and without the flag there is no teacher")
    try:
        check_proto(args.proto_denoise, args.proto_momentum, args.online_labels, args.num_classes)
    except ValueError as e:
        msg = str(e)
        for k in ("proto_denoise", "proto_momentum"):      # the keywords' names -> the flags'
            msg = msg.replace(k, "--" + k.replace("_", "-"))
        p.error(msg)


def proto_kwargs(args):
    """The trainers' keywords of --proto-denoise / --proto-momentum: nothing without the flag."""
    if getattr(args, "proto_denoise", None) is None:
        return {}
    from simt_amd.proto import DEFAULT_MOMENTUM
    return {"proto_denoise": args.proto_denoise, "proto_momentum": DEFAULT_MOMENTUM if args.proto_momentum is None else args.proto_momentum}


def proto_line(args):
    """The start-up line of --proto-denoise: the rule and its departures from ProDA's code."""
    if getattr(args, "proto_denoise", None) is None:
        return
    kw = proto_kwargs(args)
    print(f"prototype weights: the teacher's posterior times softmax(-(d - d_min) / {kw['proto_denoise']}), d = the distance of the classifier-input "
          f"feature to {args.num_classes} running class prototypes (momentum {kw['proto_momentum']}), then the label rule at --online-labels; "
          "departures: the prototypes start from the first labelled batch (no dataset pass), the features are the classifier's input (no 256-d "
          "bottleneck), no symmetric cross-entropy, no source features, prototypes per rank")


def proto_text(args, l):
    """` proto = <seen>/<C> moved <share>` of the loss line: only with --proto-denoise (losses() has `proto_seen` exactly then)."""
    return " proto = {0}/{1} moved {2:.4f}".format(l["proto_seen"], args.num_classes, l["proto_changed"]) if "proto_seen" in l else ""


def add_proto_contrast_args(p):
    """--proto-contrast / --proto-contrast-temp / --proto-contrast-min-ratio; `check_proto_contrast_args` holds their refusals."""
    from simt_amd.proto_contrast import DEFAULT_LAMBDA, DEFAULT_MIN_RATIO, DEFAULT_TEMP
    p.add_argument("--proto-contrast", nargs="?", type=float, const=DEFAULT_LAMBDA, default=None, metavar="LAMBDA",
                   help="with --proto-denoise: the prototype contrastive term of SePiCo / ProDA on the student's layer-4 features (simt_cell_labels / "
                        "simt_proto_contrast_prep / simt_proto_contrast / _finalize; DESIGN 7.27) -- every pass adds LAMBDA * the mean over the valid cells "
                        f"of -log softmax_seen(cos(f, prototype_c) / T)[y] (no value: LAMBDA = {DEFAULT_LAMBDA}); --model DeepLab only")
    p.add_argument("--proto-contrast-temp", type=float, default=None, metavar="T",
                   help=f"the temperature of the cosine logits, a finite T > 0 (default {DEFAULT_TEMP})")
    p.add_argument("--proto-contrast-min-ratio", type=float, default=None, metavar="R",
                   help=f"a cell takes the class that fills at least R of its label window, 0.5 < R <= 1 (default {DEFAULT_MIN_RATIO})")


def check_proto_contrast_args(p, args):
    """argparse's error (exit status 2) naming the flag: a --proto-contrast-* flag without --proto-contrast, --proto-contrast without
    --proto-denoise, beside --feat-dist, with a one-output model, or with a value its keyword refuses."""
    from simt_amd.proto_contrast import check_proto_contrast
    if args.proto_contrast is not None and args.model != "DeepLab":
        p.error(f"--proto-contrast with --model {args.model}: the term seeds the backward at layer 4's output, which is built for --model DeepLab "
                "only (DESIGN 7.27, not built: DeepLabv3 and DeepLabVGG)")
    if args.proto_contrast is not None and args.proto_denoise is None:
        p.error("--proto-contrast needs --proto-denoise: the prototypes are --proto-denoise's (--proto-denoise 1e30 leaves the labels all but untouched)")
    try:
        check_proto_contrast(args.proto_contrast, args.proto_contrast_temp, args.proto_contrast_min_ratio, args.proto_denoise, args.feat_dist,
                             args.num_classes)
    except ValueError as e:
        msg = str(e)
        for k in ("proto_contrast_min_ratio", "proto_contrast_temp", "proto_contrast", "proto_denoise", "feat_dist"):      # the keywords' names -> the flags'
            msg = msg.replace(k, "--" + k.replace("_", "-"))          # (longest names first: a replaced name no longer has an underscore)
        p.error(msg)


def proto_contrast_kwargs(args):
    """The trainer's keywords of --proto-contrast and its two flags: nothing without the flag."""
    if getattr(args, "proto_contrast", None) is None:
        return {}
    from simt_amd.proto_contrast import DEFAULT_MIN_RATIO, DEFAULT_TEMP
    return {"proto_contrast": args.proto_contrast,
            "proto_contrast_temp": DEFAULT_TEMP if args.proto_contrast_temp is None else args.proto_contrast_temp,
            "proto_contrast_min_ratio": DEFAULT_MIN_RATIO if args.proto_contrast_min_ratio is None else args.proto_contrast_min_ratio}


def proto_contrast_line(args):
    """The start-up line of --proto-contrast: the term and its departures from the published methods."""
    if getattr(args, "proto_contrast", None) is None:
        return
    kw = proto_contrast_kwargs(args)
    print(f"prototype contrast: every pass adds {kw['proto_contrast']} * the mean over the valid layer-4 cells of -log softmax_seen(cos(f, prototype_c) / "
          f"{kw['proto_contrast_temp']})[y], y the class that fills {kw['proto_contrast_min_ratio']} of the cell's label window; departures: cosine "
          "logits, prototypes from the teacher's features of thresholded cells, no distribution (variance) term, lambda and T are conventional "
          "InfoNCE values and not checked against SePiCo's published configuration")


def proto_contrast_text(args, l):
    """` pc = <proto_contrast> (<cells>)` of the loss line: only with --proto-contrast."""
    if getattr(args, "proto_contrast", None) is None:
        return ""
    return " pc = {0:.4f} ({1:d})".format(l["proto_contrast"], l["proto_contrast_cells"])


def add_uncertainty_args(p):
    """--uncertainty-rectify; `check_uncertainty_args` holds its refusals."""
    p.add_argument("--uncertainty-rectify", nargs="?", type=float, const=1.0, default=None, metavar="LAMBDA_KL",
                   help="--model DeepLab only: Zheng & Yang's rectification of noisy pseudo labels, in the fused head (simt_head_loss_uncertain; "
                        "DESIGN 7.28) -- a pixel's cross-entropy times exp(-KL between the two heads), plus LAMBDA_KL * the mean KL (no value: 1.0; "
                        "0: the rectified cross-entropy alone)")


def check_uncertainty_args(p, args):
    """argparse's error (exit status 2) naming the flag: a model with one head, a LAMBDA_KL that is not finite and >= 0, --entropy-min beside it."""
    from simt_amd.online_labels import check_uncertainty
    if args.uncertainty_rectify is None:
        return
    if args.model != "DeepLab":
        p.error(f"--uncertainty-rectify needs --model DeepLab: the uncertainty is the KL divergence between its two classifier heads, and "
                f"{args.model} has one")
    try:
        check_uncertainty(args.uncertainty_rectify, args.entropy_min)
    except ValueError as e:
        p.error(str(e).replace("uncertainty_rectify", "--uncertainty-rectify").replace("entropy_min", "--entropy-min"))


def uncertainty_kwargs(args):
    """The trainer's keyword of --uncertainty-rectify: nothing without the flag."""
    if getattr(args, "uncertainty_rectify", None) is None:
        return {}
    return {"uncertainty_rectify": args.uncertainty_rectify}


def uncertainty_line(args):
    """The start-up line of --uncertainty-rectify: the rule and its departures from the published method."""
    if getattr(args, "uncertainty_rectify", None) is None:
        return
    where = "the target pass" if getattr(args, "online_source", False) else "every pass"
    print(f"uncertainty rectification: cross-entropy * exp(-KL between the two heads) + {args.uncertainty_rectify} * mean KL on {where}, both heads, "
          "the gradient through both arguments, inside the fused head; departures: the cross-entropy keeps its division by the labelled pixels "
          "(the paper: both means over all pixels), one --lambda-seg for both of the auxiliary head's terms, no class weights")


def uncertainty_text(l):
    """` unc = <K_2> x<rectify2>` of the loss line (losses() has `uncertainty2` exactly with the flag)."""
    return " unc = {0:.3f} x{1:.3f}".format(l["uncertainty2"], l["rectify2"]) if "uncertainty2" in l else ""


def step_args(args, mb, sb=None):
    """The micro-batches `batches` handed out -> the arguments of the trainer's step(): (image, label), with --online-labels
    (image, None) and the keyword teacher_image where the loader made a weak view; sb: the micro-batches of `source_batches`
    (--online-source) -> the keywords source_image / source_label."""
    one = args.iter_size == 1
    img = mb[0][0] if one else [m[0] for m in mb]
    if args.online_labels is None:
        return (img, mb[0][1] if one else [m[1] for m in mb]), {}
    kw = {}
    if sb is not None:
        kw.update(source_image=sb[0][0] if one else [m[0] for m in sb], source_label=sb[0][1] if one else [m[1] for m in sb])
    if mb[0][2] is None:
        return (img, None), kw
    kw["teacher_image"] = mb[0][2] if one else [m[2] for m in mb]
    return (img, None), kw


def labelled_text(args, l):
    """` labelled = 0.xxx` of the loss line: only with --online-labels."""
    return " labelled = {0:.3f}".format(l["labelled"]) if args.online_labels is not None else ""


def thresholds_text(args, l):
    """` thr = <min>..<max>` of the loss line, the lowest and the highest per-class threshold: only with --online-labels-balanced."""
    if getattr(args, "online_labels_balanced", None) is None:
        return ""
    return " thr = {0:.3f}..{1:.3f}".format(min(l["label_thresholds"]), max(l["label_thresholds"]))


def quality_text(args, l):
    """` q = <min>..<max>` of the loss line, the lowest and the highest weight of the last micro-batch: only with --online-labels-weighted."""
    if getattr(args, "online_labels_weighted", None) is None:
        return ""
    return " q = {0:.3f}..{1:.3f}".format(min(l["label_quality"]), max(l["label_quality"]))


def source_text(args, l):
    """` src = <loss_seg2 of the source pass>` of the loss line: only with --online-source."""
    return " src = {0:.3f}".format(l["source_seg2"]) if getattr(args, "online_source", False) else ""


def rcs_text(source):
    """` rcs = <share>` of the loss line, the share of the source items since the last line whose chosen window met the bar: only with
    --rare-class-sampling and --scale-crop (read behind tr.losses(), which has synchronised)."""
    share = source.rcs_share() if hasattr(source, "rcs_share") else None
    return "" if share is None else " rcs = {0:.3f}".format(share)


def balanced_kwargs(args):
    """The trainers' keywords of --online-labels-balanced / --online-labels-momentum, and of --online-mix (seeded by --random-seed),
    --online-labels-weighted and --online-source when on."""
    kw = {"online_labels_balanced": args.online_labels_balanced, "online_labels_momentum": args.online_labels_momentum}
    if args.online_mix is not None:
        kw.update(online_mix=args.online_mix, online_mix_seed=args.random_seed)
    if getattr(args, "online_labels_weighted", None) is not None:
        kw.update(online_labels_weighted=args.online_labels_weighted)
    if getattr(args, "online_source", False):
        kw.update(online_source=True)
    return kw


def check_model(args):
    """--model names one of trainV2_simt.MODELS (as trainV2_simt.check_model_args checks it); --iter-size works for all three."""
    if args.model not in MODELS:
        raise SystemExit(f"--model {args.model!r}: expected one of {', '.join(MODELS)}")


def restore_single(state, path, model, required):
    """--restore-from of the one-output warm-up: a checkpoint in the module's keys, or a torchvision ImageNet file mapped onto them
    (simt_amd.pretrained.checkpoint_layout); then the key / shape filter of trainV2_simt.restore.  -> (tensors loaded, layout name)."""
    from simt_amd.pretrained import checkpoint_layout
    seen = []

    def remap(saved):
        layout, mapped = checkpoint_layout(saved, model)
        seen.append(layout)
        return mapped
    n = restore(state, path, required=required, remap=remap)
    return n, (seen[0] if seen else "no file")


def build_trainer(args, h, w, rank, dev, pg):
    """What --model decides: the state and its restore, the trainer (WarmupTrainer | WarmupSingleTrainer, the flags' keywords composed once for
    both), the head of the start-up `restored` line, the model's own part of the loss line (a format of losses()) and the Evaluator's
    model= / layers=.  -> (trainer, restored text, loss format, evaluator keywords)."""
    C, required = args.num_classes, not (args.synthetic or args.from_scratch)
    hyper = dict(num_classes=C, open_classes=0, lr=args.learning_rate, iter_size=args.iter_size, momentum=args.momentum,
                 weight_decay=args.weight_decay, power=args.power, num_steps=args.num_steps)
    kw = dict(dtype=torch.bfloat16 if args.compute_dtype == "bf16" else torch.float32, device=dev, process_group=pg, ema_decay=args.ema,
              online_labels=args.online_labels, online_labels_every=args.online_labels_every,
              **balanced_kwargs(args), **args.optimizer_kwargs, **entropy_kwargs(args), **proto_kwargs(args))
    if args.model == "DeepLab":
        shapes = ms.state_shapes(C, 0, False)
        state = ms.reference_init(shapes, seed=args.random_seed)
        # trainV1_warmup.py:177: keys of the pretrained checkpoint carry a 6-character prefix (`k[6:]`); shapes are filtered
        n = restore(state, args.restore_from, strip_prefix=6, required=required)
        tr = WarmupTrainer(state, Hyper(lambda_seg=args.lambda_seg, **hyper), args.batch_size, h, w, **kw, **feat_dist_kwargs(args, shapes, rank),
                           **proto_contrast_kwargs(args), **uncertainty_kwargs(args))
        return tr, f"restored {n} tensors", "loss_seg1 = {loss_seg1:.3f} loss_seg2 = {loss_seg2:.3f}", {}
    from simt_amd.step_single import WarmupSingleTrainer
    model, layers = ENGINE_MODEL[args.model], tuple(args.v3_layers)
    state = single_model_state(args.model, C, layers, seed=args.random_seed)
    n, layout = restore_single(state, args.restore_from, model, required=required)
    tr = WarmupSingleTrainer(model, state, Hyper(**hyper), args.batch_size, h, w, arch={"layers": layers} if model == "v3" else None, **kw)
    return (tr, f"{args.model}: restored {n} tensors ({layout} layout) from {args.restore_from}", "loss_seg = {loss_seg:.3f}",
            dict(model=model, layers=layers if model == "v3" else None))


def loss_tail(args, l, source):
    """What the flags add to the loss line behind the model's own losses, in this order; each term is "" without its flag."""
    return (labelled_text(args, l) + thresholds_text(args, l) + quality_text(args, l) + source_text(args, l) + rcs_text(source) +
            feat_dist_text(args, l) + entropy_text(l) + uncertainty_text(l) + proto_text(args, l) + proto_contrast_text(args, l))


def main(argv=None):
    args = get_arguments(argv)
    check_model(args)
    rank, world, dev, pg = setup_devices(args, "trainV1_warmup needs a GPU: no CPU fallback")
    if rank == 0:
        print("Start: " + time.asctime(time.localtime(time.time())))                       # :158
    w, h = map(int, args.input_size_target.split(","))
    tr, restored, losses, eval_kw = build_trainer(args, h, w, rank, dev, pg)
    cd = ms.load_class_dist("bapa")
    if rank == 0:
        optimizer_line(args)
        online_label_line(args)
        entropy_line(args)
        uncertainty_line(args)
        proto_line(args)
        proto_contrast_line(args)
        patch_mask_line(args, frozen=False)
        print(f"{restored}; {world} GPU(s), batch {args.batch_size}/GPU, {h}x{w}, {args.compute_dtype}")
        os.makedirs(args.snapshot_dir, exist_ok=True)                                       # :185-186
    source = None

    def open_data(start_batch):
        nonlocal source
        data = batches(args, args.batch_size, h, w, cd, rank, world, dev, start_batch=start_batch)
        source = source_batches(args, args.batch_size, h, w, cd, rank, world, dev, start_batch=start_batch) if args.online_source else None
        fda = fda_transfer(args, args.batch_size, h, w, dev, rank)

        def next_step():
            mb = [next(data) for _ in range(args.iter_size)]             # gradient accumulation: iter_size micro-batches per step
            sb = [next(source) for _ in range(args.iter_size)] if source is not None else None      # --online-source: a source pair beside each
            if fda is not None:
                sb = fda_source(fda, mb, sb)
            return step_args(args, mb, sb)      # (this module's, looked up at every step)
        return next_step

    def loss_line(i_iter, l, rate):
        return "iter = {0:8d}/{1:8d}, {2}{3}  lr = {4:.2e}  ({5:.1f} img/s)".format(
            i_iter, args.num_steps, losses.format(**l), loss_tail(args, l, source), model_lr(args, i_iter), rate)
    train(args, tr, "GTA5_BAPA_warmup_iter", cd, rank, world, open_data, loss_line, scorer(args, tr, 0, dev, rank, world, pg, **eval_kw))


if __name__ == "__main__":
    main()
