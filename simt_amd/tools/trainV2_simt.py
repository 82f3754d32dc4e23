#!/usr/bin/env python3
"""SimT training stage on MI355X: the reference's tools/trainV2_simt.py with the same command-line flags
(tools/trainV2_simt.py:72-157) driving `SimTTrainer` (simt_amd/step.py) -- the whole iteration body of the reference
(:308-436) runs as HIP kernels; this script is what surrounds it: flags, checkpoint restore by key filter (:248-255), data, the loss line
of every 100 iterations (:438-441), the snapshot and train-state keepers.  The loop itself (step, print, snapshots :447-450, evaluation
:452-464) and the device set-up are simt_amd/tools/train_loop.py's, shared with trainV1_warmup and the same for all three --model values:
`main` builds the trainer of --model (`build_trainer`) and hands the loop its step arguments (`step_args`), loss line and evaluation.

    python -m simt_amd.tools.trainV2_simt --open-classes 15 --learning-rate 6e-4 --learning-rate-T 6e-3 ...
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 8 -m simt_amd.tools.trainV2_simt ...   (data parallel)

Data: `cityscapesPseudo(--data-dir-target, --data-list-target)` through `GpuLoader` (decode on host threads, Pillow-exact resize +
BGR-mean on the GPU, pinned double-buffered uploads; simt_amd/data/pipeline.py), shuffled, --random-mirror as the reference writes
it; `--synthetic` feeds Cityscapes-shaped synthetic batches instead.  Pointing --data-dir-target at a missing directory
without --synthetic is an error (a run that silently trains on noise would still write checkpoints that look like results).
Every --save-pred-every iterations: evaluate_simt on the validation set (--data-dir-val ...) and the best-mIoU snapshot rotation of
trainV2_simt.py:452-464.  Additions over the reference (all optional): --synthetic, --compute-dtype, --eval-dtype (fp32 like the
reference unless bf16 is asked for), --print-every, --data-dir-val,
--data-list-val, --gt-dir-val, --devkit-dir, --class-dist (the prior of other pseudo labels: simt_amd.tools.make_pseudo_labels),
--cache-dataset device [--cache-gb G]: the resized uint8 training set stays in HBM after the first epoch (simt_amd/data/cache.py; default off:
the batches are the same, bit for bit, only PNG decoding after epoch one is saved),
--scale-crop [S ...]: random scale + crop of every training item on the device, one launch per batch (simt_amd/data/scale_crop.py; default
off; --random-scale stays what the reference makes of it: parsed and ignored),
--class-mix [P]: ClassMix of every batch on the device -- with probability P (no value: 1) an item receives the pixels and labels of half
of the classes of its neighbour in the batch (simt_amd/data/class_mix.py; default off; needs --batch-size 2 ... 32, --num-classes <= 32),
--colour-jitter [S] / --gaussian-blur [P]: the photometric half of the strong augmentation, on the finished (mixed) batch on the device:
with probability 0.8 brightness, contrast and saturation factors from [1 - S, 1 + S] and a hue turn from [-S, S] (no value: S = 0.2;
0 < S <= 0.5), then with probability P (no value: 0.5) a Gaussian blur, sigma from [0.15, 1.15] (simt_amd/data/photometric.py; default off;
either flag alone is allowed),
--train-state FILE [--train-state-every N]: resume from FILE if it exists and keep it current (simt_amd/train_state.py).  The snapshots hold
the model only; FILE also holds the SGD momentum, both NTMs and W with their Adam moments, the iteration counter, the snapshot rotation's
bookkeeping (with --ema: the shadow, its update count and the second rotation's too) -- the loader continues at the batch the stopped run would have drawn next, so stopping after step k and re-issuing the same
command line (with a later --num-steps-stop) continues bit for bit as if nothing had happened.  --restore-from stays the same: the frozen
model is not in FILE, its SHA-256 is.  Without the flag the tool writes and prints what it always did.
--ema [D]: keep an exponential moving average of the weights beside the trained ones (simt_amd/ema.py: one launch per step; no value: D = 0.999;
0 <= D < 1).  Training is bit for bit what it is without the flag.  Every evaluation also scores the averaged model (an `EMA mIoU` line) and
a second rotation keeps its best snapshot `GTA5_ema_iter<i>_mIoU<m>.pth` (without a validation set: a rolling `GTA5_ema_iter<i>.pth`); the
stop writes `GTA5_<stop>_ema.pth` beside `GTA5_<stop>.pth` -- same keys, loads wherever the other does.  Default: off.
--ema-teacher [N]: with --ema, the frozen model FOLLOWS the averaged one (simt_amd/ema_teacher.py): behind every N-th EMA update (no value:
N = 1) its weights, BatchNorm affine and running statistics become copies of their shadows and its packed operands are rebuilt -- three to
five launches on the stream of the EMA update, no synchronisation.  Until the first refresh the run is bit for bit the one without the flag;
from then on the confidence labels come from a moving teacher.  --restore-from still names the model the run STARTS beside (its SHA-256 is
what --train-state checks); the state file carries the teacher as it is, N and the refresh count, and refuses a command line that drops the
flag, adds it or changes N.  All three --model values.  Default: off.
--weak-teacher: the frozen model labels the WEAK view.  Needs --class-mix, --colour-jitter or --gaussian-blur (and not
--synthetic, where they do nothing): the loader then also hands out the batch as it was before the mix and the photometric step, the frozen
model's forward runs on that one, and the fused head reads every pixel's frozen posterior from the item the pixel was pasted from (the mix's
item map), so the teacher's predictions are mixed with the same mask as the pixels and the labels.  The student still trains on the strong
view.  Not one loader draw changes; without the flag nothing does.  --train-state refuses a resume with the flag added or dropped.  All
three --model values.  Default: off.
--mask-patches [R] [--mask-patch-size P]: MIC patch masking (Hoyer et al., CVPR'23) -- every P x P patch (default 64) of the
student's image is blanked to the mean colour with probability R (no value: 0.7; 0 < R < 1), behind --class-mix, --colour-jitter and
--gaussian-blur, by one launch per 16 items on the copy stream (simt_amd/data/patch_mask.py); labels stay.  --input-size-target may need at
most 32 x 32 patches.  It satisfies --weak-teacher on its own: the frozen model then labels the whole image and the student predicts those
labels for the blanked regions from their context; without --weak-teacher both models see the masked image (one start-up line says so).
Draws of its own generator: not one other draw changes; --train-state refuses a resume with the flag added, dropped or changed.  Default: off.

--model: DeepLab (the reference's DeeplabMulti, `SimTTrainer`), DeepLabv3 (model/deeplabv3.py, trunk depth --v3-layers) or
DeepLabVGG (model/deeplab_vgg.py); the last two run `SimTSingleTrainer` (simt_amd/step_single.py), the reference's loop with the
auxiliary head removed, and are evaluated and checkpointed like the first (their state dicts load into the nn.Modules of
simt_amd.model).  --iter-size > 1 is implemented for DeepLab only.
"""
import argparse
import os
import os.path as osp

import numpy as np
import torch

from simt_amd import model_spec as ms
from simt_amd.step import Hyper, SimTTrainer, lr_at
from simt_amd.tools.train_loop import scorer, setup_devices, train
from simt_amd.train_state import save_atomic      # (its home; the tools and their users keep importing it from here)


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description="SimT (DeepLab-ResNet) on MI355X")
    p.add_argument("--model", type=str, default="DeepLab", help="DeepLab | DeepLabv3 | DeepLabVGG")
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
    p.add_argument("--Threshold-high", type=float, default=0.8)
    p.add_argument("--Threshold-low", type=float, default=0.2)
    p.add_argument("--lambda-Place", type=float, default=0.1)
    p.add_argument("--lambda-Convex", type=float, default=0.5)
    p.add_argument("--lambda-Volume", type=float, default=0.1)
    p.add_argument("--lambda-Anchor", type=float, default=0.5)
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
    p.add_argument("--snapshot-dir", type=str, default="../snapshots/SimT/")
    p.add_argument("--weight-decay", type=float, default=0.0005)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--set", type=str, default="train")
    p.add_argument("--log-dir", type=str, default="./log/")
    # additions
    p.add_argument("--synthetic", action="store_true", help="synthetic Cityscapes-shaped batches")
    p.add_argument("--compute-dtype", choices=["bf16", "f32"], default="bf16")
    p.add_argument("--eval-dtype", choices=["f32", "bf16"], default="f32",
                   help="arithmetic of the periodic evaluation: fp32 like the reference (evaluate_cityscapes.py:96-162); bf16 is a labelled opt-in")
    p.add_argument("--print-every", type=int, default=100)
    p.add_argument("--data-dir-val", type=str, default="", help="Cityscapes root for the in-loop evaluation (evaluate_cityscapes.py:26)")
    p.add_argument("--data-list-val", type=str, default="../dataset/cityscapes_list/val.txt")
    p.add_argument("--gt-dir-val", type=str, default="", help="directory of *_gtFine_labelIds.png (evaluate_cityscapes.py:140)")
    p.add_argument("--devkit-dir", type=str, default="../dataset/cityscapes_list")
    p.add_argument("--from-scratch", action="store_true", help="allow training from the constructor init (no --restore-from)")
    p.add_argument("--class-dist", type=str, default=None,
                   help="class prior .npy of the pseudo labels (make_pseudo_labels writes it); default: ClassDist_bapa.npy")
    add_v3_layers(p)
    add_cache_args(p)
    add_scale_crop_args(p)
    add_class_mix_args(p)
    add_photometric_args(p)
    add_patch_mask_args(p)
    add_train_state_args(p)
    add_ema_args(p)
    add_ema_teacher_args(p)
    add_optimizer_args(p)
    p.add_argument("--weak-teacher", action="store_true",
                   help="the frozen model sees the batch before --class-mix / --colour-jitter / --gaussian-blur / --mask-patches (needs one of "
                        "them) and its predictions are mixed with the pixels' mask; the student trains on the augmented batch.  Default: off")
    args = p.parse_args(argv)
    check_patch_mask_args(p, args)
    optimizer_kwargs(p, args)
    if args.ema_teacher is not None and args.ema is None:
        p.error("--ema-teacher needs --ema: the frozen model follows the weight EMA")
    if args.weak_teacher and (args.synthetic or (args.class_mix is None and args.colour_jitter is None and args.gaussian_blur is None
                                                 and args.mask_patches is None)):
        p.error("--weak-teacher needs --class-mix, --colour-jitter or --gaussian-blur, or --mask-patches, on real data (with --synthetic "
                "they do nothing): without an augmentation the two views are the same batch")
    return args


MODELS = ("DeepLab", "DeepLabv3", "DeepLabVGG")
ENGINE_MODEL = {"DeepLab": "v2", "DeepLabv3": "v3", "DeepLabVGG": "vgg"}      # --model -> Evaluator / SimTSingleTrainer model name
RESTORE_LAST = {"DeepLab": ("layer5", "layer6"), "DeepLabv3": ("conv.", "conv_1."), "DeepLabVGG": ("classifier.",)}   # --not-restore-last


def add_cache_args(p):
    p.add_argument("--cache-dataset", choices=["off", "device"], default="off",
                   help="device: keep every training item's resized uint8 frame in HBM after its first decode (simt_amd/data/cache.py); "
                        "PNGs are decoded in the first epoch only.  Ignored with --synthetic")
    p.add_argument("--cache-gb", type=float, default=None,
                   help="cache budget in GB (1e9 bytes); default: what holds the whole list at the run's crop (4*h*w bytes per item)")


def add_scale_crop_args(p):
    p.add_argument("--scale-crop", type=str, nargs="*", default=None, metavar="S",
                   help="random scale + crop on the device (simt_amd/data/scale_crop.py): per item a scale is drawn from the decimal choices S "
                        "(no values: 0.5 0.6 ... 1.5; at most 16), the frame is resized once to round(crop * s) and the crop-sized window at a "
                        "uniformly drawn origin goes to the network (mean / label 255 around a smaller frame).  Default: off.  With "
                        "--cache-dataset device the cache then holds the ORIGINAL frames and the default --cache-gb is 4*Hs*Ws bytes per "
                        "item (about 25 GB for the 2 975 Cityscapes training frames).  Ignored with --synthetic")


def scale_crop_choices(args):
    """--scale-crop -> tuple of decimal strings, or None when the flag is off (a bad value is a SystemExit naming it)."""
    texts = getattr(args, "scale_crop", None)
    if texts is None:
        return None
    from simt_amd.data.scale_crop import parse_choices
    try:
        return parse_choices(texts)
    except ValueError as e:
        raise SystemExit(f"--scale-crop: {e}")


def add_class_mix_args(p):
    p.add_argument("--class-mix", type=str, nargs="?", const="1.0", default=None, metavar="P",
                   help="ClassMix on the device (simt_amd/data/class_mix.py): with probability P (no value: 1.0) item i of a batch receives, "
                        "labels included, the pixels of half of the classes (rounded up) found in the label of item (i + 1) %% B; two "
                        "launches per batch on the copy stream.  Needs --batch-size 2 ... 32 and --num-classes <= 32.  Default: off.  "
                        "Ignored with --synthetic")


def class_mix_setting(args):
    """--class-mix -> (n_classes, P), or None when the flag is off (a bad P, batch size or class count is a SystemExit naming it)."""
    value = getattr(args, "class_mix", None)
    if value is None:
        return None
    from simt_amd.data.class_mix import parse
    try:
        return parse(value, args.num_classes, args.batch_size)
    except ValueError as e:
        raise SystemExit(str(e))


def add_photometric_args(p):
    from simt_amd.data.photometric import DEFAULT_BLUR, DEFAULT_JITTER
    p.add_argument("--colour-jitter", type=str, nargs="?", const=DEFAULT_JITTER, default=None, metavar="S",
                   help="colour jitter of every batch on the device (simt_amd/data/photometric.py): with probability 0.8 an item's brightness, "
                        "contrast and saturation are scaled by factors drawn from [1 - S, 1 + S] and its hue is turned by [-S, S] turns (no "
                        "value: S = 0.2; 0 < S <= 0.5), after --class-mix.  Default: off.  Ignored with --synthetic")
    p.add_argument("--gaussian-blur", type=str, nargs="?", const=DEFAULT_BLUR, default=None, metavar="P",
                   help="Gaussian blur of every batch on the device, after the colour jitter: with probability P (no value: 0.5) an item is "
                        "blurred with a sigma drawn from [0.15, 1.15] (radius 5, reflected edges).  Default: off.  Ignored with --synthetic")


def photometric_setting(args):
    """--colour-jitter / --gaussian-blur -> (S | None, P | None), or None when both flags are off (a bad value is a SystemExit naming it)."""
    jitter, blur = getattr(args, "colour_jitter", None), getattr(args, "gaussian_blur", None)
    if jitter is None and blur is None:
        return None
    from simt_amd.data.photometric import parse
    try:
        return parse(jitter, blur)
    except ValueError as e:
        raise SystemExit(str(e))


def add_patch_mask_args(p):
    from simt_amd.data.patch_mask import DEFAULT_PATCH, DEFAULT_RATIO
    p.add_argument("--mask-patches", type=str, nargs="?", const=DEFAULT_RATIO, default=None, metavar="R",
                   help="MIC patch masking on the device (simt_amd/data/patch_mask.py): every patch of the student's image is blanked to the "
                        f"mean colour with probability R (no value: {DEFAULT_RATIO}; 0 < R < 1), after --class-mix, --colour-jitter and "
                        "--gaussian-blur; one launch per 16 items on the copy stream; labels are not touched.  With --weak-teacher the frozen "
                        "model sees the whole image.  Default: off.  Ignored with --synthetic")
    p.add_argument("--mask-patch-size", type=str, default=None, metavar="P",
                   help=f"side of the square patches of --mask-patches in pixels (default: {DEFAULT_PATCH}); --input-size-target may need at "
                        "most 32 patch rows and 32 patch columns")


def check_patch_mask_args(p, args):
    """Both flags against --input-size-target, in get_arguments of both tools: a bad R, P or a crop of more than 32 x 32 patches is
    argparse's error (exit status 2) naming it, and so is --mask-patch-size without --mask-patches."""
    if args.mask_patches is None:
        if args.mask_patch_size is not None:
            p.error("--mask-patch-size needs --mask-patches: it is the patch size of that mask")
        return
    try:
        patch_mask_setting(args)
    except SystemExit as e:
        p.error(str(e))


def patch_mask_setting(args):
    """--mask-patches / --mask-patch-size -> (P, R), or None when the flag is off (a bad value is a SystemExit naming it)."""
    ratio = getattr(args, "mask_patches", None)
    if ratio is None:
        return None
    from simt_amd.data.patch_mask import DEFAULT_PATCH, parse
    patch = getattr(args, "mask_patch_size", None)
    try:
        w, h = map(int, args.input_size_target.split(","))
        return parse(ratio, DEFAULT_PATCH if patch is None else patch, (w, h))[:2]
    except ValueError as e:
        raise SystemExit(str(e))


def add_train_state_args(p):
    p.add_argument("--train-state", type=str, default=None, metavar="FILE",
                   help="resume from FILE if it exists, and keep it current (weights, momentum, NTM / W with their Adam moments, iteration, "
                        "snapshot rotation: simt_amd/train_state.py): written at every snapshot decision (--save-pred-every) and at the stop.  "
                        "Re-issue the same command line until the run is finished")
    p.add_argument("--train-state-every", type=int, default=None, metavar="N",
                   help="write --train-state every N iterations instead of at the snapshot cadence")


def _ema_decay(text):
    from simt_amd.ema import check_decay
    try:
        return check_decay(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_ema_args(p):
    p.add_argument("--ema", type=_ema_decay, nargs="?", const=0.999, default=None, metavar="D",
                   help="keep an exponential moving average of the weights (simt_amd/ema.py): one launch per optimiser step, decay "
                        "min(D, 1 - 1 / (t + 1)) at update t (no value: D = 0.999; 0 <= D < 1).  The trained model is unchanged; the averaged one is "
                        "evaluated beside it (`EMA mIoU`), kept by a rotation of its own (`..._ema_iter...`) and written at the stop as "
                        "GTA5_<stop>_ema.pth.  Default: off")


def add_optimizer_args(p):
    """--optimizer / --adam-betas / --adam-eps / --lr-warmup / --lr-warmup-ratio: both tools, all three models."""
    from simt_amd.optimizer import DEFAULT_BETAS, DEFAULT_EPS, DEFAULT_WARMUP_RATIO, OPTIMIZERS
    p.add_argument("--optimizer", choices=OPTIMIZERS, default="sgd",
                   help="sgd: the reference's optimiser with its duplicate listings.  adamw: torch.optim.AdamW's update in one launch "
                        "(simt_amd/optimizer.py), every tensor listed once, heads at 10x, no weight decay on trained BatchNorm parameters.  "
                        "--learning-rate, --weight-decay and --power keep the reference's defaults: DAFormer trains AdamW with "
                        "--learning-rate 6e-5 --weight-decay 0.01 --power 1.0 --lr-warmup.  Default: sgd")
    p.add_argument("--adam-betas", type=float, nargs=2, default=list(DEFAULT_BETAS), metavar=("B1", "B2"),
                   help=f"with --optimizer adamw: the betas, each in [0, 1).  Default: {DEFAULT_BETAS[0]} {DEFAULT_BETAS[1]}")
    p.add_argument("--adam-eps", type=float, default=DEFAULT_EPS, metavar="E", help=f"with --optimizer adamw: eps > 0.  Default: {DEFAULT_EPS}")
    p.add_argument("--lr-warmup", type=int, nargs="?", const=1500, default=0, metavar="N",
                   help="linear warm-up of the model's learning rate over the first N iterations (simt_amd.step.lr_at; no value: N = 1500, "
                        "DAFormer's): the poly value times a factor rising from --lr-warmup-ratio to 1.  --learning-rate-T is not warmed up.  "
                        "Default: 0 (off)")
    p.add_argument("--lr-warmup-ratio", type=float, default=DEFAULT_WARMUP_RATIO, metavar="R",
                   help=f"with --lr-warmup: the factor at iteration 0, in [0, 1].  Default: {DEFAULT_WARMUP_RATIO}")


def optimizer_kwargs(p, args):
    """The trainers' optimiser keywords from the flags; argparse's error naming the flag that does not fit."""
    from simt_amd.optimizer import check_optimizer
    try:
        check_optimizer(args.optimizer, args.adam_betas, args.adam_eps, args.lr_warmup, args.lr_warmup_ratio)
    except ValueError as e:
        p.error(f"optimiser flags: {e}")
    args.optimizer_kwargs = dict(optimizer=args.optimizer, adam_betas=tuple(args.adam_betas), adam_eps=args.adam_eps, lr_warmup=args.lr_warmup,
                                 lr_warmup_ratio=args.lr_warmup_ratio)


def optimizer_line(args):
    """Said once at start-up, and only when the optimiser or the schedule is not the reference's."""
    if args.optimizer != "sgd":
        print(f"optimiser: {args.optimizer}, betas {args.adam_betas[0]} {args.adam_betas[1]}, eps {args.adam_eps}; every tensor listed once, heads "
              f"at 10x lr, weight decay {args.weight_decay} (none on trained BatchNorm parameters)")
    if args.lr_warmup:
        print(f"learning-rate warm-up: linear over the first {args.lr_warmup} iterations from {args.lr_warmup_ratio} x the poly value")


def model_lr(args, i_iter):
    """The learning rate the trainer gives the model at iteration i_iter, for the loss line: lr_poly itself without --lr-warmup."""
    return lr_at(args.learning_rate, i_iter, args.num_steps, args.power, args.lr_warmup, args.lr_warmup_ratio)


def _teacher_every(text):
    from simt_amd.ema_teacher import check_every
    try:
        return check_every(int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{text!r}: expected an integer >= 1 ({e})")


def add_ema_teacher_args(p):
    p.add_argument("--ema-teacher", type=_teacher_every, nargs="?", const=1, default=None, metavar="N",
                   help="the frozen model follows the weight EMA (simt_amd/ema_teacher.py; needs --ema): behind every N-th EMA update (no value: "
                        "N = 1; an integer >= 1) its tensors become copies of their shadows and its packed operands are rebuilt, on the stream of "
                        "the update.  Bit for bit the run without the flag until the first refresh.  --train-state carries the teacher and refuses "
                        "a run that drops the flag, adds it or changes N.  Default: off")


def _online_threshold(text):
    from simt_amd.online_labels import check_threshold
    try:
        return check_threshold(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _online_every(text):
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: expected an integer >= 1")
    return n


def _online_portion(text):
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 < v <= 1.0:
        raise argparse.ArgumentTypeError(f"{text!r}: expected the share of every class's pixels to keep, 0 < P <= 1")
    return v


def _online_momentum(text):
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError(f"{text!r}: expected the thresholds' momentum, 0 <= M < 1")
    return v


def _online_mix(text):
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 < v <= 1.0:             # (a NaN fails both comparisons)
        raise argparse.ArgumentTypeError(f"{text!r}: expected the probability that an item receives its neighbour's classes, 0 < P <= 1")
    return v


def add_online_label_args(p):
    """--online-labels / --online-labels-every, --online-labels-balanced / --online-labels-momentum (7.17), --online-mix (7.18),
    --online-labels-weighted (7.19), --online-source (7.20) and --rare-class-sampling / --rcs-* (7.21) of trainV1_warmup;
    `check_online_label_args` holds their refusals."""
    from simt_amd.online_labels import DEFAULT_PORTION, DEFAULT_THRESHOLD
    p.add_argument("--online-labels", type=_online_threshold, nargs="?", const=DEFAULT_THRESHOLD, default=None, metavar="T",
                   help="train on a teacher's labels instead of label files (simt_amd/online_labels.py): a frozen copy of the start model "
                        "labels every batch on the device, pixels whose confidence is not above T are ignored (no value: T = "
                        f"{DEFAULT_THRESHOLD}; 0 <= T < 1).  --data-list-target may then list images alone; with --colour-jitter, "
                        "--gaussian-blur or --mask-patches the teacher labels the batch before them.  Not with --class-mix.  Default: off")
    p.add_argument("--online-labels-every", type=_online_every, default=None, metavar="N",
                   help="with --online-labels and --ema: the teacher follows the weight EMA, refreshed behind every N-th update (an integer "
                        ">= 1; simt_amd/ema_teacher.py).  Default: the teacher stays at the start weights")
    p.add_argument("--online-labels-balanced", type=_online_portion, nargs="?", const=DEFAULT_PORTION, default=None, metavar="P",
                   help="with --online-labels: one confidence threshold per class, kept on the device (CBST / IAST).  Each starts at T; every batch "
                        "moves it towards the value that keeps the share P of that class's pixels, never above T (no value: P = "
                        f"{DEFAULT_PORTION}; 0 < P <= 1).  A batch is labelled with the thresholds of the batches before it.  At most 64 classes.  "
                        "Default: the one threshold T")
    p.add_argument("--online-labels-momentum", type=_online_momentum, default=None, metavar="M",
                   help="with --online-labels-balanced: thr <- M * thr + (1 - M) * the batch's threshold (0 <= M < 1).  Default: 0.9")
    p.add_argument("--online-mix", type=_online_mix, nargs="?", const=1.0, default=None, metavar="P",
                   help="with --online-labels: ClassMix by the teacher's labels, inside the trainer (simt_amd/online_labels.py; DESIGN 7.18) -- "
                        "with probability P (no value: 1.0) item i of a batch receives, image and label, the pixels of half of the classes the "
                        "teacher found in item i+1.  Needs --batch-size 2 ... 32 and --num-classes <= 32; the draws are seeded by --random-seed.  "
                        "With --colour-jitter, --gaussian-blur or --mask-patches the teacher labels the weak view and the mix selects from the "
                        "strong views.  Default: off")
    p.add_argument("--online-labels-weighted", choices=["batch", "item"], nargs="?", const="batch", default=None, metavar="MODE",
                   help="with --online-labels: the quality weights of DACS / DAFormer / MIC (simt_amd/online_labels.py; DESIGN 7.19) -- the model "
                        "trains on the teacher's arg-max at EVERY pixel and each pixel's cross-entropy is multiplied by q, the share of pixels "
                        "whose confidence is above T; T deletes nothing.  MODE batch (no value): one q for the batch, the published rule; item: "
                        "one q per image (with --online-mix a pasted pixel carries its partner's).  Needs --batch-size <= 32; not with "
                        "--online-labels-balanced.  Default: off")
    p.add_argument("--online-source", action="store_true",
                   help="with --online-labels: the published DACS step (simt_amd/online_labels.py; DESIGN 7.20) -- every batch is trained beside a "
                        "labelled source batch of --data-dir / --data-list (GTA5: images/<name>, labels/<name>) at --input-size-target, in the same "
                        "optimiser step; with --online-mix half of a source image's classes are pasted, image and ground truth, onto the target "
                        "image, and with --online-labels-weighted a pasted pixel has weight 1.  The source loader honours --random-mirror and "
                        "--scale-crop only.  Default: off")
    p.add_argument("--rare-class-sampling", nargs="?", const="0.01", default=None, metavar="T",
                   help="with --online-source: DAFormer's rare-class sampling of the source batch (simt_amd/data/rare_class.py; DESIGN 7.21) -- "
                        "a class is drawn with probability softmax((1 - f) / T) of the class frequencies f (no value: T = 0.01), then a frame "
                        "that holds it; with --scale-crop K candidate windows are drawn per item and the first that shows enough of the class "
                        "is taken, counted and picked on the device.  Needs --rcs-stats (simt_amd.tools.compute_class_stats).  Default: off")
    p.add_argument("--rcs-stats", type=str, default=None, metavar="FILE", help="the per-frame class statistics of --data-list")
    p.add_argument("--rcs-min-pixels", default=None, metavar="N",
                   help="a frame holds a class when it has at least N pixels of it, at full size.  Default: 3000")
    p.add_argument("--rcs-min-crop-ratio", default=None, metavar="R",
                   help="a window is taken when it shows more than floor(N * R) pixels of the class (0 <= R <= 1).  Default: 0.5")
    p.add_argument("--rcs-crops", default=None, metavar="K", help="candidate windows per item, 1 to 16.  Default: 10")


RCS_DEFAULTS = {"rcs_min_pixels": "3000", "rcs_min_crop_ratio": "0.5", "rcs_crops": "10"}


def rare_class_setting(args):
    """-> (T, min_pixels, ratio text, K, min_count) of --rare-class-sampling and the --rcs-* flags (rare_class.parse), or None when off."""
    if getattr(args, "rare_class_sampling", None) is None:
        return None
    from simt_amd.data.rare_class import parse
    v = {k: (d if getattr(args, k, None) is None else getattr(args, k)) for k, d in RCS_DEFAULTS.items()}
    return parse(args.rare_class_sampling, v["rcs_min_pixels"], v["rcs_min_crop_ratio"], v["rcs_crops"])


def check_online_label_args(p, args):
    """argparse's error (exit status 2) naming the flag: --online-labels-every without --online-labels or without --ema, --online-labels
    with --class-mix (the loader's mix reads the classes to paste from the partner's LABEL, which the teacher has not made yet), and --online-mix
    without --online-labels or outside the batch sizes and class counts the mix holds."""
    if args.online_labels_every is not None and args.online_labels is None:
        p.error("--online-labels-every needs --online-labels: it moves the teacher that makes the labels")
    if args.online_labels_every is not None and args.ema is None:
        p.error("--online-labels-every needs --ema: the teacher follows the weight EMA")
    if args.online_labels_balanced is not None and args.online_labels is None:
        p.error("--online-labels-balanced needs --online-labels: it balances the teacher's labels")
    if args.online_labels_momentum is not None and args.online_labels_balanced is None:
        p.error("--online-labels-momentum needs --online-labels-balanced: it averages the per-class thresholds")
    if args.online_labels_balanced is not None and args.num_classes > 64:
        p.error(f"--online-labels-balanced with --num-classes {args.num_classes}: the confidence histogram holds at most 64 classes")
    if args.online_labels is not None and args.class_mix is not None:
        p.error("--online-labels cannot be combined with --class-mix: the mix reads the classes to paste from the partner's label, and "
                "the teacher makes the labels behind the loader (--online-mix mixes behind the teacher)")
    if getattr(args, "online_labels_weighted", None) is not None:
        from simt_amd.online_labels import MAX_WEIGHTED_ITEMS
        if args.online_labels is None:
            p.error("--online-labels-weighted needs --online-labels: it weighs the teacher's labels")
        if args.online_labels_balanced is not None:
            p.error("--online-labels-weighted cannot be combined with --online-labels-balanced in this version: the weight is the share of "
                    "pixels above the one threshold T")
        if not 1 <= args.batch_size <= MAX_WEIGHTED_ITEMS:
            p.error(f"--online-labels-weighted with --batch-size {args.batch_size}: the label launch counts at most {MAX_WEIGHTED_ITEMS} items")
    if getattr(args, "online_source", False) and args.online_labels is None:
        p.error("--online-source needs --online-labels: the source batch is trained beside a target batch that a teacher labels")
    if getattr(args, "rare_class_sampling", None) is None:
        for flag in ("rcs_stats",) + tuple(RCS_DEFAULTS):
            if getattr(args, flag, None) is not None:
                p.error(f"--{flag.replace('_', '-')} needs --rare-class-sampling: it sets the sampler")
    else:
        if not getattr(args, "online_source", False):
            p.error("--rare-class-sampling needs --online-source: it samples the labelled source batch")
        try:
            rare_class_setting(args)
        except ValueError as e:
            p.error(str(e))
        if not args.synthetic and not args.rcs_stats:
            p.error("--rare-class-sampling needs --rcs-stats FILE (python -m simt_amd.tools.compute_class_stats), or --synthetic")
    if getattr(args, "online_mix", None) is not None:
        from simt_amd.data.class_mix import MAX_CLASSES, MAX_ITEMS
        if args.online_labels is None:
            p.error("--online-mix needs --online-labels: it mixes by the teacher's labels")
        if not 2 <= args.batch_size <= MAX_ITEMS:
            p.error(f"--online-mix with --batch-size {args.batch_size}: items are mixed with their neighbour in the batch, 2 to {MAX_ITEMS} of them")
        if not 1 <= args.num_classes <= MAX_CLASSES:
            p.error(f"--online-mix with --num-classes {args.num_classes}: the presence word holds 1 to {MAX_CLASSES} classes")


def online_label_line(args):
    """One start-up line: who labels, the threshold, which view the teacher sees."""
    if getattr(args, "online_labels", None) is None:
        return
    n = args.online_labels_every
    who = "a fixed teacher (the start weights)" if n is None else f"a teacher that follows the weight EMA (decay {args.ema}), refreshed every {n} update(s)"
    weak = online_weak_view(args)
    print(f"online labels: {who} labels every batch, kept where its confidence is > {args.online_labels}; the teacher sees "
          f"{'the batch before ' + ', '.join(weak) + ' (the weak view)' if weak else 'the same batch as the student'}" + balanced_clause(args) +
          mix_clause(args, weak) + weighted_clause(args))
    source_line(args)


def online_balanced(args):
    """-> [P, M] of --online-labels-balanced / --online-labels-momentum (M: the default where the flag is absent), or None when off."""
    if getattr(args, "online_labels", None) is None or getattr(args, "online_labels_balanced", None) is None:
        return None
    from simt_amd.online_labels import DEFAULT_MOMENTUM
    m = args.online_labels_momentum
    return [float(args.online_labels_balanced), float(DEFAULT_MOMENTUM if m is None else m)]


def balanced_clause(args):
    """What --online-labels-balanced adds to the start-up line ("" without it)."""
    pm = online_balanced(args)
    if pm is None:
        return ""
    return (f"; class-balanced: one threshold per class, from {args.online_labels} towards the value that keeps the share {pm[0]} of the class's "
            f"pixels in a batch (momentum {pm[1]}), never above {args.online_labels}")


def mix_clause(args, weak):
    """What --online-mix adds to the start-up line ("" without it)."""
    p = getattr(args, "online_mix", None)
    if p is None:
        return ""
    if getattr(args, "online_source", False):      # the pasted side is the labelled source batch
        return (f"; online mix: with probability {p} a target item receives, image and ground truth, half of the classes of its source item, "
                f"behind the teacher and in front of the student's forward")
    views = (f"; the mix selects from the students' strong views: a pasted region carries its partner's {', '.join(weak)}" if weak else "")
    return (f"; online mix: with probability {p} an item receives, image and label, half of the classes the teacher found in its neighbour, "
            f"behind the teacher and in front of the student's forward" + views)


def source_line(args):
    """--online-source: one start-up line that says what an optimiser step consists of."""
    if not getattr(args, "online_source", False):
        return
    parts = ["supervised cross-entropy on a labelled source batch" + (" (synthetic)" if args.synthetic else f" of {args.data_list}"),
             "the teacher's labels on the target batch" +
             (" weighted by q" if getattr(args, "online_labels_weighted", None) is not None else "")]
    if getattr(args, "online_mix", None) is not None:
        parts[1] += (f", onto which half of the source image's classes are pasted with probability {args.online_mix}: ground truth" +
                     (" and weight 1" if getattr(args, "online_labels_weighted", None) is not None else "") + " where pasted")
    print("online source: one optimiser step = (1) " + parts[0] + " + (2) " + parts[1] +
          "; both passes into one gradient, the losses summed; the source loader honours --random-mirror and --scale-crop only")


def weighted_clause(args):
    """What --online-labels-weighted adds to the start-up line ("" without it)."""
    mode = getattr(args, "online_labels_weighted", None)
    if mode is None:
        return ""
    whose = "the batch's" if mode == "batch" else "its image's"
    return (f"; quality weights ({mode}): every pixel keeps the teacher's arg-max and its loss is multiplied by the share of {whose} pixels "
            f"whose confidence is > {args.online_labels}")


def online_weak_view(args):
    """The flags that give --online-labels a weak view of its own (none with --synthetic, where they do nothing)."""
    if getattr(args, "online_labels", None) is None or args.synthetic:
        return []
    return [f for f, v in (("--colour-jitter", args.colour_jitter), ("--gaussian-blur", args.gaussian_blur),
                           ("--mask-patches", getattr(args, "mask_patches", None))) if v is not None]


def add_v3_layers(p):
    p.add_argument("--v3-layers", type=int, nargs=3, default=[3, 4, 6], metavar=("L1", "L2", "L3"),
                   help="DeepLabv3 trunk: Bottlenecks of layer1..layer3 (3 4 6: model/deeplabv3.py as written, ResNet-50; "
                        "3 4 23: the ResNet-101 depth)")


def check_model_args(args):
    """--model names one of MODELS (checked here rather than by argparse: the reference's scripts accept any string); --iter-size > 1
    needs the DeepLab trainer."""
    if args.model not in MODELS:
        raise SystemExit(f"--model {args.model!r}: expected one of {', '.join(MODELS)}")
    if args.model != "DeepLab" and args.iter_size > 1:
        raise SystemExit(f"--iter-size {args.iter_size}: gradient accumulation is implemented for --model DeepLab only "
                         f"(SimTSingleTrainer, which trains {args.model}, runs --iter-size 1)")


def single_model_states(model, num_classes, open_classes, v3_layers=(3, 4, 6), seed=1234):
    """(trainable, frozen) state dicts of the nn.Modules of a one-output model at their constructor init: DeepLabv3(nc, openc, openset=True) /
    DeepLabv3(nc), or DeeplabVGG(nc + openc) / DeeplabVGG(nc).  A DeepLabv3 trunk deeper than the file's is the same module with
    layer1..layer3 rebuilt at v3_layers (layer4 and fc, which never run, keep the ResNet-50 shapes)."""
    torch.manual_seed(seed)
    if model == "DeepLabv3":
        return _module_state(model, v3_layers, num_classes, open_classes, openset=True), _module_state(model, v3_layers, num_classes)
    if model == "DeepLabVGG":
        return _module_state(model, v3_layers, num_classes + open_classes), _module_state(model, v3_layers, num_classes)
    raise ValueError(model)


def single_model_state(model, num_classes, v3_layers=(3, 4, 6), seed=1234):
    """State dict of DeepLabv3(num_classes) / DeeplabVGG(num_classes) at its constructor init: the model the warm-up stage trains
    (trainV1_warmup --model DeepLabv3 | DeepLabVGG) and the SimT stage freezes."""
    if model not in ("DeepLabv3", "DeepLabVGG"):
        raise ValueError(model)
    torch.manual_seed(seed)
    return _module_state(model, v3_layers, num_classes)


def _module_state(model, v3_layers, *a, **kw):
    if model == "DeepLabv3":
        from simt_amd.model.deeplabv3 import DeepLabv3, _ResNet50Params
        m = DeepLabv3(*a, **kw)
        if tuple(v3_layers) != (3, 4, 6):
            m.resnet.resnet_50 = _ResNet50Params(layers=tuple(v3_layers) + (3,))
    else:
        from simt_amd.model.deeplab_vgg import DeeplabVGG
        m = DeeplabVGG(*a, **kw)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def load_class_dist_arg(path, num_classes):
    """--class-dist: the prior sig_NTM multiplies into T (model/deeplab_multi.py:255), checked before any training starts: a missing
    or malformed file (shape other than [num_classes], sum not 1 within 1e-6) is a SystemExit naming the file."""
    if not osp.isfile(path):
        raise SystemExit(f"--class-dist {path!r} does not exist")
    try:
        cd = ms.load_class_dist(path=path)
    except Exception as e:
        raise SystemExit(f"--class-dist {path!r} is not a readable .npy file: {e}")
    if cd.shape != (num_classes,) or not np.issubdtype(cd.dtype, np.floating):
        raise SystemExit(f"--class-dist {path!r}: expected a float vector of shape ({num_classes},), got {cd.dtype} {cd.shape}")
    if not np.all(np.isfinite(cd)) or abs(float(cd.sum()) - 1.0) > 1e-6:
        raise SystemExit(f"--class-dist {path!r}: the prior must sum to 1 (within 1e-6), sums to {float(cd.sum())!r}")
    return cd


def restore(state, path, not_restore_last=False, strip_prefix=0, required=False, last=("layer5", "layer6"), remap=None):
    """Filter-by-key load of an AdaptSegNet-style checkpoint into a fresh state (trainV2_simt.py:248-255).  strip_prefix=6: the warm-up
    stage's `k[6:]` (trainV1_warmup.py:177, checkpoints saved from a wrapped module) -- a key is accepted with or without the prefix.
    last: the key prefixes not_restore_last skips (the classifiers; RESTORE_LAST per --model).
    remap: optional callable applied to the loaded dict before the filter (the one-output warm-up: simt_amd.pretrained.checkpoint_layout).
    required: a missing file or zero matching tensors is an error (the reference crashes in torch.load; silently training from the
    constructor init would still produce checkpoints that look like results)."""
    if not path or not osp.exists(path):
        if required:
            raise FileNotFoundError(f"--restore-from {path!r} does not exist (pass --from-scratch to train from the constructor init)")
        return 0
    saved = torch.load(path, map_location="cpu")
    if remap is not None:
        saved = remap(saved)
    n = 0
    for k, v in saved.items():
        for cand in ((k, k[strip_prefix:]) if strip_prefix else (k,)):
            if cand in state and (not not_restore_last or not cand.startswith(tuple(last))) and state[cand].shape == v.shape:
                state[cand] = v.clone()
                n += 1
                break
    if required and n == 0:
        raise RuntimeError(f"--restore-from {path!r}: no tensor matched the model's keys / shapes")
    return n


class SnapshotKeeper:
    """The snapshot rotation of trainV2_simt.py:452-464 / trainV1_warmup.py:243-256: after an evaluation keep ONE file
    `<stem><iter>_mIoU<mIoU>.pth` for the best mIoU so far; without a validation set (the reference hard-codes one) keep ONE rolling
    periodic file `<stem><iter>.pth`.  The new file is complete on disk (save_atomic) BEFORE the old one is removed."""

    def __init__(self, snapshot_dir, stem):
        self.dir, self.stem = snapshot_dir, stem
        self.best_mIoU, self.best_iter, self.rolling_iter = 0, 0, None

    def best(self, state_dict, i_iter, mIoU):
        if not mIoU > self.best_mIoU:
            return False
        old_file = osp.join(self.dir, self.stem + str(self.best_iter) + "_mIoU" + str(self.best_mIoU) + ".pth")
        print("Saving model with mIoU: ", mIoU)
        save_atomic(state_dict, osp.join(self.dir, self.stem + str(i_iter) + "_mIoU" + str(mIoU) + ".pth"))
        if os.path.exists(old_file):
            os.remove(old_file)
        self.best_mIoU, self.best_iter = mIoU, i_iter
        return True

    def rolling(self, state_dict, i_iter):
        save_atomic(state_dict, osp.join(self.dir, self.stem + str(i_iter) + ".pth"))
        if self.rolling_iter is not None and self.rolling_iter != i_iter:
            old_file = osp.join(self.dir, self.stem + str(self.rolling_iter) + ".pth")
            if os.path.exists(old_file):
                os.remove(old_file)
        self.rolling_iter = i_iter

    def state(self):
        """What a resumed run needs to go on rotating: it still removes the file it supersedes."""
        return {"best_mIoU": self.best_mIoU, "best_iter": self.best_iter, "rolling_iter": self.rolling_iter}

    def load_state(self, st):
        self.best_mIoU, self.best_iter, self.rolling_iter = st["best_mIoU"], st["best_iter"], st["rolling_iter"]


class EmaSnapshots:
    """--ema: the averaged model's half of every snapshot decision of the training loops -- a second SnapshotKeeper whose stem is the live
    one's with `ema_` in front of `iter` (GTA5_ema_iter..., GTA5_BAPA_warmup_ema_iter...), the `EMA mIoU` line and GTA5_<stop>_ema.pth.  Its
    bookkeeping travels in --train-state (TrainStateFile.ema_keeper).  A trainer without an EMA: every method does nothing."""

    def __init__(self, tr, keeper, resume, rank):
        self.tr, self.rank = tr, rank
        self.keeper = None
        if getattr(tr, "ema", None) is not None:
            assert keeper.stem.endswith("iter")
            self.keeper = SnapshotKeeper(keeper.dir, keeper.stem[:-len("iter")] + "ema_iter")
        resume.ema_keeper = self.keeper

    def final(self, snapshot_dir, stop):
        if self.keeper is not None and self.rank == 0:
            save_atomic(self.tr.ema_state_dict(), osp.join(snapshot_dir, "GTA5_" + str(stop) + "_ema.pth"))

    def evaluated(self, score, i_iter):
        """score(params) -> mIoU: the loop's evaluation call (every rank runs it, as for the live model)."""
        if self.keeper is None:
            return
        mIoU = score(self.tr.ema_params)
        if self.rank == 0:
            print("EMA mIoU: ", mIoU)
            self.keeper.best(self.tr.ema_state_dict(), i_iter, mIoU)

    def rolling(self, i_iter):
        if self.keeper is not None and self.rank == 0:
            self.keeper.rolling(self.tr.ema_state_dict(), i_iter)


RUN_DEFAULTS = {"scale_crop": False, "class_mix": False, "photometric": False, "weak_teacher": False, "patch_mask": False,
                "online_labels": False, "online_labels_balanced": False, "online_mix": False, "online_labels_weighted": False,
                "online_source": False, "rare_class_sampling": False, "fda": False, "entropy_min": False, "proto_denoise": False,
                "proto_contrast": False, "uncertainty_rectify": False}      # run_identity keys that are absent when their flag is off: what absence means


def run_identity(args, class_dist):
    """What the LOOP feeds the trainer and no trainer can check: the seed (loader order, mirror and scale-crop draws, synthetic batches), the
    mirror switch, the scale-crop choices, the class-mix probability, the photometric pair [S, P] and the patch-mask pair [P, R] (RUN_DEFAULTS: a key is absent when its flag is off, and absent means
    False -- the state files of runs from before a flag existed are those of runs without it; with --synthetic the flags do nothing), where the data comes from
    (the list file's SHA-256) and the class prior (it enters T and the synthetic labels)."""
    import hashlib
    choices = None if args.synthetic else scale_crop_choices(args)
    ident = {"random_seed": int(args.random_seed), "random_mirror": bool(args.random_mirror), "synthetic": bool(args.synthetic),
             "class_dist_sha256": hashlib.sha256(np.ascontiguousarray(np.asarray(class_dist, dtype=np.float32)).tobytes()).hexdigest()}
    if choices is not None:
        ident["scale_crop"] = list(choices)
    mix = None if args.synthetic else class_mix_setting(args)
    if mix is not None:
        ident["class_mix"] = mix[1]
    photo = None if args.synthetic else photometric_setting(args)
    if photo is not None:
        ident["photometric"] = list(photo)          # [colour-jitter S | None, gaussian-blur P | None]
    mask = None if args.synthetic else patch_mask_setting(args)
    if mask is not None:
        ident["patch_mask"] = list(mask)            # [mask-patch-size P, mask-patches R]
    if getattr(args, "weak_teacher", False):
        ident["weak_teacher"] = True
    if getattr(args, "online_labels", None) is not None:
        ident["online_labels"] = [float(args.online_labels), args.online_labels_every]      # [T, N | None]
        if online_balanced(args) is not None:
            ident["online_labels_balanced"] = online_balanced(args)      # [P, M]
        if getattr(args, "online_mix", None) is not None:
            ident["online_mix"] = float(args.online_mix)                 # P (the seed is random_seed)
        if getattr(args, "online_labels_weighted", None) is not None:
            ident["online_labels_weighted"] = str(args.online_labels_weighted)      # "batch" | "item"
        if getattr(args, "online_source", False):
            ident["online_source"] = True
            if not args.synthetic and osp.isfile(args.data_list):
                ident["source_list_sha256"] = hashlib.sha256(open(args.data_list, "rb").read()).hexdigest()
            rcs = rare_class_setting(args)
            if rcs is not None:                                          # [T, min-pixels, ratio, K, the statistics file's SHA-256 | None]
                stats = getattr(args, "rcs_stats", None)
                sha = hashlib.sha256(open(stats, "rb").read()).hexdigest() if not args.synthetic and stats and osp.isfile(stats) else None
                ident["rare_class_sampling"] = [rcs[0], rcs[1], rcs[2], rcs[3], sha]
            if getattr(args, "fda", None) is not None:
                ident["fda"] = float(args.fda)                           # beta (it restyles --synthetic source batches too)
        if getattr(args, "entropy_min", None) is not None:               # [lambda, eta, N] (trainV1_warmup --entropy-min)
            ident["entropy_min"] = [float(args.entropy_min), float(args.entropy_eta), int(args.entropy_after)]
        if getattr(args, "proto_denoise", None) is not None:             # [temp, M] (trainV1_warmup --proto-denoise)
            from simt_amd.proto import DEFAULT_MOMENTUM
            ident["proto_denoise"] = [float(args.proto_denoise), float(DEFAULT_MOMENTUM if args.proto_momentum is None else args.proto_momentum)]
        if getattr(args, "proto_contrast", None) is not None:            # [lambda, T, R] (trainV1_warmup --proto-contrast)
            from simt_amd.proto_contrast import DEFAULT_MIN_RATIO, DEFAULT_TEMP
            ident["proto_contrast"] = [float(args.proto_contrast), float(DEFAULT_TEMP if args.proto_contrast_temp is None else args.proto_contrast_temp),
                                       float(DEFAULT_MIN_RATIO if args.proto_contrast_min_ratio is None else args.proto_contrast_min_ratio)]
    if getattr(args, "uncertainty_rectify", None) is not None:           # lambda_kl (trainV1_warmup --uncertainty-rectify; with or
        ident["uncertainty_rectify"] = [float(args.uncertainty_rectify)]   # without --online-labels; a list, so that lambda_kl = 0 is not "off")
    if not args.synthetic and osp.isfile(args.data_list_target):
        ident["data_list_sha256"] = hashlib.sha256(open(args.data_list_target, "rb").read()).hexdigest()
    return ident


class TrainStateFile:
    """--train-state FILE of both training tools: `resume()` / `complete()` before the loop, `after_iteration()` at its end, `write()` where it breaks.
    Without the flag every method does nothing.  Rank 0 writes; every rank loads (rank 0's state is the state: INTEGRATION.md)."""

    def __init__(self, args, rank, world, class_dist=None):
        self.path, self.every = getattr(args, "train_state", None), getattr(args, "train_state_every", None)
        self.run = run_identity(args, class_dist) if self.path and class_dist is not None else {}
        self.save_pred_every, self.rank, self.world = args.save_pred_every, rank, world
        self.ema_keeper = None                     # --ema: the second rotation (EmaSnapshots sets it); its bookkeeping travels in the file's loop part
        if self.every is not None and self.every < 1:
            raise SystemExit(f"--train-state-every {self.every}: expected a positive number of iterations")
        if self.every is not None and not self.path:
            raise SystemExit("--train-state-every needs --train-state FILE")

    def resume(self, tr, keeper):
        """-> the iteration the loop continues at (0: FILE does not exist yet, a fresh run)."""
        if not self.path or not osp.exists(self.path):
            return 0
        from simt_amd import train_state
        ts, ks, ls = train_state.load(self.path)
        if ls.get("world", self.world) != self.world:
            raise SystemExit(f"--train-state {self.path!r} was written by a run over {ls['world']} GPU(s), this one has {self.world}")
        saved, mine = dict(ls.get("run", {})), dict(self.run)
        if saved and mine:
            for k, v in RUN_DEFAULTS.items():
                saved.setdefault(k, v)
                mine.setdefault(k, v)
        other = [k for k, v in mine.items() if k in saved and saved[k] != v]
        if other:
            raise SystemExit(f"--train-state {self.path!r} was written by a run that differs in: " +
                             ", ".join(f"{k} (state: {saved[k]!r}, this run: {mine[k]!r})" for k in other))
        try:
            tr.load_training_state(ts)
        except ValueError as e:
            raise SystemExit(f"--train-state {self.path!r}: {e}")
        if ks is not None:
            keeper.load_state(ks)
        if self.ema_keeper is not None and ls.get("ema_keeper") is not None:
            self.ema_keeper.load_state(ls["ema_keeper"])
        if self.rank == 0:
            print(f"resumed {type(tr).__name__} from {self.path} at iteration {tr.it_done}")
        return tr.it_done

    def write(self, tr, keeper):
        if self.path and self.rank == 0:
            from simt_amd import train_state
            loop = {"world": self.world, "run": self.run}
            if self.ema_keeper is not None:
                loop["ema_keeper"] = self.ema_keeper.state()
            train_state.save(self.path, tr.training_state(), keeper.state(), loop)

    def after_iteration(self, i_iter, tr, keeper):
        if self.every is not None:
            due = (i_iter + 1) % self.every == 0
        else:
            due = i_iter % self.save_pred_every == 0 and i_iter != 0          # the loop's snapshot decision, evaluated or not
        if due:
            self.write(tr, keeper)

    def complete(self, start, stop, tr, snapshot_dir):
        """A resumed run that has nothing left to do: say so and make sure the final snapshot exists."""
        if start < stop:
            return False
        if self.rank == 0:
            final = osp.join(snapshot_dir, "GTA5_" + str(stop) + ".pth")
            print(f"the run is complete: {start} of {stop} iterations done" + ("" if osp.exists(final) else f"; writing {final}"))
            if not osp.exists(final):
                save_atomic(tr.state_dict(), final)
            final_ema = final[:-len(".pth")] + "_ema.pth"
            if getattr(tr, "ema", None) is not None and not osp.exists(final_ema):
                save_atomic(tr.ema_state_dict(), final_ema)
        return True


def teacher_line(args):
    if args.ema_teacher is not None:
        print(f"EMA teacher: the frozen model follows the weight EMA (decay {args.ema}), refreshed behind every "
              f"{'update' if args.ema_teacher == 1 else str(args.ema_teacher) + ' updates'} (N = {args.ema_teacher})")


def weak_teacher_line(args):
    if getattr(args, "weak_teacher", False):
        on = [f for f, v in (("--class-mix", args.class_mix), ("--colour-jitter", args.colour_jitter), ("--gaussian-blur", args.gaussian_blur),
                             ("--mask-patches", getattr(args, "mask_patches", None))) if v is not None]
        print(f"weak-view teacher: the frozen model sees the batch before {', '.join(on)}; its predictions follow the "
              f"{'mix mask' if args.class_mix is not None else 'pixels (no mix: no item map)'}")


def patch_mask_line(args, frozen=True):
    """--mask-patches without --weak-teacher: say once who sees the masked image (frozen=False: the warm-up tool, which has one model)."""
    mask = None if args.synthetic else patch_mask_setting(args)
    if mask is not None and not getattr(args, "weak_teacher", False):
        print(f"patch mask: {mask[0]} x {mask[0]} patches blanked with probability {mask[1]}; " +
              ("without --weak-teacher both models see the masked image" if frozen else "the model trains on the masked image"))


def batches(args, B, H, W, cd, rank, world, dev, start_batch=0):
    """-> iterator of (image f32 [B,3,H,W], label i64 [B,H,W]) resident on the device, from this rank's batch number `start_batch` on (a
    resumed run: iterations done x iter_size); with --weak-teacher of (image, label, weak image, item map [B,H,W] u8 | None); with
    --online-labels (trainV1_warmup) of (image, None, weak image | None): the list needs no label column and no label file is opened, the weak
    image is there exactly when --colour-jitter, --gaussian-blur or --mask-patches is on."""
    online = getattr(args, "online_labels", None) is not None
    choices = scale_crop_choices(args)
    mix = class_mix_setting(args)
    photo = photometric_setting(args)
    mask = patch_mask_setting(args)
    if args.synthetic:
        if mask is not None and rank == 0:
            print("--mask-patches does nothing with --synthetic: the synthetic batches are not masked")
        if choices is not None and rank == 0:
            print("--scale-crop does nothing with --synthetic: the synthetic batches are made at the crop's size")
        if mix is not None and rank == 0:
            print("--class-mix does nothing with --synthetic: the synthetic batches are not mixed")
        if photo is not None and rank == 0:
            print("--colour-jitter / --gaussian-blur do nothing with --synthetic: the synthetic batches are not augmented")

        def synth():
            it = start_batch
            while True:                                     # one global sequence of seeds, dealt round-robin to the ranks
                yield ms.synthetic_batch(B, H, W, cd, seed=args.random_seed + it * world + rank, device=dev)
                it += 1
        if online:                                          # the synthetic labels are ignored; the teacher sees the same batch
            return ((img, None, None) for (img, _lab) in synth())
        return synth()
    if not args.data_dir_target or not osp.isdir(args.data_dir_target):
        raise SystemExit(f"--data-dir-target {args.data_dir_target!r} is not a directory; pass --synthetic for synthetic batches")
    from simt_amd.data.pipeline import IMG_MEAN, GpuLoader
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    ds = cityscapesPseudo(args.data_dir_target, args.data_list_target, crop_size=(W, H), scale=False, mirror=args.random_mirror, mean=IMG_MEAN,
                          scale_crop=choices, class_mix=mix, photometric=photo,
                          teacher_view=bool(getattr(args, "weak_teacher", False)) or bool(online_weak_view(args)),
                          patch_mask=mask, labels=not online)
    cache, on_epoch = None, None
    if getattr(args, "cache_dataset", "off") == "device":
        from simt_amd.data.cache import DatasetCache, default_budget_bytes
        gb = getattr(args, "cache_gb", None)
        n_distinct = len({ds.cache_key(i) for i in range(len(ds))})
        held = (W, H)
        if choices is not None:             # the cache holds the ORIGINAL frames: their size is the first item's (read from the file's header)
            from PIL import Image
            with Image.open(ds.files[0]["img"]) as im:
                held = im.size
        budget = default_budget_bytes(n_distinct, held) if gb is None else int(gb * 1e9)
        cache = DatasetCache(held, with_label=not online, budget_bytes=budget, device=dev)

        def on_epoch(epoch, hits, misses, nbytes):
            print(f"dataset cache: rank {rank} epoch {epoch}: {hits} hits, {misses} misses, {nbytes / 1e9:.3f} GB of {budget / 1e9:.3f} GB "
                  f"in {len(cache)} slots", flush=True)
    loader = GpuLoader(ds, B, shuffle=True, num_workers=args.num_workers, device=dev, seed=args.random_seed, rank=rank, world=world,
                       hold=max(1, getattr(args, "iter_size", 1)),     # the loop keeps iter_size micro-batches alive per step
                       cache=cache, on_epoch=on_epoch, start_batch=start_batch)
    if online:
        if ds.teacher_view:
            return ((img, None, weak) for (img, _lab, _sizes, _names, weak, _item) in loader)
        return ((img, None, None) for (img, _lab, _sizes, _names) in loader)
    if ds.teacher_view:
        return ((img, lab, weak, item) for (img, lab, _sizes, _names, weak, item) in loader)
    return ((img, lab) for (img, lab, _sizes, _names) in loader)


SOURCE_SEED_OFFSET = 0x5372      # "Sr": the source loader's seed is --random-seed + this (order, mirror and scale-crop draws of its own)


class SourceStream:
    """The source loader's batches as (image, label) pairs, and, with rare-class crops, the share of items whose chosen window met the bar:
    every batch adds its count to a device word on the consumer's stream (no synchronisation); `rcs_share()` reads and clears it -- call it
    where the loop has synchronised anyway (behind tr.losses())."""

    def __init__(self, loader, min_count=None):
        self.loader, self.it, self.min_count = loader, iter(loader), min_count
        self.acc, self.n = None, 0

    def __iter__(self):
        return self

    def __next__(self):
        img, lab = next(self.it)[:2]
        win = self.loader.last_windows() if self.min_count is not None else None
        if win is not None:
            if self.acc is None:
                self.acc = torch.zeros((), dtype=torch.int64, device=win.device)
            self.acc += (win[:, 3] > self.min_count).sum()
            self.n += win.shape[0]
        return img, lab

    def rcs_share(self):
        """-> the share since the last call, or None (no rare-class crops, or no batch since)."""
        if self.acc is None or self.n == 0:
            return None
        v = int(self.acc.item()) / self.n
        self.acc.zero_()
        self.n = 0
        return v


def rare_class_line(rc):
    """One start-up line: the class probabilities and the number of frames per class."""
    print(f"rare-class sampling: T = {rc.T}, a frame holds a class with >= {rc.min_pixels} pixels; P(class) = "
          f"[{', '.join(f'{p:.4f}' for p in rc.probs)}]; frames per class = [{', '.join(str(len(l)) for l in rc.lists)}]; "
          f"with --scale-crop the first of {rc.K} windows with more than {rc.min_count} pixels of the class is taken")


def source_batches(args, B, H, W, cd, rank, world, dev, start_batch=0):
    """--online-source: -> iterator of (source image f32 [B,3,H,W], source label i64 [B,H,W]) resident on the device, from this rank's
    batch number `start_batch` on -- the position of `batches`, so a resumed run continues both loaders together.  A second GpuLoader over
    GTA5DataSet(--data-dir, --data-list) at the target's size (the plan has one geometry), seeded by --random-seed + SOURCE_SEED_OFFSET; it
    honours --random-mirror and --scale-crop and none of the target-side augmentations, and is not cached.  --synthetic: labelled
    synthetic batches from the same seed.  --rare-class-sampling: the loader samples by simt_amd/data/rare_class.py (one start-up line says
    how); the result is a SourceStream, whose rcs_share() feeds the loss line."""
    seed = args.random_seed + SOURCE_SEED_OFFSET
    if args.synthetic:
        def synth():
            it = start_batch
            while True:
                yield ms.synthetic_batch(B, H, W, cd, seed=seed + it * world + rank, device=dev)
                it += 1
        return synth()
    if not args.data_dir or not osp.isdir(args.data_dir):
        raise SystemExit(f"--online-source: --data-dir {args.data_dir!r} is not a directory; pass --synthetic for synthetic batches")
    if not osp.isfile(args.data_list):
        raise SystemExit(f"--online-source: --data-list {args.data_list!r} is not a file")
    from simt_amd.data.pipeline import IMG_MEAN, GpuLoader
    from simt_amd.dataset.gta5_dataset import GTA5DataSet
    ds = GTA5DataSet(args.data_dir, args.data_list, crop_size=(W, H), scale=False, mirror=args.random_mirror, mean=IMG_MEAN,
                     scale_crop=scale_crop_choices(args))
    rcs = rare_class_setting(args)
    if rcs is not None:
        from simt_amd.data import rare_class
        try:
            ds.rare_class = rare_class.RareClass(rare_class.load_stats(args.rcs_stats, ds), rcs[0], rcs[1], rcs[2], rcs[3])
        except (OSError, ValueError, KeyError) as e:
            raise SystemExit(f"--rcs-stats: {e}")
        if rank == 0:
            rare_class_line(ds.rare_class)
    loader = GpuLoader(ds, B, shuffle=True, num_workers=args.num_workers, device=dev, seed=seed, rank=rank, world=world,
                       hold=max(1, getattr(args, "iter_size", 1)), start_batch=start_batch)
    return SourceStream(loader, ds.rare_class.min_count if rcs is not None and ds.scale_crop is not None else None)


def step_args(args, mb):
    """The micro-batches `batches` handed out -> the arguments of the trainer's step(): (image, label) and, with --weak-teacher, the keywords
    teacher_image / fix_item; the bare tensors with --iter-size 1, lists of iter_size otherwise."""
    def col(j):
        return mb[0][j] if args.iter_size == 1 else [m[j] for m in mb]
    return (col(0), col(1)), ({"teacher_image": col(2), "fix_item": col(3)} if args.weak_teacher else {})


def build_trainer(args, cd, h, w, dev, pg):
    """What --model decides: the two states and their restore, the trainer (SimTTrainer | SimTSingleTrainer), the head of the start-up
    `restored` line, the two segmentation losses of the loss line and the Evaluator's model= / layers=.
    -> (trainer, restored text, losses() -> (loss_seg_p, loss_seg_y), evaluator keywords)."""
    C, K, required = args.num_classes, args.open_classes, not (args.synthetic or args.from_scratch)
    hp = Hyper(num_classes=C, open_classes=K, th_high=args.Threshold_high, th_low=args.Threshold_low,
               lambda_seg=args.lambda_seg, lambda_place=args.lambda_Place, lambda_convex=args.lambda_Convex,
               lambda_volume=args.lambda_Volume, lambda_anchor=args.lambda_Anchor, iter_size=args.iter_size,
               lr=args.learning_rate, lr_T=args.learning_rate_T, momentum=args.momentum,
               weight_decay=args.weight_decay, power=args.power, num_steps=args.num_steps)
    kw = dict(dtype=torch.bfloat16 if args.compute_dtype == "bf16" else torch.float32, device=dev, process_group=pg, ema_decay=args.ema,
              ema_teacher_every=args.ema_teacher, teacher_view=args.weak_teacher, **args.optimizer_kwargs)
    if args.model == "DeepLab":
        state = ms.reference_init(ms.state_shapes(C, K, True), seed=args.random_seed)
        fixed = ms.reference_init(ms.state_shapes(C, 0, False), seed=args.random_seed)
        n1 = restore(state, args.restore_from, args.not_restore_last, required=required)
        n2 = restore(fixed, args.restore_from, required=required)
        tr = SimTTrainer(state, fixed, ms.ntm_init(C, K, args.random_seed + 1), ms.ntm_init(C, K, args.random_seed + 2), hp, cd,
                         args.batch_size, h, w, **kw)
        return tr, f"restored {n1}/{n2} tensors", lambda l: (l["loss_p1"] + l["loss_p2"], l["loss_y1"] + l["loss_y2"]), {}   # :438-441 (p1+p2, y1+y2)
    from simt_amd.step_single import SimTSingleTrainer
    model, layers = ENGINE_MODEL[args.model], tuple(args.v3_layers)
    state, fixed = single_model_states(args.model, C, K, layers, seed=args.random_seed)
    n1 = restore(state, args.restore_from, args.not_restore_last, required=required, last=RESTORE_LAST[args.model])
    n2 = restore(fixed, args.restore_from, required=required)
    tr = SimTSingleTrainer(model, state, fixed, ms.ntm_init(C, K, args.random_seed + 1), hp, cd, args.batch_size, h, w,
                           arch={"layers": layers} if model == "v3" else None, **kw)
    return (tr, f"{args.model}: restored {n1}/{n2} tensors", lambda l: (l["loss_p"], l["loss_y"]),
            dict(model=model, layers=layers if model == "v3" else None))


def main(argv=None):
    args = get_arguments(argv)
    check_model_args(args)
    class_dist = load_class_dist_arg(args.class_dist, args.num_classes) if args.class_dist else None
    rank, world, dev, pg = setup_devices(args, "trainV2_simt needs a GPU: the SimT hot path has no CPU fallback")
    w, h = map(int, args.input_size_target.split(","))
    cd = class_dist if class_dist is not None else ms.load_class_dist("bapa")
    tr, restored, seg_losses, eval_kw = build_trainer(args, cd, h, w, dev, pg)
    if rank == 0:
        optimizer_line(args)
        teacher_line(args)
        weak_teacher_line(args)
        patch_mask_line(args)
        print(f"{restored} from {args.restore_from}; {world} GPU(s), batch {args.batch_size}/GPU, "
              f"{h}x{w}, {args.compute_dtype}, K={args.open_classes}")
        os.makedirs(args.snapshot_dir, exist_ok=True)

    def open_data(start_batch):
        data = batches(args, args.batch_size, h, w, cd, rank, world, dev, start_batch=start_batch)
        # gradient accumulation: iter_size micro-batches per step (check_model_args: 1 for the one-output models)
        return lambda: step_args(args, [next(data) for _ in range(args.iter_size)])

    def loss_line(i_iter, l, rate):
        return ("iter = {0:8d}/{1:8d}, loss_seg_p = {2:.3f} loss_seg_y = {3:.3f} Convex = {4:.3f} Volume = {5:.3f} "
                "Anchor = {6:.3f} Place_loss = {7:.3f}  lr = {8:.2e}  ({9:.1f} img/s)".format(
                    i_iter, args.num_steps, *seg_losses(l), l["convex"], l["volume"], l["anchor"], l["place"], model_lr(args, i_iter), rate))
    train(args, tr, "GTA5_iter", cd, rank, world, open_data, loss_line, scorer(args, tr, args.open_classes, dev, rank, world, pg, **eval_kw))


if __name__ == "__main__":
    main()
