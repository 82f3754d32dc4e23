#!/usr/bin/env python3
"""Score a SimT checkpoint on the Cityscapes validation set: the reference's tools/test.py (load a checkpoint, evaluate_simt, print the
per-class IoU and the mIoU) for all three models of this project.

    python -m simt_amd.tools.test --model DeepLabv3 --open-classes 6 --restore-from snapshots/GTA5_40000.pth \\
        --data-dir-val <cityscapes root> --gt-dir-val <gtFine/val> --devkit-dir dataset/cityscapes_list

Every flag of the reference's tools/test.py is accepted (it shares the training script's argparse; most of those flags are parsed and
not used there either, and the same holds here).  Used: --model (DeepLab | DeepLabv3 | DeepLabVGG), --num-classes, --open-classes,
--restore-from (required: a missing file, or a file none of whose tensors matches the model's keys and shapes, is an error), --gpu,
--random-seed (the constructor init of the keys the checkpoint does not hold).  Additions: the validation data of trainV2_simt
(--data-dir-val, --data-list-val, --gt-dir-val, --devkit-dir), --eval-dtype (fp32 like the reference; bf16 is a labelled opt-in) and
--v3-layers (the DeepLabv3 trunk depth the checkpoint was trained with), --eval-scales W,H [W,H ...] (the input sizes whose logits are
summed; default the reference's 1024,512 and 1280,640) and --eval-flip (test-time augmentation: also the mirrored frame of every scale).  Unlike the reference, the checkpoint is filtered by key AND
shape (trainV2_simt.restore), the filter the training tools use.
"""
import argparse
import datetime
import os.path as osp
import time

import torch

from simt_amd import model_spec as ms
from simt_amd.tools.trainV2_simt import ENGINE_MODEL, MODELS, add_v3_layers, restore, single_model_states


def _wh(s):
    try:
        w, h = (int(v) for v in s.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected W,H, got {s!r}")
    if w <= 0 or h <= 0:
        raise argparse.ArgumentTypeError(f"expected positive W,H, got {s!r}")
    return w, h


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description="Evaluate a SimT checkpoint (DeepLab-ResNet / DeepLabv3 / DeepLab-VGG16) on MI355X")
    p.add_argument("--model", type=str, default="DeepLab", help="DeepLab | DeepLabv3 | DeepLabVGG")
    p.add_argument("--target", type=str, default="cityscapes")
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--iter-size", type=int, default=1)
    p.add_argument("--num-workers", type=int, default=4)
    p.add_argument("--data-dir", type=str, default="")
    p.add_argument("--data-list", type=str, default="../dataset/gta5_list/val.txt")
    p.add_argument("--ignore-label", type=int, default=255)
    p.add_argument("--input-size", type=str, default="1024,512")
    p.add_argument("--data-dir-target", type=str, default="")
    p.add_argument("--data-list-target", type=str, default="../dataset/cityscapes_list/pseudo_bapa.lst")
    p.add_argument("--input-size-target", type=str, default="1024,512")
    p.add_argument("--is-training", action="store_true")
    p.add_argument("--learning-rate", type=float, default=2.5e-4)
    p.add_argument("--learning-rate-T", type=float, default=2.5e-3)
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
    p.add_argument("--restore-from", type=str, default="")
    p.add_argument("--save-pred-every", type=int, default=1000)
    p.add_argument("--snapshot-dir", type=str, default="../snapshots/AdaptSegNet/")
    p.add_argument("--weight-decay", type=float, default=0.0005)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--set", type=str, default="val")
    p.add_argument("--log-dir", type=str, default="./log/")
    # additions
    p.add_argument("--data-dir-val", type=str, default="", help="Cityscapes root of the validation images (evaluate_cityscapes.py:26)")
    p.add_argument("--data-list-val", type=str, default="../dataset/cityscapes_list/val.txt")
    p.add_argument("--gt-dir-val", type=str, default="", help="directory of *_gtFine_labelIds.png (evaluate_cityscapes.py:140)")
    p.add_argument("--devkit-dir", type=str, default="../dataset/cityscapes_list")
    p.add_argument("--eval-dtype", choices=["f32", "bf16"], default="f32",
                   help="arithmetic of the evaluation: fp32 like the reference (evaluate_cityscapes.py:96-162); bf16 is a labelled opt-in")
    p.add_argument("--eval-scales", type=_wh, nargs="+", default=None, metavar="W,H",
                   help="input sizes of the evaluation, their logits are summed (default 1024,512 1280,640, evaluate_cityscapes.py:103-106)")
    p.add_argument("--eval-flip", action="store_true",
                   help="test-time augmentation: every scale also on the horizontally mirrored frame (one label launch over all terms)")
    add_v3_layers(p)
    args = p.parse_args(argv)
    if args.eval_scales is not None or args.eval_flip:
        from simt_amd import ops
        try:
            ops.tta_terms([(h, w) for (w, h) in (args.eval_scales or [(1024, 512), (1280, 640)])], args.eval_flip)
        except ValueError as e:
            p.error(f"--eval-scales / --eval-flip: {e}")
    return args


def model_state(args):
    """The state dict --model evaluates (the trainable model of the SimT stage, open-set heads included) with --restore-from loaded
    over its constructor init.  Raises SystemExit for a missing file, RuntimeError when no tensor matches."""
    C, K = args.num_classes, args.open_classes
    if args.model == "DeepLab":
        state = ms.reference_init(ms.state_shapes(C, K, True), seed=args.random_seed)
    else:
        state, _ = single_model_states(args.model, C, K, tuple(args.v3_layers), seed=args.random_seed)
    if not args.restore_from or not osp.isfile(args.restore_from):
        raise SystemExit(f"--restore-from {args.restore_from!r} does not exist")
    n = restore(state, args.restore_from, required=True)
    return state, n


def main(argv=None):
    args = get_arguments(argv)
    if args.model not in MODELS:
        raise SystemExit(f"--model {args.model!r}: expected one of {', '.join(MODELS)}")
    print("Leanring_rate: ", args.learning_rate)            # the reference's start-up lines, spelling included (test.py:135-144)
    print("Leanring_rate_T: ", args.learning_rate_T)
    print("Open-set class: ", args.open_classes)
    print("Threshold_high: ", args.Threshold_high)
    print("Threshold_low: ", args.Threshold_low)
    print("lambda_Place: ", args.lambda_Place)
    print("lambda_Convex: ", args.lambda_Convex)
    print("lambda_Volume: ", args.lambda_Volume)
    print("lambda_Anchor: ", args.lambda_Anchor)
    print("restore_from: ", args.restore_from)
    if not args.data_dir_val or not osp.isdir(args.data_dir_val):
        raise SystemExit(f"--data-dir-val {args.data_dir_val!r} is not a directory")
    state, n = model_state(args)
    if not torch.cuda.is_available():
        raise SystemExit("tools/test.py needs a GPU: the evaluation has no CPU fallback")
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)
    from simt_amd.tools.evaluate_cityscapes import evaluate_simt
    model = ENGINE_MODEL[args.model]
    print(f"{args.model}: restored {n}/{len(state)} tensors from {args.restore_from}")
    print(datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"))
    mIoU = evaluate_simt(state, args.data_dir_val, args.data_list_val, args.gt_dir_val, args.devkit_dir, num_classes=args.num_classes,
                         open_classes=args.open_classes, device=dev, workers=args.num_workers,
                         dtype=torch.bfloat16 if args.eval_dtype == "bf16" else torch.float32, model=model,
                         layers=tuple(args.v3_layers) if model == "v3" else None,
                         scales=[(h, w) for (w, h) in args.eval_scales] if args.eval_scales else None, flip=args.eval_flip)
    print("Finish Evaluation: " + time.asctime(time.localtime(time.time())))
    return mIoU


if __name__ == "__main__":
    main()
