"""ImageNet starting weights of the one-output models, host only: torchvision state dicts mapped onto the keys of simt_amd.model's
DeepLabv3 and DeeplabVGG.

The reference builds both trunks from torchvision ImageNet weights: DeepLabv3 takes torchvision's `resnet50(pretrained=True)` as its
`resnet_50` (model/deeplabv3.py:12), DeeplabVGG loads a torchvision `vgg16` state dict into vgg16 BEFORE it drops pool4 (features.23)
and copies the layers over (model/deeplab_vgg.py:27-34), so conv5_x moves down one index.  The warm-up stage (tools/trainV1_warmup.py
--model DeepLabv3 | DeepLabVGG) accepts such files through `checkpoint_layout`."""
import re

RESNET_PREFIX = "resnet.resnet_50."
VGG16_CONV5 = {24: 23, 26: 25, 28: 27}      # torchvision vgg16 features index -> DeeplabVGG's (pool4, index 23, dropped)


def resnet_to_deeplabv3(sd):
    """torchvision ResNet state dict (conv1, bn1, layer1..layer4, fc: resnet50, or resnet101 for --v3-layers 3 4 23) -> DeepLabv3's keys."""
    return {RESNET_PREFIX + k: v for k, v in sd.items()}


def vgg16_to_deeplab_vgg(sd):
    """torchvision vgg16 state dict -> DeeplabVGG's keys: features below index 23 keep their index, conv5_x (24, 26, 28) becomes 23, 25, 27.
    The Linear classifier (fc6..fc8) has no counterpart: DeeplabVGG's fc6 / fc7 (features.29 / .31) and its classifier keep their init."""
    out = {}
    for k, v in sd.items():
        m = re.fullmatch(r"features\.(\d+)\.(weight|bias)", k)
        if not m:
            continue
        i = int(m.group(1))
        if i < 23:
            out[k] = v
        elif i in VGG16_CONV5:
            out[f"features.{VGG16_CONV5[i]}.{m.group(2)}"] = v
    return out


DEEPLAB_HEADS = ("layer5", "layer6", "layer5_1", "layer6_1")      # DeeplabMulti's classifier modules


def imagenet_trunk(sd, shapes):
    """The frozen ImageNet trunk of the feature distance (--feat-dist-from) -> (layout name, {trunk key: tensor}).

    sd: a torchvision `resnet101` state dict -- the trunk keys are DeeplabMulti's own (conv1, bn1, layer1..layer4), its `fc.*` keys are
    dropped -- or any file in DeeplabMulti's keys, whose head keys (layer5*, layer6*) are dropped.  shapes: {key: shape} of the trainer's
    model (model_spec.state_shapes); every trunk key of it must be in `sd` with that shape: ValueError naming the first missing or mis-shaped
    key otherwise.  `num_batches_tracked` is taken when present and is not required (files written before PyTorch 0.4.1 have none)."""
    heads = tuple(h + "." for h in DEEPLAB_HEADS)
    layout = "torchvision ResNet" if any(k.startswith("fc.") for k in sd) else "DeeplabMulti"
    out = {}
    for k, shp in shapes.items():
        if k.startswith(heads):
            continue
        if k not in sd:
            if k.endswith("num_batches_tracked"):
                continue
            raise ValueError(f"feat-dist-from: trunk key {k!r} is missing from the file ({layout} layout, {len(sd)} keys)")
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"feat-dist-from: trunk key {k!r} has shape {tuple(sd[k].shape)}, the model needs {tuple(shp)}")
        out[k] = sd[k]
    return layout, out


def checkpoint_layout(sd, model):
    """-> (layout name, state dict in the module's keys) of a checkpoint for model "v3" (DeepLabv3) or "vgg" (DeeplabVGG): the module's
    own keys (a warm-up or SimT checkpoint) are taken as they are, a torchvision ImageNet file is mapped; anything else comes back
    unchanged as "unrecognised" (the caller's key / shape filter then decides what matches)."""
    if model == "v3":
        if any(k.startswith(RESNET_PREFIX) for k in sd):
            return "DeepLabv3", sd
        if "conv1.weight" in sd and any(k.startswith("layer1.") for k in sd):
            return "torchvision ResNet", resnet_to_deeplabv3(sd)
        return "unrecognised", sd
    if model == "vgg":
        if "features.24.weight" in sd:                   # a ReLU in DeeplabVGG, conv5_1 in torchvision's vgg16
            return "torchvision vgg16", vgg16_to_deeplab_vgg(sd)
        if any(k.startswith(("features.", "classifier.conv2d_list.")) for k in sd):
            return "DeeplabVGG", sd
        return "unrecognised", sd
    raise ValueError(model)
