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
