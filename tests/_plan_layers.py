"""Layer tables of the three models for tests/_plan_replay.match_layers, shared by the launch-by-launch files (tests/test_gpu_plan_launches.py,
_v2.py, _small.py).  Not collected (no test_ prefix).

Each table is {parameter prefix: {"fwd": geometry, "bwd": geometry or None}} in _plan_replay._k's form: the conv launch whose weight operand was
packed from that parameter must have exactly this geometry.  They are functions of the depth (`layers`), the width and the storage dtype:
  * fp32 plans run the stem as an im2col matrix x a GEMM (K = 147 padded to 192) and the ASPP heads as ONE multi-tap implicit GEMM
    (K = 9 * dilations * Cin, N = Q) whose dgrad operand is K-padded to the fp32 channel quantum (32);
  * bf16 plans convolve the image directly (DeepLab-v2: the 49-tap 7x7 stem of csrc/stem7.hip) and run the heads tap-expanded
    (K = Cin, N = taps x QP, the dgrad K-padded to the bf16 quantum 64).
DeepLabv3 and DeepLab-VGG16 keep an im2col stem in both dtypes."""
import torch

from _plan_replay import STEM_TAPS, _k, _neg
from simt_amd import ops

BF = torch.bfloat16


def kq_of(dtype):
    """Channel quantum of the K dimension: one 128-byte stage (engine.TrunkPlan.kq)."""
    return 64 if dtype == BF else 32


def head_entries(out, heads, feat, B, dtype):
    """The ASPP heads of a TrunkPlan-style model: `heads` HeadCfg list, feat[layer] = (h, w, cin)."""
    one = [(0, 0)]
    kq = kq_of(dtype)
    for hd in heads:
        h, w, cin = feat[hd.feat_layer]
        assert cin == hd.cin
        taps = []
        for dil in hd.dilations:
            taps += ops.conv_taps(3, 3, dil, dil)
        if dtype == BF:
            nexp = len(taps) * ops.round_up(hd.Q, 8)
            geo = {"fwd": _k(B, h, w, cin, h, w, nexp, 1, one), "bwd": _k(B, h, w, ops.round_up(nexp, kq), h, w, cin, 1, one)}
        else:
            geo = {"fwd": _k(B, h, w, cin, h, w, hd.Q, 1, taps), "bwd": _k(B, h, w, ops.round_up(hd.Q, kq), h, w, cin, 1, _neg(taps))}
        for prefix, _c in hd.groups:
            for i in range(len(hd.dilations)):
                out[f"{prefix}.conv2d_list.{i}"] = dict(geo)
    return out


def v2_layers(B, H, W, K, layers=None, dtype=BF, heads=None):
    """DeepLab-v2 (engine.block_specs / trunk_geometry / multi_heads): layer2 strides 2 in its first conv1 and downsample, layer3 / layer4 keep
    the stride-8 map with dilation 2 / 4; the ASPP heads in the form the dtype launches (head_entries).  layers=None: the production depth,
    which must be ResNet-101's (3, 4, 23, 3); heads=None: multi_heads(19, K, K > 0)."""
    from simt_amd.engine import LAYERS, block_specs, multi_heads, trunk_geometry
    (H0, W0), (Hp, Wp), _ = trunk_geometry(H, W)
    assert (H0, W0) == ((H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1)
    if layers is None:
        assert LAYERS == (3, 4, 23, 3)
        layers = LAYERS
        assert len(block_specs(layers)) == 33
    one = [(0, 0)]
    M0 = B * H0 * W0
    if dtype == BF:
        out = {"conv1": {"fwd": _k(B, H, W, 3, H0, W0, 64, 2, STEM_TAPS), "bwd": None}}
    else:
        out = {"conv1": {"fwd": _k(1, 1, M0, 192, 1, M0, 64, 1, one), "bwd": None}}
    Hc, Wc = Hp, Wp
    feat = {}
    specs = block_specs(layers)
    assert len(specs) == sum(layers)
    for (n, inpl, p, s, dil, down) in specs:
        li, bi = int(n[5]), int(n.split(".")[1])
        assert (p, dil) == ((64, 128, 256, 512)[li - 1], (1, 1, 2, 4)[li - 1]) and s == (2 if (li == 2 and bi == 0) else 1) and down == (bi == 0)
        Ho, Wo, c4 = (Hc - 1) // s + 1, (Wc - 1) // s + 1, 4 * p
        t3 = ops.conv_taps(3, 3, dil, dil)
        out[n + ".conv1"] = {"fwd": _k(B, Hc, Wc, inpl, Ho, Wo, p, s, one), "bwd": _k(B, Ho, Wo, p, Ho, Wo, inpl, 1, one)}
        out[n + ".conv2"] = {"fwd": _k(B, Ho, Wo, p, Ho, Wo, p, 1, t3), "bwd": _k(B, Ho, Wo, p, Ho, Wo, p, 1, _neg(t3))}
        out[n + ".conv3"] = {"fwd": _k(B, Ho, Wo, p, Ho, Wo, c4, 1, one), "bwd": _k(B, Ho, Wo, c4, Ho, Wo, p, 1, one)}
        if down:
            out[n + ".downsample.0"] = {"fwd": _k(B, Hc, Wc, inpl, Ho, Wo, c4, s, one), "bwd": _k(B, Ho, Wo, c4, Ho, Wo, inpl, 1, one)}
        Hc, Wc = Ho, Wo
        feat[li] = (Hc, Wc, c4)
    if heads is None:
        heads = multi_heads(19, K, K > 0)
        assert all(hd.dilations == (6, 12) for hd in heads)
    return head_entries(out, heads, feat, B, dtype)


def v3_layers(B, H, W, layers, Q, width=64, ac=256, dtype=BF):
    """DeepLabv3, restated from the layer specs (model/deeplabv3.py via engine_v3's tables).  The stem is an im2col GEMM in both dtypes."""
    from simt_amd.engine_v3 import ASSP_BRANCHES, R50, v3_block_specs, v3_geometry
    (H0, W0), (Hp, Wp) = v3_geometry(H, W)
    one = [(0, 0)]
    out = {R50 + "conv1": {"fwd": _k(1, 1, B * H0 * W0, 192, 1, B * H0 * W0, width, 1, one), "bwd": None}}
    Hc, Wc = Hp, Wp
    t3 = ops.conv_taps(3, 3, 1, 1)
    for (n, inpl, p, s, down) in v3_block_specs(layers, width):
        Ho, Wo, c4 = (Hc - 1) // s + 1, (Wc - 1) // s + 1, 4 * p
        out[n + ".conv1"] = {"fwd": _k(B, Hc, Wc, inpl, Hc, Wc, p, 1, one), "bwd": _k(B, Hc, Wc, p, Hc, Wc, inpl, 1, one)}
        out[n + ".conv2"] = {"fwd": _k(B, Hc, Wc, p, Ho, Wo, p, s, t3), "bwd": _k(B, Hc, Wc, p, Hc, Wc, p, 1, _neg(t3))}
        out[n + ".conv3"] = {"fwd": _k(B, Ho, Wo, p, Ho, Wo, c4, 1, one), "bwd": _k(B, Ho, Wo, c4, Ho, Wo, p, 1, one)}
        if down:
            out[n + ".downsample.0"] = {"fwd": _k(B, Hc, Wc, inpl, Ho, Wo, c4, s, one), "bwd": _k(B, Ho, Wo, c4, Ho, Wo, inpl, 1, one)}
        Hc, Wc, cin = Ho, Wo, c4
    h, w = Hc, Wc
    for (i, k, dil) in ASSP_BRANCHES:
        taps = ops.conv_taps(3, 3, dil, dil) if k == 3 else one
        out[f"assp.conv{i}"] = {"fwd": _k(B, h, w, cin, h, w, ac, 1, taps), "bwd": _k(B, h, w, ac, h, w, cin, 1, _neg(taps))}
    # convf: 5 taps stepping one plane over the virtual concat; its dgrad plane by plane
    out["assp.convf"] = {"fwd": _k(1, 5 * B * h, w, ac, B * h, w, ac, 1, [(t * B * h, 0) for t in range(5)]), "bwd": _k(B, h, w, ac, h, w, ac, 1, one)}
    for pre in (("conv", "conv_1") if Q > 19 else ("conv",)):                    # classifier(s): fp32 logits, K-padded dgrad
        out[pre] = {"fwd": _k(B, h, w, ac, h, w, Q, 1, one), "bwd": _k(B, h, w, ops.round_up(Q, kq_of(dtype)), h, w, ac, 1, one)}
    return out


def vgg_layers(B, H, W, Q, table=None, dtype=BF):
    """DeepLab-VGG16 (engine_vgg.VGG_LAYERS or a reduced `table` of the same form): layer 0 through an im2col matrix (K = 27 padded to the
    channel quantum), the 2-branch head in the dtype's form."""
    from simt_amd.engine_vgg import VGG_LAYERS, vgg_head
    table = VGG_LAYERS if table is None else table
    kq = kq_of(dtype)
    one = [(0, 0)]
    out = {}
    Hc, Wc = H, W
    for li, (idx, cin, cout, dil, pool) in enumerate(table):
        M = B * Hc * Wc
        if li == 0:
            out[f"features.{idx}"] = {"fwd": _k(1, 1, M, kq, 1, M, cout, 1, one), "bwd": None}
        else:
            t3 = ops.conv_taps(3, 3, dil, dil)
            out[f"features.{idx}"] = {"fwd": _k(B, Hc, Wc, cin, Hc, Wc, cout, 1, t3), "bwd": _k(B, Hc, Wc, cout, Hc, Wc, cin, 1, _neg(t3))}
        if pool:
            Hc, Wc = Hc // 2, Wc // 2
    c = table[-1][2]
    return head_entries(out, vgg_head(Q, c), {0: (Hc, Wc, c)}, B, dtype)
