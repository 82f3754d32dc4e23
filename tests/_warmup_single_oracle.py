"""Test helper: CPU reference of the warm-up stage over a ONE-OUTPUT model (simt_amd.step_single.WarmupSingleTrainer) --
oracle.simt_oracle.OracleWarmupTrainer with one head: loss = CE(interp_target(model(x)), label), ignore_index 255, / iter_size with the
gradients summed over the micro-batches (trainV1_warmup.py:212-231 without the auxiliary head), then SGD over the model's own
optim_parameters (DeepLabv3: layer3 at lr, ASSP + conv at 10 lr; DeeplabVGG: every parameter at lr).  Built from the oracle's
v3_forward / vgg_forward, upsample (align_corners=True; the identity behind DeepLabv3's in-model upsample), v3_optim_names, sgd_step_,
lr_poly."""
import torch
import torch.nn.functional as F

from oracle import simt_oracle as so


class OracleWarmupSingleTrainer:
    def __init__(self, model, st, hp, arch, dtype=torch.float32):
        """model: "v3" | "vgg"; st: the model's state (nc = hp.num_classes outputs); arch: {"layers": ...} as for OracleSingleTrainer."""
        self.model, self.hp, self.arch, self.dtype = model, hp, arch, dtype
        st = {k: (v.to(dtype) if v.dtype != torch.long else v) for k, v in st.items()}
        stat = lambda k: k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")
        self.st = {k: (v.clone().requires_grad_(True) if not stat(k) else v.clone()) for k, v in st.items()}
        shapes = {k: tuple(v.shape) for k, v in st.items()}
        if model == "v3":
            g0, g1 = so.v3_optim_names(shapes, False)
            self.groups = [{"names": g0, "lr_mult": 1.0}, {"names": g1, "lr_mult": 10.0}]
        else:
            self.groups = [{"names": [k for k in shapes if k.endswith(".weight") or k.endswith(".bias")], "lr_mult": 1.0}]
        self.bufs, self.first = {}, True

    def forward(self, image):
        if self.model == "v3":
            return so.v3_forward(self.st, image, layers=self.arch["layers"], openset=False, train=True)
        return so.vgg_forward(self.st, image, self.arch["layers"])

    def step(self, image, label, it):
        hp = self.hp
        lr = so.lr_poly(hp.lr, it, hp.num_steps, hp.power)
        for v in self.st.values():
            if v.dtype != torch.long:
                v.grad = None
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        labels = list(label) if isinstance(label, (list, tuple)) else [label]
        assert len(images) == len(labels) == hp.iter_size
        for img, lab in zip(images, labels):
            pred = so.upsample(self.forward(img.to(self.dtype)), tuple(lab.shape[1:]))
            loss = F.cross_entropy(pred, lab, ignore_index=255)
            total = loss / hp.iter_size
            total.backward()
        with torch.no_grad():
            for g in self.groups:
                ps, gs, bs, ms = [], [], [], []
                for n in g["names"]:
                    p = self.st[n]
                    if p.grad is None:
                        continue
                    if n not in self.bufs:
                        self.bufs[n] = torch.zeros_like(p)
                    ps.append(p); gs.append(p.grad); bs.append(self.bufs[n]); ms.append(1)
                so.sgd_step_(ps, gs, bs, ms, lr * g["lr_mult"], hp.weight_decay, hp.momentum, self.first)
            self.first = False
        return {"total": total.detach(), "loss_seg": loss.detach()}
