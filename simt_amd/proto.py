"""ProDA's prototype weights on the teacher's labels (Zhang et al., CVPR'21; keywords `proto_denoise` / `proto_momentum` of the
warm-up trainers, tool flags --proto-denoise / --proto-momentum).

Every other rule of `online_labels` judges a pixel by the teacher's softmax alone; a teacher that is confidently wrong about a class keeps
teaching it.  With `proto_denoise=temp` the teacher's low-res output is weighed, cell by cell, by how close the cell's FEATURE -- the input of
the teacher's main classifier -- lies to running class prototypes eta[C][D]:

    w_c = softmax_c(-(d_c - d_min) / temp),  d_c = || f - eta_c ||_2;      posterior' = w * posterior / sum(w * posterior)

which in the logit domain is logits' = logits + log w up to a constant per cell: out = logits - (d - d_min) / temp (family 1, DeepLabv3).  So
the rectification happens at feature resolution into a map with the layout of the teacher's output, and EVERY label launch of
simt_amd/online_labels.py -- plain, class-balanced, weighted, their byte flavours, the mixes -- runs on that map unchanged: `_init_proto`
re-points their `fix` once.  Per micro-batch, behind `simt_softmax_rows` (family 0) or the teacher's forward (family 1), on the stream that
ran them and in front of the label launch (include/simt_hip.h states the contract; tests/_proto_ref.py restates it):

  1. `simt_proto_rectify`: the rectified map, byte labels at feature resolution (arg-max where the rectified confidence is > tau, the
     `online_labels` threshold, in every mode) and the number of cells whose arg-max moved,
  2. `simt_proto_accumulate`: per class the sum of the features of the cells with that label, and their count,
  3. `simt_proto_update`: eta_c <- eta_c + a * (mean_c - eta_c), a = max(1 - proto_momentum, 1 / (n_c + 1)) (the running mean of the first
     1 / (1 - M) updates, then ProDA's exponential average); a class's first update IS its mean; a class absent from the batch is untouched.

A batch is therefore labelled with the prototypes of the batches before it, and the very first micro-batch -- no class seen -- with the
teacher's output word for word: its labels are the labels without the keyword.  An unseen class takes the distance of the nearest seen one: it
is not penalised for having no prototype yet.  `losses()` gains `proto_seen` (classes with a prototype) and `proto_changed` (the share of
cells whose arg-max the weights moved, last micro-batch).  The prototypes are per rank under data parallelism: nothing is exchanged.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops

DEFAULT_TEMP = 1.0             # ProDA's proto_temperature
DEFAULT_MOMENTUM = 0.9999      # ProDA's proto_momentum
MAX_CLASSES = L.PROTO_MAX_CLASSES
MAX_DIM = L.PROTO_MAX_DIM


def check_proto(proto_denoise, proto_momentum, tau, num_classes=None):
    """The two keywords -> (temp | None, M); `tau` is check_settings' first value.  ValueError that starts with the keyword that does not fit.
    temp None: off (M must then be its default: it would change nothing)."""
    m_in = DEFAULT_MOMENTUM if proto_momentum is None else proto_momentum
    what = "expected the prototypes' momentum, 0 <= M < 1"
    try:
        m = float(m_in)
    except (TypeError, ValueError):
        raise ValueError(f"proto_momentum {proto_momentum!r}: {what}") from None
    if isinstance(m_in, bool) or not (0.0 <= m < 1.0):          # (a NaN fails both comparisons)
        raise ValueError(f"proto_momentum {proto_momentum!r}: {what}")
    if proto_denoise is None:
        if m != DEFAULT_MOMENTUM:
            raise ValueError("proto_momentum needs proto_denoise: it averages the class prototypes, and this trainer keeps none")
        return None, DEFAULT_MOMENTUM
    what = "expected the temperature of the prototype weights, a finite temp > 0 (None: no prototypes)"
    try:
        t = float(proto_denoise)
    except (TypeError, ValueError):
        raise ValueError(f"proto_denoise {proto_denoise!r}: {what}") from None
    if isinstance(proto_denoise, bool) or not (1.0e-30 <= t <= 3.0e38):          # (likewise; the launch takes a finite float32 > 0)
        raise ValueError(f"proto_denoise {proto_denoise!r}: {what}")
    if tau is None:
        raise ValueError("proto_denoise needs online_labels: it weighs the teacher's posterior, and this trainer has no teacher")
    if num_classes is not None and not 2 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"proto_denoise with num_classes = {num_classes}: a wave holds one class per lane, 2 to {MAX_CLASSES} of them")
    return t, m


def alpha(momentum, n):
    """The step of a class that has received n >= 1 updates: max(1 - M, 1 / (n + 1))."""
    return max(1.0 - momentum, 1.0 / (n + 1))


def proto_step(F, P, eta, n, temp, thr, family, momentum, dtype=np.float64):
    """The three launches in numpy (`dtype` np.float64, or np.float32 with every operation rounded on its own; sums in index order) ->
    dict(out, lab, changed, S, cnt, eta, n).  F [M, D], P [M, ldp], eta [C, D], n [C]; tests/_proto_ref.py holds the restatement the GPU tests
    compare against, and tests/test_proto_cpu.py holds this one to it."""
    dt = dtype
    with np.errstate(all="ignore"):
        F, eta, Pd, n = np.asarray(F).astype(dt), np.asarray(eta).astype(dt), np.asarray(P).astype(dt), np.asarray(n).astype(np.int32)
        C_, M = len(n), F.shape[0]

        def total(t):          # over the last axis, in index order
            if dt == np.float64:
                return t.sum(axis=-1)
            s = np.zeros(t.shape[:-1], dtype=dt)
            for k in range(t.shape[-1]):
                s = (s + t[..., k]).astype(dt)
            return s

        def arg(v):
            return np.where(np.isnan(v), -np.inf, v).argmax(axis=1)

        seen, out = n > 0, Pd.copy()
        if seen.any():
            d = np.zeros((M, C_), dtype=dt)
            for c in np.nonzero(seen)[0]:
                diff = (F - eta[c]).astype(dt)
                d[:, c] = np.sqrt(total((diff * diff).astype(dt))).astype(dt)
            dmin = np.fmin.reduce(np.where(seen, d, np.inf), axis=1).astype(dt)
            d = np.where(seen, d, dmin[:, None]).astype(dt)
            z = (-(d - dmin[:, None]).astype(dt) / dt(temp)).astype(dt)
            if family == 0:
                r = (np.exp(z).astype(dt) * Pd[:, :C_]).astype(dt)
                out[:, :C_] = (r / total(r)[:, None]).astype(dt)
            else:
                out[:, :C_] = (Pd[:, :C_] + z).astype(dt)
        o = out[:, :C_]
        mx = np.where(np.isnan(o), -np.inf, o).max(axis=1).astype(dt)
        conf = mx if family == 0 else (dt(1) / total(np.exp((o - mx[:, None]).astype(dt)).astype(dt))).astype(dt)
        lab = np.where(~np.isnan(o).any(axis=1) & (conf > dt(np.float32(thr))), arg(o), 255).astype(np.uint8)
        changed = int((arg(o) != arg(Pd[:, :C_])).sum())
        S, cnt = np.zeros_like(eta), np.zeros(C_, dtype=np.int64)
        for p0 in range(0, M, 256):          # the parts of simt_proto_accumulate, then the parts in order
            part = np.zeros_like(eta)
            for m in range(p0, min(M, p0 + 256)):
                if lab[m] < C_:
                    part[lab[m]] = (part[lab[m]] + F[m]).astype(dt)
                    cnt[lab[m]] += 1
            S = (S + part).astype(dt)
        eta2, n2 = eta.copy(), n.copy()
        for c in np.nonzero(cnt)[0]:
            mean = (S[c] / dt(cnt[c])).astype(dt)
            if n[c] == 0:
                eta2[c] = mean
            else:
                a = max(np.float32(1.0 - momentum), np.float32(1) / np.float32(n[c] + 1)) if dt == np.float32 else alpha(momentum, int(n[c]))
                eta2[c] = (eta[c] + (dt(a) * (mean - eta[c]).astype(dt)).astype(dt)).astype(dt)
            n2[c] += 1
        return dict(out=out, lab=lab, changed=changed, S=S, cnt=cnt, eta=eta2, n=n2)


def fill_rectify(F, ldF, D, P, out, ldp, eta, n, lab, changed_part, M, Cn, dtype, family, temp, thr):
    """simt_proto_rectify_desc over device tensors."""
    d = L.ProtoRectifyDesc()
    d.F, d.P, d.out, d.eta, d.n = F.data_ptr(), P.data_ptr(), out.data_ptr(), eta.data_ptr(), n.data_ptr()
    d.lab, d.changed_part = lab.data_ptr(), changed_part.data_ptr()
    d.M, d.D, d.ldF, d.C, d.ldp, d.dtype, d.family, d.temp, d.thr = M, D, ldF, Cn, ldp, ops.dt_code(dtype), family, temp, thr
    return d


def fill_accumulate(F, ldF, D, lab, ws, M, Cn, dtype):
    """simt_proto_acc_desc over device tensors."""
    d = L.ProtoAccDesc()
    d.F, d.lab, d.ws = F.data_ptr(), lab.data_ptr(), ws.data_ptr()
    d.M, d.D, d.ldF, d.C, d.dtype = M, D, ldF, Cn, ops.dt_code(dtype)
    return d


def fill_update(ws, eta, n, M, D, Cn, momentum):
    """simt_proto_update_desc over device tensors."""
    d = L.ProtoUpdateDesc()
    d.ws, d.eta, d.n = ws.data_ptr(), eta.data_ptr(), n.data_ptr()
    d.M, d.D, d.C, d.momentum = M, D, Cn, momentum
    return d


class ProtoMixin:
    """The prototypes of OnlineLabelMixin: the buffers and descriptors of the three launches, the per-micro-batch calls, the read-out."""

    def _init_proto(self, proto, feat):
        """proto: check_proto's pair (temp None: off -- no buffer, no launch, every descriptor what it was).  feat: the input of the teacher
        plan's main classifier, [M][D] in the plan's dtype.  Behind _init_online, _init_mix and _init_weighted: their descriptors' `fix` is
        re-pointed at the rectified map here, once."""
        self.proto_denoise, self.proto_momentum = proto
        if self.proto_denoise is None:
            return
        dev, M, Cn = self.dev, self.B * self.h * self.w, self.C
        assert feat.dim() == 2 and feat.shape[0] == M and feat.is_contiguous(), tuple(feat.shape)
        D = feat.shape[1]
        if D % 8 or not 8 <= D <= MAX_DIM:
            raise ValueError(f"proto_denoise: the teacher's classifier reads {D} channels; the launches take a multiple of 8 up to {MAX_DIM}")
        lib = L.load()
        parts, words = lib.simt_proto_parts(M), lib.simt_proto_ws_floats(M, Cn, D)
        if parts < 1 or words < 1:
            raise L.SimtHipError(f"simt_proto_parts / simt_proto_ws_floats: {parts} / {words} for M = {M}, C = {Cn}, D = {D}")
        self.proto_feat = feat
        self.proto_map = torch.zeros(M, self.ldf, device=dev)
        self.proto_eta = torch.zeros(Cn, D, device=dev)
        self.proto_n = torch.zeros(Cn, device=dev, dtype=torch.int32)
        self.proto_lab = torch.zeros(M, device=dev, dtype=torch.uint8)
        self.proto_changed_part = torch.zeros(parts, device=dev, dtype=torch.int32)      # every word is written by every rectify launch
        self.proto_ws = torch.zeros(words, device=dev)                                   # every word is written by every accumulate launch
        self.proto_rectify_desc = fill_rectify(feat, D, D, self.fixp, self.proto_map, self.ldf, self.proto_eta, self.proto_n, self.proto_lab,
                                               self.proto_changed_part, M, Cn, self.dtype, self._family, self.proto_denoise, self.online_labels)
        self.proto_acc_desc = fill_accumulate(feat, D, D, self.proto_lab, self.proto_ws, M, Cn, self.dtype)
        self.proto_update_desc = fill_update(self.proto_ws, self.proto_eta, self.proto_n, M, D, Cn, self.proto_momentum)
        for name in ("online_desc", "online_cb_desc", "online_u8_desc", "online_cb_u8_desc", "online_w_desc"):
            d = getattr(self, name, None)
            if d is not None:
                d.fix = self.proto_map.data_ptr()

    def _proto_launches(self, st):
        """On the stream that ran the teacher's forward (and simt_softmax_rows), in front of the label launch, which reads `proto_map` on the
        same stream.  The previous micro-batch's label launch -- the map's one reader -- and its three launches lie in front by stream
        order; the features are the teacher plan's, whose next forward runs on this stream behind these launches."""
        if getattr(self, "proto_denoise", None) is None:
            return
        L.call("simt_proto_rectify", C.byref(self.proto_rectify_desc), st)
        L.call("simt_proto_accumulate", C.byref(self.proto_acc_desc), st)
        L.call("simt_proto_update", C.byref(self.proto_update_desc), st)

    def _proto_losses(self, out):
        """losses(): adds `proto_seen` and `proto_changed` (two more small device-to-host copies)."""
        if getattr(self, "proto_denoise", None) is not None:
            out["proto_seen"] = int((self.proto_n > 0).sum().item())
            out["proto_changed"] = int(self.proto_changed_part.sum().item()) / float(self.B * self.h * self.w)
        return out
