"""The table of a multi-tensor launch (csrc/multi_sweep.h; simt_sgd_multi, simt_adamw_multi, simt_ema_multi, simt_bn_fold_multi): segment
records on the device and the (segment, chunk index) pairs its workgroups walk, one each.  The record dtypes are in _lib.py."""
import numpy as np
import torch

CHUNK = 65536            # elements per workgroup of the parameter-sized launches


class Table:
    def __init__(self, recs, dtype, count, chunk, device):
        """recs: one tuple per segment in the field order of `dtype` (trailing fields left out are zero); count: the field that holds a segment's
        length; chunk: elements per workgroup.  The workgroup order is the record order, a segment's chunks adjacent."""
        segs = np.array([tuple(r) + (0,) * (len(dtype.names) - len(r)) for r in recs], dtype=dtype)
        counts = [int(n) for n in segs[count]]
        self.pairs = [(si, ci) for si, n in enumerate(counts) for ci in range((n + chunk - 1) // chunk)]
        self.host = segs.view(np.uint8).copy()          # the segment bytes as uploaded
        self.segs = torch.from_numpy(self.host).to(device)
        self.chunks = torch.tensor(self.pairs, dtype=torch.int32).reshape(-1, 2).to(device)
        self.nchunks, self.chunk, self.elements = len(self.pairs), chunk, sum(counts)

    def bind(self, desc, skip_if=None):
        """Fill the four table fields of a launch descriptor, and its `skip_if` with the device word given (the plan's sticky fused-BatchNorm
        error word, engine.TrunkPlan.fbn_error: no update while it is set); -> desc.  The caller keeps this Table alive beside it."""
        desc.segs, desc.chunks, desc.nchunks, desc.chunk = self.segs.data_ptr(), self.chunks.data_ptr(), self.nchunks, self.chunk
        if skip_if is not None:
            desc.skip_if = skip_if.data_ptr()
        return desc
