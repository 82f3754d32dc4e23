"""The table builder of the multi-tensor launches without a GPU (simt_amd/multi_tensor.py): the (segment, chunk index) pairs and the segment
bytes against literals, and every record dtype's size against the size the kernels assert for their own struct (csrc) or ctypes reports."""
import ctypes as C
import os
import re

import numpy as np
import torch

from simt_amd import _lib as L
from simt_amd.multi_tensor import CHUNK, Table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [5, 65536, 65537, 0]


def test_pairs_and_segment_bytes_equal_literals():
    assert CHUNK == 65536
    recs = [(0x0102030405060708 + 0x100 * i, 0x1112131415161718 + 0x100 * i, n) for i, n in enumerate(COUNTS)]
    t = Table(recs, L.EMA_SEG, "n", 65536, "cpu")
    assert t.pairs == [(0, 0), (1, 0), (2, 0), (2, 1)]          # an empty segment has no workgroup
    assert t.chunks.dtype == torch.int32 and t.chunks.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1]]
    assert (t.nchunks, t.chunk, t.elements) == (4, 65536, 5 + 65536 + 65537)
    want = bytes.fromhex("0807060504030201" "1817161514131211" "0500000000000000"
                         "0808060504030201" "1818161514131211" "0000010000000000"
                         "0809060504030201" "1819161514131211" "0100010000000000"
                         "080a060504030201" "181a161514131211" "0000000000000000")
    assert t.host.dtype == np.uint8 and t.host.tobytes() == want and t.segs.numpy().tobytes() == want
    d = t.bind(L.EmaDesc())
    assert (d.segs, d.chunks, d.nchunks, d.chunk) == (t.segs.data_ptr(), t.chunks.data_ptr(), 4, 65536)
    t = Table(recs, L.EMA_SEG, "n", 1022, "cpu")
    assert t.pairs == [(0, 0)] + [(1, c) for c in range(65)] + [(2, c) for c in range(65)]          # 64 * 1022 = 65408 < 65536
    assert t.chunks.shape == (131, 2) and (t.nchunks, t.chunk, t.elements) == (131, 1022, 131078) and t.host.tobytes() == want
    empty = Table([], L.EMA_SEG, "n", 65536, "cpu")
    assert empty.pairs == [] and empty.chunks.shape == (0, 2) and empty.nchunks == 0 and empty.elements == 0 and empty.host.size == 0


def test_trailing_fields_are_zero_and_the_count_field_is_named():
    t = Table([(1, 2, 3, 4, 70000, 3)], L.ADAMW_SEG, "n", 65536, "cpu")          # `pad` left out
    assert t.host.tobytes() == bytes.fromhex("01" + "00" * 7 + "02" + "00" * 7 + "03" + "00" * 7 + "04" + "00" * 7 +
                                             "7011010000000000" + "03000000" + "00000000")
    assert t.pairs == [(0, 0), (0, 1)]
    t = Table([(1, 2, 3, 65537, 3, 1)], L.SGD_SEG, "n", 65536, "cpu")
    assert t.host.tobytes() == bytes.fromhex("01" + "00" * 7 + "02" + "00" * 7 + "03" + "00" * 7 + "0100010000000000" + "03000000" + "01000000")
    t = Table([(1, 2, 3, 4, 5, 6, 257)], L.BN_FOLD_SEG, "C", 256, "cpu")          # `reserved_` left out; the count is C
    assert t.pairs == [(0, 0), (0, 1)] and t.elements == 257
    seg = L.BnFoldSeg.from_buffer_copy(t.host)
    assert (seg.gamma, seg.beta, seg.running_mean, seg.running_var, seg.scale, seg.shift, seg.C, seg.reserved_) == (1, 2, 3, 4, 5, 6, 257, 0)


def test_record_sizes_match_the_kernels():
    asserted = {}
    for f in ("optim.hip", "ema.hip", "bn_fold_multi.hip"):
        src = open(os.path.join(ROOT, "simt_amd", "csrc", f)).read()
        asserted.update({m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(sizeof\((\w+)\) == (\d+),", src)})
    assert asserted == {"SgdSeg": 40, "AdamwSeg": 48, "EmaSeg": 24, "simt_bn_fold_seg": 56}
    assert (L.SGD_SEG.itemsize, L.ADAMW_SEG.itemsize, L.EMA_SEG.itemsize, L.BN_FOLD_SEG.itemsize) == (40, 48, 24, 56)
    assert L.BN_FOLD_SEG.itemsize == C.sizeof(L.BnFoldSeg)
    assert [L.BN_FOLD_SEG.fields[f[0]][1] for f in L.BnFoldSeg._fields_] == [getattr(L.BnFoldSeg, f[0]).offset for f in L.BnFoldSeg._fields_]
