"""The cross-domain mix of DACS restated in numpy from its contract (`simt_source_mix` of include/simt_hip.h): sets, `sorted`
and boolean masks, no bit tricks.  The yardstick of tests/test_source_mix_cpu.py and tests/test_gpu_source_mix.py; it imports nothing
from simt_amd.

Target item i is paired with source item i.  P_i = the classes c < C that occur in labs[i]; k = (|P_i| + 1) // 2; S_i = the k classes of
P_i with the smallest rank[i][c]; pixel p is pasted when apply[i] and labs[i][p] is in S_i (a 255 or an out-of-range source label is in no
P_i).  Pasted: the source's image and ground truth; elsewhere: the target's image and the teacher's byte label, widened.  The item map
names the entry of a [2B] weight table: B + i where pasted, i elsewhere."""
import numpy as np


# (B, h, w, C, seed): the launch geometries of tests/test_gpu_source_mix.py -- scalar flavour and tail; vector flavour twice; the smallest batch;
# the largest batch whose concatenation (2B items) the in-batch launches take.  The seeds were chosen on the CPU so that `conditions` holds.
GEOMETRIES = [(2, 33, 37, 19, 0), (3, 16, 64, 19, 0), (4, 64, 96, 19, 0), (1, 8, 8, 19, 0), (16, 12, 20, 32, 0)]
CASES = ("mixed", "none", "one class")


def inputs(B, h, w, C, seed, case):
    """-> (xs, labs, xt, lab8, apply, rank).  Images: random int32 words with NaN payloads, -0.0 and infinities sprinkled in; source labels:
    3 x 5 blocks of classes with a row of 255s and three out-of-range values; lab8: ALL 255 (whatever is not pasted stays unlabelled, and a
    pasted label cannot be mistaken for the target's).  "mixed": the draws of the documented generator with item 0 applied and, for B > 1,
    item 1 not; "none": apply all 0; "one class": every item applied, source item 0 holds ONE class on its left 5/8 and 255 elsewhere."""
    g = np.random.default_rng([seed, B, h, w])
    special = np.array([0x7FC00001, -0x3FFFFF, -0x80000000, 0x7F800000, -0x800000, 0x7F812345], dtype=np.int64).astype(np.int32)
    xs = g.integers(-2 ** 31, 2 ** 31, (B, 3, h, w), dtype=np.int64).astype(np.int32)
    xt = g.integers(-2 ** 31, 2 ** 31, (B, 3, h, w), dtype=np.int64).astype(np.int32)
    xs.reshape(-1)[::7] = special[np.arange(xs.size)[::7] % len(special)]
    xt.reshape(-1)[::5] = special[np.arange(xt.size)[::5] % len(special)]
    blocks = g.integers(0, C, (B, -(-h // 3), -(-w // 5)))
    labs = np.kron(blocks, np.ones((3, 5), dtype=np.int64))[:, :h, :w].astype(np.int64)
    labs[:, h // 2, :] = 255
    labs[0, 0, 0], labs[-1, -1, -1], labs[0, -1, 0] = C, -1, 300
    lab8 = np.full((B, h, w), 255, dtype=np.uint8)
    apply = g.random(B) < 0.5
    rank = g.permuted(np.tile(np.arange(C, dtype=np.uint8), (B, 1)), axis=1)
    if case == "mixed":
        apply[0] = True
        if B > 1:
            apply[1] = False
    elif case == "none":
        apply[:] = False
    else:
        apply[:] = True
        labs[0] = 255
        labs[0, :, :(5 * w) // 8] = C - 1
    return xs, np.ascontiguousarray(labs), xt, lab8, apply, rank


def conditions(labs, apply, rank, C):
    """What a case must show, from the restatement alone: every applied item has between 10 % and 90 % of its pixels pasted, and (when an
    item is applied) at least one quad -- 4 consecutive pixels, flat over h * w -- has mixed decisions."""
    m = paste_masks(labs, apply, rank, C)
    B = labs.shape[0]
    for i in range(B):
        if apply[i]:
            share = float(m[i].mean())
            assert 0.1 <= share <= 0.9, f"item {i}: {share:.3f} of its pixels pasted"
    if np.any(apply):
        flat = m.reshape(B, -1)
        n4 = flat.shape[1] // 4 * 4
        per_quad = flat[:, :n4].reshape(B, -1, 4).sum(axis=2)
        assert ((per_quad > 0) & (per_quad < 4)).any(), "no quad with mixed decisions"
    return m


def present(lab_item, C):
    return {int(v) for v in np.unique(lab_item) if 0 <= int(v) < C}


def chosen(lab_item, rank_row, C):
    P = present(lab_item, C)
    k = (len(P) + 1) // 2
    return set(sorted(P, key=lambda c: int(rank_row[c]))[:k])


def paste_masks(labs, apply, rank, C):
    """-> bool [B,h,w]: where target item i takes source item i's pixel."""
    m = np.zeros(labs.shape, dtype=bool)
    for i in range(labs.shape[0]):
        if apply[i]:
            m[i] = np.isin(labs[i], sorted(chosen(labs[i], rank[i], C)))
    return m


def mix(xs, labs, xt, lab8, apply, rank, C):
    """xs / xt: [B,3,h,w] of any 4-byte dtype (the tests pass int32 views: a select touches no bit); labs: [B,h,w] int64; lab8: [B,h,w]
    uint8.  -> (x_out, lab_out int64, item map uint8), new arrays."""
    B = labs.shape[0]
    m = paste_masks(labs, apply, rank, C)
    own = np.arange(B, dtype=np.int64).reshape(B, 1, 1)
    x_out = np.where(m[:, None, :, :], xs, xt)
    lab_out = np.where(m, labs.astype(np.int64), lab8.astype(np.int64))
    item = np.where(m, B + own, own).astype(np.uint8)
    return x_out, lab_out, item
