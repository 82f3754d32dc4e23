"""ClassMix restated in numpy from its contract: sets, `sorted` and boolean masks, no bit tricks.  The yardstick of
tests/test_class_mix_cpu.py and tests/test_gpu_class_mix.py; it must not import simt_amd.data.class_mix.

Batch of B items: x [B,3,h,w], lab [B,h,w] (values outside [0, C) are "ignore").  Item i's partner is j = (i + 1) % B; P_j = the classes
c < C that occur in lab[j]; n = |P_j|, k = (n + 1) // 2; S_j = the k classes of P_j with the smallest rank[i][c]; pixel p is pasted when
apply[i] and lab[j][p] is in S_j."""
import numpy as np

TAG = 0x436C4D78          # the documented third word of the mix generator's seed ("ClMx")


def generator(seed, rank):
    return np.random.default_rng([seed, rank, TAG])


def draws(rng, B, C, prob):
    """The documented draws of one batch, in order: random(B) < prob, then one permutation of 0 .. C-1 per item."""
    apply = rng.random(B) < prob
    rank = rng.permuted(np.tile(np.arange(C, dtype=np.uint8), (B, 1)), axis=1)
    return apply, rank


def present(lab_item, C):
    return {int(v) for v in np.unique(lab_item) if 0 <= int(v) < C}


def chosen(lab_partner, rank_row, C):
    P = present(lab_partner, C)
    k = (len(P) + 1) // 2
    return set(sorted(P, key=lambda c: int(rank_row[c]))[:k])


def paste_masks(lab, apply, rank, C):
    """-> bool [B,h,w]: where item i takes its partner's pixel."""
    B = lab.shape[0]
    m = np.zeros(lab.shape, dtype=bool)
    for i in range(B):
        if not apply[i]:
            continue
        j = (i + 1) % B
        S = chosen(lab[j], rank[i], C)
        valid = (lab[j] >= 0) & (lab[j] < C)
        m[i] = valid & np.isin(lab[j], sorted(S))
    return m


def mix(x, lab, apply, rank, C):
    """-> (x_out, lab_out), new arrays; x may be of any 4-byte dtype (the tests pass int32 views: a select touches no bit)."""
    B = lab.shape[0]
    m = paste_masks(lab, apply, rank, C)
    partner = [(i + 1) % B for i in range(B)]
    lab_out = np.where(m, lab[partner], lab)
    x_out = np.where(m[:, None, :, :], x[partner], x)
    return x_out, lab_out
