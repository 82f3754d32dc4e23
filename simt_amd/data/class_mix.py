"""ClassMix (--class-mix): the host side of csrc/class_mix.hip -- the flag's validation and the draws.  Pure Python / numpy.

ClassMix (Olsson et al., WACV'21; the mixing of DACS and DAFormer) pastes, labels included, the pixels of half of the classes found in one
item's (pseudo) label onto another item.  Here item i of a batch of B receives from its partner j = (i + 1) % B: with P_j the classes
c < n_classes that occur in lab[j], n = |P_j| and k = (n + 1) // 2 (the original's ceil(n / 2)), S_j is the k classes of P_j with the
smallest rank[i][c], and a pixel p is pasted when apply[i] and lab[j][p] is in S_j.  A label outside [0, n_classes) ("ignore", 255) is
never pasted.  The batch underneath is the loader's finished batch (after mirror / scale-crop): the mix is a selection, no value changes.

Draws come from a generator OF THEIR OWN, `generator(seed, rank)`, never the loader's: turning the flag on does not move one mirror or
scale-crop draw.  Per batch, in this order and whatever `prob` is (so a resumed loader can skip them without knowing them):
`random(B)` for apply, then one permutation of the classes per item for rank.
"""
import numpy as np

MAX_ITEMS = 32            # include/simt_hip.h SIMT_CLASS_MIX_MAX
MAX_CLASSES = 32          # SIMT_CLASS_MIX_CLASSES: one presence word per item
STREAM_TAG = 0x436C4D78   # "ClMx": the third word of the generator's seed sequence


def generator(seed, rank):
    """The mix's own generator of data-parallel rank `rank`."""
    return np.random.default_rng([int(seed), int(rank), STREAM_TAG])


def parse(value, n_classes, batch_size):
    """--class-mix's value P, the number of classes and the batch size -> (n_classes, prob).  ValueError names what is wrong."""
    try:
        prob = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"--class-mix {value!r} is not a probability") from None
    if not 0.0 < prob <= 1.0:             # (a NaN fails both comparisons)
        raise ValueError(f"--class-mix {value!r}: the probability must lie in (0, 1]")
    n_classes, batch_size = int(n_classes), int(batch_size)
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"--class-mix with {n_classes} classes: the presence word holds 1 to {MAX_CLASSES}")
    if not 2 <= batch_size <= MAX_ITEMS:
        raise ValueError(f"--class-mix with a batch of {batch_size}: items are mixed with their neighbour in the batch, 2 to {MAX_ITEMS} of them")
    return n_classes, prob


def draw_batch(rng, batch_size, n_classes, prob):
    """One batch's draws -> (apply [B] bool, rank [B, n_classes] uint8, every row a permutation)."""
    apply = rng.random(batch_size) < prob
    rank = rng.permuted(np.tile(np.arange(n_classes, dtype=np.uint8), (batch_size, 1)), axis=1)
    return apply, rank


def skip_draws(rng, batch_size, n_batches, n_classes):
    """Advance the generator by the draws of `n_batches` batches: their number does not depend on their values or on `prob`."""
    for _ in range(n_batches):
        draw_batch(rng, batch_size, n_classes, 1.0)
    return rng
