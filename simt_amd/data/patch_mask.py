"""MIC patch masking (--mask-patches): the host side of csrc/patch_mask.hip -- the flags' validation and the draws.  Pure Python / numpy.

Masked Image Consistency (Hoyer et al., CVPR'23; the step that followed DAFormer and HRDA) blanks a random set of square patches of the
image the student sees; the teacher sees the whole image, and the student has to predict the teacher's labels for the blanked regions from
their context.  Here the crop is cut into a grid of gh x gw patches of `patch` pixels (gh = ceil(h / patch), gw = ceil(w / patch); the last
row and column are partial when `patch` does not divide the crop), every patch of every item is blanked with probability `ratio`, and a
blanked pixel becomes +0.0f in all three planes: a batch holds colour - mean, so that is the mean colour -- what MIC's `image * mask` gives
after normalisation.  Labels are not touched.  The batch underneath is the loader's finished batch, after the mix and the photometric step.

Draws come from a generator OF THEIR OWN, `generator(seed, rank)`: turning the flag on does not move one mirror, scale-crop, class-mix or
photometric draw.  Per batch ONE `random((B, gh, gw))`, whatever `ratio` is and whatever comes out (so a resumed loader can skip them
without knowing them).  The masks travel as row words: bit c of word r of item i says that patch (r, c) is blanked.
"""
import numpy as np

MAX_ITEMS = 16            # include/simt_hip.h SIMT_PATCH_MASK_MAX: items per launch (a larger batch is split)
MAX_GRID = 32             # SIMT_PATCH_MASK_GRID: patch rows and patch columns per item, one uint32 row word per patch row
DEFAULT_RATIO = "0.7"     # MIC's mask ratio
DEFAULT_PATCH = 64        # MIC's patch size
STREAM_TAG = 0x4D49436D   # "MICm": the third word of the generator's seed sequence


def generator(seed, rank):
    """The mask's own generator of data-parallel rank `rank`."""
    return np.random.default_rng([int(seed), int(rank), STREAM_TAG])


def parse(ratio, patch, crop_wh):
    """--mask-patches' value R, --mask-patch-size's value P and the crop (w, h) -> (patch, ratio, gh, gw).  ValueError names what is wrong."""
    try:
        r = float(ratio)
    except (TypeError, ValueError):
        raise ValueError(f"--mask-patches {ratio!r} is not a ratio") from None
    if not 0.0 < r < 1.0:                 # (a NaN fails both comparisons)
        raise ValueError(f"--mask-patches {ratio!r}: the ratio of blanked patches must lie in (0, 1)")
    try:
        p = int(patch)
        if isinstance(patch, float) and patch != p:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"--mask-patch-size {patch!r} is not an integer") from None
    if p < 1:
        raise ValueError(f"--mask-patch-size {patch!r}: the patch size must be an integer >= 1")
    w, h = int(crop_wh[0]), int(crop_wh[1])
    gh, gw = -(-h // p), -(-w // p)
    if gh > MAX_GRID or gw > MAX_GRID:
        fit = -(-max(w, h) // MAX_GRID)
        raise ValueError(f"--mask-patch-size {p}: a crop of {w} x {h} needs {gw} x {gh} patches, a row word holds {MAX_GRID} x {MAX_GRID}: "
                         f"--mask-patch-size {fit} or larger would fit")
    return p, r, gh, gw


def pack_rows(mask):
    """[B, gh, gw] bool -> [B, MAX_GRID] uint32 row words: bit c of word r = mask[:, r, c]; the unused bits and words are 0."""
    mask = np.asarray(mask, dtype=bool)
    B, gh, gw = mask.shape
    assert gh <= MAX_GRID and gw <= MAX_GRID
    words = np.zeros((B, MAX_GRID), dtype=np.uint32)
    words[:, :gh] = (mask.astype(np.uint64) << np.arange(gw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words


def draw_batch(rng, batch_size, gh, gw, ratio):
    """One batch's draws -> [B, MAX_GRID] uint32 row words."""
    return pack_rows(rng.random((batch_size, gh, gw)) < ratio)


def skip_draws(rng, batch_size, n_batches, gh, gw):
    """Advance the generator by the draws of `n_batches` batches: their number does not depend on their values or on the ratio."""
    for _ in range(n_batches):
        draw_batch(rng, batch_size, gh, gw, 0.5)
    return rng


def blanked_share(words, h, w, patch):
    """The share of an item's pixels that its row words blank (partial edge patches counted by their pixels): [B] float64.  Reporting only."""
    gh, gw = -(-h // patch), -(-w // patch)
    ph = np.minimum(patch, h - patch * np.arange(gh)).astype(np.float64)
    pw = np.minimum(patch, w - patch * np.arange(gw)).astype(np.float64)
    bits = (np.asarray(words, dtype=np.uint32)[:, :gh, None] >> np.arange(gw, dtype=np.uint32)) & 1
    return (bits * ph[None, :, None] * pw[None, None, :]).sum(axis=(1, 2)) / float(h * w)
