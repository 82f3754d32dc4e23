"""The patch-mask contract of include/simt_hip.h (simt_patch_mask) restated in numpy, on uint32 views: nothing of simt_amd is imported, so
the draws below are the documented ones written down a second time.  Shared by tests/test_patch_mask_cpu.py and tests/test_gpu_patch_mask.py."""
import numpy as np

GRID = 32                 # SIMT_PATCH_MASK_GRID
STREAM_TAG = 0x4D49436D   # "MICm"


def generator(seed, rank):
    return np.random.default_rng([int(seed), int(rank), STREAM_TAG])


def draws(rng, B, gh, gw, ratio):
    """One batch's documented draws: ONE random((B, gh, gw)); bit c of word r of item i = (u[i][r][c] < ratio); unused bits and words 0."""
    m = rng.random((B, gh, gw)) < ratio
    words = np.zeros((B, GRID), dtype=np.uint32)
    for i in range(B):
        for r in range(gh):
            words[i, r] = sum(1 << c for c in range(gw) if m[i, r, c])
    return words


def mask_pixels(words, h, w, patch):
    """[B, 32] row words -> [B, h, w] bool: m = (rows[i][y / patch] >> (x / patch)) & 1.  Bits at column >= gw and words at row >= gh are
    never indexed: they are ignored."""
    words = np.asarray(words, dtype=np.uint32)
    ry, cx = np.arange(h) // patch, np.arange(w) // patch
    assert ry.max() < GRID and cx.max() < GRID
    return ((words[:, ry][:, :, None] >> cx[None, None, :].astype(np.uint32)) & 1).astype(bool)


def out_of_place(x_bits, words, patch):
    """x_bits [B, 3, h, w] uint32 (the words of the float32 batch) -> the words of x_out: 0x00000000 where blanked, the input word elsewhere."""
    x_bits = np.asarray(x_bits)
    assert x_bits.dtype == np.uint32 and x_bits.ndim == 4 and x_bits.shape[1] == 3
    m = mask_pixels(words, x_bits.shape[2], x_bits.shape[3], patch)
    return np.where(m[:, None], np.uint32(0), x_bits)


def in_place(x_bits, words, patch):
    """The same, written into x_bits: only the blanked words are stored."""
    assert x_bits.dtype == np.uint32
    m = mask_pixels(words, x_bits.shape[2], x_bits.shape[3], patch)
    x_bits[np.broadcast_to(m[:, None], x_bits.shape)] = 0
    return x_bits
