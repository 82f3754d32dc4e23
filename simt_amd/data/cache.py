"""Device-resident dataset cache: the RESIZED uint8 frames of the training set, kept in HBM.

What the network consumes is the resized frame, and Pillow's resize returns uint8, so an item can be kept exactly as 3*h*w bytes of RGB
plus h*w bytes of label (2 MiB at 1024 x 512: the 2 975 Cityscapes training items are 6.24 GB next to 288 GB of HBM).  Only an item's
first sighting needs the PNG decoder and PCIe; afterwards a batch is one `simt_cache_gather` launch (csrc/dataset_cache.hip) over B slots.

  * slots live in SLABS of `slab_slots` slots, allocated as they are needed: nothing is reserved up front (the trainer's buffers exist
    before the loader is built, the evaluator's come later still);
  * the key is the item's FILE PATHS, not its dataset index: `max_iters` repeats the list, and the repeats share one slot;
  * no eviction: with a shuffled order LRU buys nothing.  Once the byte budget is reached, or a slab allocation fails, `reserve`
    answers None for good and later items take the loader's transient buffers, every epoch;
  * a slot is written once (by the loader, on its copy stream, in the call that reserved it) and never rewritten.
"""
import torch


def _up16(n):
    return (n + 15) // 16 * 16


def slot_bytes(crop_wh, with_label=True):
    """Bytes one cached item occupies: image u8 [h][w][3] + label u8 [h][w], each rounded up to 16 bytes (the gather reads dwords):
    4*h*w at every crop whose h*w is a multiple of 16."""
    w, h = crop_wh
    return _up16(3 * h * w) + (_up16(h * w) if with_label else 0)


def default_budget_bytes(n_items, crop_wh, with_label=True):
    """The budget that holds `n_items` distinct items at this crop: 2 975 x 1024 x 512 -> 6.24 GB."""
    return int(n_items) * slot_bytes(crop_wh, with_label)


def _device_alloc(device):
    def alloc(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    return alloc


class DatasetCache:
    """key -> slot table over device slabs.  crop_wh = (w, h) like `crop_size`.  alloc(nbytes) -> uint8 tensor (default: on `device`);
    an allocation that raises RuntimeError (torch's out-of-memory error is one) or MemoryError ends caching, not the run."""

    def __init__(self, crop_wh, with_label=True, budget_bytes=None, slab_slots=64, device="cuda:0", alloc=None):
        self.w, self.h = int(crop_wh[0]), int(crop_wh[1])
        self.with_label = with_label
        self.img_bytes, self.lab_bytes = 3 * self.h * self.w, self.h * self.w
        self.img_stride, self.lab_stride = _up16(self.img_bytes), _up16(self.lab_bytes)
        self.slot_bytes = slot_bytes(crop_wh, with_label)
        self.budget_bytes = None if budget_bytes is None else int(budget_bytes)
        self.slab_slots = max(1, int(slab_slots))
        self._alloc = alloc if alloc is not None else _device_alloc(torch.device(device))
        self.slabs = []            # (image slab, label slab | None, number of slots)
        self.table = {}            # key -> slot = slab index * slab_slots + index inside the slab
        self.used = 0              # slots handed out of the newest slab
        self.bytes = 0             # bytes allocated
        self.closed = False        # budget reached or an allocation failed: nothing more is cached
        self.hits = self.misses = 0

    def __len__(self):
        return len(self.table)

    def lookup(self, key):
        return self.table.get(key)

    def _grow(self):
        n = self.slab_slots
        if self.budget_bytes is not None:
            n = min(n, (self.budget_bytes - self.bytes) // self.slot_bytes)
        if n <= 0:
            return False
        try:
            img = self._alloc(n * self.img_stride)
            lab = self._alloc(n * self.lab_stride) if self.with_label else None
        except (RuntimeError, MemoryError):
            return False
        self.slabs.append((img, lab, n))
        self.used = 0
        self.bytes += n * self.slot_bytes
        return True

    def reserve(self, key):
        """-> a new slot for `key`, or None when nothing more is cached.  The caller fills the slot before anything gathers from it."""
        assert key not in self.table
        if self.closed:
            return None
        if not self.slabs or self.used == self.slabs[-1][2]:
            if not self._grow():
                self.closed = True
                return None
        slot = (len(self.slabs) - 1) * self.slab_slots + self.used
        self.used += 1
        self.table[key] = slot
        return slot

    def img_view(self, slot):
        s, k = divmod(slot, self.slab_slots)
        return self.slabs[s][0][k * self.img_stride:k * self.img_stride + self.img_bytes]

    def lab_view(self, slot):
        s, k = divmod(slot, self.slab_slots)
        return self.slabs[s][1][k * self.lab_stride:k * self.lab_stride + self.lab_bytes]

    def img_ptr(self, slot):
        s, k = divmod(slot, self.slab_slots)
        return self.slabs[s][0].data_ptr() + k * self.img_stride

    def lab_ptr(self, slot):
        s, k = divmod(slot, self.slab_slots)
        return self.slabs[s][1].data_ptr() + k * self.lab_stride
