"""Host side of the device-resident dataset cache (simt_amd/data/cache.py) on a fake allocator, and the tools' flags."""
import pytest
import torch

from simt_amd.data.cache import DatasetCache, default_budget_bytes, slot_bytes


class _Alloc:
    """Host tensors instead of HBM; fails from the `fail_at`-th allocation on like an exhausted device."""

    def __init__(self, fail_at=None):
        self.sizes, self.fail_at = [], fail_at

    def __call__(self, nbytes):
        if self.fail_at is not None and len(self.sizes) >= self.fail_at:
            raise torch.cuda.OutOfMemoryError("fake: out of memory")
        self.sizes.append(nbytes)
        return torch.empty(nbytes, dtype=torch.uint8)


def test_slot_size_and_default_budget_match_the_table():
    assert slot_bytes((1024, 512)) == 2097152 and slot_bytes((768, 768)) == 2359296 and slot_bytes((512, 512)) == 1048576
    assert default_budget_bytes(2975, (1024, 512)) == 2975 * 2097152                 # 6.24 GB
    assert round(default_budget_bytes(2975, (1024, 512)) / 1e9, 2) == 6.24
    assert round(default_budget_bytes(2975, (768, 768)) / 1e9, 2) == 7.02
    assert round(default_budget_bytes(2975, (512, 512)) / 1e9, 2) == 3.12
    assert slot_bytes((1024, 512), with_label=False) == 3 * 512 * 1024
    # a crop whose planes are not 16-byte multiples: each part is rounded up, so that every slot starts on a 16-byte boundary
    assert slot_bytes((321, 321)) == (3 * 321 * 321 + 15) // 16 * 16 + (321 * 321 + 15) // 16 * 16


def test_slots_are_keyed_by_path_and_slabs_grow_on_demand():
    a = _Alloc()
    c = DatasetCache((8, 4), slab_slots=3, alloc=a)
    assert c.bytes == 0 and a.sizes == [] and len(c) == 0                            # nothing reserved up front
    keys = [("img/%d.png" % i, "lab/%d.png" % i) for i in range(7)]
    slots = [c.reserve(k) for k in keys]
    assert slots == list(range(7)) and len(c.slabs) == 3
    assert a.sizes == [3 * 96, 3 * 32] * 3                                           # image slab + label slab, three times
    assert c.bytes == 9 * slot_bytes((8, 4)) and not c.closed
    assert [c.lookup(k) for k in keys] == slots and c.lookup(("img/0.png", "lab/1.png")) is None
    # slots do not overlap and lie where the pointers say
    spans = sorted((c.img_ptr(s), c.img_ptr(s) + c.img_bytes) for s in slots)
    assert all(e0 <= b1 for (_b0, e0), (b1, _e1) in zip(spans, spans[1:]))
    for s in slots:
        assert c.img_view(s).data_ptr() == c.img_ptr(s) and c.img_view(s).numel() == 96 and c.img_ptr(s) % 16 == 0
        assert c.lab_view(s).data_ptr() == c.lab_ptr(s) and c.lab_view(s).numel() == 32 and c.lab_ptr(s) % 16 == 0
    assert c.img_ptr(1) == c.img_ptr(0) + 96 and c.lab_ptr(1) == c.lab_ptr(0) + 32   # neighbours in a slab are back to back
    with pytest.raises(AssertionError):
        c.reserve(keys[0])                                                           # a slot is written once


def test_budget_is_a_hard_limit_and_refusal_is_final():
    a = _Alloc()
    sb = slot_bytes((8, 4))
    c = DatasetCache((8, 4), budget_bytes=5 * sb + sb // 2, slab_slots=3, alloc=a)
    got = [c.reserve(("k%d" % i, None)) for i in range(8)]
    assert got == [0, 1, 2, 3, 4, None, None, None]                                  # 3 + 2 slots: the second slab is cut to the budget
    assert c.closed and c.bytes == 5 * sb and c.bytes <= c.budget_bytes and [s[2] for s in c.slabs] == [3, 2]
    assert c.lookup(("k4", None)) == 4 and c.lookup(("k5", None)) is None
    n = len(a.sizes)
    assert c.reserve(("late", None)) is None and len(a.sizes) == n                   # no further allocation is attempted
    z = DatasetCache((8, 4), budget_bytes=sb - 1, alloc=a)
    assert z.reserve(("k", None)) is None and z.closed and z.bytes == 0


def test_failed_slab_allocation_ends_caching_not_the_run():
    a = _Alloc(fail_at=2)                                                            # the first slab (image + label) fits, the second does not
    c = DatasetCache((8, 4), slab_slots=2, alloc=a)
    got = [c.reserve(("k%d" % i, "l")) for i in range(5)]
    assert got == [0, 1, None, None, None] and c.closed and len(c.slabs) == 1 and c.bytes == 2 * slot_bytes((8, 4))
    assert c.lookup(("k1", "l")) == 1


def test_images_only_cache_has_no_label_slab():
    a = _Alloc()
    c = DatasetCache((8, 4), with_label=False, slab_slots=2, alloc=a)
    assert c.reserve(("a", None)) == 0 and a.sizes == [2 * 96] and c.slabs[0][1] is None and c.slot_bytes == 96


@pytest.mark.parametrize("tool_name", ["trainV2_simt", "trainV1_warmup"])
def test_tools_parse_cache_flags_and_default_to_off(tool_name):
    import importlib
    tool = importlib.import_module("simt_amd.tools." + tool_name)
    a = tool.get_arguments([])
    assert a.cache_dataset == "off" and a.cache_gb is None
    a = tool.get_arguments(["--cache-dataset", "device", "--cache-gb", "6.5", "--model", "DeepLabVGG"])
    assert a.cache_dataset == "device" and a.cache_gb == 6.5
    with pytest.raises(SystemExit):
        tool.get_arguments(["--cache-dataset", "host"])


def test_dataset_cache_key_is_the_file_pair(tmp_path):
    from simt_amd.dataset.cityscapes_dataset import cityscapesDataSet, cityscapesPseudo
    lst = tmp_path / "p.lst"
    lst.write_text("a/1.png b/1.png\na/2.png b/2.png\n")
    ds = cityscapesPseudo(str(tmp_path), str(lst), max_iters=5)
    assert len(ds) == 6 and ds.cache_key(0) == ds.cache_key(2) == ds.cache_key(4) != ds.cache_key(1)
    assert len({ds.cache_key(i) for i in range(len(ds))}) == 2
    (tmp_path / "v.txt").write_text("x.png\ny.png\n")
    dv = cityscapesDataSet(str(tmp_path), str(tmp_path / "v.txt"))
    assert dv.cache_key(0) == (str(tmp_path / "val" / "x.png"), None)
