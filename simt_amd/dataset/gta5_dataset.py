"""`dataset.gta5_dataset` of the reference on MI355X: the labelled SOURCE set of GTA5 -> Cityscapes adaptation, with the class
name and constructor arguments of the reference's `GTA5DataSet` and the division of labour of simt_amd/dataset/cityscapes_dataset.py:

  * `decode(index)` -- host side: file IO, PNG decoding to uint8 (Pillow) and the GTA5 id -> train-id table as ONE 256-entry numpy lookup;
  * resize (BICUBIC image / NEAREST label), BGR - mean, CHW, int64 labels -- device side, through `simt_amd.data.pipeline.GpuLoader`, as for
    `cityscapesPseudo`; `scale_crop=` turns on the loader's random scale + crop the same way.

Layout: a list file of frame names, one per line; frame `<name>` is `<root>/images/<name>` with its label image `<root>/labels/<name>`.
"""
import os.path as osp

import numpy as np

from .cityscapes_dataset import _Base

# GTA5 label id -> Cityscapes train id (the 19 evaluated classes); every other id is the ignore label
ID_TO_TRAINID = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 31: 16,
                 32: 17, 33: 18}


def trainid_table(ignore_label=255):
    """-> uint8 [256]: table[id] = train id, `ignore_label` for every id outside ID_TO_TRAINID."""
    table = np.full(256, ignore_label, dtype=np.uint8)
    for k, v in ID_TO_TRAINID.items():
        table[k] = v
    return table


class GTA5DataSet(_Base):
    """Image + ground-truth label of the GTA5 set, labels as train ids."""

    def __init__(self, root, list_path, max_iters=None, crop_size=(321, 321), mean=(128, 128, 128), scale=True, mirror=True, ignore_label=255,
                 scale_crop=None, rare_class=None):
        super().__init__(root, list_path, max_iters, crop_size, mean, scale, mirror, ignore_label)
        # decimal scale choices or None: GpuLoader's random scale + crop (simt_amd/data/scale_crop.py); `scale` is stored and never read
        self.scale_crop = None if scale_crop is None else tuple(str(c) for c in scale_crop)
        # a simt_amd.data.rare_class.RareClass or None: GpuLoader's rare-class sampling (which frame; with scale_crop, which window)
        self.rare_class = rare_class
        self.id_to_trainid = dict(ID_TO_TRAINID)
        self._table = trainid_table(ignore_label)
        self.img_ids = self._repeat([i_id.strip() for i_id in open(list_path) if i_id.strip()], max_iters)
        for name in self.img_ids:
            self.files.append({"img": osp.join(self.root, "images/%s" % name), "label": osp.join(self.root, "labels/%s" % name), "name": name})

    def decode(self, index):
        """-> (rgb uint8 [h,w,3], train ids uint8 [h,w], name)."""
        from PIL import Image
        f = self.files[index]
        lab = np.asarray(Image.open(f["label"]))
        if lab.ndim != 2 or lab.dtype != np.uint8:
            raise ValueError(f"{f['label']}: expected an 8-bit single-channel label image, got {lab.dtype} {lab.shape}")
        return self._open_rgb(f["img"]), self._table[lab], f["name"]

    def __getitem__(self, index):
        rgb, lab, name = self.decode(index)
        image, label = self._device_item(rgb, lab)
        return image, label, np.array((self.crop_size[1], self.crop_size[0], 3)), name
