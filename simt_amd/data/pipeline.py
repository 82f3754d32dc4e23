"""Decoded uint8 frames -> network input on the device, and the loader that keeps the GPU fed.

Reference (CPU, per item, inside 4 DataLoader workers): dataset/cityscapes_dataset.py:97-120 `cityscapesPseudo.__getitem__`, :47-63
`cityscapesDataSet.__getitem__`; tools/trainV2_simt.py:287-294 DataLoader(shuffle=True, pin_memory=True), :345-348 `.cuda()`.
Here only file IO + PNG decoding stay on host threads; resize (Pillow-exact, csrc/input_prep.hip), BGR - mean, CHW and the label's
int64 conversion run on the GPU, and uploads go through pinned double buffers on a copy stream so that batch i+1 crosses PCIe
while batch i trains.  PyTorch supplies memory and streams only.
With a DatasetCache (simt_amd/data/cache.py) the resized uint8 frames stay in HBM: an item is decoded, uploaded and resized once, and every
batch is one gather over B cache slots (csrc/dataset_cache.hip).
"""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib as L
from . import resample as rs
from . import class_mix as cm
from . import patch_mask as pm
from . import photometric as ph
from . import rare_class as rc
from . import scale_crop as sc

IMG_MEAN = (104.00698793, 116.66876762, 122.67891434)      # tools/trainV2_simt.py:34 (BGR)


def _f32(v):
    return float(np.float32(v))


class InputPrep:
    """Device transform of a batch of decoded frames of ONE source geometry: [B, Hs, Ws, 3] u8 RGB (+ [B, Hs, Ws] u8 labels) ->
    [B, 3, h, w] fp32 (BGR - mean) (+ [B, h, w] int64).  crop = (w, h) like the reference's `crop_size` / --input-size-target."""

    def __init__(self, B, src_hw, crop_wh, device, mean=IMG_MEAN, with_label=True, scale_crop=None, class_mix=None, photometric=None,
                 patch_mask=None):
        self.B, (self.Hs, self.Ws), (self.w, self.h) = B, src_hw, crop_wh
        self.dev = torch.device(device)
        self.mean = tuple(_f32(m) for m in mean)
        self.with_label = with_label
        dev = self.dev
        self.cm, self.part = None, None
        if class_mix is not None:           # (n_classes, prob): `class_mix_batch` mixes a finished batch (simt_amd/data/class_mix.py)
            if not with_label:
                raise ValueError("--class-mix needs labels: the classes to paste are read from the partner's label")
            self.cm = cm.parse(class_mix[1], class_mix[0], B)
            self.part = torch.empty(B * L.CLASS_MIX_PARTS, dtype=torch.int32, device=dev)      # simt_label_presence's words
        self.ph, self.grey_part = None, None
        if photometric is not None:         # (S | None, P | None): `photometric_batch` jitters and blurs a finished batch (simt_amd/data/photometric.py)
            self.ph = tuple(photometric)
            self.grey_part = torch.empty(B * L.PHOTOMETRIC_PARTS, dtype=torch.int64, device=dev)      # simt_grey_mean_parts' words
        self.pm = None
        if patch_mask is not None:          # (patch, ratio): `patch_mask_batch` blanks patches of a finished batch (simt_amd/data/patch_mask.py)
            self.pm = pm.parse(patch_mask[1], patch_mask[0], crop_wh)
        self.sc = None
        if scale_crop is not None:          # the scale-crop mode (simt_amd/data/scale_crop.py): `scale_crop_batch` is the only entry point
            self.sc = sc.Tables(src_hw, crop_wh, scale_crop)
            if self.sc.lds_bytes() > L.SCALE_CROP_LDS_MAX:
                raise ValueError(f"--scale-crop: frames of {self.Ws} x {self.Hs} at crop {self.w} x {self.h} with choices "
                                 f"{' '.join(self.sc.choices)} need {self.sc.lds_bytes()} bytes of LDS per tile ({self.sc.max_rows} source "
                                 f"rows), the kernel has {L.SCALE_CROP_LDS_MAX}: drop the smallest choices")
            self.sc_tables = torch.from_numpy(self.sc.data).to(dev)
            self.need_x = self.need_y = False
            return
        self.need_x, self.need_y = self.w != self.Ws, self.h != self.Hs
        if self.need_x:
            self.kx, bx, cx = rs.bicubic_tables(self.Ws, self.w)
            self.bx, self.cx = torch.from_numpy(bx).to(dev), torch.from_numpy(cx).to(dev)
            self.tmp_x = torch.empty(B, self.Hs, self.w, 3, dtype=torch.uint8, device=dev)
        if self.need_y:
            self.ky, by, cy = rs.bicubic_tables(self.Hs, self.h)
            self.by, self.cy = torch.from_numpy(by).to(dev), torch.from_numpy(cy).to(dev)
            self.tmp_y = torch.empty(B, self.h, self.w, 3, dtype=torch.uint8, device=dev)
        if with_label:
            self.xtab = torch.from_numpy(rs.nearest_table(self.Ws, self.w)).to(dev)
            self.ytab = torch.from_numpy(rs.nearest_table(self.Hs, self.h)).to(dev)

    def run(self, rgb, x_out, lab=None, lab_out=None, mirror=False, stream=None):
        """rgb [B,Hs,Ws,3] u8, x_out [B,3,h,w] f32, lab [B,Hs,Ws] u8, lab_out [B,h,w] i64 -- all on the device; enqueues on `stream`
        (default: the current stream) and returns without synchronising.  mirror: bool or one bool per item -- the reference's
        --random-mirror branch, reproduced AS WRITTEN (cityscapes_dataset.py:108-111): the image's CHANNEL axis is reversed (net effect RGB
        order), only the label is mirrored horizontally."""
        st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
        assert rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (self.B, self.Hs, self.Ws, 3) and rgb.is_contiguous()
        assert x_out.dtype == torch.float32 and tuple(x_out.shape) == (self.B, 3, self.h, self.w) and x_out.is_contiguous()
        cur = rgb
        if self.need_x:
            L.call("simt_resample_u8", cur.data_ptr(), self.tmp_x.data_ptr(), self.B, self.Hs, self.Ws, 3, self.w, 1,
                   self.bx.data_ptr(), self.cx.data_ptr(), self.kx, st)
            cur = self.tmp_x
        if self.need_y:
            L.call("simt_resample_u8", cur.data_ptr(), self.tmp_y.data_ptr(), self.B, self.Hs, self.w, 3, self.h, 0,
                   self.by.data_ptr(), self.cy.data_ptr(), self.ky, st)
            cur = self.tmp_y
        if lab is not None:
            assert self.with_label and lab.dtype == torch.uint8 and tuple(lab.shape) == (self.B, self.Hs, self.Ws) and lab.is_contiguous()
            assert lab_out.dtype == torch.int64 and tuple(lab_out.shape) == (self.B, self.h, self.w) and lab_out.is_contiguous()
        flags = [bool(m) for m in mirror] if isinstance(mirror, (list, tuple, np.ndarray)) else [bool(mirror)] * self.B
        assert len(flags) == self.B
        # items with the same flag that sit next to each other go out in one launch (the usual case: one launch for the batch)
        b0 = 0
        while b0 < self.B:
            b1 = b0 + 1
            while b1 < self.B and flags[b1] == flags[b0]:
                b1 += 1
            n, f = b1 - b0, 1 if flags[b0] else 0
            L.call("simt_image_to_input", cur[b0].data_ptr(), x_out[b0].data_ptr(), n, self.h, self.w, self.mean[0], self.mean[1],
                   self.mean[2], f, st)
            if lab is not None:
                L.call("simt_label_nearest", lab[b0].data_ptr(), lab_out[b0].data_ptr(), n, self.Hs, self.Ws, self.h, self.w,
                       self.ytab.data_ptr(), self.xtab.data_ptr(), f, st)
            b0 = b1

    # ---- the cached path (simt_amd/data/cache.py): misses are resized into uint8 slots, one gather per batch reads B slots ----------
    def resize_into(self, rgb, lab, dests, stream):
        """rgb [M,Hs,Ws,3] u8 / lab [M,Hs,Ws] u8 | None on the device (M <= B decoded misses); dests[m] = (image u8 [h*w*3] view,
        label u8 [h*w] view | None): where item m's resized frame goes (a cache slot or a transient one).  Destinations that lie
        back to back share a launch: a batch of misses whose new slots are consecutive (the usual case) is resized with N = M."""
        M = len(dests)
        assert 0 < M <= self.B and tuple(rgb.shape) == (M, self.Hs, self.Ws, 3) and rgb.is_contiguous()
        runs, m0 = [], 0
        for m in range(1, M + 1):
            if m == M or dests[m][0].data_ptr() != dests[m - 1][0].data_ptr() + self.h * self.w * 3 or (
                    lab is not None and dests[m][1].data_ptr() != dests[m - 1][1].data_ptr() + self.h * self.w):
                runs.append((m0, m - m0))
                m0 = m
        if self.need_x and self.need_y:
            L.call("simt_resample_u8", rgb.data_ptr(), self.tmp_x.data_ptr(), M, self.Hs, self.Ws, 3, self.w, 1,
                   self.bx.data_ptr(), self.cx.data_ptr(), self.kx, stream)
        for m0, n in runs:
            dst = dests[m0][0].data_ptr()
            if self.need_y:
                src = self.tmp_x[m0] if self.need_x else rgb[m0]
                L.call("simt_resample_u8", src.data_ptr(), dst, n, self.Hs, self.w, 3, self.h, 0,
                       self.by.data_ptr(), self.cy.data_ptr(), self.ky, stream)
            elif self.need_x:
                L.call("simt_resample_u8", rgb[m0].data_ptr(), dst, n, self.Hs, self.Ws, 3, self.w, 1,
                       self.bx.data_ptr(), self.cx.data_ptr(), self.kx, stream)
            else:                                       # the files already have the crop's size
                for m in range(m0, m0 + n):
                    dests[m][0].copy_(rgb[m].reshape(-1), non_blocking=True)
            if lab is not None:
                L.call("simt_label_nearest_u8", lab[m0].data_ptr(), dests[m0][1].data_ptr(), n, self.Hs, self.Ws, self.h, self.w,
                       self.ytab.data_ptr(), self.xtab.data_ptr(), stream)

    def gather(self, img_ptrs, lab_ptrs, mirror, x_out, lab_out, stream):
        """One simt_cache_gather per batch (per SIMT_GATHER_MAX items): slot pointers + per-item mirror flags -> x_out [B,3,h,w] f32,
        lab_out [B,h,w] i64 | None.  Pointers and flags travel as kernel arguments: no copy, no synchronisation."""
        assert x_out.dtype == torch.float32 and tuple(x_out.shape) == (self.B, 3, self.h, self.w) and x_out.is_contiguous()
        assert lab_out is None or (lab_out.dtype == torch.int64 and tuple(lab_out.shape) == (self.B, self.h, self.w) and lab_out.is_contiguous())
        flags = [bool(m) for m in mirror] if isinstance(mirror, (list, tuple, np.ndarray)) else [bool(mirror)] * self.B
        assert len(flags) == self.B == len(img_ptrs)
        for b0 in range(0, self.B, L.GATHER_MAX):
            n = min(L.GATHER_MAX, self.B - b0)
            d = L.GatherDesc()
            for k in range(n):
                d.img[k] = img_ptrs[b0 + k]
                d.lab[k] = lab_ptrs[b0 + k] if lab_out is not None else None
                d.mirror[k] = 1 if flags[b0 + k] else 0
            d.x, d.lab_out = x_out[b0].data_ptr(), (lab_out[b0].data_ptr() if lab_out is not None else None)
            d.B, d.h, d.w = n, self.h, self.w
            d.mean[0], d.mean[1], d.mean[2] = self.mean
            L.call("simt_cache_gather", C.byref(d), stream)

    def scale_crop_batch(self, img_ptrs, lab_ptrs, draws, x_out, lab_out, stream):
        """One simt_scale_crop per batch (per SIMT_SCALE_CROP_MAX items): B pointers to source frames [Hs,Ws,3] u8 (+ labels [Hs,Ws] u8)
        on the device -- rows of an upload buffer or dataset-cache slots -- and draws = (mirror flags, choice indices, ox, oy), one per
        item (scale_crop.draw_batch) -> x_out [B,3,h,w] f32, lab_out [B,h,w] i64 | None."""
        assert self.sc is not None, "built without scale_crop choices"
        assert x_out.dtype == torch.float32 and tuple(x_out.shape) == (self.B, 3, self.h, self.w) and x_out.is_contiguous()
        assert lab_out is None or (lab_out.dtype == torch.int64 and tuple(lab_out.shape) == (self.B, self.h, self.w) and lab_out.is_contiguous())
        mirror, pick, ox, oy = draws
        assert len(img_ptrs) == len(mirror) == len(pick) == len(ox) == len(oy) == self.B
        for b0 in range(0, self.B, L.SCALE_CROP_MAX):
            n = min(L.SCALE_CROP_MAX, self.B - b0)
            d = L.ScaleCropDesc()
            for k in range(n):
                d.img[k] = img_ptrs[b0 + k]
                d.lab[k] = lab_ptrs[b0 + k] if lab_out is not None else None
                d.ox[k], d.oy[k], d.choice[k], d.mirror[k] = ox[b0 + k], oy[b0 + k], pick[b0 + k], 1 if mirror[b0 + k] else 0
            for c, e in enumerate(self.sc.entries):
                for name, v in e.items():
                    setattr(d.c[c], name, v)
            d.tables, d.n_tables = self.sc_tables.data_ptr(), self.sc_tables.numel()
            d.x, d.lab_out = x_out[b0].data_ptr(), (lab_out[b0].data_ptr() if lab_out is not None else None)
            d.B, d.Hs, d.Ws, d.h, d.w = n, self.Hs, self.Ws, self.h, self.w
            d.n_choices, d.max_rows = len(self.sc.entries), self.sc.max_rows
            d.mean[0], d.mean[1], d.mean[2] = self.mean
            L.call("simt_scale_crop", C.byref(d), stream)

    def rare_crop_batch(self, img_ptrs, lab_ptrs, draws, cls, min_count, x_out, lab_out, parts, win, stream):
        """scale_crop_batch whose window is picked on the device (rare-class crops, csrc/rare_crop.hip): draws = (mirror flags [B],
        choice indices [B][K], ox [B][K], oy [B][K]) (scale_crop.draw_batch_candidates), cls [B] the class counted per item (255: none).
        Three launches on `stream` per SIMT_RARE_CROP_MAX items: simt_rare_crop_counts -> parts (int32 [B, K, SIMT_RARE_CROP_PARTS]),
        simt_rare_crop_pick -> win (int32 [B, 4]: choice, ox, oy, count of the first candidate with count > min_count, else the last),
        simt_scale_crop_win -> x_out, lab_out at that window.  Nothing is read back."""
        for d in self.rare_crop_descs(img_ptrs, lab_ptrs, draws, cls, min_count, x_out, lab_out, parts, win):
            L.call("simt_rare_crop_counts", C.byref(d), stream)
            L.call("simt_rare_crop_pick", C.byref(d), stream)
            L.call("simt_scale_crop_win", C.byref(d), stream)

    def rare_crop_descs(self, img_ptrs, lab_ptrs, draws, cls, min_count, x_out, lab_out, parts, win):
        """The simt_rare_crop_desc of every SIMT_RARE_CROP_MAX items of the batch (arguments: rare_crop_batch's)."""
        assert self.sc is not None, "built without scale_crop choices"
        assert x_out.dtype == torch.float32 and tuple(x_out.shape) == (self.B, 3, self.h, self.w) and x_out.is_contiguous()
        assert lab_out is None or (lab_out.dtype == torch.int64 and tuple(lab_out.shape) == (self.B, self.h, self.w) and lab_out.is_contiguous())
        mirror, pick, ox, oy = draws
        K = len(pick[0])
        assert len(img_ptrs) == len(lab_ptrs) == len(mirror) == len(pick) == len(ox) == len(oy) == len(cls) == self.B
        assert all(len(r) == K for rows in (pick, ox, oy) for r in rows) and 1 <= K <= L.RARE_CROP_CANDS
        assert parts.dtype == torch.int32 and tuple(parts.shape) == (self.B, K, L.RARE_CROP_PARTS) and parts.is_contiguous()
        assert win.dtype == torch.int32 and tuple(win.shape) == (self.B, 4) and win.is_contiguous()
        out = []
        for b0 in range(0, self.B, L.RARE_CROP_MAX):
            n = min(L.RARE_CROP_MAX, self.B - b0)
            d = L.RareCropDesc()
            for k in range(n):
                d.img[k], d.lab[k] = img_ptrs[b0 + k], lab_ptrs[b0 + k]
                d.mirror[k], d.cls[k] = 1 if mirror[b0 + k] else 0, cls[b0 + k]
                for j in range(K):
                    d.cand_choice[k][j], d.cand_ox[k][j], d.cand_oy[k][j] = pick[b0 + k][j], ox[b0 + k][j], oy[b0 + k][j]
            for c, e in enumerate(self.sc.entries):
                for name, v in e.items():
                    setattr(d.c[c], name, v)
            d.tables, d.n_tables = self.sc_tables.data_ptr(), self.sc_tables.numel()
            d.x, d.lab_out = x_out[b0].data_ptr(), (lab_out[b0].data_ptr() if lab_out is not None else None)
            d.parts, d.win = parts[b0].data_ptr(), win[b0].data_ptr()
            d.B, d.Hs, d.Ws, d.h, d.w = n, self.Hs, self.Ws, self.h, self.w
            d.n_choices, d.max_rows = len(self.sc.entries), self.sc.max_rows
            d.K, d.min_count = K, int(min_count)
            d.mean[0], d.mean[1], d.mean[2] = self.mean
            out.append(d)
        return out

    def class_mix_batch(self, x, lab, draws, x_out, lab_out, stream, item_out=None):
        """ClassMix of a finished batch: x [B,3,h,w] f32 / lab [B,h,w] i64 -> x_out / lab_out (other buffers: item i reads item
        (i + 1) % B while another workgroup writes it).  draws = (apply [B] bool, rank [B, n_classes] permutations)
        (class_mix.draw_batch).  Two launches on `stream`: simt_label_presence, then simt_class_mix -- or, with item_out ([B,h,w] u8),
        simt_class_mix_items, which also writes the item each pixel came from (i or its partner)."""
        assert self.cm is not None, "built without class_mix"
        n_classes = self.cm[0]
        for t, o in ((x, x_out), (lab, lab_out)):
            assert t.shape == o.shape and t.dtype == o.dtype and t.is_contiguous() and o.is_contiguous() and t.data_ptr() != o.data_ptr()
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, 3, self.h, self.w)
        assert lab.dtype == torch.int64 and tuple(lab.shape) == (self.B, self.h, self.w)
        apply, rank = draws
        rank = np.ascontiguousarray(rank, dtype=np.uint8)
        assert len(apply) == self.B and rank.shape == (self.B, n_classes)
        d = L.ClassMixDesc()
        d.x, d.lab, d.x_out, d.lab_out, d.part = x.data_ptr(), lab.data_ptr(), x_out.data_ptr(), lab_out.data_ptr(), self.part.data_ptr()
        d.B, d.h, d.w, d.n_classes = self.B, self.h, self.w, n_classes
        for i in range(self.B):
            d.partner[i], d.apply[i] = (i + 1) % self.B, 1 if apply[i] else 0
            C.memmove(d.rank[i], rank[i].ctypes.data, n_classes)
        L.call("simt_label_presence", lab.data_ptr(), self.B, self.h * self.w, n_classes, self.part.data_ptr(), stream)
        if item_out is None:
            L.call("simt_class_mix", C.byref(d), stream)
        else:
            assert item_out.dtype == torch.uint8 and tuple(item_out.shape) == (self.B, self.h, self.w) and item_out.is_contiguous()
            L.call("simt_class_mix_items", C.byref(d), item_out.data_ptr(), stream)

    def photometric_batch(self, x, draws, x_out, stream):
        """Colour jitter + Gaussian blur of a finished batch: x [B,3,h,w] f32 -> x_out (another buffer: a blurred pixel reads its
        neighbours).  draws = photometric.draw_batch's dict of [B] arrays.  Two launches on `stream` per SIMT_PHOTOMETRIC_MAX items
        (items are independent, so a larger batch is split): simt_grey_mean_parts, then simt_photometric."""
        assert self.ph is not None, "built without photometric settings"
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, 3, self.h, self.w) and x.is_contiguous()
        assert x_out.dtype == torch.float32 and x_out.shape == x.shape and x_out.is_contiguous() and x_out.data_ptr() != x.data_ptr()
        assert all(len(draws[k]) == self.B for k in ("jit", "blur", "fb", "fc", "fs", "theta", "sigma"))
        for b0 in range(0, self.B, L.PHOTOMETRIC_MAX):
            n = min(L.PHOTOMETRIC_MAX, self.B - b0)
            d = L.PhotometricDesc()
            d.x, d.x_out, d.part = x[b0].data_ptr(), x_out[b0].data_ptr(), self.grey_part[b0 * L.PHOTOMETRIC_PARTS:].data_ptr()
            d.inv = ph.inv_pixels(self.h, self.w)
            d.B, d.h, d.w = n, self.h, self.w
            d.mean[0], d.mean[1], d.mean[2] = self.mean
            for k in range(n):
                i = b0 + k
                fb, fc, omfc, A, wk = ph.item_params(draws["fb"][i], draws["fc"][i], draws["fs"][i], draws["theta"][i], draws["sigma"][i])
                d.jit[k], d.blur[k] = 1 if draws["jit"][i] else 0, 1 if draws["blur"][i] else 0
                d.fb[k], d.fc[k], d.omfc[k] = float(fb), float(fc), float(omfc)
                C.memmove(d.A[k], np.ascontiguousarray(A, dtype=np.float32).ctypes.data, 36)
                C.memmove(d.wk[k], np.ascontiguousarray(wk, dtype=np.float32).ctypes.data, 24)
            L.call("simt_grey_mean_parts", C.byref(d), stream)
            L.call("simt_photometric", C.byref(d), stream)


    def patch_mask_batch(self, x, words, x_out, stream):
        """MIC patch masking of a finished batch: x [B,3,h,w] f32 -> x_out, which may BE x (in place: only the blanked words are stored).
        words = patch_mask.draw_batch's [B, 32] uint32 row words.  One simt_patch_mask launch on `stream` per SIMT_PATCH_MASK_MAX items
        (items are independent, so a larger batch is split)."""
        assert self.pm is not None, "built without patch_mask"
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, 3, self.h, self.w) and x.is_contiguous()
        assert x_out.dtype == torch.float32 and x_out.shape == x.shape and x_out.is_contiguous()
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.shape == (self.B, L.PATCH_MASK_GRID)
        for b0 in range(0, self.B, L.PATCH_MASK_MAX):
            n = min(L.PATCH_MASK_MAX, self.B - b0)
            d = L.PatchMaskDesc()
            d.x, d.x_out = x[b0].data_ptr(), x_out[b0].data_ptr()
            d.B, d.h, d.w, d.patch = n, self.h, self.w, self.pm[0]
            C.memmove(d.rows, words[b0:b0 + n].ctypes.data, n * L.PATCH_MASK_GRID * 4)
            L.call("simt_patch_mask", C.byref(d), stream)


class DevicePrefetcher:
    """Pinned double-buffered upload + device transform, one batch ahead of the consumer.

    source: iterator of (rgb u8 [B,Hs,Ws,3], label u8 [B,Hs,Ws] or None, meta) host arrays / tensors (numpy or torch; pinned
    tensors are uploaded in place, anything else is staged through this object's pinned buffers).
    Each __next__ returns (image f32 [B,3,h,w], label i64 [B,h,w] | None, meta) resident in HBM -- with teacher_view (the weak-view teacher:
    it needs mix_fn, photo_fn or mask_fn) two more: the slot's batch BEFORE the mix, the photometric and the mask launches (the loader's
    batch without any of them, bit for bit) and the item map of the mix ([B,h,w] u8: the item each pixel was taken from; None without
    mix_fn); same life time.
    mask_fn (MIC patch masking, prep.pm): a fourth stage behind the mix and the photometric step on the copy stream, ONE launch per 16
    items.  It blanks patches in place in the buffer that is about to be handed out (xp with a photometric step, else xm with a mix, else
    x); only where that buffer is also the weak view (teacher_view with neither mix nor photometric step) does it write a masked copy into
    a per-slot buffer xk of its own and leave x whole.

    Slot life time: the consumer may HOLD `hold` batches at once (gradient accumulation pulls `iter_size` micro-batches before the step
    that reads them is enqueued: tools/trainV2_simt.py `mb = [next(data) for _ in range(iter_size)]`).  The tensors returned by call k
    stay valid until call k + hold: only then is the slot's `free` event recorded on the consumer's stream (everything enqueued on
    that stream up to that point -- the step that consumed batch k included -- precedes the refill), and the copy stream waits for
    it.  2*hold slots, so the next group of `hold` batches is uploaded while the current one is being consumed."""

    def __init__(self, source, prep, mirror_fn=None, hold=1, depth=None, cache=None, draw_fn=None, mix_fn=None, photo_fn=None,
                 teacher_view=False, mask_fn=None, rare=None):
        self.src, self.prep, self.mirror_fn, self.cache = iter(source), prep, mirror_fn, cache
        self.draw_fn = draw_fn          # scale-crop mode (prep.sc): B -> (mirror flags, choice indices, ox, oy); replaces mirror_fn
        assert (draw_fn is not None) == (prep.sc is not None)
        # rare-class crops: (K, min_count); draw_fn then yields K candidates per item (scale_crop.draw_batch_candidates), the source's meta
        # carries the items' classes as its third entry, and the window is picked on the copy stream (prep.rare_crop_batch) into s["win"]
        self.rare = rare
        assert rare is None or draw_fn is not None, "rare-class crops pick among scale-crop windows"
        self.last_win = None            # the `win` words of the batch handed out last
        self.mix_fn = mix_fn            # class-mix mode (prep.cm): B -> (apply, rank); the slot's finished batch is mixed into xm / labm
        assert (mix_fn is not None) == (prep.cm is not None)
        self.photo_fn = photo_fn        # photometric mode (prep.ph): B -> draws; the finished (mixed) batch is jittered and blurred into xp
        assert (photo_fn is not None) == (prep.ph is not None)
        self.mask_fn = mask_fn          # patch-mask mode (prep.pm): B -> row words; the batch about to be handed out gets its patches blanked
        assert (mask_fn is not None) == (prep.pm is not None)
        self.teacher_view = bool(teacher_view)
        assert not self.teacher_view or mix_fn is not None or photo_fn is not None or mask_fn is not None, \
            "teacher_view: without a mix, a photometric step or a patch mask the views are one"
        # the mask runs IN PLACE in the buffer that is handed out (xp, else xm, else x) -- unless that buffer is also the weak view
        self.mask_out_of_place = mask_fn is not None and self.teacher_view and mix_fn is None and photo_fn is None
        self.hold = max(1, int(hold))
        depth = 2 * self.hold if depth is None else depth
        assert depth > self.hold, "the consumer holds `hold` slots: at least one more is needed to hand out"
        dev, B = prep.dev, prep.B
        self.copy_stream = torch.cuda.Stream(device=dev)
        self.slots = []
        for _ in range(depth):
            s = {"rgb_h": torch.empty(B, prep.Hs, prep.Ws, 3, dtype=torch.uint8).pin_memory(),
                 "rgb_d": torch.empty(B, prep.Hs, prep.Ws, 3, dtype=torch.uint8, device=dev),
                 "x": torch.empty(B, 3, prep.h, prep.w, dtype=torch.float32, device=dev),
                 "ready": torch.cuda.Event(), "free": None, "meta": None, "has_lab": False}
            if prep.with_label:
                s["lab_h"] = torch.empty(B, prep.Hs, prep.Ws, dtype=torch.uint8).pin_memory()
                s["lab_d"] = torch.empty(B, prep.Hs, prep.Ws, dtype=torch.uint8, device=dev)
                s["lab"] = torch.empty(B, prep.h, prep.w, dtype=torch.int64, device=dev)
            if rare is not None:
                s["parts"] = torch.empty(B, rare[0], L.RARE_CROP_PARTS, dtype=torch.int32, device=dev)
                s["win"] = torch.empty(B, 4, dtype=torch.int32, device=dev)
            if mix_fn is not None:                     # what __next__ hands out in class-mix mode: same life time as x / lab
                s["xm"], s["labm"] = torch.empty_like(s["x"]), torch.empty_like(s["lab"])
                if self.teacher_view:
                    s["item"] = torch.empty(B, prep.h, prep.w, dtype=torch.uint8, device=dev)
            if photo_fn is not None:                   # what __next__ hands out in photometric mode: same life time as x
                s["xp"] = torch.empty_like(s["x"])
            if self.mask_out_of_place:                 # the masked copy of x, which stays whole as the weak view: same life time as x
                s["xk"] = torch.empty_like(s["x"])
            if cache is not None:                      # transient slots for the items the cache has no room for
                s["sp_img"] = torch.empty(B * cache.img_stride, dtype=torch.uint8, device=dev)
                s["sp_lab"] = torch.empty(B * cache.lab_stride, dtype=torch.uint8, device=dev) if prep.with_label else None
            self.slots.append(s)
        self.head = 0          # next slot to hand out
        self.filled = 0
        self.calls = 0
        self.done = False
        for i in range(depth):
            self._fill(i)

    @staticmethod
    def _host(t):
        return torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t

    def _fill(self, i):
        if self.done:
            return
        try:
            rgb, lab, meta = next(self.src)
        except StopIteration:
            self.done = True
            return
        s = self.slots[i]
        if s.get("used"):
            s["ready"].synchronize()           # the previous upload out of this slot's pinned buffers has completed
        if self.cache is not None:
            return self._fill_cached(s, rgb, lab, meta)
        rgb = self._host(rgb)
        if not rgb.is_pinned():
            s["rgb_h"].copy_(rgb)
            rgb = s["rgb_h"]
        if lab is not None:
            lab = self._host(lab)
            if not lab.is_pinned():
                s["lab_h"].copy_(lab)
                lab = s["lab_h"]
        cs = self.copy_stream
        if s["free"] is not None:
            cs.wait_event(s["free"])           # the consumer's kernels that read this slot's outputs have been enqueued and finished
        with torch.cuda.stream(cs):
            s["rgb_d"].copy_(rgb, non_blocking=True)
            if lab is not None:
                s["lab_d"].copy_(lab, non_blocking=True)
            if self.draw_fn is not None:           # one launch replaces the resample, image_to_input and label_nearest launches
                self._crop(s, [s["rgb_d"][b].data_ptr() for b in range(self.prep.B)],
                           [s["lab_d"][b].data_ptr() if lab is not None else None for b in range(self.prep.B)], lab is not None, meta, cs)
            else:
                mirror = self.mirror_fn(self.prep.B) if self.mirror_fn is not None else False
                self.prep.run(s["rgb_d"], s["x"], s["lab_d"] if lab is not None else None, s["lab"] if lab is not None else None,
                              mirror=mirror, stream=cs.cuda_stream)
            self._mix(s, lab is not None, cs)
            self._photo(s, cs)
            self._mask(s, cs)
            s["ready"].record(cs)
        s["meta"], s["has_lab"], s["used"] = meta, lab is not None, True
        self.filled += 1

    def _crop(self, s, img_ptrs, lab_ptrs, has_lab, meta, cs):
        """Scale-crop mode: the batch out of B source frames on the device, on the copy stream -- one simt_scale_crop at the window drawn,
        or, with rare-class crops, counts, pick and simt_scale_crop_win over the K windows drawn."""
        if self.rare is None:
            return self.prep.scale_crop_batch(img_ptrs, lab_ptrs, self.draw_fn(self.prep.B), s["x"], s["lab"] if has_lab else None, cs.cuda_stream)
        if not has_lab:
            raise ValueError("rare-class crops: a batch without labels has no class to count")
        self.prep.rare_crop_batch(img_ptrs, lab_ptrs, self.draw_fn(self.prep.B), meta[2], self.rare[1], s["x"], s["lab"], s["parts"], s["win"],
                                  cs.cuda_stream)

    def _mix(self, s, has_lab, cs):
        """Class-mix mode: the slot's finished batch x / lab -> xm / labm, on the copy stream, behind the launches that made it."""
        if self.mix_fn is None:
            return
        if not has_lab:
            raise ValueError("--class-mix: a batch without labels cannot be mixed")
        self.prep.class_mix_batch(s["x"], s["lab"], self.mix_fn(self.prep.B), s["xm"], s["labm"], cs.cuda_stream, item_out=s.get("item"))

    def _photo(self, s, cs):
        """Photometric mode: the slot's finished batch -- xm when it was mixed, else x -> xp, on the copy stream, behind `_mix`."""
        if self.photo_fn is None:
            return
        src = s["xm"] if self.mix_fn is not None else s["x"]
        self.prep.photometric_batch(src, self.photo_fn(self.prep.B), s["xp"], cs.cuda_stream)

    def _mask(self, s, cs):
        """Patch-mask mode: the buffer about to be handed out -- xp, else xm, else x -- gets its patches blanked in place, on the copy stream,
        behind `_photo` (MIC masks the augmented image).  Where that buffer is also the weak view (teacher_view with neither mix nor
        photometric step) x stays whole and the masked copy goes to xk."""
        if self.mask_fn is None:
            return
        src = s["xp"] if self.photo_fn is not None else s["xm"] if self.mix_fn is not None else s["x"]
        self.prep.patch_mask_batch(src, self.mask_fn(self.prep.B), s["xk"] if self.mask_out_of_place else src, cs.cuda_stream)

    def _fill_cached(self, s, rgb, lab, meta):
        """With a cache the source yields only the batch's MISSES: rgb [M,Hs,Ws,3] (None when M = 0), lab likewise, and
        meta = (meta, plan) with plan[b] = (cache slot | None, index into the misses | None) per item of the batch.  Upload the
        misses, resize them straight into their slots (an item the cache has no room for: into this prefetcher slot's transient
        ones), then ONE gather over the batch's B slots.  Slot write and gather are both on the copy stream: no other ordering edge."""
        meta, plan = meta
        prep, cache, cs = self.prep, self.cache, self.copy_stream
        has_lab = prep.with_label
        M = 0 if rgb is None else len(rgb)
        if M:
            s["rgb_h"][:M].copy_(self._host(rgb))
            if has_lab:
                s["lab_h"][:M].copy_(self._host(lab))
        img_ptrs, lab_ptrs, dests, spilled = [], [], [None] * M, 0
        for slot, m in plan:
            if slot is not None:
                iv, lv = cache.img_view(slot), (cache.lab_view(slot) if has_lab else None)
            else:
                o = spilled * cache.img_stride
                iv = s["sp_img"][o:o + cache.img_bytes]
                lv = s["sp_lab"][spilled * cache.lab_stride:spilled * cache.lab_stride + cache.lab_bytes] if has_lab else None
                spilled += 1
            if m is not None:
                dests[m] = (iv, lv)
            img_ptrs.append(iv.data_ptr())
            lab_ptrs.append(lv.data_ptr() if has_lab else None)
        if s["free"] is not None:
            cs.wait_event(s["free"])
        with torch.cuda.stream(cs):
            if M:
                s["rgb_d"][:M].copy_(s["rgb_h"][:M], non_blocking=True)
                if has_lab:
                    s["lab_d"][:M].copy_(s["lab_h"][:M], non_blocking=True)
                if self.draw_fn is not None:       # the cache holds the ORIGINAL frames: a miss goes into its slot as it is
                    for m, (iv, lv) in enumerate(dests):
                        iv.copy_(s["rgb_d"][m].reshape(-1), non_blocking=True)
                        if has_lab:
                            lv.copy_(s["lab_d"][m].reshape(-1), non_blocking=True)
                else:
                    prep.resize_into(s["rgb_d"][:M], s["lab_d"][:M] if has_lab else None, dests, cs.cuda_stream)
            if self.draw_fn is not None:
                self._crop(s, img_ptrs, lab_ptrs, has_lab, meta, cs)
            else:
                mirror = self.mirror_fn(prep.B) if self.mirror_fn is not None else False
                prep.gather(img_ptrs, lab_ptrs, mirror, s["x"], s["lab"] if has_lab else None, cs.cuda_stream)
            self._mix(s, has_lab, cs)
            self._photo(s, cs)
            self._mask(s, cs)
            s["ready"].record(cs)
        s["meta"], s["has_lab"], s["used"] = meta, has_lab, True
        self.filled += 1

    def __iter__(self):
        return self

    def __next__(self):
        if self.filled == 0:
            raise StopIteration
        i = self.head
        s = self.slots[i]
        cur = torch.cuda.current_stream(self.prep.dev)
        cur.wait_event(s["ready"])
        if self.mix_fn is not None:
            out = (s["xm"], s["labm"], s["meta"])
        else:
            out = (s["x"], s["lab"] if s["has_lab"] else None, s["meta"])
        if self.photo_fn is not None:      # the label that would have been handed out anyway
            out = (s["xp"], out[1], out[2])
        if self.mask_out_of_place:         # (every other mask ran in place in the buffer `out` names)
            out = (s["xk"], out[1], out[2])
        if self.teacher_view:              # the weak view: what this slot would have handed out without the mix, the photometric step and the mask
            out = out + (s["x"], s.get("item"))
        self.last_win = s.get("win")
        self.filled -= 1
        self.calls += 1
        self.head = (i + 1) % len(self.slots)
        # release + refill the slot handed out `hold` calls ago: the consumer no longer holds it, and everything it enqueued on this
        # stream so far (the step that read it) precedes the event the copy stream will wait for
        prev = (i - self.hold) % len(self.slots)
        if self.calls > self.hold and self._handed(prev):
            ev = torch.cuda.Event()
            ev.record(cur)
            self.slots[prev]["free"] = ev
            self._fill(prev)
        return out

    def _handed(self, j):
        # slot j was handed out and not refilled yet  <=>  it is not among the `filled` slots starting at head
        n = len(self.slots)
        return all(((self.head + k) % n) != j for k in range(self.filled))


def loader_position(n_items, batch_size, rank, world, start_batch):
    """Where batch number `start_batch` (counted from the loader's first batch, over every epoch) lies: -> (epoch, batch within the
    epoch, batches per epoch).  A rank's shard is every `world`-th item of the epoch's order from `rank` on; its incomplete last batch is
    dropped.  Pure arithmetic (GpuLoader(start_batch=...), tests/test_resume_cpu.py)."""
    shard = len(range(rank, n_items, world))
    per_epoch = shard // batch_size
    if start_batch < 0:
        raise ValueError(f"start_batch {start_batch} is negative")
    if per_epoch == 0:
        if start_batch:
            raise ValueError(f"start_batch {start_batch}: the shard of rank {rank} ({shard} items) holds no batch of {batch_size}")
        return 0, 0, 0
    return start_batch // per_epoch, start_batch % per_epoch, per_epoch


def skip_mirror_draws(rng, batch_size, n_batches):
    """Advance the loader's mirror generator by the draws `n_batches` batches make: one `integers(0, 2, batch_size)` per batch, in batch
    order (GpuLoader.__iter__'s mirror_fn)."""
    for _ in range(n_batches):
        rng.integers(0, 2, batch_size)
    return rng


class GpuLoader:
    """DataLoader(dataset, batch_size, shuffle, num_workers, pin_memory=True) of tools/trainV2_simt.py:287-294, feeding the GPU:
    `num_workers` host threads read + decode PNGs (Pillow releases the GIL while decoding), batches of decoded frames are uploaded
    and transformed by DevicePrefetcher.  Yields (images f32 [B,3,h,w], labels i64 [B,h,w] | None, sizes, names) like the
    reference's batches (`images, labels, _, _ = batch`), already on the device.  Incomplete last batches are dropped (the
    reference repeats the list to max_iters, so it never sees one).

    cache: a simt_amd.data.cache.DatasetCache for the dataset's crop, or None.  With one, only an item's first sighting is decoded,
    uploaded and resized (into its cache slot); every batch is then one gather over B slots.  Order, sharding, the dropped batch and
    the mirror draws are those of the uncached loader: the batches are bit-identical.  on_epoch(epoch, hits, misses, cache bytes) is
    called when an epoch's last batch has been planned (the prefetcher runs a few batches ahead of the consumer).

    start_batch = n: the loader yields exactly what the default loader yields from its n-th batch on (a resumed run): it starts inside
    epoch n // batches-per-epoch of `_order`, the mirror generator has made the n skipped batches' draws, and no skipped item is
    decoded.  A cache starts empty and refills; the batches are the same.

    dataset.scale_crop = decimal scale choices (cityscapesPseudo(scale_crop=...), --scale-crop) turns on random scale + crop
    (simt_amd/data/scale_crop.py): per batch the generator draws, after the mirror flags, a choice and a window origin per item, and ONE
    simt_scale_crop launch makes the batch from the decoded frames.  A cache then holds the ORIGINAL frames (DatasetCache((Ws, Hs))).
    Cached and uncached batches are bit-identical and start_batch skips the same draws.  Without it not one draw changes.

    dataset.class_mix = (n_classes, prob) (cityscapesPseudo(class_mix=...), --class-mix) turns on ClassMix (simt_amd/data/class_mix.py):
    every finished batch -- plain, scale-cropped, cached or not -- is mixed on the copy stream, item i with item (i + 1) % B, before it
    is handed out.  Its draws come from a generator of their own, class_mix.generator(seed, rank): the batch underneath is the batch
    of the loader without the flag, bit for bit, and start_batch skips the mix draws too.

    dataset.photometric = (S | None, P | None) (cityscapesPseudo(photometric=...), --colour-jitter / --gaussian-blur) turns on colour
    jitter and Gaussian blur (simt_amd/data/photometric.py): the finished batch -- after the mix, when there is one -- is jittered and
    blurred on the copy stream into a buffer of its own; labels are not touched (a dataset without labels works).  Its draws come from
    photometric.generator(seed, rank): the batch underneath is the batch of the loader without the flags, bit for bit, and start_batch
    skips these draws too.

    dataset.patch_mask = (patch, ratio) (cityscapesPseudo(patch_mask=...), --mask-patches / --mask-patch-size) turns on MIC patch masking
    (simt_amd/data/patch_mask.py): the batch about to be handed out -- after the mix and the photometric step, when there are any -- has
    every patch of its patch x patch grid blanked to +0.0f (the mean colour) with probability `ratio`, by one launch per 16 items on the
    copy stream; labels are not touched.  Its draws come from patch_mask.generator(seed, rank): the batch underneath is the batch of the
    loader without the flag, bit for bit, and start_batch skips these draws too.

    dataset.teacher_view = True (--weak-teacher) needs one of the three above and hands out both views: (strong image, labels, sizes,
    names, weak image, item map | None) -- the weak image is the batch of the loader without class-mix, photometric and patch mask, bit for
    bit, the item map ([B,h,w] u8, None without class-mix) names the item each pixel of the strong view was taken from.  Not one draw changes.

    dataset.rare_class = a rare_class.RareClass (GTA5DataSet(rare_class=...), --rare-class-sampling) turns on DAFormer's rare-class
    sampling (simt_amd/data/rare_class.py).  `_order` is not used: batch n's items are the n-th rare_class.draw_batch of
    rare_class.generator(seed, rank) -- a class by softmax((1 - f) / T), then a frame that holds it -- so every rank draws its own batches
    and there is no shard; an "epoch" keeps its length (loader_position) for start_batch, on_epoch and epochs=, the decode look-ahead and
    the cache work unchanged (a repeated item is a hit).  With dataset.scale_crop the loader's generator draws K candidate windows per item
    (scale_crop.draw_batch_candidates) and the copy stream counts the item's class in each, picks the first that holds more than
    min_count pixels (else the last) and crops there (InputPrep.rare_crop_batch): nothing is read back; last_windows() names the slot's
    `win` words for logging.  Without scale_crop the sampler is all there is.  start_batch skips both generators' draws."""

    def __init__(self, dataset, batch_size, shuffle=True, num_workers=4, device="cuda:0", seed=1234, rank=0, world=1, epochs=None,
                 hold=1, cache=None, on_epoch=None, start_batch=0):
        self.ds, self.B, self.shuffle, self.workers = dataset, batch_size, shuffle, max(1, num_workers)
        self.hold = hold            # batches the consumer keeps at once (= --iter-size): see DevicePrefetcher
        self.dev, self.seed, self.rank, self.world, self.epochs = torch.device(device), seed, rank, world, epochs
        self._prep = None
        self.cache, self.on_epoch = cache, on_epoch
        self.scale_crop = getattr(dataset, "scale_crop", None)
        if self.scale_crop is not None:
            self.scale_crop = sc.parse_choices(self.scale_crop)
        self.class_mix = getattr(dataset, "class_mix", None)
        self._mix_rng = None
        if self.class_mix is not None:
            self.class_mix = cm.parse(self.class_mix[1], self.class_mix[0], batch_size)
            self._mix_rng = cm.skip_draws(cm.generator(seed, rank), batch_size, int(start_batch), self.class_mix[0])
        self.photometric = getattr(dataset, "photometric", None)
        self._photo_rng = None
        if self.photometric is not None:
            self.photometric = ph.parse(*self.photometric)      # (S, P) validated like the flags: S in (0, 0.5], P in (0, 1]
            if self.photometric is None:
                raise ValueError("dataset.photometric is (None, None): pass None for no photometric augmentation")
            self._photo_rng = ph.skip_draws(ph.generator(seed, rank), batch_size, int(start_batch))
        self.patch_mask = getattr(dataset, "patch_mask", None)
        self._mask_rng = None
        if self.patch_mask is not None:
            self.patch_mask = pm.parse(self.patch_mask[1], self.patch_mask[0], tuple(dataset.crop_size))      # (patch, ratio, gh, gw)
            self._mask_rng = pm.skip_draws(pm.generator(seed, rank), batch_size, int(start_batch), *self.patch_mask[2:])
        self.teacher_view = bool(getattr(dataset, "teacher_view", False))
        if self.teacher_view and self.class_mix is None and self.photometric is None and self.patch_mask is None:
            raise ValueError("dataset.teacher_view needs dataset.class_mix, dataset.photometric or dataset.patch_mask (--weak-teacher needs "
                             "--class-mix, --colour-jitter or --gaussian-blur, or --mask-patches): without them the two views are the same batch")
        self.rare_class = getattr(dataset, "rare_class", None)
        self._rcs_rng, self._pf = None, None
        if self.rare_class is not None:
            if self.rare_class.counts.shape[0] != len(dataset):
                raise ValueError(f"rare-class statistics of {self.rare_class.counts.shape[0]} items for a dataset of {len(dataset)}")
            self._rcs_rng = rc.skip_draws(rc.generator(seed, rank), batch_size, int(start_batch))
        self._src_hw = None         # the geometry of the first frame decoded: every other one must have it
        if cache is not None and self.scale_crop is None:
            assert (cache.w, cache.h) == tuple(dataset.crop_size), "the cache holds frames of ONE crop"
        self._rng = np.random.default_rng(seed + 7919 * rank)
        self._lock = threading.Lock()
        self.start_batch = int(start_batch)
        self._epoch0, self._batch0, _ = loader_position(len(dataset), batch_size, rank, world, self.start_batch)
        if self.start_batch and self.scale_crop is not None:
            sc.skip_scale_crop_draws(self._rng, batch_size, self.start_batch, len(self.scale_crop), bool(getattr(dataset, "is_mirror", False)),
                                     candidates=None if self.rare_class is None else self.rare_class.K)
        elif self.start_batch and getattr(dataset, "is_mirror", False):
            skip_mirror_draws(self._rng, batch_size, self.start_batch)

    def _same_geometry(self, items, ids):
        """All items of a run share one source geometry: a frame of another size raises, with its path."""
        for it, i in zip(items, ids):
            with self._lock:
                if self._src_hw is None:
                    self._src_hw = it[0].shape[:2]
            if it[0].shape[:2] != self._src_hw:
                raise ValueError(f"{self.ds.files[i]['img']}: the frame is {it[0].shape[1]} x {it[0].shape[0]}, the frames of this run are "
                                 f"{self._src_hw[1]} x {self._src_hw[0]} (one source geometry per run)")

    def _order(self, epoch):
        n = len(self.ds)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + epoch)
            idx = torch.randperm(n, generator=g).tolist()
        else:
            idx = list(range(n))
        return idx[self.rank::self.world]               # data parallel: disjoint strided shards of one global order

    def _epoch_items(self, epoch, b0):
        """-> (item indices, classes | None) of epoch `epoch`, batch b at [b * B, (b + 1) * B); the batches before b0 are never read.
        With rare-class sampling the epoch's batches from b0 on are the sampler's next draws (None stands for the skipped ones)."""
        if self.rare_class is None:
            return self._order(epoch), None
        nb = loader_position(len(self.ds), self.B, self.rank, self.world, 0)[2]
        idx, cls = [None] * (b0 * self.B), [None] * (b0 * self.B)
        for _ in range(b0, nb):
            c, i = rc.draw_batch(self._rcs_rng, self.B, self.rare_class.cdf, self.rare_class.lists)
            idx += i
            cls += c
        return idx, cls

    def _meta(self, sizes, names, cls, b):
        return (sizes, names) if cls is None else (sizes, names, cls[b * self.B:(b + 1) * self.B])

    def _host_batches(self):
        epoch, b0 = self._epoch0, self._batch0         # (start_batch: the first epoch begins at its batch b0)
        with ThreadPoolExecutor(self.workers) as pool:
            while self.epochs is None or epoch < self.epochs:
                idx, cls = self._epoch_items(epoch, b0)
                nb = len(idx) // self.B
                pending = [pool.map(self.ds.decode, idx[b * self.B:(b + 1) * self.B]) for b in range(b0, min(b0 + 2, nb))]
                for b in range(b0, nb):
                    items = list(pending.pop(0))
                    self._same_geometry(items, idx[b * self.B:(b + 1) * self.B])
                    if b + 2 < nb:
                        pending.append(pool.map(self.ds.decode, idx[(b + 2) * self.B:(b + 3) * self.B]))
                    rgb = np.stack([it[0] for it in items])
                    lab = np.stack([it[1] for it in items]) if items[0][1] is not None else None
                    sizes = np.stack([np.array([self.ds.crop_size[1], self.ds.crop_size[0], 3]) for _ in items])
                    yield rgb, lab, self._meta(sizes, [it[2] for it in items], cls, b)
                epoch, b0 = epoch + 1, 0

    def _host_batches_cached(self):
        """_host_batches with a cache: same epochs, order and batches, but only the misses are decoded.  Yields (rgb of the misses
        [M,Hs,Ws,3] | None, labels likewise, ((sizes, names), plan)); plan[b] = (cache slot | None, index into the misses | None).
        A slot is reserved when the item's decode is submitted, so a later sighting -- in the same batch, or in one of the batches
        planned ahead -- is a hit; batches reach the copy stream in this order, so the slot's write precedes every gather from it."""
        cache, ds = self.cache, self.ds
        epoch, b0 = self._epoch0, self._batch0

        def plan(pool, ids):
            out = []
            for i in ids:
                key = ds.cache_key(i)
                slot = cache.lookup(key)
                if slot is not None:
                    cache.hits += 1
                    out.append((slot, None, i))
                else:
                    cache.misses += 1
                    out.append((cache.reserve(key), pool.submit(ds.decode, i), i))
            return out

        with ThreadPoolExecutor(self.workers) as pool:
            while self.epochs is None or epoch < self.epochs:
                idx, cls = self._epoch_items(epoch, b0)
                nb = len(idx) // self.B
                h0, m0 = cache.hits, cache.misses
                pending = [plan(pool, idx[b * self.B:(b + 1) * self.B]) for b in range(b0, min(b0 + 2, nb))]
                for b in range(b0, nb):
                    entries = pending.pop(0)
                    if b + 2 < nb:
                        pending.append(plan(pool, idx[(b + 2) * self.B:(b + 3) * self.B]))
                    items = [fut.result() for (_slot, fut, _i) in entries if fut is not None]
                    self._same_geometry(items, [i for (_slot, fut, i) in entries if fut is not None])
                    rgb = np.stack([it[0] for it in items]) if items else None
                    lab = np.stack([it[1] for it in items]) if items and items[0][1] is not None else None
                    sizes = np.stack([np.array([ds.crop_size[1], ds.crop_size[0], 3]) for _ in entries])
                    m, where = 0, []
                    for slot, fut, _i in entries:
                        where.append((slot, m if fut is not None else None))
                        m += fut is not None
                    yield rgb, lab, (self._meta(sizes, [ds.files[i]["name"] for (_s, _f, i) in entries], cls, b), where)
                if self.on_epoch is not None:
                    self.on_epoch(epoch, cache.hits - h0, cache.misses - m0, cache.bytes)
                epoch, b0 = epoch + 1, 0

    def __iter__(self):
        first = None
        gen = self._host_batches() if self.cache is None else self._host_batches_cached()
        try:
            first = next(gen)
        except StopIteration:
            return iter(())
        Hs, Ws = first[0].shape[1:3]
        assert self.cache is None or self.cache.with_label or first[1] is None, "the dataset has labels, the cache no label slab"
        if self.class_mix is not None and first[1] is None:
            raise ValueError("--class-mix: the dataset yields no labels, and the classes to paste are read from the partner's label")
        self._prep = InputPrep(self.B, (Hs, Ws), tuple(self.ds.crop_size), self.dev, mean=self.ds.mean, with_label=first[1] is not None,
                               scale_crop=self.scale_crop, class_mix=self.class_mix, photometric=self.photometric,
                               patch_mask=None if self.patch_mask is None else self.patch_mask[:2])
        if self.scale_crop is not None and self.cache is not None:
            assert (self.cache.w, self.cache.h) == (Ws, Hs), "with scale-crop the cache holds the ORIGINAL frames: DatasetCache((Ws, Hs))"

        def chain():
            yield first
            yield from gen
        # `flip = np.random.choice(2) * 2 - 1` per item (cityscapes_dataset.py:109)
        mirror_fn = (lambda n: (self._rng.integers(0, 2, n) == 0).tolist()) if getattr(self.ds, "is_mirror", False) else None
        draw_fn = None
        if self.scale_crop is not None:
            mirror_on = bool(getattr(self.ds, "is_mirror", False))
            draw_fn = lambda n: sc.draw_batch(self._rng, n, self.scale_crop, tuple(self.ds.crop_size), mirror_on)
            if self.rare_class is not None:
                draw_fn = lambda n: sc.draw_batch_candidates(self._rng, n, self.rare_class.K, self.scale_crop, tuple(self.ds.crop_size), mirror_on)
        mix_fn = None
        if self.class_mix is not None:
            mix_fn = lambda n: cm.draw_batch(self._mix_rng, n, *self.class_mix)
        photo_fn = None
        if self.photometric is not None:
            photo_fn = lambda n: ph.draw_batch(self._photo_rng, n, self.photometric)
        mask_fn = None
        if self.patch_mask is not None:
            mask_fn = lambda n: pm.draw_batch(self._mask_rng, n, self.patch_mask[2], self.patch_mask[3], self.patch_mask[1])
        pf = DevicePrefetcher(chain(), self._prep, mirror_fn=mirror_fn, hold=self.hold, cache=self.cache, draw_fn=draw_fn, mix_fn=mix_fn,
                              photo_fn=photo_fn, teacher_view=self.teacher_view, mask_fn=mask_fn,
                              rare=None if self.rare_class is None or draw_fn is None else (self.rare_class.K, self.rare_class.min_count))
        self._pf = pf
        if self.teacher_view:
            return ((x, lab, meta[0], meta[1], xw, item) for (x, lab, meta, xw, item) in pf)
        return ((x, lab, meta[0], meta[1]) for (x, lab, meta) in pf)

    def last_windows(self):
        """Rare-class crops: the `win` words (int32 [B, 4] on the device: choice, ox, oy, count) of the batch handed out last, valid as long
        as that batch; None without them.  For logging: reading it synchronises, so read it where the consumer synchronises anyway."""
        return None if self._pf is None else self._pf.last_win
