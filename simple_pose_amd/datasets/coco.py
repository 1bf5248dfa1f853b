"""Input contract of the hot path: the normalisation half of the reference's `MSCOCO.collate_fn`
(`datasets/coco.py:124-148`), on the GPU; and `GpuAugmentLoader`, the training loader that replaces `MSCOCO`'s per-sample
transform + `collate_fn` with one batched GPU transform (`commons.transforms.RefineSimpleTransform.batch`).  COCO parsing stays out
of scope.  A sample carries either its decoded image on the device (`.img`) or the bytes of its baseline or progressive JPEG file (`.jpeg`), which
the loader decodes on the device, a batch's files in one call (`datasets.jpeg.JpegDecoder`: libjpeg-turbo's pixels bit for bit, EXIF
orientation not applied)."""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np
import torch

from .. import _lib
from ..sharding import rank_indices

rgb_mean = [0.485, 0.456, 0.406]   # datasets/coco.py:10 (std is NOT applied: coco.py:134-136)


def normalize_crops(img_u8_bhwc_bgr: torch.Tensor) -> torch.Tensor:
    """uint8 [B,H,W,3] BGR crops on the GPU -> fp32 [B,3,H,W] RGB, `x / 255 - mean` (coco.py:136), the tensor `model(x)` takes.
    Ships 1 byte per value over PCIe instead of 4 and removes the per-sample numpy work from the dataloader."""
    t = img_u8_bhwc_bgr
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[-1] == 3):
        raise _lib.HipLibraryError("normalize_crops: expected a CUDA uint8 tensor [B,H,W,3]")
    t = t.contiguous()
    B, H, W, _ = t.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=t.device)
    if B == 0:
        return out
    mean = (ctypes.c_float * 3)(*rgb_mean)
    _lib.check(_lib.lib().sp_u8hwc_bgr_to_nchw_f32(_lib.ptr(t), _lib.ptr(out), B, H, W, mean, _lib.current_stream()),
               "sp_u8hwc_bgr_to_nchw_f32")
    return out


COCO_JOINT_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]   # left/right key points (coco.py:25)


def _img_id(sample) -> int:
    iid = getattr(sample, "img_id", None)
    if iid is not None:
        return int(iid)
    return int(os.path.splitext(os.path.basename(sample.img_path))[0])      # what collate_fn derives (coco.py:132)


class _DecodedSample:
    """A `.jpeg` sample with the image the loader decoded for this batch; every other attribute is the sample's own."""
    __slots__ = ("_sample", "img")

    def __init__(self, sample, img):
        self._sample, self.img = sample, img

    def __getattr__(self, name):
        return getattr(self._sample, name)


class GpuAugmentLoader:
    """Training batches straight from decoded images (or JPEG file bytes) in HBM: `MSCOCO(augment=...)` + `DistributedSampler(shuffle=True, seed)` +
    `DataLoader(batch_size, drop_last=True, collate_fn=MSCOCO.collate_fn)` of the reference, as one iterable that
    `DDPProcessor(train_loader=...)` takes.  Yields (input fp32 [B,3,256,192], heat_maps fp32 [B,J,64,48], masks fp32 [B,J],
    trans_inv fp32 [B,2,3], img_ids).

    `samples`: objects with `.img` (CUDA uint8 [H,W,3] BGR) or `.jpeg` (the bytes of a baseline or progressive JPEG file; decoded on `device`, one
    `JpegDecoder.decode` call per batch, just before the transform - a batch may mix both kinds), `.box` (x1, y1, x2, y2), `.joints` ([J,3] float32, host), `.shape`
    (w, h) and `.img_id` or `.img_path`.  The epoch's order is DistributedSampler's (torch.randperm under a generator seeded with
    seed + epoch, padded by wrap-around, every `world`-th index from `rank`, whole batches only); the augmentation draws of an
    epoch come from one (random.Random, np.random.RandomState) pair seeded by (seed, epoch, rank).  A completed pass advances the epoch by
    one (DDPProcessor calls no set_epoch), so pass e sees what `set_epoch(e)` gives.  `augment=False`: the
    reference's validation transform (no flip, scale 1, rotation 0, no random crop)."""

    def __init__(self, samples, batch_size: int, rank: int = 0, world: int = 1, augment: bool = True, seed: int = 0,
                 input_shape=(192, 256), device=None):
        from ..commons.transforms import RefineSimpleTransform
        self.device, self._jpeg = device, None      # device of the JPEG decoder (default: the current device); made on first use
        self.samples, self.batch_size, self.rank, self.world, self.seed = list(samples), int(batch_size), int(rank), int(world), int(seed)
        self.epoch = 0
        out_shape = (input_shape[0] // 4, input_shape[1] // 4)
        if augment:
            self.transform = RefineSimpleTransform(COCO_JOINT_PAIRS, input_shape, out_shape, scale=(0.7, 1.3), ratio=(-40, 40), rand_crop=True)
        else:
            self.transform = RefineSimpleTransform(None, input_shape, out_shape, scale=(1.0, 1.0), ratio=(0, 0), rand_crop=False)

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def indices(self):
        """This rank's sample indices of the current epoch, in order (whole batches only)."""
        n = len(self.samples)
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        perm = torch.randperm(n, generator=g).tolist()
        return [perm[i] for i in rank_indices(n, self.rank, self.world, batch_size=self.batch_size)]

    def rng(self):
        """The (random.Random, np.random.RandomState) pair of this (seed, epoch, rank)."""
        s = np.random.SeedSequence([self.seed, self.epoch, self.rank]).generate_state(2)
        return random.Random(int(s[0])), np.random.RandomState(int(s[1]))

    def __len__(self):
        return len(self.indices()) // self.batch_size

    def _decoded(self, batch):
        """The batch with every `.jpeg` sample's image decoded on the device (one call); `.img` samples pass through untouched."""
        todo = []
        for i, s in enumerate(batch):
            if getattr(s, "img", None) is not None:
                continue
            if not isinstance(getattr(s, "jpeg", None), (bytes, bytearray, memoryview)):
                raise _lib.HipLibraryError(f"sample {i} of the batch has neither .img (a CUDA uint8 [H,W,3] image) nor .jpeg (the bytes of a JPEG file)")
            todo.append(i)
        if not todo:
            return batch
        if self._jpeg is None:
            from .jpeg import JpegDecoder
            self._jpeg = JpegDecoder(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
        imgs = self._jpeg.decode([batch[i].jpeg for i in todo])
        batch = list(batch)
        for i, img in zip(todo, imgs):
            batch[i] = _DecodedSample(batch[i], img)
        return batch

    def __iter__(self):
        idx, rng = self.indices(), self.rng()
        for b0 in range(0, len(idx), self.batch_size):
            batch = self._decoded([self.samples[i] for i in idx[b0:b0 + self.batch_size]])
            x, hm, mask, tinv = self.transform.batch(batch, rng)
            yield x, hm, mask, tinv, [_img_id(s) for s in batch]
        self.epoch += 1                     # a full pass moves on: epoch e sees what set_epoch(e) gives, also under DDPProcessor
