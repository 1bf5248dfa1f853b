"""Heat-map target encoders, MI355X-native: drop-in for `get_heat_map` of the reference's
`commons/transforms.py` (RefineSimpleTransform :167-191 - the one the dataset uses - and BasicSimpleTransform :80-116).

The reference encodes one sample at a time in numpy inside a dataloader worker (3.7 ms / image).  Here the same
function also takes a whole batch `[B,J,3]` that already lives on the GPU and returns device tensors (one launch);
a numpy `[J,3]` argument keeps the reference's numpy-in / numpy-out contract (upload, launch, download).

`RefineSimpleTransform.batch` is the training-side transform itself (box jitter / crop, scale, rotation, flip, warp, encode) plus
the collate normalisation, for a batch of samples from many source images.
"""
from __future__ import annotations

import ctypes
import random
from typing import NamedTuple, Sequence

import numpy as np
import torch

from .. import _lib
from .joint_utils import affine_transform_batch, box_crop, box_to_center_scale, flip_joints, get_affine_transform_batch

rgb_mean = [0.485, 0.456, 0.406]   # datasets/coco.py:10 (the collate normalisation: x / 255 - mean, no std)


def _run(fn_name, joints, sigma, shape, stride=None):
    is_np = isinstance(joints, np.ndarray)
    j = torch.from_numpy(np.ascontiguousarray(joints, dtype=np.float32)).cuda() if is_np else joints
    j = _lib.require_cuda_f32(j, "joints")
    single = j.dim() == 2
    if single:
        j = j[None]
    if j.dim() != 3 or j.shape[-1] != 3:
        raise ValueError(f"joints must be [J,3] or [B,J,3], got {tuple(joints.shape)}")
    j = j.contiguous()
    B, J, _ = j.shape
    W, H = int(shape[0]), int(shape[1])  # the reference passes shape=(w, h) and returns [J, h, w]
    targets = torch.empty((B, J, H, W), dtype=torch.float32, device=j.device)
    weights = torch.empty((B, J), dtype=torch.float32, device=j.device)
    lib = _lib.lib()
    if B == 0:
        rc = 0                          # empty batch: empty targets / weights, nothing to launch
    elif stride is None:
        rc = lib.sp_encode_gauss_refine(_lib.ptr(j), B, J, H, W, float(sigma), _lib.ptr(targets), _lib.ptr(weights),
                                        _lib.current_stream())
    else:
        rc = lib.sp_encode_gauss_basic(_lib.ptr(j), B, J, H, W, float(sigma), int(stride), _lib.ptr(targets),
                                       _lib.ptr(weights), _lib.current_stream())
    _lib.check(rc, fn_name)
    if single:
        targets, weights = targets[0], weights[0]
    if is_np:
        return targets.cpu().numpy(), weights.cpu().numpy()
    return targets, weights


class BasicSimpleTransform(object):
    @staticmethod
    def get_heat_map(joints, sigma=2.0, shape=(48, 64), stride=4):
        """transforms.py:80-116: joints in INPUT px; centre quantised to int(j/stride+0.5); 13x13 truncated patch."""
        return _run("sp_encode_gauss_basic", joints, sigma, shape, stride)


class SampleGeometry(NamedTuple):
    """Host half of one augmented batch (B samples, J joints): what `RefineSimpleTransform.__call__` computes per sample besides the
    pixels and the heat maps."""
    m_fwd: np.ndarray         # [B,2,3] float64: image -> input crop (img_trans), for the flipped image where flip is set
    flip: np.ndarray          # [B] int32: 1 = the sample is warped from np.fliplr(img)
    trans_inv: np.ndarray     # [B,2,3] float64: heat-map px -> image px (joint_trans_inv)
    joints: np.ndarray        # [B,J,3] float32: joints in input-crop px (joint_info.joints after __call__)
    hm_joints: np.ndarray     # [B,J,3] float32: joints in heat-map px (what get_heat_map encodes)
    boxes: np.ndarray         # [B,4] float32: center_scale_to_box(center, scale) (joint_info.box after __call__)


class RefineSimpleTransform(object):
    """The reference's training transform (commons/transforms.py:147-223) + `MSCOCO.collate_fn` (datasets/coco.py:124-148), batched.

    `batch(samples)` draws every sample's augmentation on the host in the reference's order and from the reference's sources, builds the
    same matrices, warps all samples (each from its own source image, horizontal flip read mirrored) straight into the collate's fp32
    input tensor in one launch per 32 samples, and encodes the heat maps with the refine encoder.  There is no per-sample GPU
    `__call__`: forked DataLoader workers cannot use the GPU, so the batched path replaces transform + collate_fn."""

    def __init__(self, joint_pairs=None, input_shape=(192, 256), output_shape=(48, 64), scale=(0.7, 1.3), ratio=(-40, 40),
                 rand_crop=True):
        self.input_shape = input_shape
        self.output_shape = output_shape
        self.joint_pairs = joint_pairs
        self.w_h_ratio = self.input_shape[0] / self.input_shape[1]
        self.scale = scale
        self.ratio = ratio
        self.rand_crop = rand_crop

    @staticmethod
    def get_heat_map(joints, sigma=2.0, shape=(48, 64)):
        """transforms.py:167-191: joints in heat-map px (un-quantised); full-map Gaussian; weight 0 if the 3-sigma box
        misses the map."""
        return _run("sp_encode_gauss_refine", joints, sigma, shape)

    def geometry(self, samples: Sequence, rng=None) -> SampleGeometry:
        """The host half of `batch`: per sample, in the reference's order, box_crop (if rand_crop) -> centre/scale -> scale draw ->
        rotation draw -> flip draw (only with joint_pairs) -> the two affine maps; then the joints through both maps, vectorised over
        the batch (element-wise float64, so every joint has the bits of the per-sample computation).  `rng`: (random.Random,
        np.random.RandomState), default the global modules.  Samples need `.box`, `.joints` [J,3], `.shape` (w, h) and `.img`
        (only its width is read, for the joint flip)."""
        py, npr = rng if rng is not None else (random, np.random)
        n = len(samples)
        centers, scales, rots = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n)
        flip = np.zeros(n, np.int32)
        gts = []
        for i, s in enumerate(samples):
            gt = np.array(s.joints, np.float32, copy=True)
            img_w, img_h = s.shape
            bbox = box_crop(s.box, img_w, img_h, (py, npr)) if self.rand_crop else s.box
            x1, y1, x2, y2 = bbox[0], bbox[1], bbox[2], bbox[3]
            center, scale = box_to_center_scale(x1, y1, x2 - x1, y2 - y1, self.w_h_ratio)
            scales[i] = scale * npr.uniform(self.scale[0], self.scale[1])
            rots[i] = npr.uniform(self.ratio[0], self.ratio[1])
            if self.joint_pairs is not None and npr.uniform() < 0.5:
                flip[i] = 1
                gt = flip_joints(gt, s.img.shape[1], self.joint_pairs)
                center[0] = img_w - center[0] - 1
            centers[i] = center
            gts.append(gt)
        # the maps of all samples at once: element-wise, with the bits of the per-sample get_affine_transform calls
        (m_fwd, _), (jtrans, tinv) = get_affine_transform_batch(centers, scales, rots, (self.input_shape, self.output_shape))
        w, h = scales[:, 0] * 1.0, scales[:, 1] * 1.0                     # center_scale_to_box, element-wise
        xmin, ymin = centers[:, 0] - w * 0.5, centers[:, 1] - h * 0.5
        boxes = np.stack([xmin, ymin, xmin + w, ymin + h], axis=-1).astype(np.float32)
        gt = np.stack(gts) if n else np.zeros((0, 0, 3), np.float32)
        return SampleGeometry(m_fwd, flip, tinv, affine_transform_batch(gt, m_fwd), affine_transform_batch(gt, jtrans), boxes)

    def batch(self, samples: Sequence, rng=None, out=None, crops=None, sigma=2.0):
        """`[transform(s) for s in samples]` + `MSCOCO.collate_fn`, on the GPU: -> (input fp32 [B,3,h,w] RGB `x/255 - mean`,
        heat_maps fp32 [B,J,h/4,w/4], masks fp32 [B,J], trans_inv fp32 [B,2,3]), all on the samples' device.  Sample images are CUDA
        uint8 [H,W,3] BGR (any size, several samples may share one).  `out`: optional preallocated tuple of those four tensors (e.g. a
        trainer's static input) written in place; `crops`: optional uint8 [B,h,w,3] CUDA tensor that receives the BGR crops."""
        geo = self.geometry(samples, rng)
        n = len(samples)
        J = geo.joints.shape[1] if n else 0
        dev = samples[0].img.device if n else torch.device("cuda", torch.cuda.current_device())
        iw, ih = int(self.input_shape[0]), int(self.input_shape[1])
        ow, oh = int(self.output_shape[0]), int(self.output_shape[1])
        shapes = ((n, 3, ih, iw), (n, J, oh, ow), (n, J), (n, 2, 3))
        if out is None:
            out = tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes)
        else:
            for t, sh, name in zip(out, shapes, ("input", "heat_maps", "masks", "trans_inv")):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == sh and t.is_contiguous()
                        and t.device == dev):
                    raise _lib.HipLibraryError(f"out {name}: expected a contiguous CUDA float32 tensor {sh} on {dev}")
        if crops is not None and not (isinstance(crops, torch.Tensor) and crops.is_cuda and crops.dtype == torch.uint8
                                      and tuple(crops.shape) == (n, ih, iw, 3) and crops.is_contiguous() and crops.device == dev):
            raise _lib.HipLibraryError(f"crops: expected a contiguous CUDA uint8 tensor {(n, ih, iw, 3)} on {dev}")
        x, hm, mask, tinv = out
        if n == 0:                          # empty batch: empty outputs, nothing to launch
            return x, hm, mask, tinv
        srcs = np.empty(n, np.uint64)
        hw = np.empty((n, 2), np.int32)
        for i, s in enumerate(samples):
            img = s.img
            if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[-1] == 3
                    and img.is_contiguous() and img.device == dev):
                raise _lib.HipLibraryError(f"sample {i}: expected a contiguous CUDA uint8 image [H,W,3] on {dev}")
            srcs[i], hw[i] = img.data_ptr(), img.shape[:2]
        m_fwd = np.ascontiguousarray(geo.m_fwd)
        lib = _lib.lib()
        stream = _lib.current_stream(dev)
        mean = (ctypes.c_float * 3)(*rgb_mean)
        _lib.check(lib.sp_warp_affine_batch_u8c3_to_nchw_f32(srcs.ctypes.data, hw.ctypes.data, geo.flip.ctypes.data, m_fwd.ctypes.data, n,
                                                              ih, iw, mean, _lib.ptr(x), _lib.ptr(crops), stream),
                   "sp_warp_affine_batch_u8c3_to_nchw_f32")
        # the tiny per-joint values: one upload each, then the refine encoder on the same stream
        hmj = torch.from_numpy(np.ascontiguousarray(geo.hm_joints)).to(dev)
        _lib.check(lib.sp_encode_gauss_refine(_lib.ptr(hmj), n, J, oh, ow, float(sigma), _lib.ptr(hm), _lib.ptr(mask), stream),
                   "sp_encode_gauss_refine")
        tinv.copy_(torch.from_numpy(geo.trans_inv.astype(np.float32)))
        return x, hm, mask, tinv
