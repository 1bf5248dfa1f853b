"""YOLOv5 (detector/nets/yolov5.py) as a parameter holder with the reference's state_dict keys, order and parameter counts; forward() runs
the HIP program (simple_pose_amd.engine.yolov5_program).  No torch op computes anything and a CPU input raises."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from ... import engine
from ..._lib import HipLibraryError, require_cuda_f32
from .commons import BottleNeckCSP, CBR, Focus, SPP, depth_grow, model_scale, width_grow

default_anchors = [
    [10, 13, 16, 30, 33, 23],
    [30, 61, 62, 45, 59, 119],
    [116, 90, 156, 198, 373, 326],
]
default_strides = [8., 16., 32.]


class YOLOv5Backbone(nn.Module):
    def __init__(self, in_channel=3, depth_multiples=0.33, width_multiples=0.50):
        super().__init__()
        c64, c128, c256, c512, c1024 = (width_grow(c, width_multiples) for c in (64, 128, 256, 512, 1024))
        self.out_channels = [c256, c512, c1024]
        self.stem = Focus(in_channel, c64, 3)
        self.layer1 = nn.Sequential(CBR(c64, c128, 3, 2), BottleNeckCSP(c128, c128, depth_grow(3, depth_multiples)))
        self.layer2 = nn.Sequential(CBR(c128, c256, 3, 2), BottleNeckCSP(c256, c256, depth_grow(9, depth_multiples)))
        self.layer3 = nn.Sequential(CBR(c256, c512, 3, 2), BottleNeckCSP(c512, c512, depth_grow(9, depth_multiples)))
        self.layer4 = nn.Sequential(CBR(c512, c1024, 3, 2), SPP(c1024, c1024, (5, 9, 13)),
                                    BottleNeckCSP(c1024, c1024, depth_grow(3, depth_multiples), shortcut=False))


class YOLOv5Neck(nn.Module):
    def __init__(self, c3, c4, c5, blocks=1):
        super().__init__()
        self.latent_c5 = CBR(c5, c4, 1, 1)
        self.c4_fuse = BottleNeckCSP(c4 * 2, c4, blocks=blocks, shortcut=False)
        self.latent_c4 = CBR(c4, c3)
        self.c3_out = BottleNeckCSP(c3 * 2, c3, blocks=blocks, shortcut=False)
        self.c3_c4 = CBR(c3, c3, 3, 2)
        self.c4_out = BottleNeckCSP(c3 * 2, c4, blocks=blocks, shortcut=False)
        self.c4_c5 = CBR(c4, c4, 3, 2)
        self.c5_out = BottleNeckCSP(c4 * 2, c5, blocks=blocks, shortcut=False)


class YOLOv5Head(nn.Module):
    def __init__(self, c3, c4, c5, num_cls=80, strides=None, anchors=None):
        super().__init__()
        self.num_cls = num_cls
        self.output_num = num_cls + 5
        self.anchors = anchors if anchors is not None else default_anchors
        self.strides = strides if strides is not None else default_strides
        assert len(self.anchors) == len(self.strides) == 3, "three detection levels"
        self.layer_num = len(self.anchors)
        self.anchor_per_grid = len(self.anchors[0]) // 2
        a = torch.tensor(self.anchors).float().view(self.layer_num, -1, 2)
        normalize_anchors = a / torch.tensor(self.strides).float().view(3, 1, 1)
        self.register_buffer("normalize_anchors", normalize_anchors.clone())
        self.register_buffer("anchor_grid", a.clone().view(self.layer_num, 1, -1, 1, 1, 2))
        self.heads = nn.ModuleList(nn.Conv2d(x, self.output_num * self.anchor_per_grid, 1) for x in [c3, c4, c5])
        with torch.no_grad():                       # the reference's prior on obj / cls (yolov5.py:125-129)
            for mi, s in zip(self.heads, self.strides):
                b = mi.bias.view(self.anchor_per_grid, -1)
                b[:, 4] += math.log(8. / (640. / s) ** 2)
                b[:, 5:] += math.log(0.6 / (self.num_cls - 0.99))


class YOLOv5(nn.Module):
    def __init__(self, in_channel=3, num_cls=80, scale_name="s", strides=None, anchors=None):
        super().__init__()
        if in_channel != 3:
            raise NotImplementedError("the letterbox / Focus launch reads 3-channel images")
        depth_multiples, width_multiples = model_scale(scale_name)
        self.backbones = YOLOv5Backbone(in_channel, depth_multiples, width_multiples)
        c3, c4, c5 = self.backbones.out_channels
        self.neck = YOLOv5Neck(c3, c4, c5, blocks=depth_grow(3, depth_multiples))
        self.head = YOLOv5Head(c3, c4, c5, num_cls=num_cls, strides=strides, anchors=anchors)
        self.num_cls = num_cls
        self._programs = {}
        self._state = None          # the state_dict tensors, in key order (refreshed by .to() / load_state_dict; see hip_program)

    def _apply(self, fn, *args, **kwargs):              # .to() / .cuda() may replace every tensor
        self._state = None
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._state = None
        return super().load_state_dict(*args, **kwargs)

    def hip_program(self, in_h: int, in_w: int, device, slice_idx: int = -1, source: str = "nchw") -> engine.Program:
        """The fp32 program of this letterboxed shape (cached per shape / head cut / input kind; rebuilt when a parameter changes in place,
        moves, or is loaded).  Validating the cache walks a cached tensor list (~0.15 ms for s) instead of building a state_dict per call
        (~1 ms), which was half of a batch-1 single_predict.  A parameter REPLACED by attribute assignment needs `model._state = None`."""
        if self._state is None:
            self._state = list(self.state_dict(keep_vars=True).items())
        ver = tuple((v.data_ptr(), v._version) for _, v in self._state)
        key = (in_h, in_w, str(device), slice_idx, source)
        hit = self._programs.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        for k, v in self._state:
            if not v.is_cuda or v.device != torch.device(device):
                raise HipLibraryError(f"parameter {k} is on {v.device}, not {device}: simple_pose_amd runs on the MI355X only; call .to(device)")
        prog = engine.yolov5_program({k: v.detach() for k, v in self._state}, num_cls=self.num_cls, in_h=in_h, in_w=in_w, slice_idx=slice_idx,
                                     strides=tuple(self.head.strides), source=source)
        if len(self._programs) >= 8:
            self._programs.pop(next(iter(self._programs)))
        self._programs[key] = (ver, prog)
        return prog

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 RGB [B,3,H,W] in [0,1] (H, W multiples of 32) on the GPU -> the eval-mode head output [B, N, num_cls + 5]."""
        x = require_cuda_f32(x, "input")
        if self.training:
            raise NotImplementedError("training the detector is out of scope: call .eval()")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"expected [B,3,H,W] with H,W multiples of 32, got {tuple(x.shape)}")
        return self.hip_program(x.shape[2], x.shape[3], x.device).run(x)
