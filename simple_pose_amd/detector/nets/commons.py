"""Parameter holders of detector/nets/commons.py (CBR, Focus, BottleNeck, BottleNeckCSP, SPP) and its scale helpers.

The modules only own parameters and buffers under the reference's names and in its registration order; nothing here computes.  The
forward pass is simple_pose_amd.engine.yolov5_program: every convolution (with its BatchNorm folded and the Hardswish in the epilogue) on
the implicit GEMM, the rest in csrc/detect.hip.
"""
from __future__ import annotations

import math

from torch import nn


def model_scale(name="s"):
    name_dict = {"s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.00, 1.00), "x": (1.33, 1.25)}
    multiples = name_dict.get(name, None)
    if multiples is None:
        raise NotImplementedError("scale_name only support s,m,l,x")
    return multiples


def make_divisible(x, divisor):
    return math.ceil(x / divisor) * divisor


def depth_grow(x: int, depth_multiples: float):
    return max(round(x * depth_multiples), 1) if x > 1 else x


def width_grow(x, width_multiples):
    return make_divisible(x * width_multiples, 8)


class CBR(nn.Module):
    """conv (no bias) -> BatchNorm2d -> Hardswish (commons.py:32)."""

    def __init__(self, in_channel, out_channel, kernel_size=1, stride=1, padding=None, groups=1):
        super().__init__()
        if padding is None:
            padding = (kernel_size - 1) // 2
        if groups != 1:
            raise NotImplementedError("grouped CBR")
        self.conv = nn.Conv2d(in_channel, out_channel, kernel_size, stride, padding, bias=False)
        self.bn = nn.BatchNorm2d(out_channel)


class Focus(nn.Module):
    def __init__(self, in_channel, out_channel, kernel=1, stride=1, padding=None, groups=1):
        super().__init__()
        self.conv = CBR(in_channel * 4, out_channel, kernel, stride, padding, groups)


class BottleNeck(nn.Module):
    def __init__(self, in_channel, out_channel, shortcut=True, groups=1, expansion=0.5):
        super().__init__()
        inner_channel = int(out_channel * expansion)
        self.conv1 = CBR(in_channel, inner_channel, 1, 1)
        self.conv2 = CBR(inner_channel, out_channel, 3, 1, groups=groups)
        self.add = shortcut and inner_channel == out_channel


class BottleNeckCSP(nn.Module):
    def __init__(self, in_channel, out_channel, blocks=1, shortcut=True, groups=1, expansion=0.5):
        super().__init__()
        inner_channel = int(out_channel * expansion)
        self.conv1_0 = CBR(in_channel, inner_channel, 1, 1)
        self.conv2_0 = nn.Conv2d(in_channel, inner_channel, 1, 1, bias=False)
        self.conv1_n = nn.Conv2d(inner_channel, inner_channel, 1, 1, bias=False)
        self.conv3 = CBR(2 * inner_channel, out_channel, 1, 1)
        self.bn = nn.BatchNorm2d(2 * inner_channel)
        self.conv1_s = nn.Sequential(*[BottleNeck(inner_channel, inner_channel, shortcut, groups, expansion=1) for _ in range(blocks)])


class SPP(nn.Module):
    def __init__(self, in_channel, out_channel, k=(5, 9, 13)):
        super().__init__()
        if tuple(k) != (5, 9, 13):
            raise NotImplementedError("SPP pools 5 / 9 / 13")
        inner_channel = in_channel // 2
        self.conv1 = CBR(in_channel, inner_channel, 1, 1)
        self.conv2 = CBR(inner_channel * (len(k) + 1), out_channel, 1, 1)
