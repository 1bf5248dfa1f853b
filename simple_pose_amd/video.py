"""Video frames: YUV 4:2:0 (NV12 / I420) <-> packed uint8 BGR on the device.

    f = YuvFrame.from_surface(buf, H, W, pitch)             # a hardware decoder's NV12 surface in HBM: Y rows, then UV rows, one pitch
    f = YuvFrame.from_i420(buf, H, W)                       # ffmpeg / PyAV's packed yuv420p buffer (numpy, on the host)
    f = YuvFrame((y, uv), H, W, "nv12", "bt709", False)     # planes as views: CUDA uint8 tensors or numpy arrays, stride(0) = the pitch
    bgr = to_bgr(f)                                         # CUDA uint8 [H, W, 3];  to_bgr([f0, f1, ...]) -> a list, ONE launch
    f = from_bgr(result.image, "nv12")                      # the reverse, e.g. for a hardware encoder

Every image entry point of the package (TopDownPoseEstimator.estimate / estimate_batch / estimate_boxes, PoseTracker.update,
MultiStreamTracker.update, YOLOv5Detector.single_predict / predict) takes a YuvFrame where it takes a BGR image: the frame is converted
straight into the estimator's static source buffer (one launch in place of the copy), a list of differently sized frames by one launch
through a table of `sp_yuv_ref` in device memory.  The arithmetic (include/simple_pose_hip.h states it) is libjpeg's 16.16 fixed point
with replicated chroma on the way in and the 2x2 average on the way out; four modes: BT.601 / BT.709, limited / full range.
Host planes and the table reach the device in ONE pinned host-to-device copy, as mixed_batch.MixedBatch does it.  There is no CPU fallback:
a CPU tensor is refused (a numpy array is host data to upload)."""
from __future__ import annotations

import ctypes
from typing import Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import HipLibraryError, YuvRef, _device_index

MAX_SIDE = 32767
FORMATS = {"nv12": _lib.SP_YUV_NV12, "i420": _lib.SP_YUV_I420}
MATRICES = {"bt601": _lib.SP_YUV_BT601, "bt709": _lib.SP_YUV_BT709}
REF_BYTES = ctypes.sizeof(YuvRef)
# sp_yuv_ref as a numpy record: a call's table is written into the pinned buffer in one assignment
REF_DTYPE = np.dtype([(n, "<u8") for n in ("y", "u", "v", "bgr")] + [(n, "<i4") for n in ("h", "w", "pitch_y", "pitch_c", "pitch_bgr", "format",
                                                                                          "matrix", "range")])
assert REF_DTYPE.itemsize == REF_BYTES == 64 and [n for n, _ in YuvRef._fields_] == list(REF_DTYPE.names)


def _codes(format, matrix, full_range):
    if format not in FORMATS:
        raise ValueError(f"format: expected one of {sorted(FORMATS)}, got {format!r}")
    if matrix not in MATRICES:
        raise ValueError(f"matrix: expected one of {sorted(MATRICES)}, got {matrix!r}")
    if not isinstance(full_range, (bool, np.bool_)):
        raise TypeError(f"full_range: expected a bool, got {full_range!r}")
    return FORMATS[format], MATRICES[matrix], _lib.SP_YUV_FULL if full_range else _lib.SP_YUV_LIMITED


def _check_size(height, width):
    for name, v in (("height", height), ("width", width)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not (1 <= int(v) <= MAX_SIDE):
            raise ValueError(f"{name}: expected an int in 1..{MAX_SIDE}, got {v!r}")
    return int(height), int(width)


def _plane(p, name: str, rows: int, row_bytes: int):
    """One plane [rows, row_bytes] (the NV12 chroma plane also as [rows, cw, 2]) -> (the plane, its pitch in bytes).  A CUDA uint8 tensor or
    a numpy uint8 array, unit inner stride, stride(0) the pitch."""
    if isinstance(p, torch.Tensor):
        if not p.is_cuda:
            raise HipLibraryError(f"{name}: tensor is on {p.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        if p.dtype != torch.uint8:
            raise TypeError(f"{name}: expected uint8, got {p.dtype}")
        shape, strides = tuple(p.shape), tuple(p.stride())
    elif isinstance(p, np.ndarray):
        if p.dtype != np.uint8:
            raise TypeError(f"{name}: expected uint8, got {p.dtype}")
        shape, strides = tuple(p.shape), tuple(p.strides)
    else:
        raise TypeError(f"{name}: expected a CUDA uint8 tensor or a numpy uint8 array, got {type(p).__name__}")
    if len(shape) == 3 and shape[2] == 2 and row_bytes == 2 * shape[1] and strides[1:] == (2, 1):
        shape, strides = (shape[0], 2 * shape[1]), (strides[0], 1)           # [ch, cw, 2] pairs: the same bytes as [ch, 2 * cw]
        p = p.as_strided(shape, strides) if isinstance(p, torch.Tensor) else np.lib.stride_tricks.as_strided(p, shape, strides, writeable=False)
    if shape != (rows, row_bytes):
        raise ValueError(f"{name}: expected [{rows}, {row_bytes}], got {tuple(p.shape)}")
    if strides[1] != 1:
        raise ValueError(f"{name}: the inner stride must be 1, got {strides[1]}")
    pitch = int(strides[0]) if rows > 1 else max(int(strides[0]), row_bytes)
    if pitch < row_bytes:
        raise ValueError(f"{name}: pitch {pitch} is below the row ({row_bytes} bytes)")
    if pitch > 2 ** 31 - 1:
        raise ValueError(f"{name}: pitch {pitch} does not fit an int32")
    return p, pitch


class YuvFrame(object):
    """One YUV 4:2:0 frame of `height` x `width` luma samples (1 .. 32767 a side, odd sizes legal; chroma is ceil(height / 2) x
    ceil(width / 2)).  `planes`: for "nv12" (Y [h, w], UV [ch, 2 * cw] or [ch, cw, 2]), for "i420" (Y [h, w], U [ch, cw], V [ch, cw]; U and
    V with the same pitch) - CUDA uint8 tensors on one device, or numpy uint8 arrays (host frames, uploaded by the call that uses them), as
    views with unit inner stride whose stride(0) is the pitch.  `matrix`: "bt601" or "bt709"; `full_range`: False = limited ("TV") range.
    Everything is checked here, before any launch.  `.shape` is that of the BGR image it stands for, (height, width, 3)."""

    def __init__(self, planes, height: int, width: int, format: str = "nv12", matrix: str = "bt601", full_range: bool = False):
        self.height, self.width = _check_size(height, width)
        self.format, self.matrix, self.full_range = format, matrix, bool(full_range)
        self.codes = _codes(format, matrix, full_range)
        if not isinstance(planes, (list, tuple)):
            raise TypeError(f"planes: expected a tuple of planes, got {type(planes).__name__}")
        want = 2 if format == "nv12" else 3
        if len(planes) != want:
            raise ValueError(f"planes: {format} has {want} planes, got {len(planes)}")
        h, w = self.height, self.width
        ch, cw = (h + 1) // 2, (w + 1) // 2
        y, self.pitch_y = _plane(planes[0], "planes[0] (Y)", h, w)
        if format == "nv12":
            u, self.pitch_c = _plane(planes[1], "planes[1] (UV)", ch, 2 * cw)
            self.planes = (y, u)
        else:
            u, self.pitch_c = _plane(planes[1], "planes[1] (U)", ch, cw)
            v, pv = _plane(planes[2], "planes[2] (V)", ch, cw)
            if ch == 1:
                self.pitch_c = pv = max(self.pitch_c, pv)
            if pv != self.pitch_c:
                raise ValueError(f"planes: U and V share one pitch, got {self.pitch_c} and {pv}")
            self.planes = (y, u, v)
        kinds = {isinstance(p, np.ndarray) for p in self.planes}
        if len(kinds) != 1:
            raise TypeError("planes: all CUDA tensors or all numpy arrays")
        self.is_host = kinds == {True}
        self.device = None if self.is_host else _lib.same_device(*self.planes)
        # device pointers, taken once (the frame holds its planes): y, u, v (0 for NV12)
        self.ptrs = None if self.is_host else tuple(p.data_ptr() for p in self.planes) + ((0,) if format == "nv12" else ())

    @property
    def shape(self):
        return (self.height, self.width, 3)

    def __getitem__(self, key):
        if key is not None:
            raise TypeError("a YuvFrame is not an array: frame[None] (a batch of one) is the only index")
        return YuvBatch([self])

    def __repr__(self):
        where = "host" if self.is_host else str(self.device)
        return (f"YuvFrame({self.height}x{self.width} {self.format} {self.matrix} {'full' if self.full_range else 'limited'}, "
                f"pitch {self.pitch_y}/{self.pitch_c}, {where})")

    @classmethod
    def from_surface(cls, buf, height: int, width: int, pitch: int = None, matrix: str = "bt601", full_range: bool = False) -> "YuvFrame":
        """A decoder's NV12 surface: one uint8 buffer (CUDA tensor or numpy, flat or [rows, pitch]) holding `height` Y rows followed by
        ceil(height / 2) UV rows, all `pitch` bytes apart (default: the buffer's row length, or the tight even width for a flat one).  A
        surface whose UV plane starts at an aligned row instead is two views: YuvFrame((buf[:h, :w], buf[uv_row:uv_row + ch, :2 * cw]), ...)."""
        h, w = _check_size(height, width)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if not isinstance(buf, (torch.Tensor, np.ndarray)):
            raise TypeError(f"buf: expected a CUDA uint8 tensor or a numpy uint8 array, got {type(buf).__name__}")
        if pitch is None:
            pitch = int(buf.shape[1]) if len(buf.shape) == 2 else 2 * cw
        if not isinstance(pitch, (int, np.integer)) or isinstance(pitch, bool) or pitch < 2 * cw:
            raise ValueError(f"pitch: {pitch!r} is below the row ({2 * cw} bytes)")
        if len(buf.shape) == 2 and (buf.shape[1] != pitch or (buf.stride(1) if isinstance(buf, torch.Tensor) else buf.strides[1]) != 1):
            raise ValueError(f"buf: rows of {buf.shape[1]} bytes, pitch {pitch}")
        flat = buf.reshape(-1) if len(buf.shape) == 2 else buf
        need = (h + ch - 1) * pitch + 2 * cw
        if len(flat.shape) != 1 or flat.shape[0] < need:
            raise ValueError(f"buf: {tuple(buf.shape)} holds fewer than the {need} bytes of {h} + {ch} rows at pitch {pitch}")
        rows = h + ch
        if flat.shape[0] >= rows * pitch:
            grid = flat[:rows * pitch].reshape(rows, pitch)
            y, uv = grid[:h, :w], grid[h:, :2 * cw]
        elif isinstance(flat, torch.Tensor):                     # the last row ends with the image: strided views over the flat buffer
            y = flat.as_strided((h, w), (pitch, 1))
            uv = flat.as_strided((ch, 2 * cw), (pitch, 1), h * pitch)
        else:
            y = np.lib.stride_tricks.as_strided(flat, (h, w), (pitch, 1), writeable=False)
            uv = np.lib.stride_tricks.as_strided(flat[h * pitch:], (ch, 2 * cw), (pitch, 1), writeable=False)
        return cls((y, uv), h, w, "nv12", matrix, full_range)

    @classmethod
    def from_i420(cls, buf, height: int, width: int, matrix: str = "bt601", full_range: bool = False) -> "YuvFrame":
        """ffmpeg's packed yuv420p: one flat uint8 buffer (numpy or CUDA) of h * w Y bytes, then ch * cw of U, then ch * cw of V."""
        h, w = _check_size(height, width)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if not isinstance(buf, (torch.Tensor, np.ndarray)):
            raise TypeError(f"buf: expected a numpy uint8 array or a CUDA uint8 tensor, got {type(buf).__name__}")
        if len(buf.shape) != 1 or buf.shape[0] != h * w + 2 * ch * cw:
            raise ValueError(f"buf: expected {h * w + 2 * ch * cw} bytes ({h}x{w} yuv420p), got {tuple(buf.shape)}")
        a, b = h * w, h * w + ch * cw
        return cls((buf[:a].reshape(h, w), buf[a:b].reshape(ch, cw), buf[b:].reshape(ch, cw)), h, w, "i420", matrix, full_range)


class YuvBatch(object):
    """Same-sized YuvFrames standing where a [B, H, W, 3] batch stands (what `frame[None]` and the estimator's shape check hand on)."""

    def __init__(self, frames: Sequence[YuvFrame]):
        self.frames = list(frames)
        if not self.frames or any(not isinstance(f, YuvFrame) for f in self.frames):
            raise TypeError("expected a non-empty list of YuvFrame")
        if len({f.shape for f in self.frames}) != 1:
            raise ValueError("the images of one batch share one size")
        self.shape = (len(self.frames),) + self.frames[0].shape


def _align(n: int) -> int:
    return (n + 255) // 256 * 256


def _check_bgr(t, i: int, h: int = None, w: int = None) -> int:
    """A BGR image of the device side: CUDA uint8 [h, w, 3], pixels packed (strides (pitch, 3, 1)).  Returns its pitch in bytes."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"image {i}: expected a CUDA uint8 tensor [H, W, 3], got {type(t).__name__}")
    if not t.is_cuda:
        raise HipLibraryError(f"image {i}: tensor is on {t.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
    if t.dtype != torch.uint8:
        raise TypeError(f"image {i}: expected uint8, got {t.dtype}")
    shape = tuple(t.shape)
    if len(shape) != 3 or shape[2] != 3 or 0 in shape or (h is not None and shape[:2] != (h, w)):
        raise ValueError(f"image {i}: expected uint8 BGR [{'H' if h is None else h}, {'W' if w is None else w}, 3], got {shape}")
    if shape[0] > MAX_SIDE or shape[1] > MAX_SIDE:
        raise ValueError(f"image {i}: {shape[0]}x{shape[1]} is above {MAX_SIDE} pixels a side")
    if t.stride(2) != 1 or t.stride(1) != 3 or (shape[0] > 1 and t.stride(0) < 3 * shape[1]):
        raise ValueError(f"image {i}: expected packed pixels, strides (pitch >= {3 * shape[1]}, 3, 1), got {tuple(t.stride())}")
    return max(int(t.stride(0)), 3 * shape[1])


def _stage_buffers(stage, nbytes: int, device):
    """The pinned staging buffer and its device twin, `nbytes` at least: kept in `stage` (a dict the caller owns between calls, who then
    synchronises with the stream before the next call) or fresh ones."""
    if stage is None:
        stage = {}
    if stage.get("host") is None or stage["host"].numel() < nbytes or stage["dev"].device != device:
        stage["host"] = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
        stage["dev"] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    return stage["host"], stage["dev"]


def _upload(frames: Sequence[YuvFrame], bgr: Sequence[torch.Tensor], pitches: Sequence[int], device, stage):
    """The table of `sp_yuv_ref` for (frames[i], bgr[i]) in device memory; host planes ride behind it in the same pinned buffer (rows
    packed tight, every plane 256-byte aligned) and the ONE host-to-device copy of the call.  Returns the table."""
    n = len(frames)
    off, where = _align(n * REF_BYTES), {}
    for i, f in enumerate(frames):
        if f.is_host:
            where[i] = []
            for p in f.planes:
                where[i].append(off)
                off += _align(p.shape[0] * p.shape[1])
    host, dev = _stage_buffers(stage, off, device)
    hview = host.numpy()
    rows_, base = [], dev.data_ptr()
    for i, f in enumerate(frames):
        if f.is_host:
            ptrs = []
            for p, o in zip(f.planes, where[i]):
                rows, rb = p.shape
                np.copyto(hview[o:o + rows * rb].reshape(rows, rb), p)
                ptrs.append(base + o)
            ptrs, py, pc = tuple(ptrs) + ((0,) if len(ptrs) == 2 else ()), f.planes[0].shape[1], f.planes[1].shape[1]
        else:
            ptrs, py, pc = f.ptrs, f.pitch_y, f.pitch_c
        rows_.append(ptrs + (bgr[i].data_ptr(), f.height, f.width, py, pc, pitches[i]) + f.codes)
    hview[:n * REF_BYTES].view(REF_DTYPE)[:] = np.array(rows_, dtype=REF_DTYPE)
    dev[:off].copy_(host[:off], non_blocking=True)               # the call's one host-to-device copy
    return dev[:n * REF_BYTES]


def _launch_table(to_bgr_dir: bool, frames: Sequence[YuvFrame], bgr: Sequence[torch.Tensor], pitches: Sequence[int], device, stage) -> None:
    """The table's upload and the one `_images` launch over it, on the current stream.  Without a `stage` the buffers are this call's own:
    the allocators hand them on in stream order (the pinned one after the copy's event), so nothing has to be kept."""
    if not frames:
        return
    table = _upload(frames, bgr, pitches, device, stage)
    fn = "sp_yuv420_to_bgr_images_u8c3" if to_bgr_dir else "sp_bgr_to_yuv420_images_u8c3"
    _lib.check(getattr(_lib.lib(), fn)(table.data_ptr(), len(frames), max(f.height for f in frames), max(f.width for f in frames),
                                       _lib.current_stream(device)), fn)


def _frames_device(frames: Sequence[YuvFrame], others: Sequence = (), device=None) -> torch.device:
    """The one device of a call: that of the device-side frames and tensors, else `device`, else the current one."""
    devs = {f.device for f in frames if not f.is_host} | {t.device for t in others if isinstance(t, torch.Tensor) and t.is_cuda}
    if device is not None:
        devs.add(torch.device("cuda", _device_index(torch.device(device))))
    if len(devs) > 1:
        raise HipLibraryError(f"operands on different devices: {sorted(str(d) for d in devs)}")
    return devs.pop() if devs else torch.device("cuda", torch.cuda.current_device())


def convert_into(frames: Sequence[YuvFrame], outs: Sequence[torch.Tensor], stage: dict = None, dense: torch.Tensor = None) -> None:
    """frames[i] -> outs[i] (CUDA uint8 [h_i, w_i, 3] views, packed pixels, any row pitch), one launch on the current stream: a single frame
    already on the device through sp_yuv420_to_bgr_u8c3 (nothing is uploaded), anything else through the table (sp_yuv420_to_bgr_images_u8c3)
    behind its one pinned copy.  Every check happens before the launch.  `dense`: the contiguous CUDA uint8 [n, h, w, 3] block whose images
    `outs` are (the estimator's static source): one check of the block stands for the checks of its images."""
    if len(frames) != len(outs):
        raise ValueError(f"out: {len(outs)} images for {len(frames)} frames")
    for i, f in enumerate(frames):
        if not isinstance(f, YuvFrame):
            raise TypeError(f"frame {i}: expected a YuvFrame, got {type(f).__name__}")
    if dense is not None:
        n, (h, w, _) = len(frames), frames[0].shape if frames else (0, 0, 0)
        if not (dense.is_cuda and dense.dtype == torch.uint8 and dense.is_contiguous() and tuple(dense.shape) == (n, h, w, 3)) or \
                any(f.shape != (h, w, 3) for f in frames):
            raise ValueError(f"dense: expected a contiguous CUDA uint8 [{n}, {h}, {w}, 3] block for frames of one size")
        pitches = [3 * w] * n
    else:
        pitches = [_check_bgr(o, i, f.height, f.width) for i, (f, o) in enumerate(zip(frames, outs))]
    if not frames:
        return
    device = _frames_device(frames, outs)
    lib, stream = _lib.lib(), _lib.current_stream(device)
    if len(frames) == 1 and not frames[0].is_host:
        f, P = frames[0], _lib.ptr
        _lib.check(lib.sp_yuv420_to_bgr_u8c3(f.ptrs[0], f.ptrs[1], f.ptrs[2] or None, f.height, f.width, f.pitch_y, f.pitch_c, f.codes[0], f.codes[1],
                                             f.codes[2], P(outs[0]), pitches[0], stream), "sp_yuv420_to_bgr_u8c3")
        return
    _launch_table(True, frames, outs, pitches, device, stage)


def to_bgr(frames: Union[YuvFrame, Sequence[YuvFrame]], out=None, device=None):
    """One YuvFrame -> CUDA uint8 BGR [H, W, 3]; a list of frames of any sizes, formats and modes -> a list of them.  Host planes and the
    table of frames travel in one pinned host-to-device copy, the conversion is ONE launch (sp_yuv420_to_bgr_images_u8c3) on the current
    stream, and nothing synchronises.  `out`: the image (or the list of images) to write, CUDA uint8 [H, W, 3] with packed pixels and any
    row pitch; `device`: where host frames go (default: the device of the other operands, else the current one)."""
    single = isinstance(frames, YuvFrame)
    fl = [frames] if single else frames
    if not isinstance(fl, (list, tuple)):
        raise TypeError(f"expected a YuvFrame or a list of them, got {type(frames).__name__}")
    for i, f in enumerate(fl):
        if not isinstance(f, YuvFrame):
            raise TypeError(f"frame {i}: expected a YuvFrame, got {type(f).__name__}")
    if out is not None:
        outs = [out] if single else out
        if not isinstance(outs, (list, tuple)) or len(outs) != len(fl):
            raise ValueError(f"out: expected {'one image' if single else f'a list of {len(fl)} images'}")
        for i, (f, o) in enumerate(zip(fl, outs)):
            _check_bgr(o, i, f.height, f.width)
    else:
        outs = None
    if not fl:
        return []
    dev = _frames_device(fl, outs or (), device)
    if outs is None:
        outs = [torch.empty(f.shape, dtype=torch.uint8, device=dev) for f in fl]
    pitches = [_check_bgr(o, i, f.height, f.width) for i, (f, o) in enumerate(zip(fl, outs))]
    _launch_table(True, fl, outs, pitches, dev, None)
    return outs[0] if single else list(outs)


def _new_planes(h: int, w: int, format: str, device):
    """Fresh planes for one frame, pitches multiples of 16 (the kernels' 16-byte path): NV12 as one surface (Y rows, then UV rows)."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if format == "nv12":
        pitch = (2 * cw + 15) // 16 * 16
        buf = torch.empty((h + ch, pitch), dtype=torch.uint8, device=device)
        return buf[:h, :w], buf[h:, :2 * cw]
    py, pc = (w + 15) // 16 * 16, (cw + 15) // 16 * 16
    return (torch.empty((h, py), dtype=torch.uint8, device=device)[:, :w], torch.empty((ch, pc), dtype=torch.uint8, device=device)[:, :cw],
            torch.empty((ch, pc), dtype=torch.uint8, device=device)[:, :cw])


def from_bgr(images, format: str = "nv12", matrix: str = "bt601", full_range: bool = False, out=None):
    """One CUDA uint8 BGR image [H, W, 3] (packed pixels, any row pitch; e.g. PoseResult.image) -> a YuvFrame on its device; a list of
    images of any sizes -> a list of frames.  Chroma is the rounded mean of each 2x2 block (an edge pixel counts twice at an odd size).
    One launch on the current stream (sp_bgr_to_yuv420_u8c3 for one image, sp_bgr_to_yuv420_images_u8c3 behind the table's pinned copy
    for a list); nothing synchronises.  `out`: the YuvFrame (or list of them) to write, device planes, of the images' sizes - its own
    format and mode apply, and `format` / `matrix` / `full_range` are not read; default: fresh planes with 16-byte pitches."""
    _codes(format, matrix, full_range)
    single = isinstance(images, torch.Tensor)
    il = [images] if single else images
    if not isinstance(il, (list, tuple)):
        raise TypeError(f"expected a CUDA uint8 BGR image [H, W, 3] or a list of them, got {type(images).__name__}")
    pitches = [_check_bgr(t, i) for i, t in enumerate(il)]
    dev = _lib.same_device(*il) if il else None
    if out is not None:
        outs = [out] if single else out
        if not isinstance(outs, (list, tuple)) or len(outs) != len(il):
            raise ValueError(f"out: expected {'one YuvFrame' if single else f'a list of {len(il)} YuvFrames'}")
        for i, (f, t) in enumerate(zip(outs, il)):
            if not isinstance(f, YuvFrame) or f.is_host:
                raise TypeError(f"out {i}: expected a YuvFrame with device planes")
            if f.shape != tuple(t.shape):
                raise ValueError(f"out {i}: a {f.height}x{f.width} frame for a {t.shape[0]}x{t.shape[1]} image")
            if f.device != dev:
                raise HipLibraryError(f"out {i}: on {f.device}, the image on {dev}")
    else:
        outs = [YuvFrame(_new_planes(t.shape[0], t.shape[1], format, dev), t.shape[0], t.shape[1], format, matrix, full_range) for t in il]
    if not il:
        return []
    lib, stream, P = _lib.lib(), _lib.current_stream(dev), _lib.ptr
    if single:
        f = outs[0]
        _lib.check(lib.sp_bgr_to_yuv420_u8c3(P(il[0]), pitches[0], f.height, f.width, f.codes[0], f.codes[1], f.codes[2], P(f.planes[0]),
                                             P(f.planes[1]), P(f.planes[2]) if len(f.planes) == 3 else None, f.pitch_y, f.pitch_c, stream),
                   "sp_bgr_to_yuv420_u8c3")
        return f
    _launch_table(False, outs, il, pitches, dev, None)
    return list(outs)


def resolve(imgs, device=None, stage: dict = None) -> list:
    """A list of images in which YuvFrames stand next to BGR images -> the same list with every YuvFrame replaced by its BGR CUDA tensor
    (one table launch for all of them); the other entries are handed on untouched."""
    idx = [i for i, im in enumerate(imgs) if isinstance(im, YuvFrame)]
    if not idx:
        return list(imgs)
    frames = [imgs[i] for i in idx]
    dev = _frames_device(frames, [im for im in imgs if isinstance(im, torch.Tensor)], device)
    outs = [torch.empty(f.shape, dtype=torch.uint8, device=dev) for f in frames]
    _launch_table(True, frames, outs, [3 * f.width for f in frames], dev, stage)
    res = list(imgs)
    for i, o in zip(idx, outs):
        res[i] = o
    return res
