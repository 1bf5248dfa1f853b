"""Baseline JPEG decoding on the device: file bytes in, uint8 BGR images in HBM out (csrc/jpeg.hip behind sp_jpeg_parse /
sp_jpeg_decode_batch).  The pixels are libjpeg-turbo's default decode (what cv2.imread and PIL give) bit for bit.  EXIF orientation is
not applied.  Accepted: SOF0, 8-bit, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan; anything else raises
HipLibraryError with the parser's reason - there is no CPU decode path.

    info = parse(open(path, "rb").read())                 # host only
    dec = JpegDecoder("cuda:0")
    imgs = dec.decode([bytes, ...])                       # list of CUDA uint8 [H,W,3] BGR, views of one arena
    dec.decode_into([bytes, ...], frames)                 # equal-sized files into a [B,H,W,3] tensor (what estimate_batch takes)
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

_ALIGN = 64                     # every image's region in an arena starts on a multiple of this many bytes


@dataclass
class JpegInfo:
    width: int
    height: int
    components: int
    sampling: Tuple[Tuple[int, int], ...]         # (h, v) per component
    quant_sel: Tuple[int, ...]
    dc_sel: Tuple[int, ...]
    ac_sel: Tuple[int, ...]
    restart_interval: int
    mcus: Tuple[int, int]                         # (x, y)
    ecs_offset: int
    ecs_end: int
    seg_offsets: Tuple[int, ...]                  # first entropy byte of every restart segment
    quant: np.ndarray                             # uint16 [4, 64], natural order
    huff_counts: np.ndarray                       # uint8 [8, 16]: [4 * class + index]
    huff_values: np.ndarray                       # uint8 [8, 256]


def _as_bytes(data, what="data"):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    raise TypeError(f"{what}: expected the bytes of a JPEG file, got {type(data).__name__}")


def _parse_raw(data: bytes, seg_buf: np.ndarray):
    """-> (JpegDesc, int32 segment offsets, scratch).  `seg_buf`: scratch int32 array; a file with more segments is parsed again into a
    larger one, which is returned for the caller to keep."""
    desc = _lib.JpegDesc()
    lib = _lib.lib()
    rc = lib.sp_jpeg_parse(data, len(data), ctypes.byref(desc), seg_buf.ctypes.data, seg_buf.size)
    if rc == 0 and desc.segments > seg_buf.size:
        seg_buf = np.empty(desc.segments, np.int32)
        rc = lib.sp_jpeg_parse(data, len(data), ctypes.byref(desc), seg_buf.ctypes.data, seg_buf.size)
    _lib.check(rc, "sp_jpeg_parse")
    return desc, seg_buf[:desc.segments].copy(), seg_buf


def parse(data) -> JpegInfo:
    """Headers of one file (host only, no GPU call).  Raises HipLibraryError with the reason for anything the decoder does not take."""
    d, segs, _ = _parse_raw(_as_bytes(data), np.empty(1024, np.int32))
    n = d.components
    return JpegInfo(d.width, d.height, n, tuple((d.h_samp[c], d.v_samp[c]) for c in range(n)), tuple(d.quant_sel[:n]), tuple(d.dc_sel[:n]),
                    tuple(d.ac_sel[:n]), d.restart_interval, (d.mcus_x, d.mcus_y), d.ecs_offset, d.ecs_end, tuple(int(s) for s in segs),
                    np.ctypeslib.as_array(d.quant).copy(), np.ctypeslib.as_array(d.huff_counts).copy(),
                    np.ctypeslib.as_array(d.huff_values).copy())


def _round_up(v: int, m: int = _ALIGN) -> int:
    return (v + m - 1) // m * m


class JpegDecoder:
    """Batched decoder with reusable arenas on one device.  `decode` / `decode_into` run on torch's current stream of that device: one
    pinned upload (descriptors, segment tables and file bytes in one buffer) and four launches (zero, entropy, IDCT, colour).  The tensors `decode`
    returns are views of the output arena and are overwritten by the next call."""

    def __init__(self, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.HipLibraryError(f"JpegDecoder: device {dev}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        self.device = torch.device("cuda", _lib._device_index(dev))
        self._seg_scratch = np.empty(1024, np.int32)
        self._pinned = self._upload_done = None
        self._upload = self._coef = self._planes = self._out = None
        self.status = None                        # int32 [B] on the device after a call (0 = decoded; bits: _lib.SP_JPEG_STATUS)
        self.coefficients = None                  # (int16 arena, [offset per image], [count per image]) of the last call, for tests and tools
        self.relaunch = None                      # after a call: relaunch(stages=SP_JPEG_STAGE_ALL) runs the same batch again without an upload

    # ---- host side: parse every file, lay the arenas out ------------------------------------------------------------------------------------
    def _plan(self, files: Sequence):
        if isinstance(files, (bytes, bytearray, memoryview, torch.Tensor)) or not isinstance(files, (list, tuple)):
            raise TypeError("files: expected a list or tuple of bytes objects (one per JPEG file)")
        datas = [_as_bytes(f, f"files[{i}]") for i, f in enumerate(files)]
        descs = (_lib.JpegDesc * max(1, len(datas)))()
        segs = []
        seg_at = file_at = coef_at = plane_at = out_at = 0
        for i, data in enumerate(datas):
            try:
                d, s, self._seg_scratch = _parse_raw(data, self._seg_scratch)
            except _lib.HipLibraryError as e:
                raise _lib.HipLibraryError(f"files[{i}]: {e}") from None
            d.seg_index, d.file_offset, d.coef_offset, d.plane_offset, d.out_offset = seg_at, file_at, coef_at, plane_at, out_at
            descs[i] = d
            segs.append(s)
            seg_at += len(s)
            file_at += _round_up(len(data))
            coef_at += _round_up(d.coef_count * 2) // 2
            plane_at += _round_up(d.plane_bytes)
            out_at += _round_up(d.out_bytes)
        return datas, descs, segs, (seg_at, file_at, coef_at, plane_at, out_at)

    def _grow(self, name: str, size: int, dtype):
        t = getattr(self, name)
        if t is None or t.numel() < size:
            t = torch.empty(max(size, 1), dtype=dtype, device=self.device)
            setattr(self, name, t)
        return t

    def _run(self, files, out_tensor=None, check=True):
        datas, descs, segs, (n_seg, n_bytes, n_coef, n_plane, n_out) = self._plan(files)
        n = len(datas)
        if out_tensor is not None:
            for i in range(n):
                if (descs[i].height, descs[i].width) != tuple(out_tensor.shape[1:3]):
                    raise _lib.HipLibraryError(f"decode_into: files[{i}] is {descs[i].width}x{descs[i].height}, out holds "
                                               f"{out_tensor.shape[2]}x{out_tensor.shape[1]} frames")
                descs[i].out_offset = i * descs[0].out_bytes
            n_out = n * descs[0].out_bytes if n else 0
        # one upload: [descriptors | segment offsets | file bytes]
        desc_bytes = ctypes.sizeof(_lib.JpegDesc) * n
        seg_off = _round_up(desc_bytes)
        byte_off = _round_up(seg_off + 4 * n_seg)
        total = byte_off + n_bytes
        if self._upload_done is not None:
            self._upload_done.synchronize()       # the previous call's copy out of the pinned buffer (check=False does not wait for it)
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
        host = self._pinned.numpy()
        if n:
            host[:desc_bytes] = np.frombuffer(descs, np.uint8, desc_bytes)
            host[seg_off:seg_off + 4 * n_seg] = np.concatenate(segs).astype(np.int32).view(np.uint8)
        for i, data in enumerate(datas):
            o = byte_off + descs[i].file_offset
            host[o:o + len(data)] = np.frombuffer(data, np.uint8)
        up = self._grow("_upload", total, torch.uint8)
        coef = self._grow("_coef", n_coef, torch.int16)
        planes = self._grow("_planes", n_plane, torch.uint8)
        out = out_tensor if out_tensor is not None else self._grow("_out", n_out, torch.uint8)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            up[:total].copy_(self._pinned[:total], non_blocking=True)
            self._upload_done = torch.cuda.Event()
            self._upload_done.record()
            base = up.data_ptr()

            def launch(stages=_lib.SP_JPEG_STAGE_ALL):
                _lib.check(_lib.lib().sp_jpeg_decode_batch(descs, base, n, base + byte_off, n_bytes, base + seg_off, n_seg, _lib.ptr(coef),
                                                           coef.numel(), _lib.ptr(planes), planes.numel(), _lib.ptr(out), out.numel(),
                                                           _lib.ptr(status), stages, _lib.current_stream(self.device)), "sp_jpeg_decode_batch")
            launch()
        self.relaunch = launch                    # tools/bench_jpeg.py: the same batch again, or one stage of it (SP_JPEG_STAGE_*), no upload
        self.status = status
        self.coefficients = (coef, [descs[i].coef_offset for i in range(n)], [descs[i].coef_count for i in range(n)])
        if check and n:
            st = status.cpu().numpy()
            bad = np.nonzero(st)[0]
            if bad.size:
                i = int(bad[0])
                why = ", ".join(t for b, t in _lib.SP_JPEG_STATUS.items() if st[i] & b)
                raise _lib.HipLibraryError(f"JpegDecoder: files[{i}] is damaged (status {int(st[i])}: {why}); {bad.size} of {n} files failed")
        return descs, out

    # ---- public --------------------------------------------------------------------------------------------------------------------------------
    def decode(self, files: Sequence[bytes], check: bool = True) -> List[torch.Tensor]:
        """One batch of files (any sizes, any accepted sampling) -> a list of CUDA uint8 [H,W,3] BGR tensors, views of one arena that the
        next call overwrites.  check=True: one small device-to-host copy of the status words; a damaged file raises HipLibraryError
        naming its index and the reason.  check=False: no synchronisation, `self.status` (int32 [B]) stays on the device."""
        descs, out = self._run(files, None, check)
        return [out[descs[i].out_offset:descs[i].out_offset + descs[i].out_bytes].view(descs[i].height, descs[i].width, 3) for i in range(len(files))]

    def decode_into(self, files: Sequence[bytes], out: torch.Tensor, check: bool = True) -> torch.Tensor:
        """Equal-sized files into `out`, a contiguous CUDA uint8 [B,H,W,3] tensor on the decoder's device."""
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 4 and out.shape[-1] == 3
                and out.is_contiguous() and out.device == self.device):
            raise _lib.HipLibraryError(f"decode_into: out: expected a contiguous CUDA uint8 tensor [B,H,W,3] on {self.device}")
        if not isinstance(files, (list, tuple)) or len(files) != out.shape[0]:
            raise _lib.HipLibraryError(f"decode_into: {len(files) if isinstance(files, (list, tuple)) else type(files).__name__} files for out {tuple(out.shape)}")
        self._run(files, out, check)
        return out
