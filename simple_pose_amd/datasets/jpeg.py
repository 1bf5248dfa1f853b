"""JPEG decoding on the device: file bytes in, uint8 BGR images in HBM out (csrc/jpeg.hip behind sp_jpeg_parse /
sp_jpeg_decode_batch; csrc/jpeg_prog.hip behind sp_jpeg_parse_scans / sp_jpeg_progressive_entropy for progressive files).  The pixels are
libjpeg-turbo's default decode (what cv2.imread and PIL give) bit for bit.  EXIF orientation is not applied.  Accepted: 8-bit, 1 or 3
components, 4:4:4 / 4:2:2 / 4:2:0; baseline SOF0 with one interleaved scan, or progressive SOF2 with a complete progression (every
component's DC and zigzag coefficients 1..9 down to bit 0).  Anything else - incomplete progressions and multi-scan SOF0 among it -
raises HipLibraryError with the parser's reason: there is no CPU decode path.

    info = parse(open(path, "rb").read())                 # host only; baseline files
    info, scans = parse_scans(open(path, "rb").read())    # host only; progressive files
    dec = JpegDecoder("cuda:0")
    imgs = dec.decode([bytes, ...])                       # list of CUDA uint8 [H,W,3] BGR, views of one arena
    dec.decode_into([bytes, ...], frames)                 # equal-sized files into a [B,H,W,3] tensor (what estimate_batch takes)

The way back (csrc/jpeg_enc.hip behind sp_jpeg_enc_plan / sp_jpeg_encode_batch): uint8 BGR frames in HBM in, the bytes of baseline JPEG
files out, equal to what libjpeg-turbo writes with its defaults (PIL's save with optimize=False) byte for byte.

    enc = JpegEncoder("cuda:0", quality=75, subsampling="4:2:0", restart_interval=0)
    files = enc.encode(frames)                            # [B,H,W,3] CUDA uint8 BGR, or a list of [H,W,3] of any sizes -> list[bytes]
    arena, offsets, lengths = enc.encode_device(frames)   # no synchronisation; lengths int32 [B] on the device
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


@dataclass
class JpegScanInfo:
    components: Tuple[int, ...]                   # frame component indices, ascending; more than one: interleaved over the MCU grid
    ss: int
    se: int
    ah: int
    al: int
    restart_interval: int                         # MCUs per segment; blocks of the component when the scan has one component
    segments: int


def _parse_scans_raw(data: bytes, scan_buf, seg_buf: np.ndarray):
    """-> (JpegDesc, JpegScan array of the file's scans, int32 segment offsets, scan scratch, segment scratch).  The scratch arrays are
    replaced by larger ones when the file needs them, and returned for the caller to keep."""
    desc, count = _lib.JpegDesc(), ctypes.c_int32(0)
    lib = _lib.lib()
    for _ in range(2):
        rc = lib.sp_jpeg_parse_scans(data, len(data), ctypes.byref(desc), ctypes.addressof(scan_buf), len(scan_buf), ctypes.byref(count),
                                     seg_buf.ctypes.data, seg_buf.size)
        if rc != 0 or (count.value <= len(scan_buf) and desc.segments <= seg_buf.size):
            break
        if count.value > len(scan_buf):
            scan_buf = (_lib.JpegScan * count.value)()
        if desc.segments > seg_buf.size:
            seg_buf = np.empty(desc.segments, np.int32)
    _lib.check(rc, "sp_jpeg_parse_scans")
    scans = (_lib.JpegScan * count.value)()
    ctypes.memmove(scans, scan_buf, ctypes.sizeof(scans))
    return desc, scans, seg_buf[:desc.segments].copy(), scan_buf, seg_buf


def parse_scans(data) -> Tuple[JpegInfo, Tuple[JpegScanInfo, ...]]:
    """Headers and scan list of one progressive file (host only, no GPU call).  The JpegInfo has no Huffman tables (they are per scan) and
    the restart interval of the first scan; seg_offsets lists the segments of every scan, in file order.  Raises HipLibraryError with
    the reason for anything the decoder does not take - baseline files among it, which `parse` takes."""
    d, scans, segs, _, _ = _parse_scans_raw(_as_bytes(data), (_lib.JpegScan * 16)(), np.empty(1024, np.int32))
    n = d.components
    info = JpegInfo(d.width, d.height, n, tuple((d.h_samp[c], d.v_samp[c]) for c in range(n)), tuple(d.quant_sel[:n]), tuple(d.dc_sel[:n]),
                    tuple(d.ac_sel[:n]), d.restart_interval, (d.mcus_x, d.mcus_y), d.ecs_offset, d.ecs_end, tuple(int(s) for s in segs),
                    np.ctypeslib.as_array(d.quant).copy(), np.ctypeslib.as_array(d.huff_counts).copy(),
                    np.ctypeslib.as_array(d.huff_values).copy())
    return info, tuple(JpegScanInfo(tuple(s.comp[:s.components]), s.ss, s.se, s.ah, s.al, s.restart_interval, s.segments) for s in scans)


def _round_up(v: int, m: int = _ALIGN) -> int:
    return (v + m - 1) // m * m


class JpegDecoder:
    """Batched decoder with reusable arenas on one device.  `decode` / `decode_into` run on torch's current stream of that device: one
    pinned upload (descriptors, segment tables and file bytes in one buffer) and four launches (zero, entropy, IDCT, colour).  A batch
    with progressive files uploads their scan records in the same buffer and launches the entropy stage per kind (baseline files, then
    progressive ones: zero + entropy each) before one IDCT and one colour launch over all files.  The tensors `decode` returns are views
    of the output arena and are overwritten by the next call."""

    def __init__(self, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.HipLibraryError(f"JpegDecoder: device {dev}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        self.device = torch.device("cuda", _lib._device_index(dev))
        self._seg_scratch = np.empty(1024, np.int32)
        self._scan_scratch = (_lib.JpegScan * 16)()
        self._pinned = self._upload_done = None
        self._upload = self._coef = self._planes = self._out = None
        self.status = None                        # int32 [B] on the device after a call (0 = decoded; bits: _lib.SP_JPEG_STATUS)
        self.coefficients = None                  # (int16 arena, [offset per image], [count per image]) of the last call, for tests and tools
        self.relaunch = None                      # after a call: relaunch(stages=SP_JPEG_STAGE_ALL) runs the same batch again without an upload

    # ---- host side: parse every file, lay the arenas out ------------------------------------------------------------------------------------
    def _plan(self, files: Sequence):
        """-> (datas, descs, by_file, order, n_base, scans, scan_range, segs, arena sizes).  descs: [baseline files..., progressive files...]
        (n_base of the first kind), each with its own offsets, laid out in the caller's order; descs[k] is files[order[k]] and by_file[i]
        the descriptor of files[i] (a view into descs); scans: the progressive files' scan records, file k's at scan_range[k - n_base]."""
        if isinstance(files, (bytes, bytearray, memoryview, torch.Tensor)) or not isinstance(files, (list, tuple)):
            raise TypeError("files: expected a list or tuple of bytes objects (one per JPEG file)")
        datas = [_as_bytes(f, f"files[{i}]") for i, f in enumerate(files)]
        parsed = []                               # per file: (descriptor, segment offsets, scan records or None)
        file_at = coef_at = plane_at = out_at = 0
        for i, data in enumerate(datas):
            try:
                try:
                    d, s, self._seg_scratch = _parse_raw(data, self._seg_scratch)
                    scans = None
                except _lib.HipLibraryError as e:             # the baseline parser first; what it refuses as progressive goes to the scan parser
                    if getattr(e, "code", 0) != _lib.SP_JPEG_EPROGRESSIVE:
                        raise
                    d, scans, s, self._scan_scratch, self._seg_scratch = _parse_scans_raw(data, self._scan_scratch, self._seg_scratch)
            except _lib.HipLibraryError as e:
                raise _lib.HipLibraryError(f"files[{i}]: {e}") from None
            d.file_offset, d.coef_offset, d.plane_offset, d.out_offset = file_at, coef_at, plane_at, out_at
            parsed.append((d, s, scans))
            file_at += _round_up(len(data))
            coef_at += _round_up(d.coef_count * 2) // 2
            plane_at += _round_up(d.plane_bytes)
            out_at += _round_up(d.out_bytes)
        order = [i for i, p in enumerate(parsed) if p[2] is None] + [i for i, p in enumerate(parsed) if p[2] is not None]
        n_base = sum(p[2] is None for p in parsed)
        descs = (_lib.JpegDesc * max(1, len(datas)))()
        segs, scan_range, seg_at = [], [0], 0
        for k, i in enumerate(order):
            d, s, scans = parsed[i]
            d.seg_index = seg_at
            descs[k] = d
            segs.append(s)
            seg_at += len(s)
            if scans is not None:
                scan_range.append(scan_range[-1] + len(scans))
        scans = (_lib.JpegScan * max(1, scan_range[-1]))()
        at = 0
        for i in order[n_base:]:
            ctypes.memmove(ctypes.byref(scans, at * ctypes.sizeof(_lib.JpegScan)), parsed[i][2], ctypes.sizeof(parsed[i][2]))
            at += len(parsed[i][2])
        by_file = [None] * len(datas)
        for k, i in enumerate(order):
            by_file[i] = descs[k]
        return datas, descs, by_file, order, n_base, scans, scan_range, segs, (seg_at, file_at, coef_at, plane_at, out_at)

    def _grow(self, name: str, size: int, dtype):
        t = getattr(self, name)
        if t is None or t.numel() < size:
            t = torch.empty(max(size, 1), dtype=dtype, device=self.device)
            setattr(self, name, t)
        return t

    def _run(self, files, out_tensor=None, check=True):
        datas, descs, by_file, order, n_base, scans, scan_range, segs, (n_seg, n_bytes, n_coef, n_plane, n_out) = self._plan(files)
        n = len(datas)
        n_prog, n_scans = n - n_base, scan_range[-1]
        if out_tensor is not None:
            for i in range(n):
                if (by_file[i].height, by_file[i].width) != tuple(out_tensor.shape[1:3]):
                    raise _lib.HipLibraryError(f"decode_into: files[{i}] is {by_file[i].width}x{by_file[i].height}, out holds "
                                               f"{out_tensor.shape[2]}x{out_tensor.shape[1]} frames")
                by_file[i].out_offset = i * by_file[0].out_bytes
            n_out = n * by_file[0].out_bytes if n else 0
        # one upload: [descriptors | segment offsets | scan records | scan ranges | caller's order | file bytes]; the three in the middle
        # are empty without progressive files
        desc_size, scan_size = ctypes.sizeof(_lib.JpegDesc), ctypes.sizeof(_lib.JpegScan)
        desc_bytes = desc_size * n
        seg_off = _round_up(desc_bytes)
        scan_off = _round_up(seg_off + 4 * n_seg)
        range_off = _round_up(scan_off + scan_size * n_scans)
        perm_off = _round_up(range_off + (4 * (n_prog + 1) if n_prog else 0))
        byte_off = _round_up(perm_off + (8 * n if n_prog else 0))
        total = byte_off + n_bytes
        if self._upload_done is not None:
            self._upload_done.synchronize()       # the previous call's copy out of the pinned buffer (check=False does not wait for it)
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
        host = self._pinned.numpy()
        if n:
            host[:desc_bytes] = np.frombuffer(descs, np.uint8, desc_bytes)
            host[seg_off:seg_off + 4 * n_seg] = np.concatenate(segs).astype(np.int32).view(np.uint8)
        if n_prog:
            host[scan_off:scan_off + scan_size * n_scans] = np.frombuffer(scans, np.uint8, scan_size * n_scans)
            host[range_off:range_off + 4 * (n_prog + 1)] = np.asarray(scan_range, np.int32).view(np.uint8)
            where = np.empty(n, np.int64)
            where[order] = np.arange(n)           # files[i] is descriptor where[i]
            host[perm_off:perm_off + 8 * n] = where.view(np.uint8)
        for i, data in enumerate(datas):
            o = byte_off + by_file[i].file_offset
            host[o:o + len(data)] = np.frombuffer(data, np.uint8)
        up = self._grow("_upload", total, torch.uint8)
        coef = self._grow("_coef", n_coef, torch.int16)
        planes = self._grow("_planes", n_plane, torch.uint8)
        out = out_tensor if out_tensor is not None else self._grow("_out", n_out, torch.uint8)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        range_host = (ctypes.c_int32 * (n_prog + 1))(*scan_range)
        with torch.cuda.device(self.device):
            up[:total].copy_(self._pinned[:total], non_blocking=True)
            self._upload_done = torch.cuda.Event()
            self._upload_done.record()
            base = up.data_ptr()
            where_dev = up[perm_off:perm_off + 8 * n].view(torch.int64) if n_prog else None

            def batch(first, count, stages):
                _lib.check(_lib.lib().sp_jpeg_decode_batch(ctypes.addressof(descs) + first * desc_size, base + first * desc_size, count, base + byte_off,
                                                           n_bytes, base + seg_off, n_seg, _lib.ptr(coef), coef.numel(), _lib.ptr(planes),
                                                           planes.numel(), _lib.ptr(out), out.numel(), status.data_ptr() + 4 * first, stages,
                                                           _lib.current_stream(self.device)), "sp_jpeg_decode_batch")

            def launch(stages=_lib.SP_JPEG_STAGE_ALL):
                if not n_prog:                    # baseline files only: the one call there has always been
                    batch(0, n, stages)
                    self.status = status
                    return
                if stages & _lib.SP_JPEG_STAGE_ENTROPY:
                    if n_base:
                        batch(0, n_base, _lib.SP_JPEG_STAGE_ENTROPY)
                    _lib.check(_lib.lib().sp_jpeg_progressive_entropy(
                        ctypes.addressof(descs) + n_base * desc_size, base + n_base * desc_size, n_prog, scans, base + scan_off, range_host,
                        base + range_off, n_scans, base + byte_off, n_bytes, base + seg_off, n_seg, _lib.ptr(coef), coef.numel(),
                        status.data_ptr() + 4 * n_base, _lib.current_stream(self.device)), "sp_jpeg_progressive_entropy")
                    self.status = status.index_select(0, where_dev)      # the caller's file order
                if stages & ~_lib.SP_JPEG_STAGE_ENTROPY:
                    batch(0, n, stages & ~_lib.SP_JPEG_STAGE_ENTROPY)    # writes no status
            launch()
        self.relaunch = launch                    # tools/bench_jpeg.py: the same batch again, or one stage of it (SP_JPEG_STAGE_*), no upload
        self.coefficients = (coef, [by_file[i].coef_offset for i in range(n)], [by_file[i].coef_count for i in range(n)])
        if check and n:
            st = self.status.cpu().numpy()
            bad = np.nonzero(st)[0]
            if bad.size:
                i = int(bad[0])
                why = ", ".join(t for b, t in _lib.SP_JPEG_STATUS.items() if st[i] & b)
                raise _lib.HipLibraryError(f"JpegDecoder: files[{i}] is damaged (status {int(st[i])}: {why}); {bad.size} of {n} files failed")
        return by_file, out

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


_SUBSAMPLING = {"4:4:4": 444, "4:2:2": 422, "4:2:0": 420, 444: 444, 422: 422, 420: 420}


class JpegEncoder:
    """Batched encoder with reusable arenas on one device.  `encode` / `encode_device` run on torch's current stream of that device: one
    pinned upload (the descriptors) and the launches of sp_jpeg_encode_batch (include/simple_pose_hip.h lists them).  What
    `encode_device` returns are views of arenas that the next call overwrites.  There is no CPU encode path."""

    def __init__(self, device="cuda", quality: int = 75, subsampling="4:2:0", restart_interval: int = 0):
        if subsampling not in _SUBSAMPLING:
            raise _lib.HipLibraryError(f"JpegEncoder: subsampling {subsampling!r}; expected '4:4:4', '4:2:2' or '4:2:0'")
        for name, v in (("quality", quality), ("restart_interval", restart_interval)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"JpegEncoder: {name}: expected an int, got {type(v).__name__}")
        self.quality, self.subsampling, self.restart_interval = quality, _SUBSAMPLING[subsampling], restart_interval
        self._plans = {}
        self._plan_for(8, 8)                      # quality / restart interval out of range: the planner's own refusal, before any GPU call
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.HipLibraryError(f"JpegEncoder: device {dev}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        self.device = torch.device("cuda", _lib._device_index(dev))
        self._pinned = self._upload_done = self._host_out = None
        self._upload = self._ws = self._out = None
        self.status = None                        # int32 [B] on the device after a call (0 = encoded, SP_JPEG_ENC_STATUS_OVERFLOW = does not fit)
        self.lengths = None                       # int32 [B] on the device after a call
        self.descs = None                         # the last call's descriptors (host copy)
        self.coefficients = None                  # (int16 view of the workspace, [offset per image], [count per image]) of the last call, for tests
        self.relaunch = None                      # after a call: relaunch(stages=SP_JPEG_ENC_STAGE_ALL) runs the same batch again without an upload

    # ---- host side ------------------------------------------------------------------------------------------------------------------------------
    def _plan_for(self, w: int, h: int):
        d = self._plans.get((w, h))
        if d is None:
            d = _lib.JpegEncDesc()
            _lib.check(_lib.lib().sp_jpeg_enc_plan(w, h, self.subsampling, self.quality, self.restart_interval, ctypes.byref(d)), "sp_jpeg_enc_plan")
            if len(self._plans) < 64:
                self._plans[(w, h)] = d
        return d

    def _frames(self, frames):
        """-> list of contiguous CUDA uint8 [H,W,3] tensors on the encoder's device."""
        if isinstance(frames, torch.Tensor):
            if frames.dim() != 4:
                raise _lib.HipLibraryError(f"frames: expected a uint8 tensor [B,H,W,3] or a list of [H,W,3] tensors, got shape {tuple(frames.shape)}")
            self._check_frame(frames, "frames", 4)
            return [frames[i] for i in range(frames.shape[0])]
        if not isinstance(frames, (list, tuple)):
            raise TypeError(f"frames: expected a uint8 tensor [B,H,W,3] or a list of [H,W,3] tensors, got {type(frames).__name__}")
        for i, f in enumerate(frames):
            self._check_frame(f, f"frames[{i}]", 3)
        return list(frames)

    def _check_frame(self, f, what, dims):
        if not isinstance(f, torch.Tensor):
            raise TypeError(f"{what}: expected a torch.Tensor, got {type(f).__name__}")
        if f.dtype != torch.uint8:
            raise TypeError(f"{what}: expected uint8, got {f.dtype}")
        if not f.is_cuda or f.device != self.device:
            raise _lib.HipLibraryError(f"{what}: tensor is on {f.device}, the encoder on {self.device} (no CPU fallback)")
        if f.dim() != dims or f.shape[-1] != 3 or not f.is_contiguous() or f.shape[-2] < 1 or f.shape[-3] < 1:
            raise _lib.HipLibraryError(f"{what}: expected a contiguous BGR image{'s' if dims == 4 else ''} [{'B,' if dims == 4 else ''}H,W,3], got shape "
                                       f"{tuple(f.shape)}, strides {tuple(f.stride())}")

    def default_capacity(self, w: int, h: int) -> int:
        """Bytes reserved for one file unless the caller says otherwise: header + width * height * 3, rounded up to 64."""
        return _round_up(self._plan_for(w, h).header_bytes + w * h * 3)

    def _grow(self, name: str, size: int):
        t = getattr(self, name)
        if t is None or t.numel() < size:
            t = torch.empty(max(size, 1), dtype=torch.uint8, device=self.device)
            setattr(self, name, t)
        return t

    # ---- public ---------------------------------------------------------------------------------------------------------------------------------
    def encode_device(self, frames, capacity=None):
        """One batch of frames ([B,H,W,3] or a list of [H,W,3] of any sizes; CUDA uint8 BGR, contiguous) -> (arena, offsets, lengths): file i
        is arena[offsets[i] : offsets[i] + lengths[i]], `lengths` an int32 [B] tensor on the device.  Nothing synchronises.  `capacity`:
        bytes reserved per file (default: default_capacity); a file that does not fit has length 0 and SP_JPEG_ENC_STATUS_OVERFLOW in
        `self.status`, and nothing of it is written."""
        imgs = self._frames(frames)
        n = len(imgs)
        if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0 or capacity > 2 ** 31 - 1):
            raise _lib.HipLibraryError(f"encode_device: capacity {capacity!r}; expected 0 .. 2^31 - 1 bytes")
        descs = (_lib.JpegEncDesc * max(1, n))()
        ws_at = out_at = 0
        for i, f in enumerate(imgs):
            h, w = int(f.shape[0]), int(f.shape[1])
            try:
                plan = self._plan_for(w, h)
            except _lib.HipLibraryError as e:
                raise _lib.HipLibraryError(f"frames[{i}]: {e}") from None
            ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(plan), ctypes.sizeof(_lib.JpegEncDesc))
            d = descs[i]
            d.src, d.ws_offset, d.out_offset = f.data_ptr(), ws_at, out_at
            d.out_capacity = self.default_capacity(w, h) if capacity is None else capacity
            ws_at += _round_up(d.ws_bytes + _lib.jpeg_enc_stream_ws(d.out_capacity))
            out_at += _round_up(d.out_capacity)
        desc_bytes = ctypes.sizeof(_lib.JpegEncDesc) * n
        if self._upload_done is not None:
            self._upload_done.synchronize()       # the previous call's copy out of the pinned buffer
        if self._pinned is None or self._pinned.numel() < desc_bytes:
            self._pinned = torch.empty(max(desc_bytes, 1), dtype=torch.uint8).pin_memory()
        if n:
            self._pinned.numpy()[:desc_bytes] = np.frombuffer(descs, np.uint8, desc_bytes)
        up = self._grow("_upload", desc_bytes)
        ws = self._grow("_ws", ws_at)
        out = self._grow("_out", out_at)
        lengths = torch.empty(n, dtype=torch.int32, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            up[:desc_bytes].copy_(self._pinned[:desc_bytes], non_blocking=True)
            self._upload_done = torch.cuda.Event()
            self._upload_done.record()

            def launch(stages=_lib.SP_JPEG_ENC_STAGE_ALL):
                _lib.check(_lib.lib().sp_jpeg_encode_batch(descs, _lib.ptr(up), n, _lib.ptr(ws), ws.numel(), _lib.ptr(out), out.numel(), _lib.ptr(lengths),
                                                           _lib.ptr(status), stages, _lib.current_stream(self.device)), "sp_jpeg_encode_batch")
            launch()
        self.relaunch, self.status, self.lengths, self.descs = launch, status, lengths, descs
        self.coefficients = (ws.view(torch.int16), [(descs[i].ws_offset + descs[i].ws_coef) // 2 for i in range(n)], [descs[i].blocks * 64 for i in range(n)])
        return out, [descs[i].out_offset for i in range(n)], lengths

    def encode(self, frames, capacity=None) -> List[bytes]:
        """-> the files as bytes objects.  One small device-to-host copy of the lengths and status words, then each file's own bytes (not
        its capacity) into one pinned buffer.  A file that does not fit its capacity raises HipLibraryError naming its index."""
        return self.collect(*self.encode_device(frames, capacity))

    def collect(self, out, offsets, lengths) -> List[bytes]:
        """What `encode_device` returned -> the files as bytes objects (the second half of `encode`; waits for the stream)."""
        n = len(offsets)
        if n == 0:
            return []
        meta = torch.stack([lengths, self.status]).cpu().numpy()
        bad = np.nonzero(meta[1])[0]
        if bad.size:
            i = int(bad[0])
            raise _lib.HipLibraryError(f"JpegEncoder: frames[{i}] does not fit its {self.descs[i].out_capacity} bytes (status {int(meta[1][i])}: "
                                       f"overflow); {bad.size} of {n} files failed")
        at = np.concatenate([[0], np.cumsum(meta[0])]).astype(np.int64)
        if self._host_out is None or self._host_out.numel() < at[-1]:
            self._host_out = torch.empty(int(at[-1]), dtype=torch.uint8).pin_memory()
        with torch.cuda.device(self.device):
            for i in range(n):
                self._host_out[at[i]:at[i + 1]].copy_(out[offsets[i]:offsets[i] + int(meta[0][i])], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        host = self._host_out.numpy()
        return [host[at[i]:at[i + 1]].tobytes() for i in range(n)]
