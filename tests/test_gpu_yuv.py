"""YUV 4:2:0 <-> BGR on the MI355X: the kernels of simple_pose_amd/csrc/yuv.hip against tests/yuv_ref.py bit for bit (the edge shapes with
pitches, base offsets and guard bytes; every (Y, U, V) and every colour once), the table launch against the single-frame calls,
simple_pose_amd.video, and YuvFrame inputs through the estimator and the trackers against the same frames converted first."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import MultiStreamTracker, PoseTracker
from simple_pose_amd.video import YuvFrame, from_bgr, to_bgr
from simple_pose_amd.visualize import PoseRenderer
from tests import yuv_ref
from tests.detector_ref import detector_state_dict
from tests.yuv_ref import BT601, BT709, FULL, I420, LIMITED, MODES, NV12

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 3), (17, 23), (16, 64), (33, 130))
FMT_IDS = {NV12: "nv12", I420: "i420"}
MODE_IDS = ["bt601-full", "bt601-limited", "bt709-full", "bt709-limited"]


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _chroma_bytes(w, fmt):
    cw = (w + 1) // 2
    return 2 * cw if fmt == NV12 else cw


def _random_planes(rng, h, w, fmt):
    ch = (h + 1) // 2
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if fmt == NV12:
        return (y, rng.integers(0, 256, (ch, _chroma_bytes(w, fmt)), dtype=np.uint8))
    return (y, rng.integers(0, 256, (ch, (w + 1) // 2), dtype=np.uint8), rng.integers(0, 256, (ch, (w + 1) // 2), dtype=np.uint8))


class _Dev:
    """A tight plane in a pitched device buffer filled with 0xA5, one guard row before and after, the plane `offset` bytes off the row."""

    def __init__(self, plane, pitch, offset):
        self.rows, self.rb, self.pitch = plane.shape[0], plane.shape[1], pitch
        buf, self.start = yuv_ref.pitched(plane, pitch, offset, guard_rows=1)
        self.buf = torch.from_numpy(buf).to(DEV)
        self.ptr = self.buf.data_ptr() + self.start

    def read(self):
        """(the plane, True when every byte outside the plane's rows is still 0xA5)."""
        plane, rest = yuv_ref.unpitch(self.buf.cpu().numpy(), self.start, self.rows, self.rb, self.pitch)
        return plane, bool((rest == 0xA5).all())


def _blank(rows, rb):
    return np.full((rows, rb), 0xA5, np.uint8)


def _decode_case(rng, h, w, fmt, mode, py, pc, pb, offset):
    planes = _random_planes(rng, h, w, fmt)
    d = [_Dev(p, pitch, offset) for p, pitch in zip(planes, (py, pc, pc))]
    out = _Dev(_blank(h, 3 * w), pb, offset)
    ptrs = [x.ptr for x in d] + [None] * (3 - len(d))
    wide = _lib.lib().sp_yuv420_wide_path(ptrs[0], ptrs[1], ptrs[2], out.ptr, py, pc, pb, fmt)
    _lib.check(_lib.lib().sp_yuv420_to_bgr_u8c3(ptrs[0], ptrs[1], ptrs[2], h, w, py, pc, fmt, mode[0], mode[1], out.ptr, pb, _stream()), "to_bgr")
    got, clean = out.read()
    want = yuv_ref.yuv420_to_bgr(planes, h, w, fmt, *mode).reshape(h, 3 * w)
    tag = f"to_bgr {h}x{w} {FMT_IDS[fmt]} {mode} pitch {py}/{pc}/{pb} offset {offset}"
    np.testing.assert_array_equal(got, want, err_msg=tag)
    assert clean, tag + ": a byte outside the image rows was written"
    return wide


def _encode_case(rng, h, w, fmt, mode, py, pc, pb, offset):
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    src = _Dev(bgr.reshape(h, 3 * w), pb, offset)
    ch, cb = (h + 1) // 2, _chroma_bytes(w, fmt)
    outs = [_Dev(_blank(h, w), py, offset), _Dev(_blank(ch, cb), pc, offset)] + ([_Dev(_blank(ch, cb), pc, offset)] if fmt == I420 else [])
    ptrs = [x.ptr for x in outs] + [None] * (3 - len(outs))
    wide = _lib.lib().sp_yuv420_wide_path(ptrs[0], ptrs[1], ptrs[2], src.ptr, py, pc, pb, fmt)
    _lib.check(_lib.lib().sp_bgr_to_yuv420_u8c3(src.ptr, pb, h, w, fmt, mode[0], mode[1], ptrs[0], ptrs[1], ptrs[2], py, pc, _stream()), "from_bgr")
    want = yuv_ref.bgr_to_yuv420(bgr, fmt, *mode)
    tag = f"from_bgr {h}x{w} {FMT_IDS[fmt]} {mode} pitch {py}/{pc}/{pb} offset {offset}"
    for name, o, wnt in zip("YUV", outs, want):
        got, clean = o.read()
        np.testing.assert_array_equal(got, wnt, err_msg=f"{tag} plane {name}")
        assert clean, f"{tag}: a byte outside plane {name}'s rows was written"
    return wide


# ---- 1. edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (NV12, I420), ids=("nv12", "i420"))
@pytest.mark.parametrize("case", (_decode_case, _encode_case), ids=("to_bgr", "from_bgr"))
def test_edge_shapes_pitches_and_offsets_bit_for_bit(case, fmt):
    rng = np.random.default_rng(40 + fmt)
    k = 0
    for h, w in SHAPES:
        for pad in (0, 13):
            for offset in (0, 1):
                case(rng, h, w, fmt, MODES[k % 4], w + pad, _chroma_bytes(w, fmt) + pad, 3 * w + pad, offset)
                k += 1
    # 33x130 in 16-byte pitches: full patches on the 16-byte path next to two tail columns and the odd last row; the same frame one byte
    # off its base goes byte by byte (sp_yuv420_wide_path is the predicate the kernels evaluate)
    pc = 144 if fmt == NV12 else 80
    for mode in MODES:
        assert case(rng, 33, 130, fmt, mode, 144, pc, 400, 0) == 1
        assert case(rng, 33, 130, fmt, mode, 144, pc, 400, 1) == 0
    assert case(rng, 16, 64, fmt, MODES[0], 64, 64 if fmt == NV12 else 32, 192, 0) == 1              # tight and still aligned: no tail at all


# ---- 2. / 3. every triple once ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every_yuv():
    """4096x4096 NV12 in which every (Y, U, V) occurs once: chroma block b = 2048 i + j holds the UV pair b >> 6 and the luma 4 (b & 63) + 0..3."""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    pair, k = b >> 6, b & 63
    uv = np.empty((2048, 4096), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = pair >> 8, pair & 255
    y = np.empty((4096, 4096), np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = 4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3
    code = (y.astype(np.int64) << 16) | (np.repeat(np.repeat(pair, 2, 0), 2, 1))
    assert np.unique(code).size == 1 << 24
    return (y, uv), (torch.from_numpy(y).to(DEV), torch.from_numpy(uv).to(DEV))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_yuv_triple_decodes_as_the_reference(every_yuv, mode):
    (y, uv), (dy, duv) = every_yuv
    f = YuvFrame((dy, duv), 4096, 4096, "nv12", "bt709" if mode[0] == BT709 else "bt601", mode[1] == FULL)
    got = to_bgr(f).cpu().numpy()
    np.testing.assert_array_equal(got, yuv_ref.yuv420_to_bgr((y, uv), 4096, 4096, NV12, *mode))


def test_every_yuv_triple_decodes_from_i420_planes(every_yuv):
    (y, uv), (dy, duv) = every_yuv
    du, dv = duv[:, 0::2].contiguous(), duv[:, 1::2].contiguous()
    got = to_bgr(YuvFrame((dy, du, dv), 4096, 4096, "i420", "bt709", False)).cpu().numpy()
    np.testing.assert_array_equal(got, yuv_ref.yuv420_to_bgr((y, uv), 4096, 4096, NV12, BT709, LIMITED))


@pytest.fixture(scope="module")
def every_colour():
    """4096x4096 BGR holding every colour once, scrambled (an odd multiplier mod 2^24) so that the four pixels of a 2x2 block differ."""
    n = (np.arange(1 << 24, dtype=np.int64) * 0x9E3779) & 0xFFFFFF
    assert np.unique(n).size == 1 << 24
    bgr = np.stack([n & 255, (n >> 8) & 255, n >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    return bgr, torch.from_numpy(bgr).to(DEV)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_colour_encodes_as_the_reference(every_colour, mode):
    bgr, dbgr = every_colour
    fmt = "nv12" if mode[1] == FULL else "i420"                  # both layouts over the four modes
    f = from_bgr(dbgr, fmt, "bt709" if mode[0] == BT709 else "bt601", mode[1] == FULL)
    want = yuv_ref.bgr_to_yuv420(bgr, NV12 if fmt == "nv12" else I420, *mode)
    assert f.pitch_y % 16 == 0 and f.pitch_c % 16 == 0
    for name, got, w in zip("YUV", f.planes, want):
        np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=name)
    lo, hi = (0, 255) if mode[1] == FULL else (16, 235)
    y = f.planes[0].cpu().numpy()
    assert y.min() == lo and y.max() == hi


# ---- 4. the table launch ------------------------------------------------------------------------------------------------------------------------
def _table(entries):
    refs = (_lib.YuvRef * len(entries))()
    for r, e in zip(refs, entries):
        for k, v in e.items():
            setattr(r, k, v)
    raw = np.frombuffer(bytes(refs), np.uint8).copy()
    return torch.from_numpy(raw).to(DEV)


def test_table_launch_equals_single_calls_bit_for_bit():
    rng = np.random.default_rng(44)
    lib = _lib.lib()
    specs = ((33, 130, NV12, MODES[0], 144, 144, 400, 0), (17, 23, I420, MODES[1], 23, 12, 69, 1), (64, 48, I420, MODES[2], 48, 32, 144, 0),
             (5, 3, NV12, MODES[3], 16, 17, 22, 1))
    for to_bgr_dir in (True, False):
        single, tabled, entries = [], [], []
        for h, w, fmt, mode, py, pc, pb, offset in specs:
            ch, cb = (h + 1) // 2, _chroma_bytes(w, fmt)
            planes = _random_planes(rng, h, w, fmt) if to_bgr_dir else [_blank(h, w)] + [_blank(ch, cb)] * (2 if fmt == I420 else 1)
            bgr = _blank(h, 3 * w) if to_bgr_dir else rng.integers(0, 256, (h, 3 * w), dtype=np.uint8)
            for store in (single, tabled):
                store.append(([_Dev(p, pitch, offset) for p, pitch in zip(planes, (py, pc, pc))], _Dev(bgr, pb, offset)))
            (p1, b1), (p2, b2) = single[-1], tabled[-1]
            ptrs = [x.ptr for x in p1] + [None] * (3 - len(p1))
            if to_bgr_dir:
                _lib.check(lib.sp_yuv420_to_bgr_u8c3(ptrs[0], ptrs[1], ptrs[2], h, w, py, pc, fmt, mode[0], mode[1], b1.ptr, pb, _stream()), "single")
            else:
                _lib.check(lib.sp_bgr_to_yuv420_u8c3(b1.ptr, pb, h, w, fmt, mode[0], mode[1], ptrs[0], ptrs[1], ptrs[2], py, pc, _stream()), "single")
            entries.append(dict(y=p2[0].ptr, u=p2[1].ptr, v=p2[2].ptr if fmt == I420 else 0, bgr=b2.ptr, h=h, w=w, pitch_y=py, pitch_c=pc, pitch_bgr=pb,
                                format=fmt, matrix=mode[0], range=mode[1]))
        table = _table(entries)
        fn = lib.sp_yuv420_to_bgr_images_u8c3 if to_bgr_dir else lib.sp_bgr_to_yuv420_images_u8c3
        assert fn(None, 0, 0, 0, _stream()) == 0 and fn(table.data_ptr(), 0, 64, 130, _stream()) == 0        # count == 0: nothing happens
        torch.cuda.synchronize()
        outs = lambda store: [b.buf.cpu().numpy() for _, b in store] if to_bgr_dir else [x.buf.cpu().numpy() for p, _ in store for x in p]
        assert all((o == 0xA5).all() for o in outs(tabled))     # ... to any output
        _lib.check(fn(table.data_ptr(), len(specs), 64, 130, _stream()), "table")
        first = outs(tabled)
        for a, b in zip(outs(single), first):
            np.testing.assert_array_equal(a, b)                 # the whole buffers: image rows, padding and guard rows alike
        assert any((a != 0xA5).any() for a in first)
        _lib.check(fn(table.data_ptr(), len(specs), 64, 130, _stream()), "table")
        for a, b in zip(first, outs(tabled)):
            np.testing.assert_array_equal(a, b)                 # a second identical launch: identical bytes


# ---- 5. host-fed frames ----------------------------------------------------------------------------------------------------------------------------
def test_host_planes_convert_as_device_planes():
    rng = np.random.default_rng(45)
    host, dev, want = [], [], []
    for (h, w), fmt, mode in zip(((37, 51), (64, 96), (1, 1)), (I420, NV12, I420), (MODES[1], MODES[2], MODES[3])):
        planes = _random_planes(rng, h, w, fmt)
        names = ("nv12" if fmt == NV12 else "i420", "bt709" if mode[0] == BT709 else "bt601", mode[1] == FULL)
        if fmt == I420:                                         # ffmpeg's packed yuv420p buffer
            host.append(YuvFrame.from_i420(np.concatenate([p.reshape(-1) for p in planes]), h, w, *names[1:]))
        else:
            host.append(YuvFrame(planes, h, w, *names))
        dev.append(YuvFrame(tuple(torch.from_numpy(p).to(DEV) for p in planes), h, w, *names))
        want.append(yuv_ref.yuv420_to_bgr(planes, h, w, fmt, *mode))
    a, b = to_bgr(host, device=DEV), to_bgr(dev)
    for x, y, w in zip(a, b, want):
        assert x.is_cuda and torch.equal(x, y)
        np.testing.assert_array_equal(x.cpu().numpy(), w)
    one = to_bgr(host[0], device=DEV)
    assert torch.equal(one, a[0])
    out = torch.full((64, 128, 3), 0xA5, dtype=torch.uint8, device=DEV)           # `out`: a pitched view
    assert to_bgr(dev[1], out=out[:, :96]) .data_ptr() == out.data_ptr()
    assert torch.equal(out[:, :96], b[1]) and bool((out[:, 96:] == 0xA5).all())
    back = from_bgr([x for x in b], "i420", "bt601", True)                     # a list the other way: one table launch
    for f, x in zip(back, b):
        for got, w in zip(f.planes, yuv_ref.bgr_to_yuv420(x.cpu().numpy(), I420, BT601, FULL)):
            np.testing.assert_array_equal(got.cpu().numpy(), w)


# ---- 6. the pipeline ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    d = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))
    conf, iou, _ = golden("g14_detector.npz")["sp_a_thresh"]
    d.conf_thresh, d.iou_thresh = float(conf), float(iou)
    return d


@pytest.fixture(scope="module")
def dconv():
    from oracle import nets_oracle
    from simple_pose_amd.nets import pose_resnet_dconv
    m = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50("dconv"), 0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.compute_dtype = "fp32"
    m.autotune = False
    return m


def _nv12_surface(img, matrix="bt601", full=False, pitch_to=64):
    """The image as a decoder would hand it over: an NV12 surface in HBM, Y rows then UV rows at one pitch."""
    h, w = img.shape[:2]
    y, uv = yuv_ref.bgr_to_yuv420(img, NV12, BT709 if matrix == "bt709" else BT601, FULL if full else LIMITED)
    pitch = (uv.shape[1] + pitch_to - 1) // pitch_to * pitch_to
    buf = np.zeros((h + uv.shape[0], pitch), np.uint8)
    buf[:h, :w], buf[h:, :uv.shape[1]] = y, uv
    return YuvFrame.from_surface(torch.from_numpy(buf).to(DEV), h, w, pitch, matrix, full)


def _i420_host(img, matrix="bt709", full=True):
    h, w = img.shape[:2]
    planes = yuv_ref.bgr_to_yuv420(img, I420, BT709 if matrix == "bt709" else BT601, FULL if full else LIMITED)
    return YuvFrame.from_i420(np.concatenate([p.reshape(-1) for p in planes]), h, w, matrix, full)


def _same(got, want, tag=""):
    assert len(got) == len(want), tag
    for name in ("keypoints", "score", "box", "track_id", "keypoints_smooth"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), (tag, name)
        if a is not None:
            np.testing.assert_array_equal(a, b, err_msg=f"{tag} {name}")
    assert got.dropped == want.dropped, tag


@pytest.fixture(scope="module")
def frames(golden):
    a = np.ascontiguousarray(golden("g14_detector.npz")["sp_a_image"])
    b = np.ascontiguousarray(np.roll(a, 6, axis=1))
    return {"a": a, "b": b, "fa": _nv12_surface(a), "fb": _i420_host(b), "small": np.ascontiguousarray(a[:, :a.shape[1] - 64])}


def test_frames_convert_as_the_reference(frames):
    a, fa, fb = frames["a"], frames["fa"], frames["fb"]
    h, w = a.shape[:2]
    planes = yuv_ref.bgr_to_yuv420(a, NV12, BT601, LIMITED)
    np.testing.assert_array_equal(to_bgr(fa).cpu().numpy(), yuv_ref.yuv420_to_bgr(planes, h, w, NV12, BT601, LIMITED))
    planes = yuv_ref.bgr_to_yuv420(frames["b"], I420, BT709, FULL)
    np.testing.assert_array_equal(to_bgr(fb, device=DEV).cpu().numpy(), yuv_ref.yuv420_to_bgr(planes, h, w, I420, BT709, FULL))


def test_estimate_takes_a_frame_graph_and_eager(frames, detector, dconv):
    est = TopDownPoseEstimator(detector, dconv, capacity=32)
    bgr = to_bgr(frames["fa"])
    for graph in (False, True, True):
        est.use_graph = graph
        want, got = est.estimate(bgr), est.estimate(frames["fa"])
        assert len(want) >= 1                                   # cannot pass on nothing
        _same(got, want, f"graph={graph}")
    assert len(est._frames) == 1                                # the frame went into the same static source, through the same graph
    host = est.estimate(frames["fb"])
    _same(host, est.estimate(to_bgr(frames["fb"], device=DEV)), "host i420")
    boxes = np.array([[50, 60, 200, 400, 0.9, 0], [300, 20, 500, 460, 0.8, 0]], np.float32)
    _same(est.estimate_boxes(frames["fa"], boxes)[0], est.estimate_boxes(bgr, boxes)[0], "estimate_boxes")
    d = detector.single_predict(frames["fa"])
    assert torch.equal(d, detector.single_predict(bgr)) and d.shape[0] >= 1


def test_estimate_batch_takes_frames_same_sized_and_mixed(frames, detector, dconv):
    est = TopDownPoseEstimator(detector, dconv, capacity=32)
    fa, fb = frames["fa"], frames["fb"]
    ba, bb = to_bgr(fa), to_bgr(fb, device=DEV)
    got, want = est.estimate_batch([fa, fb]), est.estimate_batch([ba, bb])
    assert sum(len(r) for r in want) >= 2
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"same-sized {i}")
    got, want = est.estimate_batch([fa, frames["small"]]), est.estimate_batch([ba, frames["small"]])     # two sizes, one of them BGR
    assert len(want[0]) >= 1
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"mixed {i}")
    p, q = detector.predict([fa, frames["small"]]), detector.predict([ba, frames["small"]])
    assert all(torch.equal(x, y) for x, y in zip(p, q)) and p[0].shape[0] >= 1


def test_trackers_take_frames(frames, detector, dconv):
    est = TopDownPoseEstimator(detector, dconv, capacity=32)
    fa, fb = frames["fa"], frames["fb"]
    ba, bb = to_bgr(fa), to_bgr(fb, device=DEV)
    one, ref = PoseTracker(est, detect_every=2), PoseTracker(est, detect_every=2)
    kinds = []
    for k, (f, b) in enumerate(((fa, ba), (fb, bb), (fa, ba))):
        want, got = ref.update(b), one.update(f)
        assert one.last_frame_kind == ref.last_frame_kind
        kinds.append(one.last_frame_kind)
        _same(got, want, f"frame {k}")
        assert got.track_id is not None
    assert kinds == ["detector", "propagated", "detector"] and len(want) >= 1
    multi, mref = MultiStreamTracker(est, streams=2, detect_every=2), MultiStreamTracker(est, streams=2, detect_every=2)
    for k, (fs, bs) in enumerate((([fa, fb], [ba, bb]), ([fb, fa], [bb, ba]))):
        want, got = mref.update(bs), multi.update(fs)
        assert multi.last_frame_kind == mref.last_frame_kind
        for s in range(2):
            _same(got[s], want[s], f"call {k} stream {s}")
    assert sum(len(r) for r in want) >= 2


def test_canvas_leaves_as_nv12(frames, detector, dconv):
    est = TopDownPoseEstimator(detector, dconv, capacity=32, renderer=PoseRenderer())
    res = est.estimate(frames["fa"])
    assert len(res) >= 1 and not torch.equal(res.image, to_bgr(frames["fa"]))                # something was drawn
    canvas = res.image.cpu().numpy()
    out = from_bgr(res.image, "nv12")
    h, w = canvas.shape[:2]
    planes = yuv_ref.bgr_to_yuv420(canvas, NV12, BT601, LIMITED)
    for got, wnt in zip(out.planes, planes):
        np.testing.assert_array_equal(got.cpu().numpy(), wnt)
    np.testing.assert_array_equal(to_bgr(out).cpu().numpy(), yuv_ref.yuv420_to_bgr(planes, h, w, NV12, BT601, LIMITED))
