"""Redaction on the MI355X: sp_redact_u8c3 through the C ABI against tests/redact_ref.py, bit for bit, on the scenes of
tests/redact_scenes.py (seeded random backgrounds), and the redactor inside TopDownPoseEstimator / PoseTracker / MultiStreamTracker against
the reference applied to the source with the returned rows.  Every image sits between guard bytes that must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.datasets.jpeg import JpegDecoder, JpegEncoder
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import MultiStreamTracker, PoseTracker
from simple_pose_amd.visualize import PoseRenderer, Redactor
from tests import redact_ref, redact_scenes, render_ref
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
GUARD = 4096
S = redact_ref.Style


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_redact(scene, style, image=0, in_place=False, rows=None, keep_count=None, shift=0, img=None):
    """One sp_redact_u8c3 call on the scene's buffers -> the image on the host.  `shift`: bytes both images are moved off their 4-byte
    alignment.  The destination (the source when in place) lies between guard bytes, checked after the call; out of place it starts as
    0xA5 bytes, so a pixel the call does not write shows."""
    img = scene["img"] if img is None else img
    h, w = img.shape[:2]
    n = h * w * 3
    J = scene["kps"].shape[1]
    rows = scene["kps"].shape[0] if rows is None else rows
    flat = torch.full((2, (n + 2 * GUARD + 8 + 15) // 16 * 16), 0xA5, dtype=torch.uint8, device=DEV)
    src = flat[0, GUARD + shift:GUARD + shift + n]
    src.copy_(_up(img.reshape(-1)))
    dst = src if in_place else flat[1, GUARD + shift:GUARD + shift + n]
    kps, box, keep, seg = _up(scene["kps"]), _up(scene["box"]), _up(scene["keep"]), _up(scene["seg"])
    kc = _up(scene["keep_count"] if keep_count is None else np.asarray(keep_count, np.int32))
    nbytes = ctypes.c_int64()
    st = redact_scenes.style_struct(style)
    _lib.check(_lib.lib().sp_redact_workspace_bytes(rows, ctypes.byref(nbytes)), "sp_redact_workspace_bytes")
    ws = torch.full((nbytes.value + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().sp_redact_u8c3(P(src), P(dst), h, w, P(kps), P(box), P(keep), P(kc), P(seg), image, rows, J, ctypes.byref(st),
                                         P(ws) + GUARD, _lib.current_stream(torch.device(DEV))), "sp_redact_u8c3")
    torch.cuda.synchronize()
    host, wsh = flat.cpu().numpy(), ws.cpu().numpy()
    row = 0 if in_place else 1
    assert (host[row, :GUARD + shift] == 0xA5).all() and (host[row, GUARD + shift + n:] == 0xA5).all(), "bytes outside the image were written"
    assert (wsh[:GUARD] == 0x5A).all() and (wsh[GUARD + nbytes.value:] == 0x5A).all(), "bytes outside the workspace were written"
    if not in_place:
        assert (host[0, GUARD + shift:GUARD + shift + n] == img.reshape(-1)).all(), "the source was written"
    return host[row, GUARD + shift:GUARD + shift + n].reshape(h, w, 3)


def _differs(got, want, name):
    bad = np.argwhere((got != want).any(axis=2))
    print(f"MEASURED {name}: {bad.shape[0]} of {got.shape[0] * got.shape[1]} pixels differ" + (f", first at (y, x) = {bad[0].tolist()}" if bad.size else ""))
    return bad.shape[0]


_REF = {}


def _want(key, scene, style, image=0):
    """The reference of a case, computed once."""
    if key not in _REF:
        _REF[key] = redact_scenes.reference(scene, style, image)
    return _REF[key]


# ---- 1. the kernels through the C ABI -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", redact_ref.CELLS)
def test_every_cell_size_on_the_ragged_image_equals_the_reference_bitwise(cell):
    """97 x 131: w % 4 != 0 (the byte path), partial edge cells both ways, at every cell size (every tile height).  The scene holds a
    disc centred outside the image that reaches in, a person wholly outside, NaN / infinite / huge coordinates, a person without a
    visible head joint (the default fallback) and a point (r == 0)."""
    scene, style = redact_scenes.street(), S(cell=cell)
    want = _want(("street", cell), scene, style)
    assert (want != scene["img"]).any()
    assert _differs(device_redact(scene, style), want, f"street cell {cell}") == 0
    assert _differs(device_redact(scene, style, in_place=True), want, f"street cell {cell} in place") == 0


@pytest.mark.parametrize("name", ["head_mosaic", "head_fill", "person_mosaic", "person_fill"])
@pytest.mark.parametrize("shape", [(97, 131), (96, 128), (3, 5)], ids=["97x131", "96x128", "3x5"])
def test_regions_and_modes_on_the_three_geometries(shape, name):
    """Head and person regions, mosaic and fill, on the byte path (97 x 131), the 4-byte path (96 x 128) and an image smaller than one
    cell (3 x 5: one clipped cell, or a few of 4)."""
    scene, style = redact_scenes.street(*shape), redact_scenes.styles()[name]
    want = _want((shape, name), scene, style)
    assert _differs(device_redact(scene, style), want, f"{shape} {name}") == 0
    if shape == (96, 128):                                                     # the same picture off the 4-byte alignment: the byte path at w % 4 == 0
        assert _differs(device_redact(scene, style, shift=1), want, f"{shape} {name} unaligned") == 0
    if shape != (3, 5) or name.startswith("person"):
        assert (want != scene["img"]).any()


@pytest.mark.parametrize("fallback", ["box_top", "box", "none"])
def test_fallbacks(fallback):
    scene, style = redact_scenes.street(96, 128), S(cell=4, fallback=fallback, mode="fill", fill=(1, 2, 3))
    want = _want(("fallback", fallback), scene, style)
    assert _differs(device_redact(scene, style), want, f"fallback {fallback}") == 0
    others = [_want(("fallback", f), scene, S(cell=4, fallback=f, mode="fill", fill=(1, 2, 3))) for f in ("box_top", "box", "none") if f != fallback]
    assert all((o != want).any() for o in others)                              # the three are three pictures


def test_extreme_parameters_and_other_head_joints():
    scene = redact_scenes.street(96, 128)
    for name, style in (("max", S(cell=16, expand=64, head_min=256, top_frac=256)), ("min", S(cell=4, expand=16, head_min=0, top_frac=0)),
                        ("ears", S(cell=8, head_joints=(3, 4))), ("eight", S(cell=8, head_joints=(0, 1, 2, 3, 4, 5, 6, 16), in_vis_thre=0.5))):
        assert _differs(device_redact(scene, style), _want(("extreme", name), scene, style), f"extreme {name}") == 0


def test_counts_rows_and_the_second_image():
    style = redact_scenes.styles()["head_mosaic"]
    scene = redact_scenes.street()
    rows = scene["kps"].shape[0]
    for in_place in (False, True):
        assert (device_redact(scene, style, keep_count=[0], in_place=in_place) == scene["img"]).all()
        assert (device_redact(scene, style, keep_count=[-3], in_place=in_place) == scene["img"]).all()
        assert (device_redact(scene, style, rows=0, in_place=in_place) == scene["img"]).all()
    # keep_count beyond rows: clamped to the rows, as the overlay clamps it.  Every keep entry is then read, the -1 entries of the spare
    # rows too, which give empty regions: the picture is the picture of the true count
    want = _want(("street", "head_mosaic"), scene, style)
    assert _differs(device_redact(scene, style, keep_count=[rows + 5]), want, "keep_count beyond rows") == 0
    assert _differs(device_redact(scene, style, keep_count=[2 ** 31 - 1], in_place=True), want, "keep_count INT_MAX") == 0
    two = redact_scenes.two_images()
    first, second = redact_scenes.reference(two, style, 0), redact_scenes.reference(two, style, 1)
    assert (first != second).any()
    assert _differs(device_redact(two, style, image=1), second, "two images, image 1") == 0
    assert _differs(device_redact(two, style, image=0, in_place=True), first, "two images, image 0 in place") == 0


def test_more_records_than_one_scan_chunk():
    """300 persons on 64 x 64: the cells of the lower right corner are hit by records of the second chunk only (tests/test_redact_host.py
    asserts it of the scene)."""
    scene, style = redact_scenes.crowd(), S(cell=4)
    want = _want("crowd", scene, style)
    assert (want[40:, 40:] != scene["img"][40:, 40:]).any()
    assert _differs(device_redact(scene, style), want, "crowd") == 0
    assert _differs(device_redact(scene, style, in_place=True), want, "crowd in place") == 0


def test_untouched_tiles_are_copied_out_of_place_and_left_alone_in_place():
    """Out of place the destination starts as 0xA5 bytes, so an untouched tile that is not copied shows.  In place, the pixels of the
    tiles nothing hits are replaced by a sentinel in the SOURCE the device sees: they come back as the sentinel (neither rewritten from
    elsewhere nor averaged), and the hit tiles come back as the reference of the true image, which never reads those pixels."""
    scene, style = redact_scenes.street(96, 128), S(cell=8)
    img = scene["img"]
    kps, box = redact_scenes.kept_rows(scene)
    tiles = redact_ref.tile_hits(redact_ref.regions(style, kps, box), 96, 128, 8)
    assert (tiles > 0).any() and (tiles == 0).any()
    want = _want(("untouched", 8), scene, style)
    assert _differs(device_redact(scene, style), want, "untouched tiles out of place") == 0
    free = np.repeat(np.repeat(tiles == 0, 16, 0), 64, 1)[:96, :128]
    marked = img.copy()
    marked[free] = 0xC3
    got = device_redact(scene, style, in_place=True, img=marked)
    assert (got[free] == 0xC3).all()
    assert _differs(got[~free][None], want[~free][None], "hit tiles in place") == 0


# ---- 2. in the frame ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    d = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))
    conf, iou, _ = golden(G)["sp_a_thresh"]
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
    m.compute_dtype, m.autotune = "fp32", False
    return m


@pytest.fixture(scope="module")
def redactor():
    # fill: the golden image is flat patches of colour, which a mosaic leaves as they are.  in_vis_thre -1: the synthetic pose net's
    # max_val is what it is; every head joint counts, so discs are what the frames show
    return Redactor(mode="fill", fill=(255, 0, 255), cell=8, in_vis_thre=-1.0)


@pytest.fixture(scope="module")
def renderer():
    return PoseRenderer()


@pytest.fixture(scope="module")
def est(detector, dconv, redactor):
    return TopDownPoseEstimator(detector, dconv, capacity=32, redactor=redactor)


@pytest.fixture(scope="module")
def both(detector, dconv, redactor, renderer):
    return TopDownPoseEstimator(detector, dconv, capacity=32, redactor=redactor, renderer=renderer)


@pytest.fixture(scope="module")
def plain(detector, dconv):
    return TopDownPoseEstimator(detector, dconv, capacity=32)


def _ref_style(r):
    return S(r.region, r.mode, r.cell, r.expand16, r.head_min256, r.head_joints, r.fallback, r.top_frac256, r.in_vis_thre, r.fill)


def _render_style(r):
    return render_ref.Style(r.skeleton, r.joint_r, r.limb_r, r.box_r, r.opacity16, r.in_vis_thre, r.colour_by, r.palette)


def _redacted(img, res, redactor):
    return redact_ref.redact(img, _ref_style(redactor), res.keypoints, res.box)


def _same_numbers(res, ref, what):
    np.testing.assert_array_equal(res.keypoints, ref.keypoints, err_msg=what)
    np.testing.assert_array_equal(res.score, ref.score, err_msg=what)
    np.testing.assert_array_equal(res.box, ref.box, err_msg=what)
    if ref.track_id is None:
        assert res.track_id is None, what
    else:
        np.testing.assert_array_equal(res.track_id, ref.track_id, err_msg=what)


def test_estimate_image_is_the_reference_of_its_result_eager_and_graphed(golden, est, both, plain, redactor, renderer):
    a = golden(G)["sp_a_image"]
    bare = plain.estimate(a)
    assert bare.image is None and len(bare) >= 1
    keep = (est.use_graph, both.use_graph)
    try:
        for graph in (False, True):
            est.use_graph = both.use_graph = graph
            for _ in range(2 if graph else 1):                                   # the capture, then a replay
                res, drawn = est.estimate(a), both.estimate(a)
            _same_numbers(res, bare, f"redactor, use_graph={graph}")
            _same_numbers(drawn, bare, f"redactor + renderer, use_graph={graph}")
            assert res.image.is_cuda and res.image.dtype == torch.uint8 and tuple(res.image.shape) == a.shape
            want = _redacted(a, res, redactor)
            assert (want != a).any()
            assert _differs(res.image.cpu().numpy(), want, f"estimate, use_graph={graph}") == 0
            assert torch.equal(res.image, redactor.redact(a, res))               # the host-rows entry runs the same kernels
            # with a renderer too: redaction, then the capsules on the redacted canvas
            want2 = render_ref.render(want, _render_style(renderer), drawn.keypoints, drawn.box)
            assert (want2 != want).any()
            assert _differs(drawn.image.cpu().numpy(), want2, f"estimate with a renderer, use_graph={graph}") == 0
    finally:
        est.use_graph, both.use_graph = keep


def test_batches_boxes_files_and_tiling(golden, est, plain, redactor, detector, dconv):
    from simple_pose_amd.tiling import Tiling
    a = golden(G)["sp_a_image"]
    b = np.ascontiguousarray(a[:, ::-1])
    # dense batch: one call per image index
    for r, ref, img in zip(est.estimate_batch([a, b]), plain.estimate_batch([a, b]), (a, b)):
        _same_numbers(r, ref, "dense batch")
        assert _differs(r.image.cpu().numpy(), _redacted(img, r, redactor), "dense batch") == 0
    # mixed sizes: every image its own canvas
    c = np.ascontiguousarray(a[: a.shape[0] - 37, : a.shape[1] - 50])
    got, ref = est.estimate_batch([a, c]), plain.estimate_batch([a, c])
    for r, rr, img in zip(got, ref, (a, c)):
        _same_numbers(r, rr, "mixed batch")
        assert tuple(r.image.shape) == img.shape
        assert _differs(r.image.cpu().numpy(), _redacted(img, r, redactor), f"mixed batch {img.shape}") == 0
    assert sum(len(r) for r in got) >= 1
    # caller-supplied boxes
    det = np.array([[20, 30, 200, 300, 0.9, 0], [150, 40, 320, 330, 0.8, 0]], np.float32)
    rb = est.estimate_boxes(a, det)[0]
    assert len(rb) >= 1 and _differs(rb.image.cpu().numpy(), _redacted(a, rb, redactor), "estimate_boxes") == 0
    # a mosaic in the frame, on noise (the golden image's flat patches are their own means): whole persons, 32 px cells
    mosaic = Redactor(region="person", cell=32)
    noise = np.random.default_rng(8).integers(0, 256, a.shape, dtype=np.uint8)
    rm = TopDownPoseEstimator(detector, dconv, capacity=32, redactor=mosaic).estimate_boxes(noise, det)[0]
    want = _redacted(noise, rm, mosaic)
    assert len(rm) >= 1 and (want != noise).any() and _differs(rm.image.cpu().numpy(), want, "estimate_boxes, mosaic") == 0
    # files: the project's own encoder writes them, its decoder's pixels are the source
    files = JpegEncoder(DEV, quality=90, subsampling="4:4:4").encode([_up(a), _up(c)])
    decoded = [t.cpu().numpy() for t in JpegDecoder(DEV).decode(files)]
    for r, img in zip(est.estimate_files(files), decoded):
        assert _differs(r.image.cpu().numpy(), _redacted(img, r, redactor), f"estimate_files {img.shape}") == 0
    # tiling
    tiling = Tiling(tile=(320, 256), overlap=0.25)                               # 432 x 640: the frame and six 256 x 320 tiles
    tiled = TopDownPoseEstimator(detector, dconv, capacity=32, redactor=redactor, tiling=tiling)
    tiled_plain = TopDownPoseEstimator(detector, dconv, capacity=32, tiling=tiling)
    rt = tiled.estimate(a)
    _same_numbers(rt, tiled_plain.estimate(a), "tiling")
    assert _differs(rt.image.cpu().numpy(), _redacted(a, rt, redactor), "tiling") == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_tracked_frames_detector_and_propagated(golden, both, plain, redactor, renderer, graph):
    a = golden(G)["sp_a_image"]
    b = np.ascontiguousarray(a[::-1, ::-1])                                      # `a` turned by 180 degrees
    keep = (both.use_graph, plain.use_graph)
    try:
        both.use_graph = plain.use_graph = graph
        trk, bare = PoseTracker(both, detect_every=2), PoseTracker(plain, detect_every=2)
        kinds, hidden = [], 0
        for f, img in enumerate((a, b, a, a)):
            res, ref = trk.update(img), bare.update(img)
            kinds.append(trk.last_frame_kind)
            _same_numbers(res, ref, f"frame {f}")
            red = _redacted(img, res, redactor)
            hidden += int((red != img).any())
            want = render_ref.render(red, _render_style(renderer), res.keypoints, res.box, res.track_id)
            assert _differs(res.image.cpu().numpy(), want, f"tracked frame {f} ({kinds[-1]})") == 0
        assert hidden >= 2 and {"detector", "propagated"} <= set(kinds)
    finally:
        both.use_graph, plain.use_graph = keep


def test_two_streams_and_the_encoder(golden, detector, dconv, plain, redactor):
    a = golden(G)["sp_a_image"]
    b = a ^ np.uint8(1)                                                          # `a` with every byte's lowest bit flipped: the streams share one size
    enc, dec = JpegEncoder(DEV, quality=85, subsampling="4:2:0"), JpegDecoder(DEV)
    est_e = TopDownPoseEstimator(detector, dconv, capacity=32, redactor=redactor, encoder=enc)
    multi, bare = MultiStreamTracker(est_e, streams=2, detect_every=2), MultiStreamTracker(plain, streams=2, detect_every=2)
    kinds = []
    for c, frames in enumerate(([a, b], [b, a], [a, a])):
        got, ref = multi.update(frames), bare.update(frames)
        kinds.append(multi.last_frame_kind)
        for s in range(2):
            what = f"call {c} stream {s}"
            _same_numbers(got[s], ref[s], what)
            want = _redacted(frames[s], got[s], redactor)
            assert _differs(got[s].image.cpu().numpy(), want, what) == 0
            # the file is the file of the redacted canvas: the project's decoder gives the pixels of the reference canvas' file
            again = JpegEncoder(DEV, quality=85, subsampling="4:2:0").encode([_up(want)])[0]
            assert isinstance(got[s].jpeg, bytes) and got[s].jpeg == again, what
            assert torch.equal(dec.decode([got[s].jpeg])[0], dec.decode([again])[0]), what
    assert {"detector", "propagated"} <= set(kinds)
