"""The overlay on the MI355X: sp_render_poses_u8c3 through the C ABI against tests/render_ref.py, bit for bit, on the scenes of
tests/render_scenes.py (seeded random backgrounds), and the renderer inside TopDownPoseEstimator / PoseTracker against PoseRenderer.render
on the returned PoseResult.  Every image sits between guard bytes that must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import PoseTracker
from simple_pose_amd.visualize import PoseRenderer
from tests import render_ref, render_scenes
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
GUARD = 4096


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_render(scene, style, image=0, with_ids=True, in_place=False, rows=None, keep_count=None, shift=0):
    """One sp_render_poses_u8c3 call on the scene's buffers -> the image on the host.  `shift`: bytes both images are moved off their 4-byte
    alignment.  The destination (the source when in place) lies between guard bytes, checked after the call."""
    h, w = scene["img"].shape[:2]
    n = h * w * 3
    J = scene["kps"].shape[1]
    rows = scene["kps"].shape[0] if rows is None else rows
    flat = torch.full((2, (n + 2 * GUARD + 8 + 15) // 16 * 16), 0xA5, dtype=torch.uint8, device=DEV)
    src = flat[0, GUARD + shift:GUARD + shift + n]
    src.copy_(_up(scene["img"].reshape(-1)))
    dst = src if in_place else flat[1, GUARD + shift:GUARD + shift + n]
    kps, box, tid, keep, seg = _up(scene["kps"]), _up(scene["box"]), _up(scene["track_id"]), _up(scene["keep"]), _up(scene["seg"])
    kc = _up(scene["keep_count"] if keep_count is None else np.asarray(keep_count, np.int32))
    nbytes = ctypes.c_int64()
    st = render_scenes.style_struct(style)
    _lib.check(_lib.lib().sp_render_workspace_bytes(rows, J, st.edges, ctypes.byref(nbytes)), "sp_render_workspace_bytes")
    ws = torch.full((nbytes.value + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().sp_render_poses_u8c3(P(src), P(dst), h, w, P(kps), P(box), P(tid) if with_ids else None, P(keep), P(kc), P(seg), image, rows,
                                               J, ctypes.byref(st), P(ws) + GUARD, _lib.current_stream(torch.device(DEV))), "sp_render_poses_u8c3")
    torch.cuda.synchronize()
    host, wsh = flat.cpu().numpy(), ws.cpu().numpy()
    row = 0 if in_place else 1
    assert (host[row, :GUARD + shift] == 0xA5).all() and (host[row, GUARD + shift + n:] == 0xA5).all(), "bytes outside the image were written"
    assert (wsh[:GUARD] == 0x5A).all() and (wsh[GUARD + nbytes.value:] == 0x5A).all(), "bytes outside the workspace were written"
    if not in_place:
        assert (host[0, GUARD + shift:GUARD + shift + n] == scene["img"].reshape(-1)).all(), "the source was written"
    return host[row, GUARD + shift:GUARD + shift + n].reshape(h, w, 3)


def _differs(got, want, name):
    bad = np.argwhere((got != want).any(axis=2))
    print(f"MEASURED {name}: {bad.shape[0]} of {got.shape[0] * got.shape[1]} pixels differ" + (f", first at (y, x) = {bad[0].tolist()}" if bad.size else ""))
    return bad.shape[0]


# ---- 1. the kernels through the C ABI -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ids", [False, True], ids=["no_ids", "ids"])
@pytest.mark.parametrize("mode", ["person", "part"])
def test_small_ragged_image_equals_the_reference_bitwise(mode, with_ids):
    """70 x 45: w % 4 != 0 (the byte path), partial tiles both ways; invisible and NaN joints, joints outside the image, a zero-length limb,
    overlapping persons."""
    scene, style = render_scenes.ragged(), render_scenes.styles()[mode]
    want = render_scenes.reference(scene, style, 0, with_ids)
    assert (want != scene["img"]).any()
    got = device_render(scene, style, 0, with_ids)
    assert _differs(got, want, f"ragged {mode} ids={with_ids}") == 0
    if mode == "person":                                                       # ids change the colours, so the two runs are not the same picture
        other = render_scenes.reference(scene, style, 0, not with_ids)
        assert (other != want).any()


@pytest.mark.parametrize("persons", [14, 24])
def test_chunk_and_list_limits(persons):
    """132 x 40 (the 4-byte path), every person on the same 20 x 20 px spot, one joint in five invisible.  14 persons: 560 primitives, more
    than two scan chunks, most of them in one tile but fewer than the list holds (asserted below).  24 persons: 960 primitives and, by the reference's own count, more than the list's 512
    in one tile, so the tile applies its list before the scan ends and goes on."""
    scene, style = render_scenes.crowd(persons), render_scenes.styles()["part"]
    kps, box, tid = render_ref.kept(scene["kps"], scene["box"], scene["track_id"], scene["keep"], scene["keep_count"], scene["seg"], 0)
    prims = render_ref.primitives(style, kps, box, tid)
    most = int(render_ref.tile_hits(prims, 40, 132).max())
    print(f"MEASURED crowd {persons}: {len(prims)} primitives, {most} in the fullest tile")
    assert len(prims) == persons * 40 > 2 * render_scenes.CHUNK
    if persons == 24:
        assert most > render_scenes.LIST
    else:
        assert render_scenes.CHUNK < most <= render_scenes.LIST                 # one tile lists hits of more than one chunk, without a flush
    want = render_scenes.reference(scene, style)
    assert _differs(device_render(scene, style), want, f"crowd {persons}") == 0
    if persons == 14:                                                          # the same picture off the 4-byte alignment: the byte path at w % 4 == 0
        assert _differs(device_render(scene, style, shift=1), want, "crowd 14 unaligned") == 0


def test_in_place_no_ops_and_the_second_image():
    style = render_scenes.styles()["person"]
    for name, scene in (("ragged", render_scenes.ragged()), ("crowd", render_scenes.crowd(14))):
        want = render_scenes.reference(scene, style)
        assert _differs(device_render(scene, style, in_place=True), want, f"{name} in place") == 0
        for in_place in (False, True):
            assert (device_render(scene, style, keep_count=[0], in_place=in_place) == scene["img"]).all(), name
            assert (device_render(scene, style, rows=0, in_place=in_place) == scene["img"]).all(), name
    two = render_scenes.two_images()
    first, second = render_scenes.reference(two, style, 0), render_scenes.reference(two, style, 1)
    assert (first != second).any()
    assert _differs(device_render(two, style, image=1), second, "two images, image 1") == 0
    assert _differs(device_render(two, style, image=0, in_place=True), first, "two images, image 0 in place") == 0


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
def renderer():
    return PoseRenderer()


@pytest.fixture(scope="module")
def est(detector, dconv, renderer):
    return TopDownPoseEstimator(detector, dconv, capacity=32, renderer=renderer)


@pytest.fixture(scope="module")
def plain(detector, dconv):
    return TopDownPoseEstimator(detector, dconv, capacity=32)


def _style_of(r):
    return render_ref.Style(r.skeleton, r.joint_r, r.limb_r, r.box_r, r.opacity16, r.in_vis_thre, r.colour_by, r.palette)


def test_estimate_image_equals_render_of_its_result_eager_and_graphed(golden, est, plain, renderer):
    a = golden(G)["sp_a_image"]
    keep = est.use_graph
    try:
        images = {}
        for graph in (False, True):
            est.use_graph = graph
            for _ in range(2 if graph else 1):                                   # the capture, then a replay
                res = est.estimate(a)
            assert len(res) >= 1 and res.track_id is None
            assert res.image.is_cuda and res.image.dtype == torch.uint8 and tuple(res.image.shape) == a.shape
            got = res.image.clone()
            want = renderer.render(a, res)
            assert torch.equal(got, want), f"use_graph={graph}"
            images[graph] = got.cpu().numpy()
        assert (images[False] == images[True]).all() and (images[True] != a).any()
        # and against the numpy reference: the frame's picture is the rules' picture
        assert _differs(images[True], render_ref.render(a, _style_of(renderer), res.keypoints, res.box), "estimate vs render_ref") == 0
        # without a renderer: no image, the same numbers
        bare = plain.estimate(a)
        assert bare.image is None
        np.testing.assert_array_equal(bare.keypoints, res.keypoints)
        np.testing.assert_array_equal(bare.score, res.score)
        np.testing.assert_array_equal(bare.box, res.box)
        # batch and caller-supplied boxes honour the renderer, one picture per image index
        b = np.ascontiguousarray(a[:, ::-1])                                     # (the images of a batch share one size)
        for r, img in zip(est.estimate_batch([a, b]), (a, b)):
            assert torch.equal(r.image.clone(), renderer.render(img, r))
        det = np.array([[20, 30, 200, 300, 0.9, 0], [150, 40, 320, 330, 0.8, 0]], np.float32)
        rb = est.estimate_boxes(a, det)[0]
        assert len(rb) >= 1 and torch.equal(rb.image.clone(), renderer.render(a, rb))
    finally:
        est.use_graph = keep


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_tracked_frames_are_drawn_with_their_ids(golden, est, plain, renderer, graph):
    a, b = golden(G)["sp_a_image"], golden(G)["sp_b_image"]
    keep = (est.use_graph, plain.use_graph)
    try:
        est.use_graph = plain.use_graph = graph
        trk, bare = PoseTracker(est, detect_every=2), PoseTracker(plain, detect_every=2)
        kinds, drawn = [], 0
        for f, img in enumerate((a, b, a, a, b, a)):
            res, ref = trk.update(img), bare.update(img)
            kinds.append(trk.last_frame_kind)
            assert res.track_id is not None and res.image is not None and ref.image is None
            got = res.image.clone()
            assert torch.equal(got, renderer.render(img, res)), f"frame {f}"
            np.testing.assert_array_equal(res.keypoints, ref.keypoints, err_msg=f"frame {f}")
            np.testing.assert_array_equal(res.score, ref.score, err_msg=f"frame {f}")
            np.testing.assert_array_equal(res.track_id, ref.track_id, err_msg=f"frame {f}")
            drawn += int((got.cpu().numpy() != img).any())
            if f == 5 and len(res):
                want = render_ref.render(img, _style_of(renderer), res.keypoints, res.box, res.track_id)
                assert _differs(got.cpu().numpy(), want, "tracked frame vs render_ref") == 0
        assert drawn >= 3 and {"detector", "propagated"} <= set(kinds)
    finally:
        est.use_graph, plain.use_graph = keep
