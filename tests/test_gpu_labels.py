"""The overlay's text on the MI355X: sp_render_labels_u8c3 through the C ABI against tests/label_ref.py, bit for bit, on the cases of
tests/label_scenes.py (seeded random backgrounds), and the text inside TopDownPoseEstimator / PoseTracker against PoseRenderer.render on the
returned PoseResult and against the numpy reference.  Every image and every workspace sits between guard bytes that must come back
untouched."""
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
from tests import label_ref, label_scenes, render_ref
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
GUARD = 4096
CASES = label_scenes.cases()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_labels(case):
    """One sp_render_labels_u8c3 call on the case's buffers -> the image on the host.  `shift`: bytes the image is moved off its 4-byte
    alignment.  The image and the workspace lie between guard bytes, checked after the call."""
    sc = case["scene"]
    h, w = sc["img"].shape[:2]
    n, shift = h * w * 3, case["shift"]
    rows = sc["box"].shape[0] if case["rows"] is None else case["rows"]
    flat = torch.full(((n + 2 * GUARD + 8 + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    img = flat[GUARD + shift:GUARD + shift + n]
    img.copy_(_up(sc["img"].reshape(-1)))
    box, score, tid, keep, seg = _up(sc["box"]), _up(sc["score"]), _up(sc["track_id"]), _up(sc["keep"]), _up(sc["seg"])
    kc = _up(sc["keep_count"] if case["keep_count"] is None else case["keep_count"])
    cap = None if case["caption"] is None else _up(case["caption"])
    nbytes = ctypes.c_int64()
    st = label_scenes.style_struct(case["style"])
    _lib.check(_lib.lib().sp_render_labels_workspace_bytes(rows, ctypes.byref(nbytes)), "sp_render_labels_workspace_bytes")
    ws = torch.full((nbytes.value + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().sp_render_labels_u8c3(P(img), h, w, P(box), P(score), P(tid) if case["with_ids"] else None, P(keep), P(kc), P(seg),
                                                case["image"], rows, ctypes.byref(st), P(cap), P(ws) + GUARD,
                                                _lib.current_stream(torch.device(DEV))), "sp_render_labels_u8c3")
    torch.cuda.synchronize()
    host, wsh = flat.cpu().numpy(), ws.cpu().numpy()
    assert (host[:GUARD + shift] == 0xA5).all() and (host[GUARD + shift + n:] == 0xA5).all(), "bytes outside the image were written"
    assert (wsh[:GUARD] == 0x5A).all() and (wsh[GUARD + nbytes.value:] == 0x5A).all(), "bytes outside the workspace were written"
    return host[GUARD + shift:GUARD + shift + n].reshape(h, w, 3)


def _differs(got, want, name):
    bad = np.argwhere((got != want).any(axis=2))
    print(f"MEASURED {name}: {bad.shape[0]} of {got.shape[0] * got.shape[1]} pixels differ" + (f", first at (y, x) = {bad[0].tolist()}" if bad.size else ""))
    return bad.shape[0]


# ---- 1. the kernels through the C ABI -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_equals_the_reference_bitwise(case):
    """97 x 61: w % 4 != 0 (the byte path), ragged last tiles both ways; 128 x 64: the 4-byte path, and moved one byte off its alignment.
    What each case holds is written where it is built, in tests/label_scenes.py."""
    want = label_scenes.reference(case)
    assert bool((want != case["scene"]["img"]).any()) == case["draws"]
    assert _differs(device_labels(case), want, case["name"]) == 0


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
    return PoseRenderer(label="#{id} {score}", caption="cam {image}: {n}")


@pytest.fixture(scope="module")
def est(detector, dconv, renderer):
    return TopDownPoseEstimator(detector, dconv, capacity=32, renderer=renderer)


def _ref_image(img, r, res, image=0):
    """render_ref's capsules, then label_ref's text: the frame's picture by the rules alone."""
    base = render_ref.render(img, render_ref.Style(r.skeleton, r.joint_r, r.limb_r, r.box_r, r.opacity16, r.in_vis_thre, r.colour_by, r.palette),
                             res.keypoints, res.box, res.track_id)
    st = label_ref.Style(r.label or b"", r.label_scale, r.label_opacity16, r.caption_scale, r.caption_opacity16, r.caption_corner, r.palette)
    cap = None if r.caption is None else r.caption_rows(image + 1)[image]
    return label_ref.render(base, st, res.box, res.score, res.track_id, len(res), image, cap)


def test_estimate_image_equals_render_of_its_result_eager_and_graphed(golden, est, renderer):
    a = golden(G)["sp_a_image"]
    keep = est.use_graph
    try:
        images = {}
        for graph in (False, True):
            est.use_graph = graph
            for _ in range(2 if graph else 1):                                   # the capture, then a replay
                res = est.estimate(a)
            assert len(res) >= 1 and res.track_id is None
            got = res.image.clone()
            assert torch.equal(got, renderer.render(a, res)), f"use_graph={graph}"
            images[graph] = got.cpu().numpy()
        assert (images[False] == images[True]).all()
        assert _differs(images[True], _ref_image(a, renderer, res), "estimate vs render_ref + label_ref") == 0
        plain = PoseRenderer().render(a, res).cpu().numpy()
        assert (plain != images[True]).any()                                     # the text is there
        # a batch: one caption per image index, each picture render()'s with that index
        b = np.ascontiguousarray(a[:, ::-1])
        for i, (r, img) in enumerate(zip(est.estimate_batch([a, b]), (a, b))):
            assert torch.equal(r.image.clone(), renderer.render(img, r, image=i)), i
        # a list of captions of another length is refused before any launch
        renderer.caption = ["one", "two", "three"]
        with pytest.raises(ValueError, match="one per image"):
            est.estimate(a)
    finally:
        est.use_graph = keep
        renderer.caption = "cam {image}: {n}"


def test_a_new_caption_shows_with_the_next_replay_of_the_same_graph(golden, est, renderer):
    a = golden(G)["sp_a_image"]
    keep = est.use_graph
    try:
        est.use_graph = True
        est.estimate(a)
        first = est.estimate(a)
        one = first.image.clone()
        frames = list(est._frames.values())
        graph = frames[-1].graph
        assert graph is not None
        renderer.caption = "gate B {n}"
        second = est.estimate(a)
        two = second.image.clone()
        assert list(est._frames.values())[-1].graph is graph                     # not captured again
        assert not torch.equal(one, two)
        assert _differs(two.cpu().numpy(), _ref_image(a, renderer, second), "replayed frame with the new caption") == 0
    finally:
        est.use_graph = keep
        renderer.caption = "cam {image}: {n}"


def test_a_tracker_prints_the_ids_it_returns(golden, est, renderer):
    a, b = golden(G)["sp_a_image"], golden(G)["sp_b_image"]
    trk = PoseTracker(est, detect_every=2)
    drawn = 0
    for f, img in enumerate((a, b, a)):
        res = trk.update(img)
        assert res.track_id is not None and res.image is not None
        got = res.image.clone()
        assert torch.equal(got, renderer.render(img, res)), f"frame {f}"
        if len(res):
            drawn += 1
            assert _differs(got.cpu().numpy(), _ref_image(img, renderer, res), f"tracked frame {f} vs the references") == 0
            # the ids are in the picture: the same poses under other ids are another picture
            other = type(res)(res.keypoints, res.score, res.box, 0, res.track_id + 20)
            assert (_ref_image(img, renderer, other) != got.cpu().numpy()).any()
    assert drawn >= 1


def test_without_label_and_caption_the_frame_is_the_overlay_alone_and_no_text_entry_is_called(golden, detector, dconv, monkeypatch):
    a = golden(G)["sp_a_image"]
    r = PoseRenderer()
    lib = _lib.lib()
    calls = []

    class Counting:
        def __getattr__(self, name):
            if name in ("sp_render_font_glyph", "sp_render_labels_workspace_bytes", "sp_render_labels_u8c3"):
                calls.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "lib", lambda: Counting())
    plain = TopDownPoseEstimator(detector, dconv, capacity=32, renderer=r)
    res = plain.estimate(a)
    monkeypatch.undo()
    assert len(res) >= 1 and calls == []
    fr = list(plain._frames.values())[-1]
    assert fr.label_ws is None and fr.caption is None and fr.caption_host is None
    want = render_ref.render(a, render_ref.Style(r.skeleton, r.joint_r, r.limb_r, r.box_r, r.opacity16, r.in_vis_thre, r.colour_by, r.palette),
                             res.keypoints, res.box)
    assert _differs(res.image.cpu().numpy(), want, "no text: the overlay alone") == 0
