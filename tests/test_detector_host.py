"""YOLOv5 detector, host side (CPU only): parameter holder keys against the reference (g14), ScalePadding geometry, the program lowering
interpreted on the CPU against a plain-torch forward, and the numpy NMS restatement against the reference's non_max_suppression (g14)."""
import numpy as np
import pytest
import torch

from simple_pose_amd import engine
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import ScalePadding
from tests.desc_interp import TorchPacker
from tests.detector_ref import detector_state_dict, nms_np, run_yolo_program_cpu, yolov5_forward_torch

G = "g14_detector.npz"


@pytest.mark.parametrize("scale", ["s", "l"])
def test_state_dict_keys_and_parameter_count(golden, scale):
    z = golden(G)
    m = YOLOv5(scale_name=scale, num_cls=80)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[f"keys_{scale}"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(z[f"shapes_{scale}"])
    assert sum(p.numel() for p in m.parameters()) == int(z[f"params_{scale}"])
    assert len(sd) == {"s": 370, "l": 658}[scale]


def test_make_border_geometry(golden):
    for h, w, oh, ow, left, top, r in golden(G)["border"]:
        g = ScalePadding(target_size=(640, 640), minimum_rectangle=True).geometry(int(h), int(w))
        assert (g["out_h"], g["out_w"], g["left"], g["top"]) == (oh, ow, left, top) and g["ratio"] == r
        assert g["out_h"] % 32 == 0 and g["out_w"] % 32 == 0


@pytest.mark.parametrize("slice_idx", [-1, 0])
def test_program_interpreted_on_cpu_matches_torch_forward(slice_idx):
    m = YOLOv5(scale_name="s", num_cls=80)
    sd = detector_state_dict(m, seed=5)
    x = torch.from_numpy(np.random.default_rng(5).random((2, 3, 96, 128), dtype=np.float32))
    prog = engine.yolov5_program(sd, 80, 96, 128, slice_idx=slice_idx, source="nchw", packer=TorchPacker())
    kinds = {op.kind for op in prog.ops}
    assert {"focus_nchw", "conv", "spp", "upsample_slice", "yolo_decode"} <= kinds
    with torch.no_grad():
        ref = yolov5_forward_torch(sd, x)[..., engine.yolo_head_columns(85, slice_idx)]
        out = run_yolo_program_cpu(prog, x)
    assert out.shape == ref.shape
    rel = ((out - ref).abs().amax(1) / ref.abs().amax(1)).max().item()
    assert rel <= 1e-5, rel


def test_concat_buffers_are_never_copied():
    """Every concat is built by producers writing slices (SP_CONV_OUT_SLICE / spp / upsample_slice); no op reads one buffer to write a copy."""
    m = YOLOv5(scale_name="s", num_cls=80)
    prog = engine.yolov5_program(detector_state_dict(m, 1), 80, 64, 64, slice_idx=0, source="nchw", packer=TorchPacker())
    sliced = [op for op in prog.ops if op.kind == "conv" and op.desc.flags & engine.SP_CONV_OUT_SLICE]
    assert len(sliced) >= 2 * 8 and all(op.desc.out_c > op.desc.c_out for op in sliced)
    assert not any(op.kind in ("copy", "concat") for op in prog.ops)


@pytest.mark.parametrize("case", ["merge_a", "plain_a", "merge_b", "plain_b", "many"])
def test_nms_restatement_matches_reference(golden, case):
    z = golden(G)
    conf, iou, merge, max_det = z[f"nms_{case}_args"]
    got = nms_np(z[f"nms_{case}_pred"], conf, iou, merge=bool(merge), max_det=int(max_det))[0]
    want = z[f"nms_{case}_out"]
    got = np.zeros((0, 6), np.float32) if got is None else got
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[:, 4:], want[:, 4:])
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-5, atol=1e-4)


def test_nms_restatement_on_network_output_matches_single_predict(golden):
    """Case b of g14 (merge, redundancy filter, clipped boxes): the restated NMS + clip + un-letterbox on the reference's head output gives
    the reference's single_predict detections."""
    z = golden(G)
    conf, iou, _ = z["sp_b_thresh"]
    img = z["sp_b_image"]
    g = ScalePadding(target_size=(640, 640), minimum_rectangle=True).geometry(*img.shape[:2])
    got = nms_np(z["sp_b_pred"][None], conf, iou, merge=True)[0]
    f = np.float32
    got[:, [0, 2]] = (np.clip(got[:, [0, 2]], f(0), f(g["out_w"])) - f(g["left"])) / f(g["ratio"])
    got[:, [1, 3]] = (np.clip(got[:, [1, 3]], f(0), f(g["out_h"])) - f(g["top"])) / f(g["ratio"])
    want = z["sp_b_dets"]
    assert got.shape == want.shape and (g["top"], g["ratio"]) == (12, 0.8)
    np.testing.assert_array_equal(got[:, 4:], want[:, 4:])
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-5, atol=1e-3)
