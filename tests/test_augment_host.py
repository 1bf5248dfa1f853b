"""Host half of the GPU training transform (no GPU needed): the augmentation geometry against the reference's recorded outputs
(tests/golden/g13_augment.npz, tools/gen_golden_augment.py), the reference's draw order, and the loader's sample order."""
import os
import random
import types

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.commons.transforms import RefineSimpleTransform
from simple_pose_amd.datasets.coco import COCO_JOINT_PAIRS, GpuAugmentLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g13_transform(g, augment):
    inp, out = tuple(int(v) for v in g["input_shape"]), tuple(int(v) for v in g["output_shape"])
    if augment:
        return RefineSimpleTransform(g["joint_pairs"].tolist(), inp, out, scale=(0.7, 1.3), ratio=(-40, 40), rand_crop=True)
    return RefineSimpleTransform(None, inp, out, scale=(1.0, 1.0), ratio=(0, 0), rand_crop=False)


def g13_samples(g):
    out = []
    for i in range(len(g["seeds"])):
        src = g[f"src{int(g['src_index'][i])}"]
        out.append(types.SimpleNamespace(img=src, box=g["boxes"][i].tolist(), joints=g["joints"][i].copy(),
                                         shape=(src.shape[1], src.shape[0]), img_path=f"{i + 1:012d}.jpg"))
    return out


def test_geometry_matches_reference_golden(golden):
    """With g13's seeds the host geometry reproduces the reference's trans_inv and output box bit for bit, and its input-pixel
    joints to <= 1 float32 ulp (the reference's np.dot may fuse multiply-adds; ours is separately rounded float64)."""
    g = golden("g13_augment.npz")
    samples = g13_samples(g)
    not_equal = 0
    for i, s in enumerate(samples):
        boxes_before = list(s.box)
        seed = int(g["seeds"][i])
        geo = g13_transform(g, bool(g["augment"][i])).geometry([s], (random.Random(seed), np.random.RandomState(seed)))
        assert s.box == boxes_before                                          # the caller's box is not mutated
        np.testing.assert_array_equal(geo.trans_inv[0], g["trans_inv_f64"][i])
        np.testing.assert_array_equal(geo.trans_inv[0].astype(np.float32), g["trans_inv"][i])
        np.testing.assert_array_equal(geo.boxes[0], g["out_boxes"][i])
        assert bool(geo.flip[0]) == bool(g["flip"][i])
        ref = g["out_joints"][i]
        ulp = np.abs(geo.joints[0].view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (i, ulp.max())
        not_equal += int((ulp > 0).sum())
    print(f"input-pixel joints not bit-equal to the reference: {not_equal} of {g['joints'].size // 3}")


class _Recorder:
    def __init__(self, log, tag, uniform_values=()):
        self.log, self.tag, self.values = log, tag, list(uniform_values)

    def uniform(self, *args):
        self.log.append((f"{self.tag}.uniform",) + args)
        if self.values:
            return self.values.pop(0)
        return (args[0] + args[1]) / 2 if args else 0.25

    def normal(self, *args):
        self.log.append((f"{self.tag}.normal",) + args)
        return 0.0


def _draws(tf, path_scale):
    log = []
    s = types.SimpleNamespace(img=np.zeros((200, 150, 3), np.uint8), box=[10.0, 20.0, 90.0, 180.0], joints=np.ones((17, 3), np.float32),
                              shape=(150, 200))
    tf.geometry([s], (_Recorder(log, "random", [path_scale]), _Recorder(log, "np")))
    return log


def test_draw_order_every_branch():
    crop = [("random.uniform", 0, 1), ("random.uniform", 0, 1), ("random.uniform", 0, 1)]
    jitter = [("random.uniform", 0, 1), ("np.normal", -0.0142, 0.1158), ("np.normal", 0.0043, 0.068), ("np.normal", 0.0154, 0.1337),
              ("np.normal", -0.0013, 0.0711)]
    tail = [("np.uniform", 0.7, 1.3), ("np.uniform", -40, 40)]
    with_pairs = RefineSimpleTransform(COCO_JOINT_PAIRS)
    no_pairs = RefineSimpleTransform(None)
    assert _draws(with_pairs, 0.9) == crop + tail + [("np.uniform",)]
    assert _draws(with_pairs, 0.5) == jitter + tail + [("np.uniform",)]
    assert _draws(no_pairs, 0.9) == crop + tail
    assert _draws(no_pairs, 0.5) == jitter + tail
    val = RefineSimpleTransform(None, scale=(1.0, 1.0), ratio=(0, 0), rand_crop=False)
    assert _draws(val, 0.5) == [("np.uniform", 1.0, 1.0), ("np.uniform", 0, 0)]


def test_flip_and_joint_helpers():
    from simple_pose_amd.commons.joint_utils import affine_transform_batch, flip_joints
    j = np.array([[1.5, 2.0, 1.0], [10.25, 3.0, 0.0], [7.0, 8.0, 1.0]], np.float32)
    f = flip_joints(j, 20, [[1, 2]])
    np.testing.assert_array_equal(f, np.array([[17.5, 2.0, 1.0], [12.0, 8.0, 1.0], [8.75, 3.0, 0.0]], np.float32))
    t = np.array([[2.0, 0.0, 1.0], [0.0, 0.5, -1.0]])
    a = affine_transform_batch(j, t)
    np.testing.assert_array_equal(a, np.array([[4.0, 0.0, 1.0], [10.25, 3.0, 0.0], [15.0, 3.0, 1.0]], np.float32))
    assert a.dtype == np.float32 and j[0, 0] == np.float32(1.5)


@pytest.mark.parametrize("world", [1, 2, 8])
def test_loader_order_is_distributed_sampler(world):
    from torch.utils.data import BatchSampler, DistributedSampler
    n, bs, seed = 45, 4, 7
    samples = list(range(n))
    for rank in range(world):
        loader = GpuAugmentLoader(samples, bs, rank, world, seed=seed)
        for epoch in (0, 3):
            ds = DistributedSampler(samples, num_replicas=world, rank=rank, shuffle=True, seed=seed)
            ds.set_epoch(epoch)
            loader.set_epoch(epoch)
            want = [i for b in BatchSampler(ds, bs, drop_last=True) for i in b]
            assert loader.indices() == want
            assert len(loader) == len(want) // bs


def test_loader_draws_depend_on_seed_epoch_rank():
    a = GpuAugmentLoader([], 4, 0, 2, seed=1)
    b = GpuAugmentLoader([], 4, 1, 2, seed=1)
    ra, rb = a.rng(), b.rng()
    assert ra[0].random() != rb[0].random()
    assert a.rng()[1].uniform() == a.rng()[1].uniform()
    a.set_epoch(1)
    assert a.rng()[1].uniform() != GpuAugmentLoader([], 4, 0, 2, seed=1).rng()[1].uniform()


def test_header_declares_batch_warp():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    assert "int sp_warp_affine_batch_u8c3_to_nchw_f32(" in hdr
    assert "sp_warp_affine_batch_u8c3_to_nchw_f32" in _lib.SYMBOLS
    assert "#define SP_ABI_VERSION 36" in hdr and _lib.ABI_VERSION == 36


def test_empty_geometry():
    geo = RefineSimpleTransform(COCO_JOINT_PAIRS).geometry([])
    assert geo.m_fwd.shape == (0, 2, 3) and geo.trans_inv.shape == (0, 2, 3) and geo.boxes.shape == (0, 4)
    assert torch.from_numpy(geo.hm_joints).shape[0] == 0


def test_batched_maps_equal_per_sample_calls():
    """The batch geometry (element-wise over the batch) has the bits of the per-sample helpers, over many random draws."""
    from simple_pose_amd.commons.joint_utils import center_scale_to_box, get_affine_transform, get_affine_transform_batch
    rng = np.random.default_rng(0)
    n = 300
    centers = rng.uniform(-50, 700, (n, 2)).astype(np.float32)
    scales = (rng.uniform(5, 600, (n, 2)) * rng.uniform(0.7, 1.3, (n, 1))).astype(np.float32)
    rots = rng.uniform(-40, 40, n)
    rots[:5] = 0.0
    (tr, _), (jt, ji) = get_affine_transform_batch(centers, scales, rots, ((192, 256), (48, 64)))
    for i in range(n):
        a, _ = get_affine_transform(centers[i], scales[i], rots[i], (192, 256))
        b, c = get_affine_transform(centers[i], scales[i], rots[i], (48, 64))
        np.testing.assert_array_equal(tr[i], a)
        np.testing.assert_array_equal(jt[i], b)
        np.testing.assert_array_equal(ji[i], c)
    samples = [types.SimpleNamespace(img=np.zeros((480, 640, 3), np.uint8), box=[float(x), float(y), float(x + 90), float(y + 200)],
                                     joints=np.ones((17, 3), np.float32), shape=(640, 480)) for x, y in rng.uniform(0, 400, (40, 2))]
    geo = RefineSimpleTransform(COCO_JOINT_PAIRS).geometry(samples, (random.Random(2), np.random.RandomState(2)))
    r = (random.Random(2), np.random.RandomState(2))
    for i, s in enumerate(samples):                            # one sample at a time, the same draws in sequence
        one = RefineSimpleTransform(COCO_JOINT_PAIRS).geometry([s], r)
        for k in ("m_fwd", "trans_inv", "joints", "hm_joints", "boxes", "flip"):
            np.testing.assert_array_equal(getattr(geo, k)[i], getattr(one, k)[0])
    assert geo.flip.any() and not geo.flip.all()
    c = np.array([100.5, 60.25], np.float32)
    sc = np.array([90.0, 120.0], np.float32)
    assert tuple(np.float32(v) for v in center_scale_to_box(c, sc)) == (np.float32(55.5), np.float32(0.25), np.float32(145.5), np.float32(120.25))


def test_loader_epoch_advances_after_full_pass():
    loader = GpuAugmentLoader([], 4, 0, 1, seed=3)
    assert loader.epoch == 0 and list(loader) == [] and loader.epoch == 1
    loader.set_epoch(7)
    assert loader.epoch == 7
