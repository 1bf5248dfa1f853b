"""GPU training transform (RefineSimpleTransform.batch / GpuAugmentLoader / sp_warp_affine_batch_u8c3_to_nchw_f32) against the
reference's recorded outputs (g13) and the C restatement of cv.warpAffine (oracle/pose_oracle)."""
import random
import types

import numpy as np
import pytest
import torch

from oracle import pose_oracle
from simple_pose_amd import _lib
from simple_pose_amd.commons.transforms import RefineSimpleTransform
from simple_pose_amd.datasets.coco import COCO_JOINT_PAIRS, GpuAugmentLoader
from tests.test_augment_host import g13_samples, g13_transform

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)


def collate_norm(crops_bhwc_bgr):
    """datasets/coco.py:136-137 in numpy: (img[..., ::-1].astype(float32) / 255.0 - rgb_mean), HWC -> CHW."""
    x = crops_bhwc_bgr[..., ::-1].astype(np.float32) / 255.0 - np.array(MEAN, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def _smooth(rng, h, w):
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3)).astype(np.float32)
    up = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w]
    return np.clip(up + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def _warp_batch(imgs, flips, M, oh=256, ow=192):
    """Raw C-ABI call: (fp32 NCHW, uint8 crops)."""
    n = len(imgs)
    x = torch.empty((n, 3, oh, ow), dtype=torch.float32, device="cuda")
    crops = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
    srcs = np.array([t.data_ptr() for t in imgs], np.uint64)
    hw = np.array([t.shape[:2] for t in imgs], np.int32).reshape(n, 2)
    fl = np.asarray(flips, np.int32)
    M = np.ascontiguousarray(M, np.float64)
    mean = (__import__("ctypes").c_float * 3)(*MEAN)
    _lib.check(_lib.lib().sp_warp_affine_batch_u8c3_to_nchw_f32(srcs.ctypes.data, hw.ctypes.data, fl.ctypes.data, M.ctypes.data, n, oh, ow,
                                                                 mean, _lib.ptr(x), _lib.ptr(crops), _lib.current_stream()))
    return x, crops


def test_g13_against_reference(golden, measured):
    g = golden("g13_augment.npz")
    samples = g13_samples(g)
    srcs = {}
    worst, n_off = 0.0, 0
    for i, s in enumerate(samples):
        si = int(g["src_index"][i])
        s.img = srcs.setdefault(si, torch.from_numpy(g[f"src{si}"]).cuda())
        seed = int(g["seeds"][i])
        tf = g13_transform(g, bool(g["augment"][i]))
        crops = torch.empty((1, *g["crops"].shape[1:]), dtype=torch.uint8, device="cuda")
        x, hm, mask, tinv = tf.batch([s], (random.Random(seed), np.random.RandomState(seed)), crops=crops)
        geo = tf.geometry([s], (random.Random(seed), np.random.RandomState(seed)))
        np.testing.assert_array_equal(crops[0].cpu().numpy(), g["crops"][i])
        np.testing.assert_array_equal(x.cpu().numpy(), collate_norm(g["crops"][i:i + 1]))
        np.testing.assert_array_equal(mask[0].cpu().numpy(), g["masks"][i])
        np.testing.assert_array_equal(tinv[0].cpu().numpy(), g["trans_inv"][i])
        hm_e = hm[0].cpu().numpy()[:, ::2]
        ref = g["heat_maps_even_rows"][i]
        exact = np.all(geo.joints[0] == g["out_joints"][i], axis=-1)
        np.testing.assert_array_equal(hm_e[exact], ref[exact])
        if (~exact).any():
            n_off += int((~exact).sum())
            worst = max(worst, float(np.abs(hm_e[~exact] - ref[~exact]).max()))
    measured("heat_map_maxdiff_non_bit_equal_joints", worst)
    measured("joints_not_bit_equal", n_off)


@pytest.mark.parametrize("deg", [-40.0, 0.0, 40.0])
def test_flip_equals_warp_of_flipped_image(deg):
    rng = np.random.default_rng(int(deg) + 100)
    imgs = [_smooth(rng, 97, 131), _smooth(rng, 240, 321), _smooth(rng, 181, 150)]
    th = np.deg2rad(deg)
    M = []
    for k, im in enumerate(imgs):
        s = [0.9, 1.7, 0.6][k]
        c, sn = s * np.cos(th), s * np.sin(th)
        M.append([[c, -sn, 96 - c * im.shape[1] * 0.3 + sn * 40], [sn, c, 128 - sn * im.shape[1] * 0.3 - c * 60]])   # partly outside
    M = np.array(M)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    dev_f = [torch.from_numpy(np.ascontiguousarray(np.fliplr(im))).cuda() for im in imgs]
    _, c_flip = _warp_batch(dev, [1, 1, 1], M)
    _, c_pre = _warp_batch(dev_f, [0, 0, 0], M)
    c_flip, c_pre = c_flip.cpu().numpy(), c_pre.cpu().numpy()
    for k, im in enumerate(imgs):
        want = pose_oracle.warp_affine_u8c3(np.fliplr(im), M[k], (192, 256))
        np.testing.assert_array_equal(c_flip[k], want)
        np.testing.assert_array_equal(c_pre[k], want)
        assert (want.max(-1) == 0).any() and (want.max(-1) > 0).any()


@pytest.mark.parametrize("B", [1, 31, 32, 33, 70])
def test_many_sources_per_batch(B):
    rng = np.random.default_rng(B)
    sizes = [(97, 131), (480, 640), (1000, 1500), (333, 257)]
    imgs = [_smooth(rng, h, w) for h, w in sizes]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    pick = rng.integers(0, len(imgs), B)
    flips = rng.integers(0, 2, B)
    M = []
    for b in range(B):
        h, w = sizes[pick[b]]
        s, th = rng.uniform(0.3, 2.0), rng.uniform(-0.7, 0.7)
        M.append([[s * np.cos(th), -s * np.sin(th), rng.uniform(-s * w, 96)], [s * np.sin(th), s * np.cos(th), rng.uniform(-s * h, 128)]])
    M = np.array(M)
    x, crops = _warp_batch([dev[p] for p in pick], flips, M)
    x, crops = x.cpu().numpy(), crops.cpu().numpy()
    want = np.stack([pose_oracle.warp_affine_u8c3(np.fliplr(imgs[p]) if f else imgs[p], M[b], (192, 256))
                     for b, (p, f) in enumerate(zip(pick, flips))])
    np.testing.assert_array_equal(crops, want)
    np.testing.assert_array_equal(x, collate_norm(want))


def _synthetic_samples(n, seed, sizes=((480, 640), (375, 500), (427, 640), (97, 131))):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(_smooth(rng, h, w)).cuda() for h, w in sizes]
    out = []
    for i in range(n):
        img = imgs[i % len(imgs)]
        H, W = img.shape[:2]
        x1, y1 = rng.uniform(0, W * 0.6), rng.uniform(0, H * 0.5)
        x2, y2 = min(W - 1.0, x1 + rng.uniform(20, W * 0.5)), min(H - 1.0, y1 + rng.uniform(40, H * 0.5))
        j = np.zeros((17, 3), np.float32)
        j[:, 0] = rng.uniform(x1, x2, 17)
        j[:, 1] = rng.uniform(y1, y2, 17)
        j[:, 2] = (rng.random(17) > 0.2).astype(np.float32)
        out.append(types.SimpleNamespace(img=img, box=[float(x1), float(y1), float(x2), float(y2)], joints=j, shape=(W, H), img_id=1000 + i))
    return out


def test_heat_maps_and_masks_follow_host_joints():
    samples = _synthetic_samples(12, 5)
    tf = RefineSimpleTransform(COCO_JOINT_PAIRS)
    x, hm, mask, tinv = tf.batch(samples, (random.Random(3), np.random.RandomState(3)))
    geo = tf.geometry(samples, (random.Random(3), np.random.RandomState(3)))
    assert geo.flip.any() and not geo.flip.all()
    want_hm, want_m = RefineSimpleTransform.get_heat_map(torch.from_numpy(geo.hm_joints).cuda())
    assert torch.equal(hm, want_hm) and torch.equal(mask, want_m)
    np.testing.assert_array_equal(tinv.cpu().numpy(), geo.trans_inv.astype(np.float32))
    inv = geo.hm_joints[..., 2] == 0
    assert inv.any() and (mask.cpu().numpy()[inv] == 0).all() and (hm.cpu().numpy()[inv] == 0).all()
    for b in np.nonzero(geo.flip)[0]:                          # flipped samples: left/right rows swapped before the map
        from simple_pose_amd.commons.joint_utils import flip_joints
        f = flip_joints(samples[b].joints, samples[b].shape[0], COCO_JOINT_PAIRS)
        np.testing.assert_array_equal(geo.hm_joints[b][:, 2], f[:, 2])


def test_no_augment_matches_crop_boxes():
    from simple_pose_amd.datasets.naive_data import crop_boxes
    samples = _synthetic_samples(5, 9, sizes=((480, 640),))
    tf = RefineSimpleTransform(None, scale=(1.0, 1.0), ratio=(0, 0), rand_crop=False)
    crops = torch.empty((5, 256, 192, 3), dtype=torch.uint8, device="cuda")
    x, hm, mask, tinv = tf.batch(samples, crops=crops)
    c2, t2, *_ = crop_boxes(samples[0].img, np.array([s.box for s in samples]))
    assert torch.equal(crops, c2) and torch.equal(tinv, t2)


def test_empty_batch():
    x, hm, mask, tinv = RefineSimpleTransform(COCO_JOINT_PAIRS).batch([])
    assert x.shape == (0, 3, 256, 192) and hm.shape[0] == 0 and mask.shape[0] == 0 and tinv.shape == (0, 2, 3)


def test_out_buffers_written_in_place():
    samples = _synthetic_samples(4, 2)
    tf = RefineSimpleTransform(COCO_JOINT_PAIRS)
    a = tf.batch(samples, (random.Random(1), np.random.RandomState(1)))
    out = (torch.full((4, 3, 256, 192), 7.0, device="cuda"), torch.full((4, 17, 64, 48), 7.0, device="cuda"),
           torch.full((4, 17), 7.0, device="cuda"), torch.full((4, 2, 3), 7.0, device="cuda"))
    b = tf.batch(samples, (random.Random(1), np.random.RandomState(1)), out=out)
    assert all(t is o for t, o in zip(b, out)) and all(torch.equal(p, q) for p, q in zip(a, b))


def test_loader_feeds_train_step():
    from simple_pose_amd.nets import pose_resnet_dconv
    from simple_pose_amd.train import PoseTrainer
    samples = _synthetic_samples(40, 11)

    def run():
        torch.manual_seed(0)
        model = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17).cuda().train()
        trainer = PoseTrainer(model, lr=1e-3, dtype="bf16")
        loader = GpuAugmentLoader(samples, 8, 0, 1, seed=4)
        loader.set_epoch(1)
        losses, batches = [], []
        for xb, hm, mask, tinv, ids in loader:
            assert xb.shape == (8, 3, 256, 192) and hm.shape == (8, 17, 64, 48) and len(ids) == 8
            batches.append([t.clone() for t in (xb, hm, mask, tinv)] + [ids])
            loss = trainer.step(xb, hm, mask)
            losses.append(float(loss.reshape(-1)[0]))
        torch.cuda.synchronize()
        return losses, batches

    l1, b1 = run()
    l2, b2 = run()
    assert len(l1) == 5 and all(np.isfinite(l1))
    assert l1 == l2
    for p, q in zip(b1, b2):
        assert all(torch.equal(s, t) for s, t in zip(p[:4], q[:4])) and p[4] == q[4]
