"""tools/gen_golden_augment.py - TEST INFRASTRUCTURE.  Run in the build container (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_augment.py [--check]

g13_augment.npz: the reference's training transform (`RefineSimpleTransform.__call__`, commons/transforms.py:193-223) and the
arithmetic of `MSCOCO.collate_fn` (datasets/coco.py:124-148) on a handful of samples from three smooth synthetic sources of
different sizes (one with an odd width).  `random` and `np.random` are reseeded per sample with the recorded seed; the seeds are
searched deterministically so that the fixture provably covers both `box_crop` branches, flip on and off, crops that leave the
image, invisible joints, joints outside the heat map and the validation transform (augment=False).  cv2 is absent here: its two
primitives are the restatements of oracle/pose_oracle.* that oracle.ref_import plugs into the cv2 stub, so - as with g9 - this
fixture pins the reference's glue and draw order, not OpenCV's arithmetic.

To keep the file small the fixture runs the transform at input 96x128 / heat map 24x32 (the reference's 192x256 / 48x64 at half
size: same aspect ratio, same code path).  The zip is written with fixed timestamps, so a rerun reproduces the file byte for byte;
--check regenerates in memory and compares with the committed file.
"""
from __future__ import annotations

import importlib
import io
import os
import random
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_augment.npz")
INPUT_SHAPE, OUTPUT_SHAPE = (96, 128), (24, 32)
SOURCE_SEED = 13
SOURCE_HW = ((110, 150), (97, 131), (140, 101))           # (H, W); 131 and 101 are odd
JOINT_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
# (source, box x1 y1 x2 y2, augment, wanted box_crop branch ("crop": path_scale > 0.85 / "jitter" / None), wanted flip, must leave
# the image).  Boxes are lists of Python floats, as MSCOCO builds them.
SPECS = [
    (0, [40.5, 20.25, 100.75, 100.0], True, "crop", True, False),
    (0, [10.0, 30.0, 90.5, 106.0], True, "jitter", False, True),
    (1, [50.25, 5.5, 128.0, 90.75], True, "jitter", True, True),
    (1, [20.0, 15.0, 70.0, 90.0], True, "crop", False, False),
    (2, [30.5, 40.0, 90.25, 135.5], True, "jitter", True, False),
    (2, [2.0, 60.0, 70.0, 135.0], True, None, None, True),
    (0, [100.0, 40.0, 160.0, 120.0], False, None, None, True),
    (1, [30.0, 20.0, 90.0, 80.0], False, None, None, False),
]
J = 17


def sources():
    from scipy import ndimage
    rng = np.random.default_rng(SOURCE_SEED)
    out = []
    for h, w in SOURCE_HW:
        base = ndimage.gaussian_filter(rng.random((h, w, 3)), (3, 3, 0))
        base = (base - base.min()) / (base.max() - base.min())
        out.append((30 + 200 * base).astype(np.uint8))
    return out


def joints_for(k, box):
    """17 joints around the box: a few invisible, a few far outside it (they land off the heat map)."""
    rng = np.random.default_rng(100 + k)
    x1, y1, x2, y2 = box
    w, h = x2 - x1, y2 - y1
    j = np.zeros((J, 3), np.float32)
    j[:, 0] = x1 + rng.uniform(-0.1, 1.1, J) * w
    j[:, 1] = y1 + rng.uniform(-0.1, 1.1, J) * h
    j[:, 2] = 1.0
    j[rng.choice(J, 3, replace=False), 2] = 0.0
    far = rng.choice(J, 2, replace=False)
    j[far, 0] += np.float32(2.5 * w)
    return j


def predicted_draws(seed, augment):
    """The branch and flip the seed gives, by replaying the reference's draw order on fresh generators (independent of both the
    reference and the project): random.uniform (path_scale) [+ random.uniform x2 | np.random.normal x4], np.random.uniform (scale),
    np.random.uniform (rotation), np.random.uniform (flip)."""
    if not augment:
        return None, None
    r, n = random.Random(seed), np.random.RandomState(seed)
    crop = r.uniform(0, 1) > 0.85
    if not crop:
        for _ in range(4):
            n.normal(0, 1)
    n.uniform(0.7, 1.3); n.uniform(-40, 40)
    return ("crop" if crop else "jitter"), bool(n.uniform() < 0.5)


def make_transform(tr, augment):
    if augment:
        return tr.RefineSimpleTransform(joint_pairs=JOINT_PAIRS, input_shape=INPUT_SHAPE, output_shape=OUTPUT_SHAPE, scale=(0.7, 1.3),
                                        ratio=(-40, 40), rand_crop=True)
    return tr.RefineSimpleTransform(joint_pairs=None, input_shape=INPUT_SHAPE, output_shape=OUTPUT_SHAPE, scale=(1.0, 1.0), ratio=(0, 0),
                                    rand_crop=False)


def generate():
    ns = ref_import.load()
    tr = ns.transforms
    coco = importlib.import_module("datasets.coco")
    srcs = sources()
    items, seeds, joints_in, branch, flips = [], [], [], [], []
    for k, (si, box, augment, want_branch, want_flip, want_outside) in enumerate(SPECS):
        img = srcs[si]
        jin = joints_for(k, box)
        seed = 1000 * (k + 1)
        while True:
            b, f = predicted_draws(seed, augment)
            if (want_branch is None or b == want_branch) and (want_flip is None or f == want_flip):
                random.seed(seed)
                np.random.seed(seed)
                info = tr.KeyPoints(img_path=f"{k + 1:012d}.jpg", shape=(img.shape[1], img.shape[0]), box=list(box), joints=jin.copy())
                info.img = img
                out = make_transform(tr, augment)(info.clone())
                outside = bool((out.img.reshape(-1, 3).max(1) == 0).any())
                if not want_outside or outside:
                    break
            seed += 1
        items.append(out); seeds.append(seed); joints_in.append(jin); branch.append(b or ""); flips.append(bool(f))
    x, hm, mask, tinv, ids = coco.MSCOCO.collate_fn(items)
    vis_off = np.stack([(j[:, 2] > 0) & (m == 0) for j, m in zip(joints_in, mask.numpy())])
    # coverage, asserted on what the reference produced
    assert {"crop", "jitter"} <= set(branch) and True in flips and False in [f for f, s in zip(flips, SPECS) if s[2]]
    assert any(not s[2] for s in SPECS) and vis_off.any() and any((j[:, 2] == 0).any() for j in joints_in)
    crops = np.stack([it.img for it in items])
    assert (crops.reshape(len(items), -1, 3).max(-1) == 0).any(1).sum() >= 2
    data = {f"src{i}": s for i, s in enumerate(srcs)}
    data.update(
        src_index=np.array([s[0] for s in SPECS], np.int32),
        boxes=np.array([s[1] for s in SPECS], np.float64),
        augment=np.array([s[2] for s in SPECS]),
        joints=np.stack(joints_in),
        seeds=np.array(seeds, np.int64),
        branch=np.array(branch),
        flip=np.array(flips),
        input_shape=np.array(INPUT_SHAPE, np.int32),
        output_shape=np.array(OUTPUT_SHAPE, np.int32),
        joint_pairs=np.array(JOINT_PAIRS, np.int32),
        crops=crops,
        heat_maps_even_rows=np.ascontiguousarray(hm.numpy()[:, :, ::2]),      # every other row: keeps the file small
        masks=mask.numpy(),
        trans_inv=tinv.numpy(),
        trans_inv_f64=np.stack([it.trans_inv for it in items]),
        out_boxes=np.array([[float(v) for v in it.box] for it in items], np.float32),
        out_joints=np.stack([it.joints for it in items]),
        img_ids=np.array(ids, np.int64),
    )
    return data


def to_bytes(data) -> bytes:
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(data):
            arr = io.BytesIO()
            np.lib.format.write_array(arr, np.ascontiguousarray(data[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, arr.getvalue())
    return buf.getvalue()


def main():
    assert ref_import.available(), "needs the reference checkout (build container only)"
    data = generate()
    blob = to_bytes(data)
    if "--check" in sys.argv:
        same = open(OUT, "rb").read() == blob
        print("g13_augment.npz", "reproduced byte for byte" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as fh:
        fh.write(blob)
    print("g13_augment.npz", len(blob), "bytes; seeds", data["seeds"].tolist(), "branch", data["branch"].tolist(), "flip",
          data["flip"].tolist())


if __name__ == "__main__":
    main()
