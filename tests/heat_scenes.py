"""The heat-overlay scenes shared by tests/test_heat_core_cpu.py (the CPU program), tests/test_heat_host.py and tests/test_gpu_heat.py (the
kernels): the frame's buffers as sp_topdown_plan, the pose network and sp_oks_nms leave them, seeded.  A scene is a dict: img uint8
[h, w, 3], hm float32 [rows, J, mh, mw], trans_inv float32 [rows, 2, 3], keep int32 [rows], keep_count int32 [B], seg int32 [B + 1],
lut uint8 [256, 3] (random, so an index error shows)."""
import numpy as np

from tests import heat_ref


def _background(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def random_lut(seed=77):
    return np.random.default_rng(seed).integers(0, 256, (256, 3), dtype=np.uint8)


def maps(rng, J, mh, mw):
    """One person's maps: a Gaussian bump per joint (peak 0.3 .. 1.1) on a little noise below zero and above, then the special values:
    NaN (in one joint, and in every joint of a cell), infinities of both signs, values above 1 and below 0, and k / 255 and k / 510,
    whose products with the scales 255 and 510 sit on or just under integers."""
    y, x = np.mgrid[0:mh, 0:mw].astype(np.float64)
    out = np.empty((J, mh, mw), np.float32)
    for j in range(J):
        cy, cx, s = rng.uniform(0, mh), rng.uniform(0, mw), rng.uniform(0.6, max(0.7, min(mh, mw) / 5.0))
        out[j] = rng.uniform(0.3, 1.1) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)) + rng.uniform(-0.02, 0.02, (mh, mw))
    flat = out.reshape(J, -1)
    cells = flat.shape[1]
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1.7, -0.6, 37 / 255, 200 / 255, 255 / 255, 101 / 510, 1 / 255, 254.5 / 255)):
        flat[rng.integers(0, J), rng.integers(0, cells)] = v
    flat[:, rng.integers(0, cells)] = np.nan                     # no number in any joint: 0
    at = rng.integers(0, cells)
    flat[:, at] = -np.inf                                        # the maximum is -inf: 0, with scale 0 a NaN product
    flat[0, at - 1] = np.inf                                     # +inf: 255
    for k in range(0, 256, 5):                                   # a ladder of exact quotients through every joint
        flat[:, rng.integers(0, cells)] = np.float32(k) / np.float32(255)
    return out


def box_map(bx, by, bw, bh, mh, mw):
    """trans_inv that lays the mh x mw map over the image box (bx, by, bw, bh): what sp_topdown_plan gives an upright person."""
    return [[bw / mw, 0.0, bx], [0.0, bh / mh, by]]


def transforms(kind, h, w, mh, mw):
    """The persons of a scene as trans_inv matrices (heat-map px -> image px)."""
    if kind == "street":
        th = 0.45                                                # rotated by 26 degrees and sheared
        return [box_map(0.08 * w, 0.1 * h, 0.5 * w, 0.7 * h, mh, mw),                        # a and b overlap: the maximum decides
                box_map(0.3 * w, 0.25 * h, 0.45 * w, 0.6 * h, mh, mw),
                box_map(0.75 * w, 0.4 * h, 0.6 * w, 0.9 * h, mh, mw),                        # c: half outside the image
                box_map(w + 40.0, h + 30.0, 50.0, 70.0, mh, mw),                             # d: wholly outside
                [[0.5 * w / mw * np.cos(th), -0.4 * h / mh * np.sin(th) + 0.3, 0.55 * w],   # e: rotated and sheared
                 [0.5 * w / mw * np.sin(th), 0.4 * h / mh * np.cos(th), 0.02 * h]]]
    if kind == "extremes":
        inside, outside = np.float32(1.0) / np.float32(1024.0), np.nextafter(np.float32(1.0 / 1024.0), np.float32(0))
        return [[[80.0, 0.0, -70.0 * (mw / 2.0)], [0.0, 80.0, -75.0 * (mh / 2.0)]],          # a map cell covers more than a 64 x 16 tile
                [[0.9 / mw, 0.0, 0.4 * w + 0.05], [0.0, 0.9 / mh, 0.5 * h + 0.05]],          # the whole map under one pixel
                [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],                                          # singular: a dead slot's zeros
                [[inside, 0.0, round(0.3 * w) - mw / 2048.0], [0.0, inside, round(0.2 * h) - mh / 2048.0]],      # |F| == 1024: just inside; the
                                                                                             # map's middle on a pixel centre: one pixel
                [[outside, 0.0, 0.6 * w], [0.0, outside, 0.7 * h]]]                          # |F| > 1024: skipped
    if kind == "limits":
        return [[[1.0, 0.0, -1048576.0], [0.0, 1.0, 0.0]],                                   # the offset F[2] == 2^20: kept, far outside
                [[1.0, 0.0, -1048577.0], [0.0, 1.0, 0.0]],                                   # 2^20 + 1: skipped
                [[1.0, 2.0, 3.0], [2.0, 4.0, 5.0]],                                          # singular, not zero
                [[np.nan, 0.0, 0.0], [0.0, 1.0, 0.0]],                                       # not finite
                box_map(0.1 * w, 0.1 * h, 0.8 * w, 0.8 * h, mh, mw)]                         # and one that draws
    raise ValueError(kind)


def make(kind="street", h=97, w=131, mh=64, mw=48, J=17, seed=1, spare_rows=2):
    """The persons of `kind` scattered over rows + spare rows of one image; the keep list names them.  The spare rows hold maps and
    transforms that would draw, and nobody may read them."""
    rng = np.random.default_rng(seed)
    T = transforms(kind, h, w, mh, mw)
    n = len(T)
    rows = n + spare_rows
    where = rng.permutation(rows)[:n]
    hm = np.stack([maps(rng, J, mh, mw) for _ in range(rows)])
    ti = np.tile(np.array(box_map(0.0, 0.0, float(w), float(h), mh, mw), np.float32), (rows, 1, 1))
    keep = np.full(rows, -1, np.int32)
    with np.errstate(all="ignore"):
        for p in range(n):
            ti[where[p]] = np.array(T[p], np.float32)
    keep[:n] = where
    return {"img": _background(h, w, seed + 100), "hm": hm, "trans_inv": ti, "keep": keep, "keep_count": np.array([n], np.int32),
            "seg": np.array([0, rows], np.int32), "lut": random_lut(seed + 7)}


def two_images():
    """Two images' persons in one set of buffers (seg = [0, 2, 5]): image 0 keeps two rows, image 1 keeps three."""
    rng = np.random.default_rng(21)
    h, w, mh, mw = 33, 64, 6, 5
    hm = np.stack([maps(rng, 17, mh, mw) for _ in range(5)])
    ti = np.array([box_map(rng.uniform(0, 30), rng.uniform(0, 10), rng.uniform(15, 40), rng.uniform(10, 25), mh, mw) for _ in range(5)], np.float32)
    return {"img": _background(h, w, 6), "hm": hm, "trans_inv": ti, "keep": np.array([1, 0, 4, 2, 3], np.int32),
            "keep_count": np.array([2, 3], np.int32), "seg": np.array([0, 2, 5], np.int32), "lut": random_lut(9)}


def cases():
    """(name, scene, style, image) of every case the CPU program and the kernels both run; all of them draw something."""
    S = heat_ref.Style
    street = make("street")
    return [("street", street, S(), 0),
            ("street_wide", make("street", 96, 128), S(alpha="constant", opacity16=16, threshold=1), 0),
            ("tiny", make("street", 3, 5, seed=3), S(threshold=1), 0),
            ("extremes", make("extremes", seed=2), S(threshold=1, opacity16=16, alpha="constant"), 0),
            ("extremes_wide", make("extremes", 96, 128, seed=2), S(threshold=1), 0),
            ("limits", make("limits", seed=4), S(), 0),
            ("map_6x5", make("street", mh=6, mw=5, seed=5), S(), 0),
            ("map_6x5_extremes", make("extremes", 96, 128, mh=6, mw=5, seed=5), S(threshold=1), 0),
            ("map_1x1", make("street", mh=1, mw=1, J=1, seed=6), S(threshold=1), 0),
            ("one_joint_net", make("street", J=1, seed=7), S(), 0),
            ("joints_64", make("street", J=64, seed=8), S(joint_mask=(1 << 63) | (1 << 31) | 5), 0),
            ("one_joint_of_17", street, S(joint_mask=1 << 3, threshold=1), 0),
            ("scale_510", street, S(scale=510.0), 0),
            ("scale_small", street, S(scale=40.0, threshold=1), 0),
            ("two_images_0", two_images(), S(), 0), ("two_images_1", two_images(), S(alpha="constant"), 1)]


def reference(scene, style, image=0):
    rows = heat_ref.live_rows(scene["keep"], scene["keep_count"], scene["seg"], image, scene["hm"].shape[0])
    return heat_ref.overlay(scene["img"], style, scene["hm"], scene["trans_inv"], rows, scene["lut"])


def style_struct(style):
    """The heat_ref.Style as the C ABI's sp_heat_style."""
    from simple_pose_amd import _lib
    st = _lib.HeatStyle()
    st.joint_mask, st.scale, st.threshold, st.opacity16 = style.joint_mask & heat_ref.ALL_JOINTS, float(style.scale), style.threshold, style.opacity16
    st.alpha = _lib.SP_HEAT_ALPHAS[style.alpha]
    return st
