"""The overlay scenes shared by tests/test_render_core_cpu.py (the CPU program) and tests/test_gpu_render.py (the kernels): the frame's
buffers as sp_oks_nms / sp_track_associate leave them, seeded.  A scene is a dict: img uint8 [h, w, 3], kps float64 [rows, J, 3],
box float32 [rows, 5], track_id int32 [rows], keep int32 [rows], keep_count int32 [B], seg int32 [B + 1]."""
import numpy as np

from tests import render_ref

J = 17
LIST = 512                     # render.hip's RND_LIST: primitive indices a tile collects before it applies them
CHUNK = 256                    # primitives per scan step


def _background(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _frame(img, persons, boxes, ids, spare_rows=2, seed=0):
    """The persons (pick order) scattered over rows + spare rows of one image; the keep list names them in pick order."""
    rng = np.random.default_rng(seed)
    n = len(persons)
    rows = n + spare_rows
    where = rng.permutation(rows)[:n]
    kps = rng.uniform(0, 40, (rows, J, 3))
    box = rng.uniform(0, 40, (rows, 5)).astype(np.float32)
    tid = rng.integers(1, 90, rows).astype(np.int32)
    keep = np.full(rows, -1, np.int32)
    for p in range(n):
        kps[where[p]], box[where[p], :4], tid[where[p]] = persons[p], boxes[p], ids[p]
    keep[:n] = where
    return {"img": img, "kps": kps, "box": box, "track_id": tid, "keep": keep, "keep_count": np.array([n], np.int32),
            "seg": np.array([0, rows], np.int32)}


def ragged():
    """70 x 45 (w % 4 != 0, partial tiles both ways), three persons: a joint below the threshold (its limbs are absent), a NaN coordinate,
    joints left of, above and beyond the image, a zero-length limb, and two persons that overlap (the order shows)."""
    rng = np.random.default_rng(11)
    h, w = 45, 70
    a = np.concatenate([rng.uniform((5, 4), (50, 40), (J, 2)), rng.uniform(0.3, 1.0, (J, 1))], 1)
    a[7, 2] = 0.1                                   # below in_vis_thre: joint 7 and the limbs (5,7), (7,9) are absent
    a[3, 0] = np.nan                                # joint 3 and limb (1,3), (3,5) empty
    a[9, 2] = np.nan                                # a NaN confidence is not visible
    b = a + rng.uniform(-3, 3, (J, 3)) * (1, 1, 0)  # on top of a: overlapping persons
    b[:, 2] = rng.uniform(0.3, 1.0, J)
    b[13] = (-6.3, 20.2, 0.9)                       # left of the image
    b[15] = (30.1, -9.7, 0.9)                       # above it
    b[14] = (77.5, 52.25, 0.9)                      # beyond the far corner
    b[11, :2] = b[12, :2]                           # limb (11,12) has zero length
    c = np.concatenate([rng.uniform((40, 20), (69.9, 44.9), (J, 2)), rng.uniform(0.21, 1.0, (J, 1))], 1)
    c[0, :2] = (1e6, 3.0)                           # |v| > 32768: empty
    c[1, :2] = (np.inf, 3.0)
    c[2, :2] = (63.96875, 15.96875)                 # a tie of the quantisation (x.5 sixteenths) on a tile corner
    boxes = [(3.2, 2.7, 52.4, 41.1), (-4.0, -3.0, 80.0, 47.5), (38.5, 18.5, 69.5, 44.5)]
    return _frame(_background(h, w, 1), [a, b, c], boxes, [7, 0, 35], seed=2)


def crowd(persons, seed=5):
    """132 x 40 (w % 4 == 0: the 4-byte path), `persons` persons with 17 joints on the same 20 x 20 px spot, one joint in five invisible."""
    rng = np.random.default_rng(seed)
    h, w = 40, 132
    people, boxes = [], []
    for _ in range(persons):
        k = np.concatenate([rng.uniform((70, 17), (90, 31), (J, 2)), np.ones((J, 1))], 1)
        k[rng.permutation(J)[:3], 2] = 0.05         # 3 of 17: about one in five
        people.append(k)
        boxes.append((70 + rng.uniform(0, 2), 17 + rng.uniform(0, 2), 88 + rng.uniform(0, 2), 29 + rng.uniform(0, 2)))
    return _frame(_background(h, w, 3), people, boxes, list(range(1, persons + 1)), spare_rows=0, seed=4)


def two_images():
    """Two images' persons in one set of buffers (seg = [0, 2, 5]): image 0 keeps two rows, image 1 keeps three."""
    rng = np.random.default_rng(21)
    h, w = 33, 64
    kps = np.concatenate([rng.uniform((2, 2), (62, 31), (5, J, 2)), rng.uniform(0.1, 1.0, (5, J, 1))], 2)
    x1, y1 = rng.uniform(0, 20, 5), rng.uniform(0, 10, 5)
    box = np.stack([x1, y1, x1 + rng.uniform(10, 40, 5), y1 + rng.uniform(10, 20, 5), rng.uniform(0, 1, 5)], 1).astype(np.float32)
    return {"img": _background(h, w, 6), "kps": kps, "box": box, "track_id": np.array([3, 1, 4, 1, 5], np.int32),
            "keep": np.array([1, 0, 4, 2, 3], np.int32), "keep_count": np.array([2, 3], np.int32), "seg": np.array([0, 2, 5], np.int32)}


def styles():
    """Both colour modes at full and partial opacity; the skeleton is COCO's."""
    return {"person": render_ref.Style(colour_by="person"), "part": render_ref.Style(colour_by="part", opacity=11, joint_r=40, limb_r=20, box_r=12)}


def reference(scene, style, image=0, with_ids=True):
    kps, box, tid = render_ref.kept(scene["kps"], scene["box"], scene["track_id"] if with_ids else None, scene["keep"], scene["keep_count"],
                                    scene["seg"], image)
    return render_ref.render(scene["img"], style, kps, box, tid)


def style_struct(style):
    """The render_ref.Style as the C ABI's sp_render_style."""
    from simple_pose_amd import _lib
    st = _lib.RenderStyle()
    st.edges = len(style.skeleton)
    for e, (a, b) in enumerate(style.skeleton):
        st.edge[e][0], st.edge[e][1] = a, b
    st.joint_r, st.limb_r, st.box_r, st.opacity = style.joint_r, style.limb_r, style.box_r, style.opacity
    st.in_vis_thre = style.in_vis_thre
    st.colour_by = _lib.SP_RENDER_COLOUR_PART if style.colour_by == "part" else _lib.SP_RENDER_COLOUR_PERSON
    st.palette_n = style.palette.shape[0]
    for i, c in enumerate(style.palette.tolist()):
        st.palette[i][0], st.palette[i][1], st.palette[i][2] = c
    return st
