"""The redaction scenes shared by tests/test_redact_core_cpu.py (the CPU program), tests/test_redact_host.py and tests/test_gpu_redact.py
(the kernels): the frame's buffers as sp_oks_nms leaves them, seeded.  A scene is a dict: img uint8 [h, w, 3], kps float64 [rows, J, 3],
box float32 [rows, 5], keep int32 [rows], keep_count int32 [B], seg int32 [B + 1]."""
import numpy as np

from tests import redact_ref

J = 17
CHUNK = 256                    # redact.hip's scan step: records per chunk


def _background(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _frame(img, persons, boxes, spare_rows=2, seed=0):
    """The persons scattered over rows + spare rows of one image; the keep list names them in order."""
    rng = np.random.default_rng(seed)
    n = len(persons)
    rows = n + spare_rows
    where = rng.permutation(rows)[:n]
    kps = rng.uniform(0, 40, (rows, J, 3))                       # the spare rows hold visible joints nobody may read
    box = rng.uniform(0, 40, (rows, 5)).astype(np.float32)
    keep = np.full(rows, -1, np.int32)
    for p in range(n):
        kps[where[p]], box[where[p], :4] = persons[p], boxes[p]
    keep[:n] = where
    return {"img": img, "kps": kps, "box": box, "keep": keep, "keep_count": np.array([n], np.int32), "seg": np.array([0, rows], np.int32)}


def _person(rng, head_xy, spread, c=0.9):
    """17 joints: the five head joints within `spread` px of head_xy, the body below it (the body is never read)."""
    k = np.concatenate([rng.uniform(0, 90, (J, 2)), np.full((J, 1), c)], 1)
    k[:5, :2] = np.asarray(head_xy) + rng.uniform(-spread, spread, (5, 2))
    return k


def street(h=97, w=131, seed=1):
    """h x w (default 97 x 131: w % 4 != 0, partial edge cells both ways), seven persons:
    a  an ordinary head well inside the image;
    b  no visible head joint: the fallback decides;
    c  head joints with a NaN, an infinite and a huge coordinate next to two good ones, a NaN confidence, and a box with a NaN (s = 0);
    d  a head whose centre lies left of the image and whose disc still reaches in;
    e  a person wholly beyond the far corner;
    f  every head joint rejected and a huge box: empty under every fallback;
    g  one visible head joint and a degenerate box: r == 0, a point."""
    rng = np.random.default_rng(seed)
    sx, sy = w / 131.0, h / 97.0
    a = _person(rng, (30.3 * sx, 18.7 * sy), 3.0)
    b = _person(rng, (95 * sx, 40 * sy), 3.0)
    b[:5, 2] = (0.1, 0.2, 0.0, -1.0, 0.19)                       # c == thre is not visible either
    c = _person(rng, (60 * sx, 70 * sy), 2.0)
    c[0, 0], c[1, 1], c[2, 0], c[3, 2] = np.nan, np.inf, 1e6, np.nan
    d = _person(rng, (-6.2, 40.4 * sy), 0.5)
    e = _person(rng, (w + 170.0, h + 200.0), 3.0)
    f = _person(rng, (20 * sx, 80 * sy), 1.0)
    f[:5, 0] = (np.nan, -np.inf, 4e4, -32768.5, np.nan)
    g = _person(rng, (0, 0), 0.0)
    g[:5, 2] = (0.0, 0.0, 0.0, 0.0, 0.95)
    g[4, :2] = (110.03125 * sx, 90.5 * sy)
    boxes = [(10.2 * sx, 5.1 * sy, 58.7 * sx, 93.3 * sy), (118.4 * sx, 92.6 * sy, 72.3 * sx, 31.9 * sy),      # b's corners are swapped
             (np.nan, 50.0, 80.0, 96.0), (-30.0, 20.3 * sy, 8.4, 90.1 * sy), (w + 150.0, h + 180.0, w + 200.0, h + 250.0),
             (1e6, 2.0, 3.0, 4.0), (110.0 * sx, 90.0 * sy, 110.0 * sx, 90.0 * sy)]
    return _frame(_background(h, w, seed + 100), [a, b, c, d, e, f, g], boxes, seed=seed + 1)


def crowd(persons=300, seed=5):
    """64 x 64, `persons` persons with small heads: the first 256 in the left 28 columns, the others - records of the SECOND scan chunk -
    in the lower right corner, so that a kernel that stops after one chunk misses them."""
    rng = np.random.default_rng(seed)
    people, boxes = [], []
    for p in range(persons):
        at = rng.uniform((1, 1), (27, 63)) if p < CHUNK else rng.uniform((42, 42), (62, 62))
        people.append(_person(rng, at, 0.4))
        boxes.append((at[0] - 1, at[1] - 1, at[0] + 1, at[1] + 3))
    box = np.zeros((persons, 5), np.float32)
    box[:, :4] = boxes
    # rows in order: the keep list's order is the record order
    return {"img": _background(64, 64, 3), "kps": np.stack(people), "box": box, "keep": np.arange(persons, dtype=np.int32),
            "keep_count": np.array([persons], np.int32), "seg": np.array([0, persons], np.int32)}


def two_images():
    """Two images' persons in one set of buffers (seg = [0, 2, 5]): image 0 keeps two rows, image 1 keeps three."""
    rng = np.random.default_rng(21)
    h, w = 33, 64
    kps = np.stack([_person(rng, rng.uniform((4, 4), (60, 29)), 1.5) for _ in range(5)])
    x1, y1 = rng.uniform(0, 20, 5), rng.uniform(0, 10, 5)
    box = np.stack([x1, y1, x1 + rng.uniform(10, 40, 5), y1 + rng.uniform(10, 20, 5), rng.uniform(0, 1, 5)], 1).astype(np.float32)
    return {"img": _background(h, w, 6), "kps": kps, "box": box, "keep": np.array([1, 0, 4, 2, 3], np.int32),
            "keep_count": np.array([2, 3], np.int32), "seg": np.array([0, 2, 5], np.int32)}


def styles():
    return {"head_mosaic": redact_ref.Style(cell=8), "head_fill": redact_ref.Style(mode="fill", cell=8, fill=(7, 200, 91)),
            "person_mosaic": redact_ref.Style(region="person", cell=16), "person_fill": redact_ref.Style(region="person", mode="fill", cell=4, fill=(255, 0, 1))}


def kept_rows(scene, image=0):
    kps, box, _ = redact_ref.kept(scene["kps"], scene["box"], None, scene["keep"], scene["keep_count"], scene["seg"], image)
    return kps, box


def reference(scene, style, image=0):
    kps, box = kept_rows(scene, image)
    return redact_ref.redact(scene["img"], style, kps, box)


def style_struct(style):
    """The redact_ref.Style as the C ABI's sp_redact_style."""
    from simple_pose_amd import _lib
    st = _lib.RedactStyle()
    st.region, st.mode, st.cell = _lib.SP_REDACT_REGIONS[style.region], _lib.SP_REDACT_MODES[style.mode], style.cell
    st.expand, st.head_min, st.top_frac = style.expand, style.head_min, style.top_frac
    st.head_joints = len(style.head_joints)
    for i, j in enumerate(style.head_joints):
        st.head_joint[i] = j
    st.fallback = _lib.SP_REDACT_FALLBACKS[style.fallback]
    st.in_vis_thre = style.in_vis_thre
    st.fill[0], st.fill[1], st.fill[2] = style.fill
    return st
