"""The text scenes shared by tests/test_label_core_cpu.py (the CPU program) and tests/test_gpu_labels.py (the kernels): the frame's buffers
as sp_oks_nms / sp_track_associate leave them, seeded.  A scene is a dict: img uint8 [h, w, 3], box float32 [rows, 5], score float64 [rows],
track_id int32 [rows], keep int32 [rows], keep_count int32 [B], seg int32 [B + 1].  A case adds the style, the image index, the caption
array (uint8 [B, 64] or None) and the overrides of one call."""
import numpy as np

from tests import label_ref

CHUNK = 256                    # labels.hip's scan step
LIST = 512                     # labels.hip's LBL_LIST: record indices a tile collects before it applies them
TILE_W, TILE_H = 64, 16
T_FULL = b"#\x01 \x02 \x03"    # "#{id} {score} {conf}"
T_SHORT = b"#\x01 \x02"


def _background(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _frame(img, boxes, scores, ids, spare_rows=2, seed=0):
    """The persons (pick order) scattered over rows + spare rows of one image; the keep list names them in pick order."""
    rng = np.random.default_rng(seed)
    n = len(boxes)
    rows = n + spare_rows
    where = rng.permutation(rows)[:n]
    box = rng.uniform(0, 40, (rows, 5)).astype(np.float32)
    score = rng.uniform(0, 1, rows)
    tid = rng.integers(1, 90, rows).astype(np.int32)
    keep = np.full(rows, -1, np.int32)
    for p in range(n):
        box[where[p]], score[where[p]], tid[where[p]] = boxes[p], scores[p], ids[p]
    keep[:n] = where
    return {"img": img, "box": box, "score": score, "track_id": tid, "keep": keep, "keep_count": np.array([n], np.int32),
            "seg": np.array([0, rows], np.int32)}


def edges(h, w, seed=1):
    """Fourteen persons (x1, y1, x2, y2, conf | score | id): labels across the 64-pixel and the 16-row tile seams, at the top edge (the label
    flips inside), at the right edge (it shifts left), boxes wholly outside each edge, corners that are not finite or beyond q's range, the
    ids 1, 23, 2147483647, 0, -5 and every score the number format treats differently."""
    inf, nan = np.inf, np.nan
    persons = [
        ((50.3, 21.4, 80.0, 50.0, 0.5), 0.0, 1),                      # y0 = 12: rows 12 .. 20 cross the seam at 16, columns cross 64
        ((10.0, 3.2, 40.0, 30.0, 0.25), 0.004999, 23),                # top edge: the label goes inside the box
        ((w - 7.5, 40.9, w + 20.0, 60.0, 0.995), 0.995, 2147483647),  # right edge: shifted left
        ((-200.0, 30.0, -150.0, 50.0, 1.0), 1.0, 0),                  # wholly left: x0 = 0
        ((w + 300.0, 45.0, w + 400.0, 70.0, 12.345), 12.345, -5),     # wholly right: x0 = w - width
        ((20.0, -50.0, 40.0, -30.0, 0.9), 1e9, 5),                    # wholly above: nothing of the plate is left
        ((20.0, h + 100.0, 40.0, h + 150.0, 0.9), 0.5, 6),            # wholly below
        ((nan, 20.0, 30.0, 40.0, 0.9), 0.5, 7),                       # no label
        ((20.0, inf, 30.0, 40.0, 0.9), 0.5, 8),
        ((1e6, 20.0, 30.0, 40.0, 0.9), 0.5, 9),                       # |v| > 32768
        ((5.0, 58.0, 30.0, 60.0, -0.1), -0.1, 10),                    # negative: "?"
        ((30.0, 35.5, 60.0, 60.0, nan), nan, 11),
        ((2.0, 47.0, 20.0, 60.0, inf), inf, 12),
        ((63.96875, 31.96875, 90.0, 60.0, 99.994), 99.996, 13),       # a tie of the quantisation on a tile corner; the clamp at 99.99
    ]
    return _frame(_background(h, w, seed), [p[0] for p in persons], [p[1] for p in persons], [p[2] for p in persons], seed=2)


def crowd(persons=260, seed=5):
    """128 x 64, `persons` kept rows, short labels all over the image: more records than one scan chunk."""
    rng = np.random.default_rng(seed)
    h, w = 64, 128
    boxes = [(rng.uniform(-10, w), rng.uniform(-5, h), w, h, rng.uniform(0, 1)) for _ in range(persons)]
    return _frame(_background(h, w, 3), boxes, rng.uniform(0, 1, persons).tolist(), list(range(1, persons + 1)), spare_rows=0, seed=4)


def crowd_one_tile(persons=600, seed=13):
    """128 x 64, `persons` kept rows, the first corner of every box inside the tile x 0 .. 63, y 16 .. 31: a label sits above its corner, so
    nearly all plates meet that one tile, more than its list holds (`cases` asserts it), and the tile applies its list before the scan ends."""
    rng = np.random.default_rng(seed)
    h, w = 64, 128
    boxes = [(rng.uniform(0, TILE_W - 1), rng.uniform(TILE_H, 2 * TILE_H - 1), w, h, rng.uniform(0, 1)) for _ in range(persons)]
    assert all(0 <= b[0] < TILE_W and TILE_H <= b[1] < 2 * TILE_H for b in boxes)
    return _frame(_background(h, w, 12), boxes, rng.uniform(0, 1, persons).tolist(), list(range(1, persons + 1)), spare_rows=0, seed=14)


def two_images():
    """Two images' persons in one set of buffers (seg = [0, 2, 5]): image 0 keeps two rows, image 1 keeps three."""
    rng = np.random.default_rng(21)
    h, w = 33, 64
    x1, y1 = rng.uniform(0, 40, 5), rng.uniform(0, 30, 5)
    box = np.stack([x1, y1, x1 + 10, y1 + 10, rng.uniform(0, 1, 5)], 1).astype(np.float32)
    return {"img": _background(h, w, 6), "box": box, "score": rng.uniform(0, 2, 5), "track_id": np.array([3, 1, 4, 1, 5], np.int32),
            "keep": np.array([1, 0, 4, 2, 3], np.int32), "keep_count": np.array([2, 3], np.int32), "seg": np.array([0, 2, 5], np.int32)}


def overlap():
    """Two labels on the same spot at half opacity: the pick order shows."""
    return _frame(_background(40, 72, 8), [(20.0, 20.0, 60.0, 39.0, 0.8), (23.0, 23.0, 60.0, 39.0, 0.7)], [0.9, 0.8], [3, 12], seed=9)


def captions(texts):
    """uint8 [B, 64]: every text NUL-padded (64 bytes: no NUL at all)."""
    out = np.zeros((len(texts), 64), np.uint8)
    for i, t in enumerate(texts):
        assert len(t) <= 64
        out[i, :len(t)] = list(t)
    return out


def cases():
    S = label_ref.Style
    out = []

    def add(name, scene, style, image=0, with_ids=True, caption=None, rows=None, keep_count=None, shift=0, draws=True):
        out.append(dict(name=name, scene=scene, style=style, image=image, with_ids=with_ids, caption=caption, rows=rows,
                        keep_count=None if keep_count is None else np.asarray(keep_count, np.int32), shift=shift, draws=draws))

    small, wide = edges(61, 97), edges(64, 128)
    cap1 = captions([b"cam \x05: \x04 persons"])
    add("bytes_ids", small, S(T_FULL), caption=cap1)
    add("bytes_no_ids_half", small, S(T_FULL, label_opacity=8), with_ids=False)
    add("bytes_opacity0", small, S(T_FULL, label_opacity=0, caption_opacity=0), caption=cap1, draws=False)
    add("bytes_scale8_24chars", small, S(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", label_scale=8))
    add("bytes_scale3", small, S(T_SHORT, label_scale=3, caption_scale=2, caption_corner="br"), caption=cap1)
    add("wide_ids", wide, S(T_FULL, label_scale=2), caption=cap1)
    add("wide_unaligned", wide, S(T_FULL, label_scale=2), caption=cap1, shift=1)
    add("wide_scale8", wide, S(T_SHORT, label_scale=8, label_opacity=8))
    add("overlap", overlap(), S(T_SHORT, label_opacity=8))
    big = crowd(260)
    capn = captions([b"n=\x04"])
    add("crowd260", big, S(b"\x01"), caption=capn)
    add("crowd_count_above_rows", big, S(b"\x01"), caption=capn, keep_count=[300])
    add("crowd_count7", big, S(b"\x01"), caption=capn, keep_count=[7])
    add("crowd_count0", big, S(b"\x01"), caption=capn, keep_count=[0])
    add("rows0_caption", big, S(b"\x01"), caption=capn, rows=0)
    add("rows0", big, S(b"\x01"), rows=0, draws=False)
    add("crowd600_one_tile", crowd_one_tile(600), S(b"\x01", label_opacity=8))           # half opacity: the order of the plates shows
    most = int(tile_hits(plate_rects(out[-1]), 64, 128).max())
    assert most > LIST, f"crowd600_one_tile: {most} plates in the fullest tile, the list holds {LIST}"
    two = two_images()
    cap2 = captions([b"first \x05", b"cam \x05: \x04"])
    add("two_images_1", two, S(T_SHORT, caption_corner="bl"), image=1, caption=cap2)
    add("two_images_0", two, S(T_SHORT, caption_corner="tr"), image=0, caption=cap2, with_ids=False)
    full = captions([bytes(range(0x30, 0x70))])                              # 64 bytes, no NUL
    odd = captions([b"a\x80b\x01c\x7f\x04"])                                 # 0x80, a label field and DEL print '?'
    for corner in ("tl", "tr", "bl", "br"):
        add(f"caption_{corner}", small, S(b"", caption_corner=corner, caption_scale=2), caption=odd)
        add(f"caption64_{corner}", wide, S(b"", caption_corner=corner, caption_opacity=16), caption=full)
    add("no_caption_no_labels", small, S(b""), draws=False)
    return out


def reference(case):
    sc = case["scene"]
    box, score, tid, n = label_ref.kept(sc, case["image"], case["with_ids"], case["rows"], case["keep_count"])
    if case["rows"] == 0:
        box, score, tid = box[:0], score[:0], None if tid is None else tid[:0]
    cap = None if case["caption"] is None else case["caption"][case["image"]]
    return label_ref.render(sc["img"], case["style"], box, score, tid, n, case["image"], cap)


def plate_rects(case):
    """The plates label_ref pastes for the case, as it places and sizes them: (x0, y0, x1, y1), inclusive, clipped to the image."""
    h, w = case["scene"]["img"].shape[:2]
    rects, paste = [], label_ref.paste

    def record(img, text, s, x0, y0, *colours):
        if text:
            ph, pw = label_ref.plate_bitmap(text, s).shape
            r = (max(x0, 0), max(y0, 0), min(x0 + pw, w) - 1, min(y0 + ph, h) - 1)
            if r[0] <= r[2] and r[1] <= r[3]:
                rects.append(r)
        paste(img, text, s, x0, y0, *colours)

    label_ref.paste = record
    try:
        reference(case)
    finally:
        label_ref.paste = paste
    return rects


def tile_hits(rects, h, w):
    """int [tiles down, tiles across]: how many of the rectangles meet each 64 x 16 tile."""
    hits = np.zeros(((h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W), np.int64)
    for x0, y0, x1, y1 in rects:
        hits[y0 // TILE_H:y1 // TILE_H + 1, x0 // TILE_W:x1 // TILE_W + 1] += 1
    return hits


def style_struct(style):
    """The label_ref.Style as the C ABI's sp_label_style."""
    from simple_pose_amd import _lib
    st = _lib.LabelStyle()
    st.template_len = len(style.template)
    for i, c in enumerate(style.template):
        st.label_template[i] = c
    st.label_scale, st.label_opacity = style.label_scale, style.label_opacity
    st.caption_scale, st.caption_opacity = style.caption_scale, style.caption_opacity
    st.caption_corner = _lib.SP_LABEL_CORNERS[style.caption_corner]
    st.palette_n = style.palette.shape[0]
    for i, c in enumerate(style.palette.tolist()):
        st.palette[i][0], st.palette[i][1], st.palette[i][2] = c
    return st
