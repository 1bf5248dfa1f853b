"""TEST HELPER: restatements for the YOLOv5 detector (never imported by the package).

* letterbox_np: ScalePadding.make_border's cv.resize(INTER_LINEAR) + cv.copyMakeBorder on uint8 BGR, restating OpenCV's 8-bit arithmetic as
  csrc/detect.hip documents it (11-bit fixed-point coefficients, INTER_AREA's 2x2 mean for an exact 2x downscale).  OpenCV itself is not
  installed here, so this restatement is not pinned against it (DESIGN: parity unpinned).  tools/gen_golden_detector.py plugs these into
  its cv2 stub.
* nms_np: detector/yolov5_detector.py:non_max_suppression with torchvision.ops.nms written out (greedy, descending score, ties to the lower
  index), in float32 numpy.
* yolov5_forward_torch: YOLOv5.forward (eval) from a state_dict in plain torch functional ops.
* run_yolo_program_cpu: interprets an engine.yolov5_program (source="nchw") on the CPU, wrapping desc_interp.conv_desc_cpu.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn.functional as F

from simple_pose_amd._lib import SP_CONV_HARDSWISH, SP_CONV_OUT_SLICE
from tests.desc_interp import conv_desc_cpu


# ---- letterbox --------------------------------------------------------------------------------------------------------------------------
def _coefs(dsize, ssize):
    scale = 1.0 / (dsize / ssize)
    d = np.arange(dsize)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    hi = s >= ssize - 1
    f[hi], s[hi] = 0, ssize - 1
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, ssize - 1), a0, a1


def resize_np(img, new_w, new_h):
    """cv.resize(img, (new_w, new_h), interpolation=INTER_LINEAR) for uint8 [h, w, 3], restated (see module doc)."""
    h, w = img.shape[:2]
    if (new_w, new_h) == (w, h):
        return img.copy()
    src = img.astype(np.int64)
    if w == 2 * new_w and h == 2 * new_h:
        s = src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2]
        return ((s + 2) >> 2).astype(np.uint8)
    x0, x1, ax0, ax1 = _coefs(new_w, w)
    y0, y1, by0, by1 = _coefs(new_h, h)
    rows = src[:, x0] * ax0[None, :, None] + src[:, x1] * ax1[None, :, None]          # [h, new_w, 3]
    v = (rows[y0] * by0[:, None, None] + rows[y1] * by1[:, None, None] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def copy_make_border_np(img, top, bottom, left, right, value=(114, 114, 114)):
    h, w = img.shape[:2]
    out = np.empty((h + top + bottom, w + left + right, 3), dtype=np.uint8)
    out[...] = np.asarray(value, dtype=np.uint8)
    out[top:top + h, left:left + w] = img
    return out


def letterbox_np(img, geo):
    """The canvas of ScalePadding.make_border for the geometry of yolov5_detector.ScalePadding.geometry."""
    r = resize_np(img, geo["new_w"], geo["new_h"])
    return copy_make_border_np(r, geo["top"], geo["bottom"], geo["left"], geo["right"])


def focus_np(canvas):
    """uint8 BGR canvas [H, W, 3] -> the Focus input NHWC [H/2, W/2, 12] (RGB / 255, torch.cat order of Focus.forward)."""
    x = canvas[:, :, ::-1].astype(np.float32) / np.float32(255.0)
    return np.concatenate([x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]], axis=-1)


# ---- NMS --------------------------------------------------------------------------------------------------------------------------------
def _iou_f32(a, b):
    """IoU of box a [4] against boxes b [n, 4], float32, torchvision's / box_iou's operation order."""
    f = np.float32
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), f(0))
    h = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), f(0))
    inter = w * h
    return (inter / (area_a + area_b - inter)).astype(np.float32)


def greedy_nms_np(boxes, scores, thr, limit=None):
    """torchvision.ops.nms: indices kept, descending score (ties: lower index first); `limit`: stop after that many kept (the same prefix)."""
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))
    keep = []
    for i in order:
        if keep and (_iou_f32(boxes[i], boxes[np.asarray(keep)]) > np.float32(thr)).any():
            continue
        keep.append(int(i))
        if limit is not None and len(keep) >= limit:
            break
    return np.asarray(keep, dtype=np.int64)


def nms_np(pred, conf_thresh=0.1, iou_thresh=0.6, merge=False, agnostic=False, multi_label=True, max_det=300, return_candidates=False):
    """non_max_suppression (yolov5_detector.py:52-128) on float32 numpy [B, N, no]: list of None or [n, 6]."""
    f = np.float32
    out, cands = [], []
    for x in pred.astype(np.float32):
        x = x[x[:, 4] > f(conf_thresh)].copy()
        if not x.shape[0]:
            out.append(None); cands.append(None)
            continue
        x[:, 5:] *= x[:, 4:5]
        box = np.stack([x[:, 0] - x[:, 2] / f(2), x[:, 1] - x[:, 3] / f(2), x[:, 0] + x[:, 2] / f(2), x[:, 1] + x[:, 3] / f(2)], 1)
        if multi_label:
            i, j = np.nonzero(x[:, 5:] > f(conf_thresh))
            x = np.concatenate([box[i], x[i, j + 5, None], j[:, None].astype(np.float32)], 1)
        else:
            j = np.argmax(x[:, 5:], 1)
            conf = x[np.arange(len(x)), 5 + j]
            x = np.concatenate([box, conf[:, None], j[:, None].astype(np.float32)], 1)[conf > f(conf_thresh)]
        n = x.shape[0]
        if not n:
            out.append(None); cands.append(None)
            continue
        c = x[:, 5:6] * f(0 if agnostic else 4096)
        boxes, scores = x[:, :4] + c, x[:, 4]
        i = greedy_nms_np(boxes, scores, iou_thresh, limit=max_det)
        if merge and (1 < n < 3E3):
            iou = np.stack([_iou_f32(boxes[k], boxes) for k in i]) > f(iou_thresh)
            weights = iou * scores[None]
            x[i, :4] = (weights.astype(np.float64) @ x[:, :4].astype(np.float64)).astype(np.float32) / weights.sum(1, keepdims=True)
            i = i[iou.sum(1) > 1]
        out.append(x[i]); cands.append((boxes, scores))
    return (out, cands) if return_candidates else out


def nms_trace_np(boxes, scores, thr, limit=None):
    """greedy_nms_np with its bookkeeping: (keep, order, suppressed) - `order` the candidate indices by rank, `suppressed` a list of
    (rank of the suppressed candidate, rank of the FIRST kept box that suppresses it).  The scan stops like greedy_nms_np's at `limit` kept."""
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))
    keep, keep_rank, suppressed = [], [], []
    for rank, i in enumerate(order):
        hit = np.nonzero(_iou_f32(boxes[i], boxes[np.asarray(keep, dtype=np.int64)]) > np.float32(thr))[0] if keep else []
        if len(hit):
            suppressed.append((rank, keep_rank[hit[0]]))
            continue
        keep.append(int(i)); keep_rank.append(rank)
        if limit is not None and len(keep) >= limit:
            break
    return np.asarray(keep, dtype=np.int64), order, suppressed


# ---- head decode ------------------------------------------------------------------------------------------------------------------------
def head_decode_torch(heads, anchors, no, a_stride, strides, anchor_wh, dtype=torch.float64):
    """YOLOv5Head.forward's eval branch (yolov5.py:134-149) on the packed head outputs, evaluated in `dtype`: heads[l] is NHWC
    [B, ny, nx, anchors * a_stride] with anchor a's `no` values at [a * a_stride, a * a_stride + no) (the columns between are never read);
    anchor_wh [3][anchors][2].  Returns [B, N, no], rows ordered (level, anchor, y, x)."""
    ag = torch.as_tensor(anchor_wh, dtype=dtype).view(3, anchors, 2)
    z = []
    for l, t in enumerate(heads):
        B, ny, nx, _ = t.shape
        v = t.to(dtype).view(B, ny, nx, anchors, a_stride)[..., :no].permute(0, 3, 1, 2, 4).sigmoid()
        yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
        g = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).to(dtype)
        xy = (v[..., 0:2] * 2. - 0.5 + g) * torch.as_tensor(strides[l], dtype=dtype)
        wh = (v[..., 2:4] * 2) ** 2 * ag[l].view(1, anchors, 1, 1, 2)
        z.append(torch.cat([xy, wh, v[..., 4:]], -1).reshape(B, -1, no))
    return torch.cat(z, 1)


# ---- torch forward of the reference network ---------------------------------------------------------------------------------------------
def yolov5_forward_torch(sd, x, num_cls=80, strides=(8., 16., 32.)):
    """YOLOv5.forward (eval) in plain torch on `sd` (reference keys), fp32 NCHW RGB input -> [B, N, num_cls + 5]."""
    def bn(p, t):
        return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    def cbr(p, t, s=1):
        w = sd[p + ".conv.weight"]
        return F.hardswish(bn(p + ".bn", F.conv2d(t, w, stride=s, padding=(w.shape[-1] - 1) // 2)))

    def csp(p, t, shortcut):
        y = cbr(p + ".conv1_0", t)
        i = 0
        while f"{p}.conv1_s.{i}.conv1.conv.weight" in sd:
            q = f"{p}.conv1_s.{i}"
            u = cbr(q + ".conv2", cbr(q + ".conv1", y))
            y = y + u if shortcut else u
            i += 1
        y1 = F.conv2d(y, sd[p + ".conv1_n.weight"])
        y2 = F.conv2d(t, sd[p + ".conv2_0.weight"])
        return cbr(p + ".conv3", F.hardswish(bn(p + ".bn", torch.cat([y1, y2], 1))))

    def spp(p, t):
        t = cbr(p + ".conv1", t)
        return cbr(p + ".conv2", torch.cat([t] + [F.max_pool2d(t, k, 1, k // 2) for k in (5, 9, 13)], 1))

    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    bb = "backbones"
    t = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)
    t = cbr(bb + ".stem.conv", t)
    t = csp(bb + ".layer1.1", cbr(bb + ".layer1.0", t, 2), True)
    c3 = csp(bb + ".layer2.1", cbr(bb + ".layer2.0", t, 2), True)
    c4 = csp(bb + ".layer3.1", cbr(bb + ".layer3.0", c3, 2), True)
    c5 = csp(bb + ".layer4.2", spp(bb + ".layer4.1", cbr(bb + ".layer4.0", c4, 2)), False)
    l5 = cbr("neck.latent_c5", c5)
    f4 = csp("neck.c4_fuse", torch.cat([up(l5), c4], 1), False)
    l4 = cbr("neck.latent_c4", f4)
    p3 = csp("neck.c3_out", torch.cat([up(l4), c3], 1), False)
    p4 = csp("neck.c4_out", torch.cat([cbr("neck.c3_c4", p3, 2), l4], 1), False)
    p5 = csp("neck.c5_out", torch.cat([cbr("neck.c4_c5", p4, 2), l5], 1), False)
    ag = sd["head.anchor_grid"].reshape(3, -1, 2)
    A, no = ag.shape[1], num_cls + 5
    z = []
    for i, t in enumerate((p3, p4, p5)):
        y = F.conv2d(t, sd[f"head.heads.{i}.weight"], sd[f"head.heads.{i}.bias"])
        bs, _, ny, nx = y.shape
        y = y.view(bs, A, no, ny, nx).permute(0, 1, 3, 4, 2).sigmoid()
        yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
        grid = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).float()
        xy = (y[..., 0:2] * 2. - 0.5 + grid) * strides[i]
        wh = (y[..., 2:4] * 2) ** 2 * ag[i].view(1, A, 1, 1, 2)
        z.append(torch.cat([xy, wh, y[..., 4:]], -1).reshape(bs, -1, no))
    return torch.cat(z, 1)


# ---- CPU interpreter of a yolov5_program ------------------------------------------------------------------------------------------------
def _hardswish(t):
    return t * torch.clamp(t + 3, 0, 6) / 6


def run_yolo_program_cpu(prog, x):
    """x: fp32 NCHW [B, 3, H, W] (a source="nchw" program) -> prog's `pred` [B, N, no] (every launch as include/simple_pose_hip.h documents it)."""
    B = x.shape[0]
    bufs = {}
    for op in prog.ops:
        for nm in op.writes():
            if nm not in bufs and nm != prog.out_name:
                bufs[nm] = torch.full((B,) + tuple(prog.shapes[nm]), float("nan"))
        if op.kind == "focus_nchw":
            bufs[op.dst] = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1).permute(0, 2, 3, 1).contiguous()
        elif op.kind == "conv":
            d = op.desc
            d.batch = B
            if d.flags & (SP_CONV_HARDSWISH | SP_CONV_OUT_SLICE):
                dd = copy.copy(d)
                dd.flags = d.flags & ~(SP_CONV_HARDSWISH | SP_CONV_OUT_SLICE)
                dd.out_c = d.c_out
                t = torch.full((B, d.out_h, d.out_w, d.c_out), float("nan"))
                conv_desc_cpu(dd, bufs[op.src], op.w, op.scale, op.shift, None, t, B)
                if d.flags & SP_CONV_HARDSWISH:
                    t = _hardswish(t)
                if op.res:
                    t = t + bufs[op.res]
                bufs[op.dst][..., op.c0:op.c0 + d.c_out] = t
            else:
                y = torch.full((B, d.out_h, d.out_w, d.out_c), float("nan"))
                conv_desc_cpu(d, bufs[op.src], op.w, op.scale, op.shift, bufs[op.res] if op.res else None, y, B)
                bufs[op.dst] = y
        elif op.kind == "spp":
            h, w, c, ct = op.args
            t = bufs[op.dst][..., :c].permute(0, 3, 1, 2)
            for i, k in enumerate((5, 9, 13)):
                bufs[op.dst][..., (i + 1) * c:(i + 2) * c] = F.max_pool2d(t, k, 1, k // 2).permute(0, 2, 3, 1)
        elif op.kind == "upsample_slice":
            h, w, c, s_ct, s0, d_ct = op.args
            t = bufs[op.src][..., s0:s0 + c]
            bufs[op.dst][..., op.c0:op.c0 + c] = t.repeat_interleave(2, 1).repeat_interleave(2, 2)
        elif op.kind == "yolo_decode":
            h1, h2, grid, A, no, a_stride, strides, anchors = op.args
            ag = torch.tensor(anchors).view(3, A, 2)
            z = []
            for l, nm in enumerate((op.src, h1, h2)):
                ny, nx = grid[2 * l], grid[2 * l + 1]
                v = bufs[nm].view(B, ny, nx, A, a_stride)[..., :no].permute(0, 3, 1, 2, 4).sigmoid()
                yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
                g = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).float()
                xy = (v[..., 0:2] * 2. - 0.5 + g) * strides[l]
                wh = (v[..., 2:4] * 2) ** 2 * ag[l].view(1, A, 1, 1, 2)
                z.append(torch.cat([xy, wh, v[..., 4:]], -1).reshape(B, -1, no))
            bufs[op.dst] = torch.cat(z, 1)
        else:
            raise ValueError(op.kind)
    return bufs[prog.out_name]


# ---- weights -------------------------------------------------------------------------------------------------------------------------------
HEAD_GAIN = 8.0     # conditioned head weights give near-constant logits; x8 spreads the scores so that NMS has real work to do


def detector_state_dict(model, seed: int):
    """The fixture's weights for a YOLOv5 module (reference or ours: same keys): synth.conditioned_state_dict of every parameter / BN
    buffer, the head convs' weights x HEAD_GAIN, the anchor buffers the module's own."""
    from simple_pose_amd import synth
    sd0 = model.state_dict()
    shapes = [(k, tuple(v.shape), str(v.dtype)) for k, v in sd0.items() if k not in ("head.anchor_grid", "head.normalize_anchors")]
    sd = {k: torch.from_numpy(v) for k, v in synth.conditioned_state_dict(shapes, seed).items()}
    for i in range(3):
        sd[f"head.heads.{i}.weight"] = sd[f"head.heads.{i}.weight"] * np.float32(HEAD_GAIN)
    sd["head.anchor_grid"], sd["head.normalize_anchors"] = sd0["head.anchor_grid"].clone(), sd0["head.normalize_anchors"].clone()
    return sd
