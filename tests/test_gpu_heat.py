"""The heat overlay on the MI355X: sp_heat_overlay_u8c3 through the C ABI against tests/heat_ref.py, bit for bit, on the scenes of
tests/heat_scenes.py (seeded maps with NaNs, infinities and exact quotients; upright, clipped, rotated, magnified, shrunk, singular and
refused transforms; a random colour table).  The image, the source and the workspace sit between guard bytes that must come back
untouched.  Every case prints a MEASURED line with the number of differing pixels, which must be 0: there are no tolerances."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.visualize import HeatOverlay
from tests import heat_ref, heat_scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = _lib.ptr
GUARD = 4096
S = heat_ref.Style
CASES = {name: (scene, style, image) for name, scene, style, image in heat_scenes.cases()}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_heat(scene, style, image=0, in_place=False, rows=None, keep_count=None, keep=None, shift=0):
    """One sp_heat_overlay_u8c3 call on the scene's buffers -> the image on the host.  `shift`: bytes both images are moved off their
    4-byte alignment.  The destination (the source when in place) lies between guard bytes, checked after the call; out of place it
    starts as 0xA5 bytes, so a pixel the call does not write shows."""
    img = scene["img"]
    h, w = img.shape[:2]
    n = h * w * 3
    J, mh, mw = scene["hm"].shape[1:]
    rows = scene["hm"].shape[0] if rows is None else rows
    flat = torch.full((2, (n + 2 * GUARD + 8 + 15) // 16 * 16), 0xA5, dtype=torch.uint8, device=DEV)
    src = flat[0, GUARD + shift:GUARD + shift + n]
    src.copy_(_up(img.reshape(-1)))
    dst = src if in_place else flat[1, GUARD + shift:GUARD + shift + n]
    hm, ti, seg, lut = _up(scene["hm"]), _up(scene["trans_inv"]), _up(scene["seg"]), _up(scene["lut"])
    kp = _up(scene["keep"] if keep is None else np.asarray(keep, np.int32))
    kc = _up(scene["keep_count"] if keep_count is None else np.asarray(keep_count, np.int32))
    nbytes = ctypes.c_int64()
    st = heat_scenes.style_struct(style)
    _lib.check(_lib.lib().sp_heat_overlay_workspace_bytes(rows, mh, mw, ctypes.byref(nbytes)), "sp_heat_overlay_workspace_bytes")
    ws = torch.full((nbytes.value + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().sp_heat_overlay_u8c3(P(src), P(dst), h, w, P(hm), J, mh, mw, P(ti), P(kp), P(kc), P(seg), image, rows, ctypes.byref(st),
                                               P(lut), P(ws) + GUARD, _lib.current_stream(torch.device(DEV))), "sp_heat_overlay_u8c3")
    torch.cuda.synchronize()
    host, wsh = flat.cpu().numpy(), ws.cpu().numpy()
    row = 0 if in_place else 1
    assert (host[row, :GUARD + shift] == 0xA5).all() and (host[row, GUARD + shift + n:] == 0xA5).all(), "bytes outside the image were written"
    assert (wsh[:GUARD] == 0x5A).all() and (wsh[GUARD + nbytes.value:] == 0x5A).all(), "bytes outside the workspace were written"
    if not in_place:
        assert (host[0, GUARD + shift:GUARD + shift + n] == img.reshape(-1)).all(), "the source was written"
    return host[row, GUARD + shift:GUARD + shift + n].reshape(h, w, 3)


def _differs(got, want, name):
    bad = np.argwhere((got != want).any(axis=2))
    print(f"MEASURED {name}: {bad.shape[0]} of {got.shape[0] * got.shape[1]} pixels differ" + (f", first at (y, x) = {bad[0].tolist()}" if bad.size else ""))
    return bad.shape[0]


_REF = {}


def _want(key, scene, style, image=0):
    """The reference of a case, computed once."""
    if key not in _REF:
        _REF[key] = heat_scenes.reference(scene, style, image)
    return _REF[key]


@pytest.mark.parametrize("name", list(CASES))
def test_every_scene_equals_the_reference_bitwise_out_of_place_and_in_place(name):
    """97 x 131 (the byte path, ragged tiles), 96 x 128 (the 4-byte path; and shifted one byte off its alignment: the byte path at
    w % 4 == 0), 3 x 5; maps of 64 x 48 (16-byte loads), 6 x 5 (the scalar plane path) and 1 x 1; 17, 1 and 64 joints and masks of a few."""
    scene, style, image = CASES[name]
    want = _want(name, scene, style, image)
    assert (want != scene["img"]).any()
    assert _differs(device_heat(scene, style, image), want, name) == 0
    assert _differs(device_heat(scene, style, image, in_place=True), want, f"{name} in place") == 0
    if scene["img"].shape[1] % 4 == 0:
        assert _differs(device_heat(scene, style, image, shift=1), want, f"{name} unaligned") == 0
        assert _differs(device_heat(scene, style, image, shift=3, in_place=True), want, f"{name} unaligned in place") == 0


@pytest.mark.parametrize("alpha", ["constant", "value"])
def test_every_alpha_opacity_and_threshold(alpha):
    scene = CASES["street"][0]
    seen = set()
    for opacity16 in (0, 7, 16):
        for threshold in (1, 26, 255):
            style = S(alpha=alpha, opacity16=opacity16, threshold=threshold)
            want = _want(("grid", alpha, opacity16, threshold), scene, style)
            name = f"alpha {alpha} opacity16 {opacity16} threshold {threshold}"
            assert _differs(device_heat(scene, style), want, name) == 0
            assert _differs(device_heat(scene, style, in_place=True), want, name + " in place") == 0
            assert (want != scene["img"]).any() == (opacity16 > 0)
            seen.add(want.tobytes())
    assert len(seen) == 7                                                        # opacity 0 is one picture, the other six differ


def test_masks_and_scales_that_draw_nothing():
    scene = CASES["street"][0]
    for name, style in (("no joint below J", S(joint_mask=(1 << 17) | (1 << 40), threshold=1)), ("scale 0", S(scale=0.0, threshold=1)),
                        ("mask 0", S(joint_mask=0, threshold=1))):
        for in_place in (False, True):
            assert _differs(device_heat(scene, style, in_place=in_place), scene["img"], f"{name}, in place {in_place}") == 0


def test_counts_rows_bad_keep_entries_and_the_second_image():
    scene, style, _ = CASES["street"]
    rows = scene["hm"].shape[0]
    for in_place in (False, True):                                               # out of place the destination starts as 0xA5: the copy shows
        assert _differs(device_heat(scene, style, keep_count=[0], in_place=in_place), scene["img"], "keep_count 0") == 0
        assert _differs(device_heat(scene, style, keep_count=[-3], in_place=in_place), scene["img"], "keep_count -3") == 0
        assert _differs(device_heat(scene, style, rows=0, in_place=in_place), scene["img"], "rows 0") == 0
    # keep_count beyond rows: clamped to the rows, as the overlay clamps it.  Every keep entry is then read, the -1 entries of the spare
    # rows too, which are skipped: the picture is the picture of the true count
    want = _want("street", scene, style)
    assert _differs(device_heat(scene, style, keep_count=[rows + 5]), want, "keep_count beyond rows") == 0
    assert _differs(device_heat(scene, style, keep_count=[2 ** 31 - 1], in_place=True), want, "keep_count INT_MAX") == 0
    # keep entries outside 0 .. rows - 1 are skipped, the others still drawn
    keep = scene["keep"].copy()
    keep[0], keep[2] = rows, -7
    bad = dict(scene, keep=keep)
    want_bad = heat_scenes.reference(bad, style)
    assert (want_bad != want).any() and (want_bad != scene["img"]).any()
    assert _differs(device_heat(scene, style, keep=keep), want_bad, "keep rows out of range") == 0
    two = heat_scenes.two_images()
    first, second = heat_scenes.reference(two, style, 0), heat_scenes.reference(two, style, 1)
    assert (first != second).any()
    assert _differs(device_heat(two, style, image=1), second, "two images, image 1") == 0
    assert _differs(device_heat(two, style, image=0, in_place=True), first, "two images, image 0 in place") == 0
    # a frame of two images is drawn image by image, each from its own keep list: seg out of range draws nothing
    assert _differs(device_heat(dict(two, seg=np.array([0, 9, 5], np.int32)), style, image=1), two["img"], "seg beyond rows") == 0


def test_the_class_draws_every_row_with_its_own_tables():
    scene = CASES["street_wide"][0]
    img, hm, ti = scene["img"], scene["hm"], scene["trans_inv"]
    rows = list(range(hm.shape[0]))
    for kw in (dict(colormap="jet"), dict(colormap="hot", alpha="constant", opacity=1.0, threshold=0.3, joints=[0, 3, 16]),
               dict(colormap="gray", gain=0.5, threshold=0.0), dict(colormap=scene["lut"], opacity=0.25)):
        h = HeatOverlay(**kw)
        want = heat_ref.overlay(img, S(h.joint_mask, h.scale, h.threshold, h.opacity16, h.alpha), hm, ti, rows, h.lut)
        assert (want != img).any()
        got = h.overlay(img, _up(hm), _up(ti))
        assert got.is_cuda and got.dtype == torch.uint8
        assert _differs(got.cpu().numpy(), want, f"HeatOverlay {sorted(kw)}") == 0
        src = _up(img)
        assert h.overlay(src, _up(hm), _up(ti), out=src) is src and _differs(src.cpu().numpy(), want, "HeatOverlay in place") == 0
    assert torch.equal(HeatOverlay().overlay(img, _up(hm[:0]), _up(ti[:0])), _up(img))          # no rows: a copy
    with pytest.raises(TypeError, match="float32"):
        HeatOverlay().overlay(img, _up(hm).double(), _up(ti))
    with pytest.raises(ValueError, match="trans_inv"):
        HeatOverlay().overlay(img, _up(hm), _up(ti[:2]))
