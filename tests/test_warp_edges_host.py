"""CPU side of the crop warp's edge tests: the C oracle (pose_oracle.warp_affine_u8c3) against the closed forms and inside the derived bound
of the float64 bilinear reference on every case of tests/warp_edges.py - if it were outside, the derivation there would be wrong - and the
launchers' refusals by name, before any launch."""
import ctypes

import numpy as np
import pytest

from simple_pose_amd import _lib
from tests import warp_edges as we


@pytest.mark.parametrize("h,w", we.SOURCE_SIZES, ids=[f"src{h}x{w}" for h, w in we.SOURCE_SIZES])
def test_oracle_meets_closed_forms_and_the_derived_bound_on_every_case(h, w):
    kinds = set()
    for src in (we.hard_source(h, w), we.smooth_source(h, w)):
        for (oh, ow), n in zip(we.OUT_SIZES, we.COUNTS):
            for i, (kind, arg, fwd) in enumerate(we.cases(h, w, oh, ow, n)):
                we.expected(src, kind, arg, fwd, i % 3 == 1, oh, ow)          # asserts closed form and bound inside
                kinds.add(kind)
    assert kinds == set(we.CLOSED) | {"frac", "general"}


def test_the_bound_is_under_one_grey_level_on_smooth_sources_and_bites():
    for h, w in we.SOURCE_SIZES:
        s = we.smooth_source(h, w)
        gx, gy = we.gradients(s)
        assert gx <= 8 and gy <= 8 and we.bound(s) < 0.77, (h, w, gx, gy)
    s = we.smooth_source(37, 29)
    assert s.max() == 8 * 15 and s[0, 0, 0] == 8 and s[18, 14, 2] == 6 * 15
    # a reference half a pixel off is outside the bound: the bound can tell a wrong position from a right one
    fwd, off = we.fwd_of("general", (17.0, 0.7, 14.0, 18.0, 15.0, 16.0)), we.fwd_of("general", (17.0, 0.7, 14.5, 18.0, 15.0, 16.0))
    got = we.expected(s, "general", None, fwd, False, 33, 31)
    assert np.abs(got - we.bilinear_f64(s, off, 33, 31)).max() > we.bound(s)


def test_closed_forms_say_what_their_names_say():
    s = we.hard_source(37, 29)
    ident = we.expected(s, "shift", (0, 0), we.fwd_of("shift", (0, 0)), False, 33, 31)
    assert np.array_equal(ident[:, :29], s[:33]) and not ident[:, 29:].any()          # the top left of the source, zeros beyond it
    flipped = we.expected(s, "shift", (0, 0), we.fwd_of("shift", (0, 0)), True, 33, 31)
    assert np.array_equal(flipped[:, :29], np.fliplr(s)[:33])
    col = we.expected(s, "shift", (1, 1), we.fwd_of("shift", (1, 1)), False, 5, 7)
    assert not col[0].any() and not col[:, 0].any() and np.array_equal(col[1:, 1:], s[:4, :6])      # row / column -1: no tap counts
    half = we.expected(s, "half_x", -0.5, we.fwd_of("half_x", -0.5), False, 5, 7)
    assert np.array_equal(half[:, 0], (s[:5, 0].astype(int) + 1) >> 1)                # between column -1 and 0: one tap inside
    assert not we.expected(s, "shift", (100000, 0), we.fwd_of("shift", (100000, 0)), False, 5, 7).any()
    one = we.hard_source(1, 1)
    assert (we.expected(one, "degenerate", None, we.fwd_of("degenerate", None), False, 5, 7) == one[0, 0]).all()
    for k, a in we.base_maps(37, 29, 5, 7):                                           # the closed forms' inverses are exact in binary
        if k in we.CLOSED and k != "degenerate":
            inv = we.invert_affine(we.fwd_of(k, a))
            assert np.array_equal(inv * 1024, np.round(inv * 1024)), (k, a, inv)


def test_warp_refusals_are_by_name_and_launch_nothing():
    """A source 32768 wide, capacity 0 and 2049, batch 0 and a null pointer per launcher: each returns SP_EINVAL with its own name in the
    message.  The non-null pointers are not device memory; every call returns before a launch."""
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    m = (ctypes.c_double * 6)(1, 0, 0, 0, 1, 0)
    mp = ctypes.cast(m, ctypes.c_void_p)

    def refused(rc, *words):
        msg = lib.sp_last_error()
        assert rc == -1 and all(wd in msg for wd in words), (rc, msg, words)

    refused(lib.sp_warp_affine_u8c3(one, 8, 32768, mp, 1, one, 4, 4, None), b"sp_warp_affine_u8c3", b"8x32768")
    refused(lib.sp_warp_affine_u8c3(one, 32768, 8, mp, 1, one, 4, 4, None), b"sp_warp_affine_u8c3", b"32768x8")
    refused(lib.sp_warp_affine_u8c3(one, 8, 8, mp, 0, one, 4, 4, None), b"sp_warp_affine_u8c3", b"crops=0")
    for args in ((None, 8, 8, mp, 1, one), (one, 8, 8, None, 1, one), (one, 8, 8, mp, 1, None)):
        refused(lib.sp_warp_affine_u8c3(*args, 4, 4, None), b"sp_warp_affine_u8c3", b"null")

    plan = lambda src=one, batch=1, w=8, m_inv=one, idx=one, seg=one, cap=5, dst=one: \
        lib.sp_warp_affine_plan_u8c3(src, batch, 8, w, m_inv, idx, seg, cap, dst, 4, 4, None)
    refused(plan(w=32768), b"sp_warp_affine_plan_u8c3", b"8x32768")
    refused(plan(batch=0), b"sp_warp_affine_plan_u8c3", b"batch=0")
    refused(plan(cap=0), b"sp_warp_affine_plan_u8c3", b"capacity 0")
    refused(plan(cap=2049), b"sp_warp_affine_plan_u8c3", b"capacity 2049")
    for kw in ("src", "m_inv", "idx", "seg", "dst"):
        refused(plan(**{kw: None}), b"sp_warp_affine_plan_u8c3", b"null")

    images = lambda table=one, batch=1, m_inv=one, idx=one, seg=one, cap=5, dst=one: \
        lib.sp_warp_affine_plan_images_u8c3(table, batch, m_inv, idx, seg, cap, dst, 4, 4, None)
    refused(images(batch=0), b"sp_warp_affine_plan_images_u8c3", b"batch=0")
    refused(images(cap=0), b"sp_warp_affine_plan_images_u8c3", b"capacity 0")
    refused(images(cap=2049), b"sp_warp_affine_plan_images_u8c3", b"capacity 2049")
    for kw in ("table", "m_inv", "idx", "seg", "dst"):
        refused(images(**{kw: None}), b"sp_warp_affine_plan_images_u8c3", b"null")

    srcs = (ctypes.c_void_p * 2)(16, 16)
    hw = (ctypes.c_int * 4)(8, 8, 8, 32768)
    ok_hw = (ctypes.c_int * 4)(8, 8, 8, 8)
    mm = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0)
    mean = (ctypes.c_float * 3)(*we.MEAN)
    V = lambda a: ctypes.cast(a, ctypes.c_void_p)
    batch = lambda s=V(srcs), sizes=V(hw), maps=V(mm), n=2, mean_=mean, out=one: \
        lib.sp_warp_affine_batch_u8c3_to_nchw_f32(s, sizes, None, maps, n, 4, 4, mean_, out, None, None)
    refused(batch(), b"sp_warp_affine_batch_u8c3_to_nchw_f32", b"sample 1", b"8x32768")
    refused(batch(sizes=V(ok_hw), n=0), b"sp_warp_affine_batch_u8c3_to_nchw_f32", b"batch=0")
    null_src = (ctypes.c_void_p * 2)(16, None)
    refused(batch(s=V(null_src), sizes=V(ok_hw)), b"sp_warp_affine_batch_u8c3_to_nchw_f32", b"sample 1", b"null")
    for kw in ("s", "sizes", "maps", "mean_", "out"):
        refused(batch(**{kw: None, **({} if kw == "sizes" else {"sizes": V(ok_hw)})}), b"sp_warp_affine_batch_u8c3_to_nchw_f32", b"null")
