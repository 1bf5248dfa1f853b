"""The single-stage form of the fp32 implicit GEMM (conv_igemm_single_kernel / conv_igemm_tapskip_single_kernel, csrc/conv_igemm.hip), host side
(no GPU): which launches the launcher hands to it (sp_conv2d_single_stage against the rule stated in include/simple_pose_hip.h), the LDS bytes
of its launch, and that the knob moves no string of sp_conv2d_kernel_name."""
import ctypes

import pytest

from simple_pose_amd import _lib, conv_geometry

IGEMM = _lib.SP_CONV_KERNEL_IGEMM


@pytest.fixture(autouse=True)
def _knobs_back_on():
    yield
    _lib.lib().sp_conv_set_single_stage(1)
    _lib.lib().sp_conv_set_tap_skip(1)


def _conv(c_in, c_out, k=1, *, h=8, w=6, stride=1, batch=128, tile=(128, 128), flags=0, k_pad=None, panel=0, kernel=IGEMM):
    n_pad = conv_geometry.n_pad_for(c_out)
    bke = 64 if flags & _lib.SP_CONV_BF16 else 32
    k_pad = k_pad or conv_geometry.round_up(k * k * (panel or c_in), bke)
    d = conv_geometry.conv_fwd(h, w, c_in, c_out, n_pad, k, k, k, k, k_pad, stride, k // 2, flags, panel=panel)
    d.batch, d.kernel = batch, kernel
    if not panel:
        d.tile_m, d.tile_n = tile
    return d


def _deconv(c_in, c_out, tile=(128, 128), batch=128):
    d = conv_geometry.deconv_k4s2p1_fwd(4, 3, c_in, c_out, conv_geometry.n_pad_for(c_out))
    d.batch, d.tile_m, d.tile_n, d.kernel = batch, tile[0], tile[1], IGEMM
    return d


def _rule(d) -> bool:
    """The launcher's rule as the header states it: fp32, tile 128x128, whole K tiles per tap, at most 32 taps, no groups."""
    return (not d.flags & _lib.SP_CONV_BF16 and (d.tile_m, d.tile_n) == (128, 128) and d.c_in % 32 == 0 and d.taps_h * d.taps_w <= 32 and
            d.c_in_group == 0 and d.kernel == IGEMM)


# name, descriptor, has_residual, what the rule says (stated here as well: the table must hold both answers)
TABLE = [
    ("pw_64_128", _conv(64, 128), False, True),
    ("pw_32_256_res_relu", _conv(32, 256, flags=_lib.SP_CONV_RELU), True, True),
    ("pw_160_120_ragged_n", _conv(160, 120), False, True),
    ("pw_batch1", _conv(64, 128, batch=1), False, True),
    ("c3_64_128_tapskip", _conv(64, 128, 3), False, True),
    ("c3_64_128_batch1_plain", _conv(64, 128, 3, batch=1), True, True),
    ("c3s2_32_128", _conv(32, 128, 3, stride=2), False, True),
    ("c3_64_128_nchw", _conv(64, 128, 3, flags=_lib.SP_CONV_OUT_NCHW), False, True),
    ("c3_128_512_relu", _conv(128, 512, 3, flags=_lib.SP_CONV_RELU), False, True),
    ("deconv_64_128", _deconv(64, 128), False, True),
    ("pw_64_128_bf16", _conv(64, 128, flags=_lib.SP_CONV_BF16), False, False),
    ("pw_64_128_bf16_f32out", _conv(64, 128, flags=_lib.SP_CONV_BF16 | _lib.SP_CONV_OUT_F32), False, False),
    ("g32_128_grouped", _conv(128, 128, 3, panel=128), False, False),
    ("pw_16_128_non_uniform", _conv(16, 128), False, False),
    ("c7_4_128_non_uniform", _conv(4, 128, 7), False, False),
    ("pw_64_128_tile_64x128", _conv(64, 128, tile=(64, 128)), False, False),
    ("pw_64_128_tile_128x64", _conv(64, 128, tile=(128, 64)), False, False),
    ("pw_64_128_tile_64x64", _conv(64, 128, tile=(64, 64)), False, False),
    ("pw_64_128_tile_256x64", _conv(64, 128, tile=(256, 64)), False, False),
    ("c3_64_128_tile_128x64", _conv(64, 128, 3, tile=(128, 64)), False, False),
    ("deconv_64_128_tile_64x128", _deconv(64, 128, (64, 128)), False, False),
    ("pw_64_256_streaming_kernel", _conv(64, 256, kernel=_lib.SP_CONV_KERNEL_PW, tile=(0, 0)), False, False),
]


@pytest.mark.parametrize("name,d,res,want", TABLE, ids=[t[0] for t in TABLE])
def test_query_mirrors_the_launchers_rule(name, d, res, want):
    lib = _lib.lib()
    assert _rule(d) == want, name
    for tap_skip in (1, 0):
        lib.sp_conv_set_tap_skip(tap_skip)
        lib.sp_conv_set_single_stage(1)
        on = _lib.conv_single_stage(d, res)
        name_on = _lib.conv_kernel_name(d, res)
        lib.sp_conv_set_single_stage(0)
        off = _lib.conv_single_stage(d, res)
        name_off = _lib.conv_kernel_name(d, res)
        assert on == want and off is False, (name, tap_skip, on, off)
        assert name_on == name_off, (name_on, name_off)          # the knob moves no name
    if d.taps_h * d.taps_w > 1 and want and d.batch >= 64 and not d.flags & _lib.SP_CONV_OUT_NCHW:
        lib.sp_conv_set_tap_skip(1)
        assert _lib.conv_kernel_name(d, res) == "conv_igemm_tapskip_kernel<128, 128, 2, 2>"
    elif want:
        assert _lib.conv_kernel_name(d, res) == "conv_igemm_kernel<128, 128, 2, 2, true, false, false, false, false, false>"


def test_statistics_launches_keep_their_instantiations():
    """The train-mode forward (variant 1) and the dgrad with the BatchNorm sums (variant 2) are instantiations of their own: the same names
    whatever the knob says, and not the plain one the single-stage form stands in for.
    LIMITATION: sp_conv2d_single_stage asks about sp_conv2d_fwd launches only (it has no variant argument), so "a STATS / BSTATS launch
    answers 0" cannot be asked of it.  That such a launch never reaches the single-stage launcher follows from the code (launch<> returns
    through launch_t<..., STATS / BSTATS> before the single-stage branch); what is asserted here is its visible consequence: the name still
    carries the STATS / BSTATS flag, and no single-stage kernel has one."""
    lib = _lib.lib()
    d = _conv(64, 128)
    for variant, tail in ((1, "true, false, false, true, false, false>"), (2, "true, false, false, false, false, true>")):
        names = []
        for knob in (1, 0):
            lib.sp_conv_set_single_stage(knob)
            names.append(_lib.conv_kernel_name(d, False, variant))
        assert names[0] == names[1] and names[0].endswith(tail), names


def test_invalid_descriptor_answers_zero():
    d = _conv(64, 128)
    d.k_pad = 48
    assert _lib.conv_single_stage(d) is False
    assert b"k_pad" in _lib.lib().sp_last_error()


def test_lds_bytes_of_the_launches():
    """One operand stage: (BM + BN) * 32 floats + the row table [BM][4] ints = 34,816 bytes at 128x128, against 67,584 with two stages; four of
    the first but only two of the second fit the 160 KiB of a CU (registers cap the first at three)."""
    lib = _lib.lib()
    got = []
    for which in range(4):
        n = ctypes.c_int(-1)
        _lib.check(lib.sp_conv_igemm_resident_workgroups(which, None, ctypes.byref(n)), "sp_conv_igemm_resident_workgroups")
        got.append(n.value)
    one, two = (128 + 128) * 32 * 4 + 128 * 16, 2 * (128 + 128) * 32 * 4 + 128 * 16
    assert (one, two) == (34816, 67584) and got == [two, two, one, one]
    assert 160 * 1024 // two == 2 and 160 * 1024 // one >= 3
    assert lib.sp_conv_igemm_resident_workgroups(4, None, ctypes.byref(ctypes.c_int())) != 0
