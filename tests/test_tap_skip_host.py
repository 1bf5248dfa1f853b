"""conv_geometry.tap_skip_k_tiles (no GPU): the K tiles the tap-skipping implicit GEMM executes, against a brute-force count over output positions,
and against the share of all-padding K tiles the headline program's layers were estimated at."""
import pytest
import torch

from oracle import nets_oracle
from simple_pose_amd import conv_geometry, engine, synth
from tests.desc_interp import TorchPacker


def _brute_valid_taps(d, py=0, px=0):
    """Valid taps of every output position of one phase, by walking the taps (no masks, no ordering)."""
    out = []
    for gy in range(d.grid_h):
        for gx in range(d.grid_w):
            n = 0
            for ty in range(d.taps_h):
                for tx in range(d.taps_w):
                    iy = gy * d.stride + d.dy0 + py + ty * d.dy_step
                    ix = gx * (d.stride_x or d.stride) + d.dx0 + px + tx * d.dx_step
                    n += 0 <= iy < d.in_h and 0 <= ix < d.in_w
            out.append(n)
    return out


def _conv3x3(h, w, c_in, stride=1):
    return conv_geometry.conv_fwd(h, w, c_in, 64, 64, 3, 3, 3, 3, 9 * c_in, stride, 1)


SHAPES = [("3x2 c32", _conv3x3(3, 2, 32)), ("3x2 c64", _conv3x3(3, 2, 64)), ("1x1 c32", _conv3x3(1, 1, 32)), ("1x1 c64", _conv3x3(1, 1, 64)),
          ("5x4 c64", _conv3x3(5, 4, 64)), ("4x4 c64", _conv3x3(4, 4, 64)), ("5x5 s2 c64", _conv3x3(5, 5, 64, stride=2)),
          ("deconv 2x3 c64", conv_geometry.deconv_k4s2p1_fwd(2, 3, 64, 64, 64))]


@pytest.mark.parametrize("name,d", SHAPES, ids=[n for n, _ in SHAPES])
def test_counts_equal_brute_force(name, d):
    phases = [(py, px) for py in range(d.phases_y) for px in range(d.phases_x)]
    taps, per_tap = d.taps_h * d.taps_w, d.c_in // 32
    positions = d.grid_h * d.grid_w
    for batch, tile_m in ((128, 64), (128, 128), (64, 64), (256, 128)):
        # a whole number of tiles per position: every tile is one position, the count is order-free
        want = sum(n for py, px in phases for n in _brute_valid_taps(d, py, px)) * per_tap * (batch // tile_m)
        full = len(phases) * positions * (batch // tile_m) * taps * per_tap
        assert conv_geometry.tap_skip_k_tiles(d, batch, tile_m) == (want, full)
    # ragged: tiles straddle positions and run the union of their taps - never fewer K tiles than the rows' own taps need, never more than all
    for batch, tile_m in ((70, 64), (70, 128), (100, 128)):
        done, full = conv_geometry.tap_skip_k_tiles(d, batch, tile_m)
        tiles_m = -(-batch * positions // tile_m)
        assert full == len(phases) * tiles_m * taps * per_tap
        rows = sum(n for py, px in phases for n in _brute_valid_taps(d, py, px)) * batch * per_tap        # row x K tile pairs that hold image data
        assert rows <= done * tile_m and per_tap * len(phases) * tiles_m <= done <= full
    # fewer than half a tile of images per position, or a single tap: the launcher keeps the full loop
    assert len(set(conv_geometry.tap_skip_k_tiles(d, 1, 64))) == 1 and len(set(conv_geometry.tap_skip_k_tiles(d, 31, 64))) == 1
    assert len(set(conv_geometry.tap_skip_k_tiles(d, 63, 128))) == 1


def test_positions_are_a_permutation_longest_first():
    for name, d in SHAPES:
        for py in range(d.phases_y):
            for px in range(d.phases_x):
                pos = conv_geometry.tap_skip_positions(d, py, px)
                assert sorted(pos) == [(gy, gx) for gy in range(d.grid_h) for gx in range(d.grid_w)], name
                n = [bin(conv_geometry.tap_mask(d, gy, gx, py, px)).count("1") for gy, gx in pos]
                assert n == sorted(n, reverse=True), (name, n)       # (true of these shapes: at most one tap row / column outside per side)
    one = conv_geometry.conv_fwd(4, 4, 64, 64, 64, 1, 1, 1, 1, 64, 1, 0)
    assert len(set(conv_geometry.tap_skip_k_tiles(one, 128, 64))) == 1


# the share of K tiles that multiply only padding, per layer of the headline (ResNet50-DConv 256x192, batch 128), as the lead was estimated
SHARE = {"deconv_layers.0": 14.1, "layer3.1.conv2": 9.5, "layer3.2.conv2": 9.5, "layer3.3.conv2": 9.5, "layer3.4.conv2": 9.5, "layer3.5.conv2": 9.5,
         "layer4.1.conv2": 18.5, "layer4.2.conv2": 18.5, "deconv_layers.6": 3.6, "layer2.1.conv2": 4.8, "layer2.2.conv2": 4.8, "layer2.3.conv2": 4.8,
         "deconv_layers.3": 7.2, "layer4.0.conv2": 9.7, "layer1.0.conv2": 2.4, "layer1.1.conv2": 2.4, "layer1.2.conv2": 2.4, "layer2.0.conv2": 2.4,
         "layer3.0.conv2": 4.9}


def test_share_of_the_headline_layers():
    """Figures of the estimate are printed to one decimal; the function's are compared at that precision, to +-0.2 points.
    (layer4.0.conv2, stride 2 from 16x12: 1 - (23/24)(17/18) = 9.49 %, printed 9.5 against the estimate's 9.7.)"""
    sd = {k: torch.from_numpy(v) for k, v in synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50("dconv"), seed=3).items()}
    prog = engine.resnet_program(sd, "dconv", in_h=256, in_w=192, packer=TorchPacker())
    ops = {op.name: op for op in prog.ops}
    for layer, want in SHARE.items():
        d = ops[layer].desc
        for tile_m in (64, 128):
            done, full = conv_geometry.tap_skip_k_tiles(d, 128, tile_m)
            share = round(100.0 * (1.0 - done / full), 1)
            print(layer, tile_m, done, full, f"{100.0 * (1.0 - done / full):.2f}")
            assert abs(share - want) <= 0.2 + 1e-9, (layer, tile_m, share, want)
