"""The crop warp's four launchers (csrc/warp.hip) on the MI355X at their edges, against expected values that come from three sources at once
(tests/warp_edges.py: closed forms, a float64 bilinear reference with a derived bound, and the C oracle bit for bit - `expected` asserts all
three before a kernel is compared with the result).  Every source is cut out of one larger device buffer filled with 255, so a read outside
the image stays inside the allocation and shows up as a wrong pixel; every destination is prefilled, with guard bytes before and behind."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from tests import warp_edges as we

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8192          # bytes of 255 around every source: more than any neighbouring row of the largest one (29 x 3 B)
GUARD = 64             # guard bytes before and behind a destination (64: the destination itself stays 16-byte aligned)
FILL = 0xAB


def _stream():
    return _lib.current_stream(torch.device(DEV))


class Sources:
    """Sources packed into ONE device buffer of 255s at odd offsets, MARGIN apart; `extra` more bytes of 255 at the end."""

    def __init__(self, arrays, extra=0):
        offs, pos = [], MARGIN + 1
        for a in arrays:
            offs.append(pos)
            pos += a.size + MARGIN + (1 - (a.size & 1))                      # keep the offsets odd
        host = np.full(pos + extra + MARGIN, 255, np.uint8)
        for a, o in zip(arrays, offs):
            host[o:o + a.size] = a.reshape(-1)
        self.buf = torch.from_numpy(host).to(DEV)
        self.ptr = [self.buf.data_ptr() + o for o in offs]
        self.extra_ptr = self.buf.data_ptr() + pos                           # `extra` bytes of 255, with MARGIN behind them
        self.host = host

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.host)


class Dest:
    """`nbytes` of FILL (or NaN floats) on the device behind GUARD + `shift` bytes, with a guard behind."""

    def __init__(self, nbytes, shift=0, dtype=torch.uint8):
        self.n, self.off, self.dtype = nbytes, GUARD + shift, dtype
        self.buf = torch.full((GUARD + shift + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        if dtype == torch.float32:
            assert shift == 0 and nbytes % 4 == 0
            self.buf[GUARD:GUARD + nbytes].view(torch.float32).fill_(float("nan"))
        self.ptr = self.buf.data_ptr() + self.off

    def read(self):
        raw = self.buf.cpu().numpy()
        assert (raw[:self.off] == FILL).all() and (raw[self.off + self.n:] == FILL).all(), "wrote outside its destination"
        body = raw[self.off:self.off + self.n]
        return body.view(np.float32) if self.dtype == torch.float32 else body


def _src(h, w, i):
    return we.hard_source(h, w, seed=i) if i % 2 == 0 else we.smooth_source(h, w)


# ---- 1. sp_warp_affine_u8c3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", we.SOURCE_SIZES, ids=[f"src{h}x{w}" for h, w in we.SOURCE_SIZES])
def test_crops_of_one_image_at_every_edge(h, w):
    """31 / 32 / 33 / 65 crops (one and two and three launches of WARP_BATCH) per output size, of a hard and of a smooth source."""
    srcs = Sources([_src(h, w, 0), _src(h, w, 1)])
    for k in (0, 1):
        src = _src(h, w, k)
        for (oh, ow), n in zip(we.OUT_SIZES, we.COUNTS):
            cs = we.cases(h, w, oh, ow, n)
            want = np.stack([we.expected(src, kind, arg, fwd, False, oh, ow) for kind, arg, fwd in cs])
            m = np.ascontiguousarray(np.stack([fwd for _, _, fwd in cs]), np.float64)
            dst = Dest(n * oh * ow * 3)
            _lib.check(_lib.lib().sp_warp_affine_u8c3(srcs.ptr[k], h, w, m.ctypes.data, n, dst.ptr, oh, ow, _stream()), "sp_warp_affine_u8c3")
            got = dst.read().reshape(n, oh, ow, 3)
            bad = [(i, cs[i][0], cs[i][1]) for i in range(n) if not np.array_equal(got[i], want[i])]
            assert not bad, ((h, w), (oh, ow), k, bad[:4])
    assert srcs.unchanged()


# ---- 2. sp_warp_affine_batch_u8c3_to_nchw_f32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out,n", list(zip(we.OUT_SIZES, we.COUNTS)), ids=[f"out{a}x{b}_n{n}" for (a, b), n in zip(we.OUT_SIZES, we.COUNTS)])
def test_training_batch_mixes_sources_sizes_and_flips(out, n):
    """Sample i: source size i mod 5 (hard and smooth alternate), its own case i of that size's list, flipped when i mod 3 == 1; samples
    0 - 4 are the identity with flip = 1, whose crop is the top left of np.fliplr(src), for every source size.  The fp32
    planes are (float)v / 255.0f - mean on the expected bytes, bit for bit; `crops` given and null."""
    oh, ow = out
    arrays = [_src(*we.SOURCE_SIZES[i % 5], i) for i in range(10)]
    srcs = Sources(arrays)
    pick, flips, maps, want = [], [], [], []
    for i in range(n):
        h, w = we.SOURCE_SIZES[i % 5]
        kind, arg, fwd = we.cases(h, w, oh, ow, n)[0 if i < 5 else i]            # the first five: np.fliplr of every source size
        pick.append(i % 10); flips.append(int(i < 5 or i % 3 == 1)); maps.append(fwd)
        want.append(we.expected(arrays[i % 10], kind, arg, fwd, bool(flips[-1]), oh, ow))
    want = np.stack(want)
    for i in range(5):
        h, w = we.SOURCE_SIZES[i]
        assert np.array_equal(want[i][:h, :w], np.fliplr(arrays[i])[:oh, :ow]) and not want[i][h:].any() and not want[i][:, w:].any()
    ptrs =np.array([srcs.ptr[p] for p in pick], np.uint64)
    hw = np.array([arrays[p].shape[:2] for p in pick], np.int32).reshape(n, 2)
    fl = np.array(flips, np.int32)
    m = np.ascontiguousarray(np.stack(maps), np.float64)
    mean = (ctypes.c_float * 3)(*we.MEAN)
    assert {0, 1} <= set(flips) and len({tuple(s) for s in hw}) == 5
    want_f32 = we.normalised(want)
    for with_crops in (True, False):
        out_f32 = Dest(n * 3 * oh * ow * 4, dtype=torch.float32)
        crops = Dest(n * oh * ow * 3)
        _lib.check(_lib.lib().sp_warp_affine_batch_u8c3_to_nchw_f32(ptrs.ctypes.data, hw.ctypes.data, fl.ctypes.data, m.ctypes.data, n, oh, ow, mean,
                                                                     out_f32.ptr, crops.ptr if with_crops else None, _stream()),
                   "sp_warp_affine_batch_u8c3_to_nchw_f32")
        got = out_f32.read().reshape(n, 3, oh, ow)
        bad = [i for i in range(n) if not np.array_equal(got[i].view(np.uint32), want_f32[i].view(np.uint32))]
        assert not bad, (out, with_crops, bad[:8])
        body = crops.read()
        if with_crops:
            assert np.array_equal(body.reshape(n, oh, ow, 3), want)
        else:
            assert (body == FILL).all()
    assert srcs.unchanged()


# ---- 3. / 4. the plan launchers -------------------------------------------------------------------------------------------------------------
CAP, LIVE = 5, 3       # capacity 5, seg[B] = 3: slots 3 and 4 are dead whatever their index says
SLOT_CASE = (20, 10, 13)   # of we.base_maps: a rotated and scaled map, the half pixel between column -1 and 0, the 2x decimation


def _plan_inputs(slot_cases, index):
    """Device m_inv [CAP, 6] (NaN in the slots without a case: a dead slot's map is not read) and src_index [CAP]."""
    m_inv = np.full((CAP, 6), np.nan, np.float64)
    for s, c in slot_cases.items():
        m_inv[s] = we.invert_affine(c[2])
    return torch.from_numpy(m_inv).to(DEV), torch.tensor(index, dtype=torch.int32, device=DEV)


def _check_slots(dst, want, oh, ow, where):
    got = dst.read().reshape(CAP, oh, ow, 3)
    for s in range(CAP):
        w = want.get(s)
        if w is None:
            assert not got[s].any(), (where, s, "a dead slot is zero-filled, every byte")
        else:
            assert np.array_equal(got[s], w), (where, s, "a live slot holds its crop; a neighbour's fill does not reach it")
    assert not want or any(w.any() for w in want.values()), (where, "the live crops are not all border")


@pytest.mark.parametrize("oh,ow,shift", [(5, 7, 0), (5, 7, 3), (4, 4, 0), (4, 4, 3)], ids=["5x7", "5x7_unaligned", "4x4", "4x4_unaligned"])
@pytest.mark.parametrize("h,w", [(37, 29), (1, 9)], ids=["src37x29", "src1x9"])
def test_plan_crops_dead_slots_and_bad_indices(h, w, oh, ow, shift):
    """sp_warp_affine_plan_u8c3, B = 2 images: a source index of -1 and one equal to B inside the live range, slots from seg[B] on, at
    105-byte slots (byte fill; every other slot starts unaligned) and 48-byte slots (16-byte fill when the destination is aligned, byte fill
    when it is not).  Live slots next to dead ones keep their crops."""
    B = 2
    imgs = [_src(h, w, 0), _src(h, w, 1)]
    srcs = Sources([np.stack(imgs)])
    seg = torch.tensor([0, 2, LIVE], dtype=torch.int32, device=DEV)
    cs = we.cases(h, w, oh, ow, 25)
    for index in ([0, -1, 1, 0, 1], [B, 0, 1, 1, 0], [1, 1, B + 5, 0, 0]):
        slot_cases = {s: cs[SLOT_CASE[s]] for s in range(LIVE) if 0 <= index[s] < B}
        m_inv, idx = _plan_inputs(slot_cases, index)
        want = {s: we.expected(imgs[index[s]], *c, False, oh, ow) for s, c in slot_cases.items()}
        dst = Dest(CAP * oh * ow * 3, shift)
        _lib.check(_lib.lib().sp_warp_affine_plan_u8c3(srcs.ptr[0], B, h, w, m_inv.data_ptr(), idx.data_ptr(), seg.data_ptr(), CAP, dst.ptr, oh, ow,
                                                       _stream()), "sp_warp_affine_plan_u8c3")
        _check_slots(dst, want, oh, ow, ((h, w), (oh, ow), shift, index))
    assert srcs.unchanged()


def _table(entries):
    """[(data pointer or 0, h, w)] -> the sp_image_ref table on the device (the letterbox fields are not read by the warp)."""
    refs = (_lib.ImageRef * len(entries))()
    for r, (p, h, w) in zip(refs, entries):
        r.data, r.h, r.w = p, h, w
        r.new_h, r.new_w, r.top, r.left, r.ratio, r.dst_index = 1, 1, 0, 0, 1.0, 99
    raw = np.frombuffer(bytes(refs), np.uint8).reshape(len(entries), ctypes.sizeof(_lib.ImageRef))
    return torch.from_numpy(raw.copy()).to(DEV)


@pytest.mark.parametrize("oh,ow,shift", [(5, 7, 0), (5, 7, 3), (4, 4, 0), (4, 4, 3)], ids=["5x7", "5x7_unaligned", "4x4", "4x4_unaligned"])
def test_plan_images_refuses_table_entries_it_cannot_read(oh, ow, shift):
    """sp_warp_affine_plan_images_u8c3 on a table of five entries: a 37 x 29 image, one with a null pointer, one with h = 0, one 40000 wide
    and a 1 x 9 image.  Slots that name the three bad entries, -1 or B are zero-filled like the slots from seg[B] on.  (The 40000-wide entry
    points at 2 x 40000 x 3 bytes of 255 inside the allocation: were it read, the crop would be 255s, not a fault.)"""
    B = 5
    imgs = {0: _src(37, 29, 0), 4: _src(1, 9, 1)}
    srcs = Sources([imgs[0], imgs[4]], extra=2 * 40000 * 3)
    table = _table([(srcs.ptr[0], 37, 29), (0, 37, 29), (srcs.ptr[0], 0, 29), (srcs.extra_ptr, 2, 40000), (srcs.ptr[1], 1, 9)])
    seg = torch.tensor([0, 1, 2, 2, 3, LIVE], dtype=torch.int32, device=DEV)
    for index in ([0, 1, 4, 0, 4], [2, 0, 3, 0, 0], [-1, 4, B, 4, 0], [4, 0, 4, 1, 2]):
        slot_cases = {}
        for s in range(LIVE):
            if index[s] in imgs:
                h, w = imgs[index[s]].shape[:2]
                slot_cases[s] = we.cases(h, w, oh, ow, 25)[SLOT_CASE[s]]
        m_inv, idx = _plan_inputs(slot_cases, index)
        want = {s: we.expected(imgs[index[s]], *c, False, oh, ow) for s, c in slot_cases.items()}
        dst = Dest(CAP * oh * ow * 3, shift)
        _lib.check(_lib.lib().sp_warp_affine_plan_images_u8c3(table.data_ptr(), B, m_inv.data_ptr(), idx.data_ptr(), seg.data_ptr(), CAP, dst.ptr, oh,
                                                              ow, _stream()), "sp_warp_affine_plan_images_u8c3")
        _check_slots(dst, want, oh, ow, ((oh, ow), shift, index))
    assert srcs.unchanged()
