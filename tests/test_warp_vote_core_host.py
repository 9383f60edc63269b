"""The walk warp_vote_bytes makes for an item (qoi_amd/csrc/qoi_warp_vote_core.h: tile -> work item -> the s x s nearest sub-samples of its
pixel and the centre value, each with the item's border -> the counts -> the largest word -> store), compiled with g++
(tests/host/warp_vote_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU, bit for bit: both VOTE flags, both modes, 3
and 4 output channels, the fill and every border, odd output addresses, rectangles of 1 x 1, 1 x 7, 2 x 2 and 17 x 9, maps that are the
whole-factor reduction, turn and reduce, shear, lie hundreds of periods away and stand next to +-2**56, and a negative a.  The rectangles
hold label images with stripes one pixel wide (tests/labelimg.py), so that ties arise.  The staging outside the rectangle holds a sentinel
and every load is checked to lie inside the rectangle; the loads are counted: exactly one per sub-sample and per centre that lies inside
the rectangle (or is brought into it by the border) - none for one that takes the fill.  A guard band around the output stays untouched
and every output byte is written exactly once.  Items without a VOTE flag walk warp_super_work through the same work item.  The same
source is also built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing
sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
import labelimg
from hostbuild import cint, cuint, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import warp
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4, WRAP

SRC = "warp_vote_host.cpp"
SENTINEL = 0x5A
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
RECTS = ((3, 2, 1, 1), (3, 2, 1, 7), (3, 2, 2, 2), (3, 2, 17, 9))
FILL = 0xFF000007                                                     # r 7, g 0, b 0, a 255: a class of the palette, so the fill joins votes


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "warp_vote_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, cint, u64, u64, u8p, u8p, u64]),
        "warp_vote_host_flags": (None, [ctypes.POINTER(cuint)])})


def staged(rect, margin, seed):
    """a staging array whose rectangle holds a label image with stripes one pixel wide and everything else the sentinel: as uint8[rows, w, 4]
    for the model and as dwords for the core"""
    x, y, cw, rh = rect
    px = np.full((y + rh, x + cw + margin, 4), SENTINEL, dtype=np.uint8)
    R = labelimg.label_image(cw, rh, 4, seed, cell=3)
    R[:, 1::4] = labelimg.PALETTE[2]                                   # stripes one pixel wide
    R[2::5, :] = labelimg.PALETTE[5]
    px[y:, x:x + cw] = R
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, rect, out_size, matrix, flags, fill, och, mode, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    band = hostbuild.Banded(ow * oh * och, a)
    m = (ctypes.c_longlong * 6)(*matrix)
    loads = lib.warp_vote_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, fill, och, mode, *band.args)
    what = (rect, out_size, matrix, flags, och, mode, a)
    assert loads >= 0, (what, loads)                                  # no load outside the rectangle, no store outside the output or unaligned
    return loads, band.inside(what)


def loads_of(rect, out_size, matrix, flags):
    """what the model says must be loaded: the sub-samples and the centres that do not take the fill"""
    _, _, cw, rh = rect
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    L = warp.vote_log2(flags)
    s = 1 << L

    def inside(Px, Py):
        return int((warp._border(Px >> 17, cw, flags)[1] & warp._border(Py >> 17, rh, flags)[1]).sum())

    total = inside(a * U + b * V + c, d * U + e * V + f)
    for j in range(s):
        for i in range(s):
            Us, Vs = s * U + (2 * i + 1 - s), s * V + (2 * j + 1 - s)
            total += inside(((a * Us + b * Vs) >> L) + c, ((d * Us + e * Vs) >> L) + f)
    return total


def test_the_flags_are_the_model_s(lib):
    got = (cuint * 3)()
    lib.warp_vote_host_flags(got)
    assert tuple(got) == (VOTE2, VOTE4, warp.VOTES) == (8192, 16384, 8192 | 16384)
    assert (VOTE4 << 16) == 1 << 30                                    # the flags fit WarpEntry::cfg


def maps_of(rect, out_size, s):
    _, _, cw, rh = rect
    S = ONE
    return [(s * S, 0, 0, 0, s * S, 0),                                                  # the whole-factor reduction where s divides: every sub-sample a pixel centre
            warp.rotation((cw, rh), out_size, 30.0, 1 / 3), (S, 23000, -40000, -9000, S + 700, 12345),
            (3 * S, 0, 2 * S * cw * 300 + 777, 0, 3 * S, -2 * S * rh * 500 - 999),        # hundreds of periods away
            (S, 0, 2 ** 56 - 1, 0, S, 1 - 2 ** 56), (S, 31, 1 - 2 ** 56, -17, S, 2 ** 56 - 1),   # next to +-2**56: positions near 2**57
            (-2 ** 31, 2 ** 31 - 1, 2 ** 56 - 1, 3, -5, 1 - 2 ** 56),                     # the limits
            (-3 * S - 1, 1, 2 * S * cw + 5, -1, -2 * S - 3, 2 * S * rh + 1)]              # a half turn that reduces: negative a, odd sums


@pytest.mark.parametrize("flag,s", [(VOTE2, 2), (VOTE4, 4)])
@pytest.mark.parametrize("border", BORDERS)
def test_walk_against_the_model(lib, border, flag, s):
    flags = border | flag
    spared = 0
    census = {}
    for rect in RECTS:
        px, dwords = staged(rect, 2, 5)
        for out_size in ((19, 18), (33, 5)) if rect[2] == 17 else ((19, 18),):
            for matrix in maps_of(rect, out_size, s):
                want_loads = loads_of(rect, out_size, matrix, flags)
                spared += want_loads < (s * s + 1) * out_size[0] * out_size[1]
                want4 = warp.warp(px, rect, out_size, matrix, flags, FILL)
                if rect[2] == 17 and out_size == (19, 18):
                    assert np.array_equal(want4, warp.vote_reference(px, rect, out_size, matrix, flags, FILL, census)), (rect, matrix)
                for och in (3, 4):
                    want = np.ascontiguousarray(want4[:, :, :och]).reshape(-1)     # (och 3 drops alpha after the vote)
                    for mode in (PLAIN, ALPHA_WEIGHTED):
                        for a in (0, 1, 3) if mode == PLAIN else (7,):
                            loads, got = run(lib, px, dwords, rect, out_size, matrix, flags, FILL, och, mode, a)
                            assert np.array_equal(got, want), (rect, out_size, matrix, och, mode, a, int(np.argmax(got != want)))
                            assert loads == want_loads, (rect, out_size, matrix, loads, want_loads)
    assert (spared > 0) == (border == 0)                                # only the fill spares a load
    assert census.get("unique", 0) > 0 and census.get("centre", 0) > 0, census       # (test_warp_vote_model.py asserts the lowest key too)


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_items_without_a_vote_flag_walk_as_before(lib, mode):
    """the same work item serves every other item: the branch is the item's"""
    rect = (3, 2, 11, 9)
    px, dwords = staged(rect, 2, 9)
    m = warp.rotation((11, 9), (33, 18), 30.0)
    for och in (3, 4):
        for flags in (0, REPLICATE, NEAREST, NEAREST | WRAP, BICUBIC, BICUBIC | REPLICATE, REFLECT, REFLECT_101 | BICUBIC, WRAP, SUPER2, SUPER4 | REFLECT):
            want = warp.warp(px[:, :, :och], rect, (33, 18), m, flags, FILL, mode).reshape(-1)
            loads, got = run(lib, px, dwords, rect, (33, 18), m, flags, FILL, och, mode, 1)
            assert np.array_equal(got, want), (och, flags)
            assert loads <= (1 if flags & NEAREST else (16 if flags & BICUBIC else (64 if flags & SUPER4 else (16 if flags & SUPER2 else 4)))) * 33 * 18


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "WARP_VOTE_HOST_MAIN", tmp_path) == "warp_vote_host: 2240 items ok\n"
