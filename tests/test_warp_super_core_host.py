"""The walk warp_super_bytes makes for an item (qoi_amd/csrc/qoi_warp_super_core.h: tile -> work item -> the s x s sub-samples of its pixel ->
each one's positions, 2 x 2 taps and weights with the item's border -> the sums -> one rounding -> store), compiled with g++
(tests/host/warp_super_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU, bit for bit: both SUPER flags, both modes,
3 and 4 output channels, the fill and every border, odd output addresses, rectangles of 1 x 1, 1 x 7, 2 x 2 and 17 x 9, maps that are the
box, turn and reduce, shear, lie hundreds of periods away and stand next to +-2**56, and a negative a.  The staging outside the rectangle
holds a sentinel and every load is checked to lie inside the rectangle; the loads are counted: exactly one per tap that has a weight and
lies inside the rectangle (or is brought into it by the border) - none for a tap with the weight 0, none for a tap that takes the fill.  A
guard band around the output stays untouched and every output byte is written exactly once.  The position of a sub-sample is compared with
Python's integers at the largest U and V with negative coefficients, where the shift floors a negative sum next to -2**55.  Items without a
SUPER flag walk warp_border_work through the same work item.  The same source is also built as a stand-alone program with the address and
undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, cuint, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import warp
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, WRAP

SRC = "warp_super_host.cpp"
SENTINEL = 0x5A
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
RECTS = ((3, 2, 1, 1), (3, 2, 1, 7), (3, 2, 2, 2), (3, 2, 17, 9))
FILL = 0x80C04020


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "warp_super_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, cint, u64, u64, u8p, u8p, u64]),
        "warp_super_host_flags": (None, [ctypes.POINTER(cuint)]),
        "warp_super_host_position": (i64, [cint, cint, i64, u32, u32, u32, u32, u32])})


def staged(rect, margin, seed):
    """a staging array whose rectangle holds random pixels - mostly transparent, so A == 0 arises - and everything else the sentinel: as
    uint8[rows, w, 4] for the model and as dwords for the core"""
    x, y, cw, rh = rect
    px = np.full((y + rh, x + cw + margin, 4), SENTINEL, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    R = rng.integers(0, 256, size=(rh, cw, 4), dtype=np.uint8)
    R[:, :, 3] *= rng.integers(0, 3, size=(rh, cw), dtype=np.uint8) == 0
    px[y:, x:x + cw] = R
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, rect, out_size, matrix, flags, fill, och, mode, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    band = hostbuild.Banded(ow * oh * och, a)
    m = (ctypes.c_longlong * 6)(*matrix)
    loads = lib.warp_super_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, fill, och, mode, *band.args)
    what = (rect, out_size, matrix, flags, och, mode, a)
    assert loads >= 0, (what, loads)                                  # no load outside the rectangle, no store outside the output or unaligned
    return loads, band.inside(what)


def loads_of(rect, out_size, matrix, flags):
    """what the model says must be loaded: over all sub-samples, the taps that have a weight on both axes and do not take the fill"""
    _, _, cw, rh = rect
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    L = warp.super_log2(flags)
    s = 1 << L
    total = 0
    for j in range(s):
        for i in range(s):
            Us, Vs = s * U + (2 * i + 1 - s), s * V + (2 * j + 1 - s)
            _, wx, inx = warp._axis(((a * Us + b * Vs) >> L) + c, cw, flags)
            _, wy, iny = warp._axis(((d * Us + e * Vs) >> L) + f, rh, flags)
            total += int((((wy != 0) & iny).sum(axis=-1) * ((wx != 0) & inx).sum(axis=-1)).sum())
    return total


def test_the_flags_and_the_position_are_the_model_s(lib):
    got = (cuint * 2)()
    lib.warp_super_host_flags(got)
    assert tuple(got) == (SUPER2, SUPER4) == (1024, 2048)
    top = 2 ** 20 - 2                                                  # the largest X and Y: U = V = 2**21 - 3
    floored = 0
    for L in (1, 2):
        s = 1 << L
        for m, n in ((-2 ** 31, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31 + 1, -3), (-65537, 3), (ONE, 0), (-1, 0), (0, -1)):
            for o in (0, 2 ** 56 - 1, 1 - 2 ** 56):
                for X, Y in ((top, top), (top, 0), (0, top), (0, 0), (5, 3)):
                    for i in range(s):
                        for j in range(s):
                            Us, Vs = s * (2 * X + 1) + 2 * i + 1 - s, s * (2 * Y + 1) + 2 * j + 1 - s
                            assert 0 < Us < 2 ** 23 and 0 < Vs < 2 ** 23 and abs(m * Us + n * Vs) < 2 ** 55
                            want = ((m * Us + n * Vs) >> L) + o           # (Python's >> floors)
                            floored += (m * Us + n * Vs) < 0 and (m * Us + n * Vs) % s != 0
                            assert abs(want) < 2 ** 57
                            assert lib.warp_super_host_position(m, n, o, X, Y, i, j, L) == want, (L, m, n, o, X, Y, i, j)
    assert floored > 0                                                 # a negative sum that the shift does not divide


def maps_of(rect, out_size, s):
    _, _, cw, rh = rect
    S = ONE
    return [(s * S, 0, 0, 0, s * S, 0),                                                  # the box where s divides: every sub-sample a pixel centre
            warp.rotation((cw, rh), out_size, 30.0, 1 / 3), (S, 23000, -40000, -9000, S + 700, 12345),
            (3 * S, 0, 2 * S * cw * 300 + 777, 0, 3 * S, -2 * S * rh * 500 - 999),        # hundreds of periods away
            (S, 0, 2 ** 56 - 1, 0, S, 1 - 2 ** 56), (S, 31, 1 - 2 ** 56, -17, S, 2 ** 56 - 1),   # next to +-2**56: positions near 2**57
            (-2 ** 31, 2 ** 31 - 1, 2 ** 56 - 1, 3, -5, 1 - 2 ** 56),                     # the limits
            (-3 * S - 1, 1, 2 * S * cw + 5, -1, -2 * S - 3, 2 * S * rh + 1)]              # a half turn that reduces: negative a, odd sums


@pytest.mark.parametrize("flag,s", [(SUPER2, 2), (SUPER4, 4)])
@pytest.mark.parametrize("border", BORDERS)
def test_walk_against_the_model(lib, border, flag, s):
    flags = border | flag
    spared = filled = 0
    for rect in RECTS:
        px, dwords = staged(rect, 2, 5)
        for out_size in ((19, 18), (33, 5)) if rect[2] == 17 else ((19, 18),):
            for matrix in maps_of(rect, out_size, s):
                want_loads = loads_of(rect, out_size, matrix, flags)
                spared += want_loads < 4 * s * s * out_size[0] * out_size[1]
                for och in (3, 4):
                    for mode in (PLAIN, ALPHA_WEIGHTED):
                        want = warp.warp(px[:, :, :och], rect, out_size, matrix, flags, FILL, mode).reshape(-1)
                        for a in (0, 1, 3) if mode == PLAIN else (7,):
                            loads, got = run(lib, px, dwords, rect, out_size, matrix, flags, FILL, och, mode, a)
                            assert np.array_equal(got, want), (rect, out_size, matrix, och, mode, a, int(np.argmax(got != want)))
                            assert loads == want_loads, (rect, out_size, matrix, loads, want_loads)
    assert spared > 0                                                   # taps with the weight 0 (or, without a border, outside R) were not read


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_items_without_a_super_flag_walk_as_before(lib, mode):
    """the same work item serves every other item: the branch is the item's"""
    rect = (3, 2, 11, 9)
    px, dwords = staged(rect, 2, 9)
    m = warp.rotation((11, 9), (33, 18), 30.0)
    for och in (3, 4):
        for flags in (0, REPLICATE, NEAREST, NEAREST | WRAP, BICUBIC, BICUBIC | REPLICATE, REFLECT, REFLECT_101 | BICUBIC, WRAP):
            want = warp.warp(px[:, :, :och], rect, (33, 18), m, flags, FILL, mode).reshape(-1)
            loads, got = run(lib, px, dwords, rect, (33, 18), m, flags, FILL, och, mode, 1)
            assert np.array_equal(got, want), (och, flags)
            assert loads <= (1 if flags & NEAREST else (16 if flags & BICUBIC else 4)) * 33 * 18


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "WARP_SUPER_HOST_MAIN", tmp_path) == "warp_super_host: 2240 items ok\n"
