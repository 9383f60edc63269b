"""The walk warp_proj_bytes makes for an item (qoi_amd/csrc/qoi_warp_proj_core.h: tile -> work item -> the denominator of its pixel -> both
positions as exact quotients -> the item's border and sampling through the position-taking forms -> store), compiled with g++
(tests/host/warp_proj_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU, bit for bit: the quotient against Python's
big integers at its extremes (N within 1 of +-2**54, W at 2**(F-3) and next to 5 * 2**F, F from 14 to 34, negative N that floor); F, the
least denominator and both positions of pixels of outputs up to (2**20 - 1) x 3; the three samplings, the fill and every border, both modes,
3 and 4 output channels, odd output addresses, rectangles of 1 x 1, 1 x 7, 2 x 2 and 17 x 9, maps that turn, shear, lie hundreds of periods
away and stand next to +-2**53, denominators that are 1, tilt and come next to the limit of 1/8.  The staging outside the rectangle holds a
sentinel and every load is checked to lie inside the rectangle; a guard band around the output stays untouched and every output byte is
written exactly once.  Items without the flag walk warp_vote_work through the same work item.  The same source is also built as a
stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into
this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, cuint, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import warp
from qoi_amd.warp import (ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, PROJECTIVE, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4,
                          WRAP)

SRC = "warp_proj_host.cpp"
SENTINEL = 0x5A
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
SAMPLINGS = (0, NEAREST, BICUBIC)
RECTS = ((3, 2, 1, 1), (3, 2, 1, 7), (3, 2, 2, 2), (3, 2, 17, 9))
FILL = 0x80FF4007


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "warp_proj_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, u32, cint, u64, u64, u8p, u8p, u64]),
        "warp_proj_host_position": (i64, [i64, i64, u32]),
        "warp_proj_host_pixel": (i64, [u32, u32, i64p, u32, u32, u32, i64p]),
        "warp_proj_host_bits": (u32, [u32, u32]),
        "warp_proj_host_least": (i64, [u32, u32, u32]),
        "warp_proj_host_consts": (None, [ctypes.POINTER(cuint)])})


def staged(rect, margin, seed):
    """a staging array whose rectangle holds noise with alpha of every kind and everything else the sentinel: as uint8[rows, w, 4] for the
    model and as dwords for the core"""
    x, y, cw, rh = rect
    px = np.full((y + rh, x + cw + margin, 4), SENTINEL, dtype=np.uint8)
    R = np.random.default_rng(seed).integers(0, 256, (rh, cw, 4), dtype=np.uint8)
    R[::2, ::3, 3] = 0
    R[1::2, 1::3, 3] = 255
    px[y:, x:x + cw] = R
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, rect, out_size, matrix, flags, reserved, fill, och, mode, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    band = hostbuild.Banded(ow * oh * och, a)
    m = (ctypes.c_longlong * 6)(*matrix)
    loads = lib.warp_proj_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, reserved, fill, och, mode, *band.args)
    what = (rect, out_size, matrix, flags, reserved, och, mode, a)
    assert loads >= 0, (what, loads)                                  # no load outside the rectangle, no store outside the output or unaligned
    return loads, band.inside(what)


def test_the_constants_are_the_model_s(lib):
    got = (cuint * 4)()
    lib.warp_proj_host_consts(got)
    assert tuple(got) == (PROJECTIVE, warp.PROJ_BASE, 17, 53) and warp.PROJ_MAX_OFFSET == 1 << 53
    for ow, oh in ((1, 1), (2, 1), (1, 2), (3, 3), (4, 4), (5, 4), (16, 16), (17, 9), (33, 40), (65536, 1), (65537, 1), (70000, 3), (2 ** 20 - 1, 3), (3, 2 ** 20 - 1)):
        assert lib.warp_proj_host_bits(ow, oh) == warp.proj_bits(ow, oh), (ow, oh)
        for g, h in ((0, 0), (1, -1), (-32768, 32767), (32767, -32768), (-955, 12)):
            F = warp.proj_bits(ow, oh)
            assert lib.warp_proj_host_least(warp.proj_reserved(g, h), ow, oh) == 2 ** F - abs(g) * (ow - 1) - abs(h) * (oh - 1), (ow, oh, g, h)


def test_the_quotient_against_big_integers(lib):
    rng = np.random.default_rng(11)
    n = 0
    for F in (14, 15, 17, 18, 25, 31, 33, 34):
        one = 1 << F
        for W in (one >> 3, (one >> 3) + 1, one - 1, one, one + 1, 2 * one - 1, 5 * one - 1, 5 * one - 2, one - one // 3):
            Ns = [2 ** 54 - 1, 2 ** 54 - 2, 1 - 2 ** 54, 2 - 2 ** 54, 0, 1, -1, ONE, -ONE, 2 ** 53 + 1, -2 ** 53 - 1, 131071, -131073]
            Ns += [k * W + dlt for k in (-7, -1, 1, 3, 1000003) for dlt in (-1, 0, 1)]                  # the floor at a boundary
            Ns += [int(v) for v in rng.integers(-2 ** 54 + 1, 2 ** 54, 300)]
            for N in Ns:
                assert lib.warp_proj_host_position(N, W, F) == N * 2 ** F // W, (N, W, F)
                n += 1
    assert n > 20000


@pytest.mark.parametrize("out_size,matrix,proj", [
    ((2 ** 20 - 1, 3), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 53 - 1, -2 ** 31, -2 ** 31, 1 - 2 ** 53), (-14336, 10)),      # F = 34: W falls to 2**(F-3) on the right
    ((2 ** 20 - 1, 3), (-2 ** 31, 5, 1 - 2 ** 53, 7, -2 ** 31, 2 ** 53 - 1), (14336, -10)),
    ((70000, 3), (ONE, 0, 0, 0, ONE, 0), (-26843, 0)),                                                              # F = 31
    ((1, 1), (2 ** 31 - 1, -2 ** 31, 2 ** 53 - 1, -2 ** 31, 2 ** 31 - 1, 1 - 2 ** 53), (32767, -32768)),             # F = 14
    ((16, 16), (-3 * ONE - 1, 1, -5, -1, -2 * ONE - 3, -131073), (477, -478)),                                       # negative N that floor
    ((33, 40), warp.rotation((17, 9), (33, 40), 30.0, 0.7), (-3000, 2500))])
def test_the_positions_of_pixels(lib, out_size, matrix, proj):
    """the denominator and both positions as the work item forms them, against ``positions``"""
    ow, oh = out_size
    reserved = warp.proj_reserved(*proj)
    assert warp._wrong(ow, oh, (0, 0, 1, 1), out_size, matrix, PROJECTIVE, reserved) == ""
    Px, Py = warp.positions(out_size, matrix, PROJECTIVE, reserved)
    m = (ctypes.c_longlong * 6)(*matrix)
    P = (ctypes.c_longlong * 2)()
    F = warp.proj_bits(ow, oh)
    for Y in sorted({0, 1, oh // 2, oh - 1} & set(range(oh))):
        for X in sorted({0, 1, 2, ow // 3, ow // 2, ow - 2, ow - 1} & set(range(ow))):
            W = lib.warp_proj_host_pixel(ow, oh, m, reserved, X, Y, P)
            assert W == 2 ** F + proj[0] * (2 * X + 1 - ow) + proj[1] * (2 * Y + 1 - oh) >= 2 ** (F - 3)
            assert (P[0], P[1]) == (int(Px[Y, X]), int(Py[Y, X])), (X, Y)


def maps_of(rect, out_size):
    _, _, cw, rh = rect
    S = ONE
    return [warp.rotation((cw, rh), out_size, 30.0, 0.7), (S, 23000, -40000, -9000, S + 700, 12345),
            (3 * S, 0, 2 * S * cw * 300 + 777, 0, 3 * S, -2 * S * rh * 500 - 999),        # hundreds of periods away
            (S, 31, 2 ** 53 - 1, -17, S, 1 - 2 ** 53),                                    # next to +-2**53: positions near 2**56
            (-2 ** 31, 2 ** 31 - 1, 1 - 2 ** 53, 3, -5, 2 ** 53 - 1)]                     # the limits


def tilts_of(out_size):
    """(g, h): none, a moderate one, and two next to the limit 2**F - |g| (ow - 1) - |h| (oh - 1) >= 2**(F - 3)"""
    ow, oh = out_size
    room = 7 * 2 ** (warp.proj_bits(ow, oh) - 3)
    return [(0, 0), (min(room // (4 * max(ow - 1, 1)), 32767), -min(room // (5 * max(oh - 1, 1)), 32768)), (-min(room // max(ow - 1, 1), 32768), 0),
            (min(room // (2 * max(ow - 1, 1)), 32767), min(room // (2 * max(oh - 1, 1)), 32767))]


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("border", BORDERS)
def test_walk_against_the_model(lib, border, sampling):
    flags = border | sampling | PROJECTIVE
    taps = 1 if sampling == NEAREST else (16 if sampling == BICUBIC else 4)
    spared = 0
    for rect in RECTS:
        px, dwords = staged(rect, 2, 5)
        for out_size in ((19, 18), (33, 5)) if rect[2] == 17 else ((19, 18),):
            for matrix in maps_of(rect, out_size):
                for proj in tilts_of(out_size):
                    reserved = warp.proj_reserved(*proj)
                    assert warp._wrong(px.shape[1], px.shape[0], rect, out_size, matrix, flags, reserved) == "", (out_size, proj)
                    for och in (3, 4):
                        for mode in (PLAIN, ALPHA_WEIGHTED):
                            want = warp.warp(px[:, :, :och], rect, out_size, matrix, flags, FILL, mode, reserved=reserved).reshape(-1)
                            for a in (0, 1, 3) if mode == PLAIN else (7,):
                                loads, got = run(lib, px, dwords, rect, out_size, matrix, flags, reserved, FILL, och, mode, a)
                                assert np.array_equal(got, want), (rect, out_size, matrix, proj, och, mode, a, int(np.argmax(got != want)))
                                assert 0 <= loads <= taps * out_size[0] * out_size[1]
                                spared += loads < out_size[0] * out_size[1]
    assert spared > 0 or border != 0                                    # the fill spares loads


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_zero_coefficients_and_items_without_the_flag_walk_as_before(lib, mode):
    """g = h = 0 with the flag is the item without it, byte for byte and load for load; the same work item serves every older item: the
    branch is the item's"""
    rect = (3, 2, 11, 9)
    px, dwords = staged(rect, 2, 9)
    m = warp.rotation((11, 9), (33, 18), 30.0)
    for och in (3, 4):
        for flags in (0, REPLICATE, NEAREST, NEAREST | WRAP, BICUBIC, BICUBIC | REPLICATE, REFLECT, REFLECT_101 | BICUBIC, WRAP, SUPER2, SUPER4 | REFLECT, VOTE2, VOTE4 | WRAP):
            voted = flags & warp.VOTES
            want = warp.warp(px if voted else px[:, :, :och], rect, (33, 18), m, flags, FILL, mode, och=och if voted else 0).reshape(-1)
            loads, got = run(lib, px, dwords, rect, (33, 18), m, flags, 0, FILL, och, mode, 1)
            assert np.array_equal(got, want), (och, flags)
            if not flags & (warp.SUPERS | warp.VOTES):
                loads0, got0 = run(lib, px, dwords, rect, (33, 18), m, flags | PROJECTIVE, 0, FILL, och, mode, 1)
                assert np.array_equal(got0, want) and loads0 == loads, (och, flags)
            # reserved is not looked at without the flag (the host rejects it; the table carries zeros)
            assert np.array_equal(run(lib, px, dwords, rect, (33, 18), m, flags, 0x7FFF7FFF, FILL, och, mode, 1)[1], want)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "WARP_PROJ_HOST_MAIN", tmp_path) == "warp_proj_host: 162240 quotients, 4800 items ok\n"
