"""The walk warp_gather makes for an item with QOIMI_WARP_NEAREST (qoi_amd/csrc/qoi_warp_core.h: tile -> work item -> position -> one sample or
the fill -> store), compiled with g++ (tests/host/warp_nearest_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU: both
output channel counts, both modes, both borders, a set of alignments, outputs of one pixel, of one row and one column past a tile and of
several tiles, maps that turn, shear, reduce, reach past the top-left corner, leave the rectangle altogether and stand at the limits.  The
output equals the model, a guard band around it stays untouched, every output byte is written exactly once, every load lies inside the
rectangle, there is at most one load per output pixel, every store is a whole aligned one inside the output.  The same source is also built
as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded
into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, cuint, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import warp

WARP_SRC = "warp_nearest_host.cpp"


@pytest.fixture(scope="module")
def warp_lib(tmp_path_factory):
    return hostbuild.shared(WARP_SRC, tmp_path_factory, {
        "warp_nearest_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, cint, u64, u64, u8p, u8p, u64]),
        "warp_nearest_host_flag": (cuint, [])})


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes: as dwords for the core, as uint8[rows, w, 4] for the model"""
    px = np.random.default_rng(seed).integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


# ---------------------------------------------------------------------------------- the warp with the NEAREST flag
def warp_run(lib, px, dwords, rect, out_size, matrix, flags, fill, och, mode, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    band = hostbuild.Banded(ow * oh * och, a)
    m = (ctypes.c_longlong * 6)(*matrix)
    loads = lib.warp_nearest_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, fill, och, mode, *band.args)
    what = (rect, out_size, matrix, flags, och, mode, a)
    assert 0 <= loads <= ow * oh, (what, loads)                       # one load per pixel at most, none outside the rectangle
    return loads, band.inside(what)


@pytest.mark.parametrize("mode", [warp.PLAIN, warp.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_warp_nearest_walk_against_the_model(warp_lib, och, mode):
    assert warp_lib.warp_nearest_host_flag() == warp.NEAREST == 4
    S, fill = warp.ONE, 0x80C04020
    x, y, cw, rh = 3, 2, 11, 9
    px, dwords = staged(cw + x + 2, y + rh, 5)
    maps = [warp.IDENTITY, (0, -S, 2 * S * cw, S, 0, 0), warp.rotation((cw, rh), (33, 18), 30.0), (S, 23000, -40000, -9000, S + 700, 12345),
            (177124, 0, -3 * S, 0, 21140, 5), (S, 0, -5 * S - 1, 0, S, -3 * S - 1), (S, 0, 40 * S * cw, 0, S, -37 * S * rh),
            (-2 ** 31, 2 ** 31 - 1, 2 ** 56 - 1, 3, -5, 1 - 2 ** 56)]
    inside_and_outside = 0
    for out_size in [(1, 1), (17, 1), (1, 17), (33, 18)]:
        for matrix in maps:
            for rep in (0, warp.REPLICATE):
                want = warp.warp(px[:, :, :och], (x, y, cw, rh), out_size, matrix, rep | warp.NEAREST, fill, mode).reshape(-1)
                for a in (0, 1, 2, 3, 7):
                    loads, got = warp_run(warp_lib, px, dwords, (x, y, cw, rh), out_size, matrix, rep | warp.NEAREST, fill, och, mode, a)
                    assert np.array_equal(got, want), (out_size, matrix, rep, a, int(np.argmax(got != want)))
                    assert rep == 0 or loads == out_size[0] * out_size[1]
                    inside_and_outside += 0 < loads < out_size[0] * out_size[1]
    assert inside_and_outside > 0
    # without the flag the same program is the bilinear walk: the branch is the item's
    want = warp.warp(px[:, :, :och], (x, y, cw, rh), (33, 18), maps[2], 0, fill, mode).reshape(-1)
    assert np.array_equal(warp_run(warp_lib, px, dwords, (x, y, cw, rh), (33, 18), maps[2], 0, fill, och, mode, 1)[1], want)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(WARP_SRC, "WARP_NEAREST_HOST_MAIN", tmp_path) == "warp_nearest_host: 2304 items ok\n"
