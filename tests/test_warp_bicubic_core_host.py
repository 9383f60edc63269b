"""The walk warp_bicubic_bytes makes for an item (qoi_amd/csrc/qoi_warp_cubic_core.h: tile -> work item -> positions -> four weights per axis
-> row by row up to four samples, their blend -> one rounding -> store), compiled with g++ (tests/host/warp_bicubic_host.cpp) and compared
with the Python model qoi_amd/warp.py on the CPU, bit for bit: both output channel counts, both modes, both borders, a set of alignments,
rectangles of 1 x 1, 2 x 2 and 11 x 9, outputs of one pixel, of one row and one column past a tile and of several tiles, maps that turn,
shear, reduce, reach past the top-left corner, leave the rectangle altogether and stand at the limits.  The staging outside the rectangle
holds a sentinel and every load is checked to lie inside the rectangle; the loads are counted: exactly one per sample that has a weight and
does not take the fill - none for a tap with q == 0.  A guard band around the output stays untouched and every output byte is written
exactly once.  Items without the flag walk warp_pixel / warp_nearest through the same work item.  The same source is also built as a
stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into
this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, cuint, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import warp

SRC = "warp_bicubic_host.cpp"
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "warp_bicubic_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, cint, u64, u64, u8p, u8p, u64]),
        "warp_bicubic_host_flag": (cuint, []),
        "warp_bicubic_host_weights": (None, [u32, ctypes.POINTER(ctypes.c_int32)])})


def staged(rect, margin, seed):
    """a staging array whose rectangle holds random pixels - mostly transparent, so A <= 0 arises - and everything else the sentinel: as
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
    loads = lib.warp_bicubic_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, fill, och, mode, *band.args)
    what = (rect, out_size, matrix, flags, och, mode, a)
    assert loads >= 0, (what, loads)                                  # no load outside the rectangle, no store outside the output or unaligned
    return loads, band.inside(what)


def loads_of(rect, out_size, matrix, flags):
    """the samples that have a weight and lie inside the rectangle (all of them with REPLICATE): what the model says must be loaded"""
    _, _, cw, rh = rect
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    _, qx, inx = warp._cubic_axis(a * U + b * V + c, cw, bool(flags & warp.REPLICATE))
    _, qy, iny = warp._cubic_axis(d * U + e * V + f, rh, bool(flags & warp.REPLICATE))
    col, row = inx & (qx != 0), iny & (qy != 0)
    return int((row.sum(axis=-1) * col.sum(axis=-1)).sum())


def test_the_weights_are_the_model_s(lib):
    assert lib.warp_bicubic_host_flag() == warp.BICUBIC == 16
    fr = np.concatenate([np.arange(0, 1 << 17, 13), [1, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 17) - 1]])
    want = warp.cubic_weights(fr)
    q = (ctypes.c_int32 * 4)()
    for f, w in zip(fr.tolist(), want.tolist()):
        lib.warp_bicubic_host_weights(f, q)
        assert list(q) == w, f


@pytest.mark.parametrize("mode", [warp.PLAIN, warp.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_walk_against_the_model(lib, och, mode):
    S, fill = warp.ONE, 0x80C04020
    spared = partly = 0
    for rect in ((3, 2, 11, 9), (3, 2, 1, 1), (3, 2, 2, 2)):
        x, y, cw, rh = rect
        px, dwords = staged(rect, 2, 5)
        maps = [warp.IDENTITY, (0, -S, 2 * S * cw, S, 0, 0), warp.rotation((cw, rh), (33, 18), 30.0), (S, 23000, -40000, -9000, S + 700, 12345),
                (177124, 0, -3 * S, 0, 21140, 5), (S, 0, -5 * S - 1, 0, S, -3 * S - 1), (S, 0, 40 * S * cw, 0, S, -37 * S * rh),
                (S // 2, 0, S // 2, 0, S // 2, S // 2), (-2 ** 31, 2 ** 31 - 1, 2 ** 56 - 1, 3, -5, 1 - 2 ** 56)]
        for out_size in [(1, 1), (17, 1), (1, 17), (33, 18)] if cw > 2 else [(17, 17), (33, 5)]:
            for matrix in maps:
                for rep in (0, warp.REPLICATE):
                    flags = rep | warp.BICUBIC
                    want = warp.warp(px[:, :, :och], rect, out_size, matrix, flags, fill, mode).reshape(-1)
                    want_loads = loads_of(rect, out_size, matrix, flags)
                    for a in (0, 1, 2, 3, 7) if cw > 2 else (0, 3):
                        loads, got = run(lib, px, dwords, rect, out_size, matrix, flags, fill, och, mode, a)
                        assert np.array_equal(got, want), (rect, out_size, matrix, rep, a, int(np.argmax(got != want)))
                        assert loads == want_loads, (rect, out_size, matrix, rep, loads, want_loads)
                    n = out_size[0] * out_size[1]
                    spared += want_loads < 16 * n and rep != 0              # taps with q == 0 were not read
                    partly += 0 < want_loads < 16 * n and rep == 0          # some taps took the fill
    assert spared > 0 and partly > 0
    # at a pixel centre one load per pixel, whatever the border
    rect = (3, 2, 11, 9)
    px, dwords = staged(rect, 2, 5)
    for rep in (0, warp.REPLICATE):
        assert run(lib, px, dwords, rect, (11, 9), warp.IDENTITY, rep | warp.BICUBIC, fill, och, mode, 0)[0] == 99


@pytest.mark.parametrize("mode", [warp.PLAIN, warp.ALPHA_WEIGHTED])
def test_items_without_the_flag_walk_as_before(lib, mode):
    """the same work item serves bilinear and nearest items: the branch is the item's"""
    rect, fill = (3, 2, 11, 9), 0x80C04020
    px, dwords = staged(rect, 2, 9)
    m = warp.rotation((11, 9), (33, 18), 30.0)
    for och in (3, 4):
        for flags in (0, warp.REPLICATE, warp.NEAREST, warp.NEAREST | warp.REPLICATE):
            want = warp.warp(px[:, :, :och], rect, (33, 18), m, flags, fill, mode).reshape(-1)
            loads, got = run(lib, px, dwords, rect, (33, 18), m, flags, fill, och, mode, 1)
            assert np.array_equal(got, want), (och, flags)
            assert loads <= (1 if flags & warp.NEAREST else 4) * 33 * 18


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "WARP_BICUBIC_HOST_MAIN", tmp_path) == "warp_bicubic_host: 2688 items ok\n"
