"""The walk the GPU kernel makes (qoi_amd/csrc/qoi_warp_core.h: tile and work item -> output pixel -> both positions -> samples, weights and
border -> blend -> pixel -> stores) compiled with g++ (tests/host/warp_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU,
tile by tile as warp_gather walks an item over staged uint8[rows, w, 4] whose last row is the rectangle's last row: every alignment 0..3 of
the output, both channel counts, both borders, both modes, outputs of 1 x 1, 17 x 1, 1 x 17 and 33 x 18, a rectangle of 1 x 1, maps that put
the whole output outside.  The counting memory functor checks that each output byte is written exactly once, that no byte beside an output is
written, that every store is naturally aligned and that no load falls outside the rectangle (so none outside its staged rows).  The same
source is built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing
sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, i64, i64p, u32, u32p, u64, u8p, ull, ullp
from qoi_amd import warp
from qoi_amd.warp import ALPHA_WEIGHTED, ONE, PLAIN, REPLICATE

SRC = "warp_host.cpp"
FILL = 0x40C08020


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "warp_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, cint, u64, u64, u8p, u8p, u64, ullp]),
        "warp_host_tiles": (ull, [u32, u32]),
        "warp_host_place": (cint, [u32, u32, u32, u32, u32p, u32p])})


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes, a fifth of them transparent and one block of transparent pixels: as dwords for the core, as
    uint8[rows, w, 4] for the model"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    px[:, :, 3][rng.integers(0, 5, size=(rows, w)) == 0] = 0
    px[rows // 2:, : w // 2, 3] = 0
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, rect, out_size, m, flags, och, mode, a):
    """one item written at BASE + BAND + a; returns (tiles walked, loads, output bytes); asserts guards and the write counts"""
    x, y, cw, rh = rect
    ow, oh = out_size
    band = hostbuild.Banded(ow * oh * och, a)
    tiles = ctypes.c_ulonglong(0)
    loads = lib.warp_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, (ctypes.c_longlong * 6)(*m), FILL, och, mode,
                              *band.args, ctypes.byref(tiles))
    what = (och, mode, a, flags, rect, out_size, m)
    assert loads >= 0, (what, loads)      # (negative: a load outside the rectangle, a store out of bounds or misaligned)
    assert tiles.value == warp.tiles(ow, oh) == lib.warp_host_tiles(ow, oh), what
    return tiles.value, loads, band.inside(what)


def maps(cw, rh, ow, oh):
    return {"identity": warp.IDENTITY, "quarter": (0, -ONE, 2 * cw * ONE, ONE, 0, 0), "rot30": warp.rotation((cw, rh), (ow, oh), 30.0),
            "shear": (ONE, 23000, -40000, -9000, ONE + 700, 12345), "down-up": (177124, 0, -3 * ONE, 0, 21140, 5),
            "outside": (ONE, 0, 40 * cw * ONE, 0, ONE, -37 * rh * ONE), "outside-left": (ONE, 0, -40 * ow * ONE, 0, ONE, 0),
            "limits": (-2 ** 31, 2 ** 31 - 1, (1 << 56) - 1, 3, -5, 1 - (1 << 56))}


def taken(cw, rh, ow, oh, m, replicate):
    """the loads the definition asks for: samples with a weight that lie inside the rectangle (all of them with REPLICATE)"""
    a, b, c, d, e, f = m
    n = 0
    for Y in range(oh):
        for X in range(ow):
            U, V = 2 * X + 1, 2 * Y + 1
            cols, rows = [], []
            for P, n_src, dst in ((a * U + b * V + c, cw, cols), (d * U + e * V + f, rh, rows)):
                p = P - ONE
                for k, wgt in ((p >> 17, 2 * ONE - (p & (2 * ONE - 1))), ((p >> 17) + 1, p & (2 * ONE - 1))):
                    if wgt and (replicate or 0 <= k < n_src):
                        dst.append(k)
            n += len(cols) * len(rows)
    return n


OUTS = [(1, 1), (17, 1), (1, 17), (33, 18)]


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_walk_against_the_model(host_lib, och, mode):
    for rect in [(3, 2, 11, 9), (4, 1, 1, 1)]:
        x, y, cw, rh = rect
        px, dwords = staged(cw + x + 2, y + rh, cw * 100 + rh)                # the staging ends with the rectangle's last row
        for out_size in OUTS:
            for name, m in maps(cw, rh, *out_size).items():
                for flags in (0, REPLICATE):
                    want = warp.warp(px[:, :, :och], rect, out_size, m, flags, FILL, mode).reshape(-1)
                    n_loads = taken(cw, rh, *out_size, m, bool(flags))
                    for a in range(4):
                        tiles, loads, got = run(host_lib, px, dwords, rect, out_size, m, flags, och, mode, a)
                        assert np.array_equal(got, want), (och, mode, a, flags, rect, out_size, name, int(np.argmax(got != want)))
                        assert loads == n_loads, (name, flags, loads, n_loads)  # a sample without a weight or with the fill is not loaded
                    if name.startswith("outside") and not flags:
                        assert n_loads == 0 and np.all(want.reshape(-1, och) == [0x20, 0x80, 0xC0, 0x40][:och])


def test_place_and_tiles(host_lib):
    X, Y = ctypes.c_uint32(), ctypes.c_uint32()
    for ow, oh in OUTS + [(16, 16), (48, 32), ((1 << 20) - 1, 381)]:
        n = host_lib.warp_host_tiles(ow, oh)
        assert n == warp.tiles(ow, oh)
        for tile in sorted({0, n // 2, n - 1}):
            for t in (0, 15, 16, 63, 64, 255):
                ok = host_lib.warp_host_place(tile, t, ow, oh, ctypes.byref(X), ctypes.byref(Y))
                want = warp.place(tile, t, ow, oh)
                assert (None if not ok else (X.value, Y.value)) == want, (ow, oh, tile, t)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "WARP_HOST_MAIN", tmp_path) == "warp_host: 2016 items ok\n"
