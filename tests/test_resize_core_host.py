"""The walk the GPU kernel makes (qoi_amd/csrc/qoi_resize_core.h: work item -> columns and rows -> weighted sums -> pixel -> stores) compiled
with g++ (tests/host/resize_host.cpp) and compared with the Python model qoi_amd/resize.py on the CPU, tile by tile as resize_filter walks an
item over staged uint8[rows, w, 4] whose last row is the item's last row: both output channel counts, both modes, all four flag values, every
alignment of the output, outputs of one pixel and of more than one tile, an item with 65 taps per axis, an upscale.  The output equals
resize.resize, a guard band around it stays untouched, every output byte is written exactly once, no load leaves the staged rows and every
store is naturally aligned.  The same source is built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a
program of its own: nothing sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, i64, u32, u32p, u64, u8p, ull, ullp
from qoi_amd import resize

SRC = "resize_host.cpp"


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "resize_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, cint, u64, u64, u8p, u8p, u64, ullp]),
        "resize_host_split": (None, [u32, u32, u32p, u32p]),
        "resize_host_taps": (u32, [u32, u32]),
        "resize_host_tiles": (ull, [u32, u32, u32]),
        "resize_host_div_round": (u32, [u64, u64])})


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes, a fifth of them transparent and one run of transparent pixels: as dwords for the core, as
    uint8[rows, w, 4] for the model"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    px[:, :, 3][rng.integers(0, 5, size=(rows, w)) == 0] = 0
    px[rows // 2:, : w // 2, 3] = 0
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, x, y, cw, rh, ow, oh, flags, och, mode, a):
    """one item written at BASE + BAND + a; returns (tiles walked, loads, output bytes); asserts guards and the write counts"""
    band = hostbuild.Banded(ow * oh * och, a)
    tiles = ctypes.c_ulonglong(0)
    loads = lib.resize_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, och, mode, *band.args, ctypes.byref(tiles))
    what = (och, mode, a, flags, cw, rh, ow, oh)
    assert loads >= ow * oh, (what, loads)                          # (negative: a load outside the staged rows, a store out of bounds or misaligned)
    assert tiles.value == resize.tiles(cw, ow, oh) == lib.resize_host_tiles(cw, ow, oh), what
    return tiles.value, loads, band.inside(what)


def check(lib, cw, rh, ow, oh, och, mode, alignments=range(16), flag_values=range(4), x=3, y=2, seed=0):
    px, dwords = staged(cw + x + 2, y + rh, seed + cw * 1000 + rh)          # the staging ends with the item's last row
    tiles = 0
    for flags in flag_values:
        want = resize.resize(px[:, :, :och], (x, y, cw, rh), (ow, oh), flags, mode).reshape(-1)
        for a in alignments:
            tiles, loads, got = run(lib, px, dwords, x, y, cw, rh, ow, oh, flags, och, mode, a)
            assert np.array_equal(got, want), (och, mode, a, flags, cw, rh, ow, oh, int(np.argmax(got != want)))
            # every column of every output pixel is loaded once: no two lanes share one, none is left out
            assert loads == int(np.count_nonzero(resize.weights(cw, ow))) * int(np.count_nonzero(resize.weights(rh, oh)))
    return tiles


@pytest.mark.parametrize("mode", [resize.PLAIN, resize.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_walk_against_the_model(host_lib, och, mode):
    # one pixel out of one and of many; identity; whole multiples; fractions down; an upscale; down in x with up in y and the reverse
    for (cw, rh, ow, oh) in [(1, 1, 1, 1), (11, 9, 1, 1), (11, 9, 11, 9), (12, 8, 3, 2), (11, 9, 3, 2), (11, 9, 5, 4), (5, 3, 13, 7), (1, 1, 3, 2),
                             (11, 3, 4, 9), (3, 11, 9, 4)]:
        check(host_lib, cw, rh, ow, oh, och, mode)


@pytest.mark.parametrize("mode", [resize.PLAIN, resize.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_65_taps_per_axis(host_lib, och, mode):
    """127 -> 2 and 191 -> 3: 63.5 and 63.67 source pixels per output pixel, 65 columns and rows under the middle ones; 16 lanes of 5 columns"""
    assert resize.taps(127, 2) == 65 and resize.split(127, 2) == (4, 5)
    assert int(np.count_nonzero(resize.weights(191, 3)[1])) == 65 and int(np.count_nonzero(resize.weights(127, 2)[0])) == 64
    check(host_lib, 191, 191, 3, 3, och, mode, alignments=(0, 5), flag_values=(0, 3))
    check(host_lib, 128, 64, 2, 1, och, mode, alignments=(1,), flag_values=(1,))             # the cap exactly: 64 taps


@pytest.mark.parametrize("och", [3, 4])
def test_more_than_one_tile(host_lib, och):
    """130 x 70 -> 37 x 23: 851 pixels of 2 lanes, 7 tiles; 40 x 30 -> 41 x 33: 1353 pixels of one lane, 6 tiles"""
    assert check(host_lib, 130, 70, 37, 23, och, resize.ALPHA_WEIGHTED, alignments=(0, 1, 7), flag_values=(0, 1, 2, 3), x=0, y=0) == 7
    assert check(host_lib, 40, 30, 41, 33, och, resize.PLAIN, alignments=(3,), flag_values=(2,)) == 6


def test_split_taps_and_tiles(host_lib):
    lg, c = ctypes.c_uint32(), ctypes.c_uint32()
    for ow in range(1, 9):
        for cw in range(1, 64 * ow + 1):
            t = int(np.count_nonzero(resize.weights(cw, ow), axis=1).max())
            assert t <= resize.taps(cw, ow) == host_lib.resize_host_taps(cw, ow) <= 65, (cw, ow)
            host_lib.resize_host_split(cw, ow, ctypes.byref(lg), ctypes.byref(c))
            assert (lg.value, c.value) == resize.split(cw, ow) and lg.value <= 4 and c.value <= 5 and c.value << lg.value >= resize.taps(cw, ow), (cw, ow)
            assert c.value <= 4 or resize.taps(cw, ow) == 65
    for (cw, ow, oh) in [(1, 1, 1), (130, 37, 23), (64, 1, 1), (5, 99999, 99999), (4096, 64, 1 << 20), (1, 1 << 20, 1 << 20), (3, 4294967295, 4294967295)]:
        want = resize.tiles(cw, ow, oh) if ow * oh < 2 ** 40 else 2 ** 32
        assert host_lib.resize_host_tiles(cw, ow, oh) == want, (cw, ow, oh)


def test_div_round_at_the_extremes(host_lib):
    """divisors T below 400 000 000 and sums of alphas A up to 255 * T; numerators up to 255 * 255 * T"""
    rng = np.random.default_rng(5)
    cases = [(0, 1), (1, 1), (255, 1), (127, 2), (255 * 399999999, 399999999), (255 * 255 * 399999999, 255 * 399999999), (2 ** 32 - 1, 2 ** 32 - 1),
             (2 ** 32, 2 ** 32 - 1), (255 * 2 ** 28, 2 ** 28), (255 * 2 ** 36, 2 ** 36), (2 ** 32 + 5, 3), (254 * (2 ** 33 + 1) + 2 ** 32, 2 ** 33 + 1)]
    for _ in range(2000):
        d = int(rng.integers(1, 255 * 399999999))
        cases.append((int(rng.integers(0, 256)) * d - int(rng.integers(0, d)) if rng.integers(0, 2) else int(rng.integers(0, 255 * d + 1)), d))
    for n, d in cases:
        n = max(n, 0)
        assert host_lib.resize_host_div_round(n, d) == (n + d // 2) // d, (n, d)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "RESIZE_HOST_MAIN", tmp_path) == "resize_host: 1056 items ok\n"
