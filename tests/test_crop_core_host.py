"""The item loop the GPU kernel runs (qoi_amd/csrc/qoi_crop_core.h: item -> bytes -> staged pixels -> stores) compiled with g++
(tests/host/crop_host.cpp) and compared with the Python model qoi_amd/crops.py on the CPU, tile by tile as crop_gather walks a crop: both
output channel counts, every alignment of the output, all four flag values, widths and heights down to one pixel and a crop of more than one
tile.  The output equals crops.crop, a guard band around it stays untouched, every output byte is written exactly once, no load leaves the
rows the crop needs and every store is naturally aligned.  The same source is built as a stand-alone program with the address and
undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import numpy as np
import pytest

import hostbuild
from hostbuild import BAND, BASE, i64, u32, u32p, u64, u8p, ull
from qoi_amd import crops

SRC = "crop_host.cpp"


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "crop_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u64, u64, u8p, u8p, u64]),
        "crop_host_items": (ull, [u64, u64]),
        "crop_host_tiles": (ull, [u64, u64])})


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes: as dwords for the core, as uint8[rows, w, 4] for the model"""
    px = np.random.default_rng(seed).integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, x, y, cw, ch, flags, och, a):
    """one crop written at BASE + BAND + a; returns (items walked, output bytes); asserts guards and the write counts"""
    B = cw * ch * och
    band = hostbuild.Banded(B, a)
    walked = lib.crop_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, ch, flags, och, *band.args)
    what = (och, a, flags, cw, ch)
    assert walked == len(crops.items(band.q, B)) == lib.crop_host_items(band.q, B), (what, walked)     # (negative: a load or store out of bounds / misaligned)
    return walked, band.inside(what)


@pytest.mark.parametrize("och", [3, 4])
def test_item_loop_against_the_model(host_lib, och):
    for cw in (1, 2, 3, 5, 16, 17):
        for ch in (1, 2, 7):
            x, y = 3, 2
            px, dwords = staged(cw + 5, y + ch, cw * 100 + ch)              # the staging ends with the crop's last row
            for flags in range(4):
                want = crops.crop(px[:, :, :och], (x, y, cw, ch), flags).reshape(-1)
                for a in range(16):
                    _, got = run(host_lib, px, dwords, x, y, cw, ch, flags, och, a)
                    assert np.array_equal(got, want), (och, a, flags, cw, ch)


@pytest.mark.parametrize("och", [3, 4])
def test_more_than_one_tile(host_lib, och):
    """130 x 70: 27300 / 36400 bytes, 7 / 9 tiles of 256 items; the whole image, so column 0 and the last column are both read"""
    px, dwords = staged(130, 70, 7)
    for flags in range(4):
        want = crops.crop(px[:, :, :och], (0, 0, 130, 70), flags).reshape(-1)
        for a in (0, 1, 7, 15):
            walked, got = run(host_lib, px, dwords, 0, 0, 130, 70, flags, och, a)
            assert walked > 256 and host_lib.crop_host_tiles(BASE + BAND + a, want.size) == -(-walked // 256) >= 7
            assert np.array_equal(got, want), (och, a, flags)


def test_items_and_tiles(host_lib):
    for q in list(range(BASE, BASE + 16)) + [2 ** 47 + 5]:
        for B in list(range(1, 41)) + [4096, 4097, 399999999 * 4]:
            n = ((q + B + 15) >> 4) - (q >> 4)
            assert host_lib.crop_host_items(q, B) == n and host_lib.crop_host_tiles(q, B) == -(-n // 256), (q, B)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "CROP_HOST_MAIN", tmp_path) == "crop_host: 2432 crops ok\n"
