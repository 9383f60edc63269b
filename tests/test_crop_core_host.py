"""The item loop the GPU kernel runs (qoi_amd/csrc/qoi_crop_core.h: item -> bytes -> staged pixels -> stores) compiled with g++
(tests/host/crop_host.cpp) and compared with the Python model qoi_amd/crops.py on the CPU, tile by tile as crop_gather walks a crop: both
output channel counts, every alignment of the output, all four flag values, widths and heights down to one pixel and a crop of more than one
tile.  The output equals crops.crop, a guard band around it stays untouched, every output byte is written exactly once, no load leaves the
rows the crop needs and every store is naturally aligned.  The same source is built as a stand-alone program with the address and
undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from qoi_amd import crops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "crop_host.cpp")
GUARD = 0xA5
BASE = 1 << 20                      # the virtual address of out[0]: a multiple of 16
BAND = 48


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("crophost") / "libcrop_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, SRC], check=True)
    lib = ctypes.CDLL(out)
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.crop_host_run.restype = ctypes.c_longlong
    lib.crop_host_run.argtypes = [ctypes.POINTER(u32), u64, u32, u32, u32, u32, u32, u32, u32, u64, u64, u8p, u8p, u64]
    lib.crop_host_items.restype = ctypes.c_ulonglong
    lib.crop_host_items.argtypes = [u64, u64]
    lib.crop_host_tiles.restype = ctypes.c_ulonglong
    lib.crop_host_tiles.argtypes = [u64, u64]
    return lib


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes: as dwords for the core, as uint8[rows, w, 4] for the model"""
    px = np.random.default_rng(seed).integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, x, y, cw, ch, flags, och, a):
    """one crop written at BASE + BAND + a; returns (items walked, output bytes); asserts guards and the write counts"""
    B = cw * ch * och
    out = np.full(BAND + a + B + BAND, GUARD, dtype=np.uint8)
    writes = np.zeros(out.size, dtype=np.uint8)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    q = BASE + BAND + a
    walked = lib.crop_host_run(dwords.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), dwords.size, px.shape[1], x, y, cw, ch, flags, och, q, BASE,
                               out.ctypes.data_as(u8p), writes.ctypes.data_as(u8p), out.size)
    what = (och, a, flags, cw, ch)
    assert walked == len(crops.items(q, B)) == lib.crop_host_items(q, B), (what, walked)     # (negative: a load or store out of bounds / misaligned)
    lo, hi = BAND + a, BAND + a + B
    assert np.all(writes[lo:hi] == 1) and not writes[:lo].any() and not writes[hi:].any(), what
    assert np.all(out[:lo] == GUARD) and np.all(out[hi:] == GUARD), what
    return walked, out[lo:hi]


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
    """the same source with its own main(), built with -fsanitize=address,undefined and the sanitizer runtimes linked statically: a program
    of its own that needs nothing from its environment"""
    exe = str(tmp_path / "crop_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DCROP_HOST_MAIN",
                    "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "crops ok" in r.stdout and "runtime error" not in r.stderr
