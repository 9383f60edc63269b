"""The walk warp_gather makes for an item with QOIMI_WARP_NEAREST (qoi_amd/csrc/qoi_warp_core.h: tile -> work item -> position -> one sample or
the fill -> store), compiled with g++ (tests/host/warp_nearest_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU: both
output channel counts, both modes, both borders, a set of alignments, outputs of one pixel, of one row and one column past a tile and of
several tiles, maps that turn, shear, reduce, reach past the top-left corner, leave the rectangle altogether and stand at the limits.  The
output equals the model, a guard band around it stays untouched, every output byte is written exactly once, every load lies inside the
rectangle, there is at most one load per output pixel, every store is a whole aligned one inside the output.  The same source is also built
as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded
into this process)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from qoi_amd import warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARP_SRC = os.path.join(ROOT, "tests", "host", "warp_nearest_host.cpp")
GUARD = 0xA5
BASE = 1 << 20                      # the virtual address of out[0]: a multiple of 16
BAND = 48
u32, u64 = ctypes.c_uint32, ctypes.c_uint64
u8p = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def warp_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("warpnearesthost") / "libwarp_nearest_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, WARP_SRC], check=True)
    lib = ctypes.CDLL(out)
    lib.warp_nearest_host_run.restype = ctypes.c_longlong
    lib.warp_nearest_host_run.argtypes = [ctypes.POINTER(u32), u64, u32, u32, u32, u32, u32, u32, u32, u32, ctypes.POINTER(ctypes.c_longlong), u32, u32, ctypes.c_int,
                                          u64, u64, u8p, u8p, u64]
    lib.warp_nearest_host_flag.restype = ctypes.c_uint
    return lib


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes: as dwords for the core, as uint8[rows, w, 4] for the model"""
    px = np.random.default_rng(seed).integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


# ---------------------------------------------------------------------------------- the warp with the NEAREST flag
def warp_run(lib, px, dwords, rect, out_size, matrix, flags, fill, och, mode, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    B = ow * oh * och
    out = np.full(BAND + a + B + BAND, GUARD, dtype=np.uint8)
    writes = np.zeros(out.size, dtype=np.uint8)
    m = (ctypes.c_longlong * 6)(*matrix)
    loads = lib.warp_nearest_host_run(dwords.ctypes.data_as(ctypes.POINTER(u32)), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, fill, och, mode, BASE + BAND + a,
                                      BASE, out.ctypes.data_as(u8p), writes.ctypes.data_as(u8p), out.size)
    what = (rect, out_size, matrix, flags, och, mode, a)
    assert 0 <= loads <= ow * oh, (what, loads)                       # one load per pixel at most, none outside the rectangle
    lo, hi = BAND + a, BAND + a + B
    assert np.all(writes[lo:hi] == 1) and not writes[:lo].any() and not writes[hi:].any(), what
    assert np.all(out[:lo] == GUARD) and np.all(out[hi:] == GUARD), what
    return loads, out[lo:hi]


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


def build_and_run(tmp_path, src, define, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-D" + define, "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "items ok" in r.stdout and "runtime error" not in r.stderr


def test_sanitized_stand_alone_program(tmp_path):
    """the same source with its own main(), built with -fsanitize=address,undefined and the sanitizer runtimes linked statically: a program
    of its own that needs nothing from its environment"""
    build_and_run(tmp_path, WARP_SRC, "WARP_NEAREST_HOST_MAIN", "warp_nearest_host_main")
