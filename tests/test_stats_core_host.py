"""The tile loop the GPU kernel runs (qoi_amd/csrc/qoi_stats_core.h: tile, lane -> pixels -> a lane's share -> 64-bit totals) compiled with g++
(tests/host/stats_host.cpp) and compared with the Python model qoi_amd/pixelstats.py on the CPU, tile by tile as stats_reduce walks a region:
regions of one pixel, one row, one column, TILE_PX - 1, TILE_PX and TILE_PX + 1 pixels, an odd interior rectangle of a wider image (the memory
policy counts every load outside the region), every number of tiles per workgroup, and white runs whose square sums pass 2^32 above the lane
and inside it.  The same source is built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its
own: nothing sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cuint, i64, u32, u32p, u64, u64p, ull
from qoi_amd import pixelstats as ps

SRC = "stats_host.cpp"
T = ps.TILE_PX


class Acc(ctypes.Structure):
    """qoi_stats_core.h: StatsAcc"""
    _fields_ = [("sum", ctypes.c_uint64 * 4), ("sum_sq", ctypes.c_uint64 * 4), ("opaque", ctypes.c_uint64), ("transparent", ctypes.c_uint64),
                ("grey", ctypes.c_uint64), ("mn", ctypes.c_uint32 * 4), ("mx", ctypes.c_uint32 * 4), ("first", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    accp = ctypes.POINTER(Acc)
    assert ctypes.sizeof(Acc) == 128
    return hostbuild.shared(SRC, tmp_path_factory, {
        "stats_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, accp, u32p, u64p]),
        "stats_host_init": (None, [accp]),
        "stats_host_flags": (cuint, [accp, u64]),
        "stats_host_tiles": (ull, [u32, u32]),
        "stats_host_tile_px": (cuint, [])})


def run(lib, px, x, y, cw, ch, flags, per_wg, with_hist):
    """one region of the staged pixels px uint8[rows, w, 4]; the staging ends with the region's last pixel.  Returns (fields as
    pixelstats.stats gives them, histogram or None, the largest square sum a lane held)"""
    w = px.shape[1]
    dwords = np.ascontiguousarray(px).view(np.uint32).reshape(-1)[:w * (y + ch - 1) + x + cw]
    acc = Acc()
    lib.stats_host_init(ctypes.byref(acc))
    hist = np.zeros(1024, dtype=np.uint32) if with_hist else None
    lane_max = ctypes.c_uint64(0)
    walked = lib.stats_host_run(dwords.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), dwords.size, w, x, y, cw, ch, flags, per_wg, ctypes.byref(acc),
                                hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if with_hist else None, ctypes.byref(lane_max))
    assert walked == cw * ch, ("a load outside the region" if walked < 0 else "pixels walked", walked, (x, y, cw, ch))
    got = {"pixels": cw * ch, "sum": tuple(acc.sum), "sum_sq": tuple(acc.sum_sq), "min": tuple(acc.mn), "max": tuple(acc.mx), "first": acc.first,
           "opaque_pixels": acc.opaque, "transparent_pixels": acc.transparent, "grey_pixels": acc.grey,
           "flags": lib.stats_host_flags(ctypes.byref(acc), cw * ch)}
    return got, hist.reshape(4, 256) if with_hist else None, lane_max.value


def staged(w, rows, seed, alpha=None):
    px = np.random.default_rng(seed).integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    if alpha is not None:
        px[..., 3] = np.random.default_rng(seed + 1).choice(np.array(alpha, dtype=np.uint8), size=(rows, w))
    return px


def test_constants(host_lib):
    assert host_lib.stats_host_tile_px() == T == 1024
    for (cw, ch) in [(1, 1), (T - 1, 1), (T, 1), (T + 1, 1), (1, T + 1), (130, 70), (19999, 20000)]:
        assert host_lib.stats_host_tiles(cw, ch) == ps.tiles(cw, ch) == -(-cw * ch // T)


def test_small_regions_and_tile_edges(host_lib):
    shapes = [(1, 1), (2, 1), (1, 2), (5, 1), (1, 7), (3, 3), (T - 1, 1), (T, 1), (T + 1, 1), (1, T + 1), (T // 4, 4), (T // 4 + 1, 4), (341, 3)]
    assert {cw * ch for cw, ch in shapes} >= {1, T - 1, T, T + 1}
    for k, (cw, ch) in enumerate(shapes):
        x, y = 3, 2
        px = staged(cw + 5, y + ch, k, alpha=(0, 255, 255, 7))
        for flags in range(4):
            for with_hist in (False, True):
                got, hist, _ = run(host_lib, px, x, y, cw, ch, flags, 1 + k % 3, with_hist)
                assert got == ps.stats(px, (x, y, cw, ch, flags)), (cw, ch, flags)
                if with_hist:
                    assert np.array_equal(hist, ps.hist(px, (x, y, cw, ch))), (cw, ch)


def test_odd_interior_rectangle_of_a_wider_image(host_lib):
    """129 x 67 at (1, 3) of 135 x 70: 9 tiles; any load of a pixel outside the rectangle is counted by the memory policy and fails run()"""
    px = staged(135, 70, 11)
    px[10:40, 20:90, :3] = px[10:40, 20:90, :1]                # a grey patch
    want, want_hist = ps.stats(px, (1, 3, 129, 67)), ps.hist(px, (1, 3, 129, 67))
    assert ps.tiles(129, 67) == 9 and 0 < want["grey_pixels"] < want["pixels"]
    for per_wg in (1, 2, 4, 9, 100):
        got, hist, _ = run(host_lib, px, 1, 3, 129, 67, 0, per_wg, True)
        assert got == want and np.array_equal(hist, want_hist), per_wg
    for flags in range(1, 4):
        got, _, _ = run(host_lib, px, 1, 3, 129, 67, flags, 3, False)
        assert got == ps.stats(px, (1, 3, 129, 67, flags))


def test_flags_of_the_core(host_lib):
    white = np.full((6, 40, 4), 255, dtype=np.uint8)
    cases = [(white, ps.CONSTANT | ps.OPAQUE | ps.GREY)]
    d = white.copy(); d[-1, -1, 1] = 0
    cases.append((d, ps.OPAQUE))
    d = white.copy(); d[3, 20, 3] = 254
    cases.append((d, ps.GREY))
    d = np.zeros((6, 40, 4), dtype=np.uint8); d[..., 1] = 9
    cases.append((d, ps.CONSTANT | ps.TRANSPARENT))
    for px, flags in cases:
        got, _, _ = run(host_lib, px, 0, 0, 40, 6, 0, 1, False)
        assert got["flags"] == flags == ps.stats(px, (0, 0, 40, 6))["flags"]


def test_white_run_through_one_workgroup(host_lib):
    """More than 66 052 all-white pixels through ONE workgroup's range: 66 052 is where 255^2 * n passes 2^32.  300 x 260 = 78 000 pixels are 77
    tiles; with 77 tiles per workgroup the 256 lanes hold 308 or fewer pixels each and their fold - everything above the lane - passes 2^32:
    5 071 950 000.  The sums are exact."""
    px = np.full((260, 300, 4), 255, dtype=np.uint8)
    assert 300 * 260 > 66052 and 65025 * 66052 > 2 ** 32 > 65025 * 66051
    got, hist, lane_max = run(host_lib, px, 0, 0, 300, 260, 0, 77, True)
    assert got["sum_sq"] == (65025 * 78000,) * 4 and got["sum_sq"][0] > 2 ** 32 > lane_max
    assert got["sum"] == (255 * 78000,) * 4 and got["opaque_pixels"] == got["grey_pixels"] == 78000 and got["transparent_pixels"] == 0
    assert got["flags"] == ps.CONSTANT | ps.OPAQUE | ps.GREY and got == ps.stats(px, (0, 0, 300, 260))
    assert np.all(hist[:, 255] == 78000) and int(hist.sum()) == 4 * 78000


def test_a_lane_passes_32_bits(host_lib):
    """A lane holds 4 pixels of every tile of its workgroup's range: 4200 x 4100 white pixels through one workgroup are 16 817 tiles, 67 268
    pixels per lane, and the LANE's square sum passes 2^32 - the reason it is 64 bits wide (qoi_stats_core.h states the bounds)."""
    px = np.full((4100, 4200, 4), 255, dtype=np.uint8)
    n = 4200 * 4100
    assert 4 * ps.tiles(4200, 4100) > 66052
    got, _, lane_max = run(host_lib, px, 0, 0, 4200, 4100, 0, ps.tiles(4200, 4100), False)
    assert lane_max > 2 ** 32
    assert got["sum_sq"] == (65025 * n,) * 4 and got["sum"] == (255 * n,) * 4 and got["opaque_pixels"] == n


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "STATS_HOST_MAIN", tmp_path) == "stats_host: 72 regions ok\n"
