"""The walk the GPU kernel makes (qoi_amd/csrc/qoi_bilinear_core.h: work item -> columns and rows -> weighted sums -> D -> pixel -> stores)
compiled with g++ (tests/host/bilinear_host.cpp) and compared with the Python model qoi_amd/bilinear.py on the CPU, tile by tile as
bilinear_filter walks an item over staged uint8[rows, w, 4] whose last row is the item's last row: both output channel counts, both modes, all
four flag values, every alignment of the output, outputs of one pixel and of more than one tile, every number of lanes per pixel, the ratio of
32 in both axes, enlargements.  The output equals bilinear.bilinear, a guard band around it stays untouched, every output byte is written
exactly once, no load leaves the staged rows, every tap with a weight is loaded once and every store is naturally aligned.  Single output
pixels of geometries no array can hold - sizes at the product limit of 2**30, positions beyond 2**32 on the line - are compared with Python
`int` arithmetic over pixels made from their index.  The same source is built as a stand-alone program with the address and
undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, i64, u32, u32p, u64, u64p, u8p, ull, ullp
from qoi_amd import bilinear

SRC = "bilinear_host.cpp"


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "bilinear_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, cint, u64, u64, u8p, u8p, u64, ullp]),
        "bilinear_host_pixel": (i64, [u64, u32, u32, u32, u32, u32, u32, u32, cint, u32, u32, u32p, u64p]),
        "bilinear_host_synth": (u32, [u64]),
        "bilinear_host_split": (None, [u32, u32, u32p, u32p]),
        "bilinear_host_taps": (u32, [u32, u32]),
        "bilinear_host_first": (u32, [u32, u32, u32]),
        "bilinear_host_tent": (u32, [u32, u32, u32, u32]),
        "bilinear_host_tiles": (ull, [u32, u32, u32])})


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
    loads = lib.bilinear_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, och, mode, *band.args, ctypes.byref(tiles))
    what = (och, mode, a, flags, cw, rh, ow, oh)
    assert loads >= ow * oh, (what, loads)                          # (negative: a load outside the staged rows, a store out of bounds or misaligned)
    assert tiles.value == bilinear.tiles(cw, ow, oh) == lib.bilinear_host_tiles(cw, ow, oh), what
    return tiles.value, loads, band.inside(what)


def check(lib, cw, rh, ow, oh, och, mode, alignments=range(16), flag_values=range(4), x=3, y=2, seed=0):
    px, dwords = staged(cw + x + 2, y + rh, seed + cw * 1000 + rh)          # the staging ends with the item's last row
    tiles = 0
    for flags in flag_values:
        want = bilinear.bilinear(px[:, :, :och], (x, y, cw, rh), (ow, oh), flags, mode).reshape(-1)
        for a in alignments:
            tiles, loads, got = run(lib, px, dwords, x, y, cw, rh, ow, oh, flags, och, mode, a)
            assert np.array_equal(got, want), (och, mode, a, flags, cw, rh, ow, oh, int(np.argmax(got != want)))
            # every sample with a weight of every output pixel is loaded once: no two lanes share one, none is left out
            assert loads == int(np.count_nonzero(bilinear.weights(cw, ow))) * int(np.count_nonzero(bilinear.weights(rh, oh)))
    return tiles


@pytest.mark.parametrize("mode", [bilinear.PLAIN, bilinear.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_walk_against_the_model(host_lib, och, mode):
    # one pixel out of one and of many; identity; reductions with 1, 2, 4 lanes; enlargements; down in x with up in y and the reverse
    for (cw, rh, ow, oh) in [(1, 1, 1, 1), (11, 9, 1, 1), (11, 9, 11, 9), (12, 8, 3, 2), (11, 9, 3, 2), (11, 9, 5, 4), (5, 3, 13, 7), (1, 1, 4, 4), (3, 1, 2, 1),
                             (11, 3, 4, 9), (3, 11, 9, 4), (21, 5, 3, 2)]:
        check(host_lib, cw, rh, ow, oh, och, mode)


@pytest.mark.parametrize("mode", [bilinear.PLAIN, bilinear.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_the_ratio_of_32(host_lib, och, mode):
    """128 x 64 -> 4 x 2: 64 taps in both axes under the inner pixels, sixteen lanes of four columns; 191 -> 6 just below the cap; 45 -> 3
    eight lanes"""
    assert bilinear.taps(128, 4) == 64 and bilinear.split(128, 4) == (4, 4) and int(np.count_nonzero(bilinear.weights(128, 4)[1])) == 64
    assert bilinear.split(191, 6) == (4, 4) and bilinear.split(45, 3)[0] == 3
    check(host_lib, 128, 64, 4, 2, och, mode, alignments=(0, 5), flag_values=(0, 3))
    check(host_lib, 191, 95, 6, 3, och, mode, alignments=(1,), flag_values=(1,))
    check(host_lib, 45, 31, 3, 1, och, mode, alignments=(2,), flag_values=(2,))


@pytest.mark.parametrize("och", [3, 4])
def test_more_than_one_tile(host_lib, och):
    """130 x 70 -> 37 x 23: 851 pixels of 2 lanes, 7 tiles; 37 x 23 -> 80 x 50: 4000 pixels of one lane, 16 tiles"""
    assert check(host_lib, 130, 70, 37, 23, och, bilinear.ALPHA_WEIGHTED, alignments=(0, 1, 7), flag_values=(0, 1, 2, 3), x=0, y=0) == 7
    assert check(host_lib, 37, 23, 80, 50, och, bilinear.PLAIN, alignments=(3,), flag_values=(2,)) == 16


def test_first_tent_split_taps_and_tiles(host_lib):
    lg, c = ctypes.c_uint32(), ctypes.c_uint32()
    for ow in list(range(1, 9)) + [37, 224]:
        for cw in list(range(1, 32 * min(ow, 8) + 1)) + [32 * ow, 32 * ow - 1]:
            w = bilinear.weights(cw, ow)
            assert int(np.count_nonzero(w, axis=1).max()) <= bilinear.taps(cw, ow) == host_lib.bilinear_host_taps(cw, ow) <= 64, (cw, ow)
            host_lib.bilinear_host_split(cw, ow, ctypes.byref(lg), ctypes.byref(c))
            assert (lg.value, c.value) == bilinear.split(cw, ow) and lg.value <= 4 and c.value <= 4 and c.value << lg.value >= bilinear.taps(cw, ow), (cw, ow)
            for X in {0, ow // 2, ow - 1}:
                k0 = host_lib.bilinear_host_first(X, cw, ow)
                assert k0 == bilinear.first(X, cw, ow) == int(np.nonzero(w[X])[0][0]), (cw, ow, X)
                for k in {0, k0, min(cw - 1, k0 + 1), cw - 1}:
                    assert host_lib.bilinear_host_tent(X, k, cw, ow) == int(w[X, k]), (cw, ow, X, k)
    # where the numerator of the first sample is negative, zero and just positive; sizes whose line passes 2**32
    for (Z, n_src, n_out) in [(0, 1, 1), (0, 32, 1), (0, 64, 2), (1, 64, 2), (0, 1, 1000), (999, 1, 1000), (1, 3, 2), (0, 3, 2), (2 ** 24 - 1, 2 ** 29 - 1, 2 ** 24),
                              (2 ** 23, 2 ** 29 - 1, 2 ** 24), (2 ** 29 - 2, 3, 2 ** 29 - 1), (0, 3, 2 ** 29 - 1), (12345, 2 ** 29 - 1, 2 ** 29 - 1)]:
        assert host_lib.bilinear_host_first(Z, n_src, n_out) == bilinear.first(Z, n_src, n_out), (Z, n_src, n_out)
    for (cw, ow, oh) in [(1, 1, 1), (130, 37, 23), (32, 1, 1), (5, 30000, 30000), (4096, 128, 1 << 18), (1, 1 << 15, (1 << 15) - 1)]:
        assert host_lib.bilinear_host_tiles(cw, ow, oh) == bilinear.tiles(cw, ow, oh), (cw, ow, oh)


def synth(i):
    z = ((i + 1) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    z ^= z >> 29
    return (z >> 16) & 0xFFFFFFFF


def int_pixel(w, x, y, cw, rh, ow, oh, X, Y, weighted):
    """(pixel as a dword, [N_r, N_g, N_b, N_a, M_r, M_g, M_b, Wx, Wy]) in Python integers over the synthetic staged pixels"""
    def taps(Z, n_src, n_out):
        rad, o = 2 * max(n_src, n_out), (2 * Z + 1) * n_src
        mid = o // (2 * n_out)
        return [(k, rad - abs(o - (2 * k + 1) * n_out)) for k in range(max(0, mid - 70), min(n_src, mid + 70)) if rad - abs(o - (2 * k + 1) * n_out) > 0]

    cols, rows = taps(X, cw, ow), taps(Y, rh, oh)
    Wx, Wy = sum(t for _, t in cols), sum(t for _, t in rows)
    N, M = [0] * 4, [0] * 3
    for r, ty in rows:
        for k, tx in cols:
            px = synth((y + r) * w + x + k)
            ch = [(px >> (8 * c)) & 255 for c in range(4)]
            for c in range(4):
                N[c] += ty * tx * ch[c]
            for c in range(3):
                M[c] += ty * tx * ch[c] * ch[3]
    D = Wx * Wy
    out = [(n + D // 2) // D for n in N]
    if weighted and N[3] > 0:
        out[:3] = [(m + N[3] // 2) // N[3] for m in M]
    return out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24, N + M + [Wx, Wy], len(cols) * len(rows)


# (cw, rh, ow, oh): the product limit with the ratio of 32 in both axes at once; the limit when enlarging; a line of 2**54 positions in x,
# reducing by just under 32 and enlarging by 2**27
LIMIT = [(32768, 32767, 1024, 1024), (1, 1, 32768, 32767), (2 ** 29 - 1, 2, 2 ** 24, 1), (3, 2, 2 ** 29 - 1, 2), (32767, 1, 32768, 32767)]


@pytest.mark.parametrize("weighted", [0, 1])
def test_single_pixels_at_the_limits(host_lib, weighted):
    assert synth(0) == host_lib.bilinear_host_synth(0) and synth(2 ** 31 + 12345) == host_lib.bilinear_host_synth(2 ** 31 + 12345)
    largest = [0, 0, 0, 0]
    for (cw, rh, ow, oh) in LIMIT:
        assert max(cw, ow) * max(rh, oh) < 2 ** 30 <= (max(cw, ow) + 1) * (max(rh, oh) + 1) and cw <= 32 * ow and rh <= 32 * oh
        x, y, w = 5, 3, cw + 7
        stage_px = w * (y + rh)                                           # the staging ends with the item's last row
        for X in sorted({0, ow // 2, ow - 1}):
            for Y in sorted({0, oh - 1}):
                px, sums = ctypes.c_uint32(0), (ctypes.c_uint64 * 9)()
                loads = host_lib.bilinear_host_pixel(stage_px, w, x, y, cw, rh, ow, oh, weighted, X, Y, ctypes.byref(px), sums)
                want, want_sums, taps = int_pixel(w, x, y, cw, rh, ow, oh, X, Y, weighted)
                if not weighted:
                    want_sums[4:7] = [0, 0, 0]
                assert loads == taps and list(sums) == want_sums and px.value == want, ((cw, rh, ow, oh), X, Y, loads, taps)
                rad = 4 * max(cw, ow) * max(rh, oh)
                largest = [max(a, b) for a, b in zip(largest, (rad, sums[7] * sums[8], max(sums[:4]), max(sums[4:7])))]
    print("largest rad_x * rad_y %d, D %d, N %d, M %d" % tuple(largest))
    assert 2 ** 31 < largest[0] < 2 ** 32 and 2 ** 40 < largest[1] < 2 ** 44 and 2 ** 46 < largest[2] < 2 ** 52
    if weighted:
        assert 2 ** 52 < largest[3] < 2 ** 60


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "BILINEAR_HOST_MAIN", tmp_path) == "bilinear_host: 1152 items ok\n"
