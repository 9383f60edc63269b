"""The walk the GPU kernel makes (qoi_amd/csrc/qoi_cubic_core.h: tile -> normalised column and row tables -> work item -> signed sums -> clamped
pixel -> the tensor store of qoi_tensor_core.h as u8 HWC) compiled with g++ (tests/host/bicubic_host.cpp) and compared with the Python model
qoi_amd/bicubic.py on the CPU, tile by tile as tensor_cubic walks an item over staged uint8[rows, w, 4] whose last row is the item's last row:
both output channel counts, both modes, all four flag values, every alignment of the output, outputs of one pixel and of more than one tile,
every number of lanes per pixel, the ratio of 16 in both axes, enlargements.  The output equals bicubic.bicubic, a guard band around it stays
untouched, every output byte is written exactly once, no load leaves the staged rows, every tap with a weight is loaded once, every store is
naturally aligned, the tables of a tile fit the kernel's LDS and hold exactly the tile's columns and rows - each normalised once per tile.
Single output pixels at the size limits are compared with Python `int` arithmetic over pixels made from their index.  The same source is
built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is
loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, cintp, i64, i64p, u32, u32p, u64, u8p, ull, ullp
from qoi_amd import bicubic

SRC = "bicubic_host.cpp"


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "bicubic_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, cint, u64, u64, u8p, u8p, u64, ullp, ullp]),
        "bicubic_host_pixel": (i64, [u64, u32, u32, u32, u32, u32, u32, u32, cint, u32, u32, u32p, i64p]),
        "bicubic_host_synth": (u32, [u64]),
        "bicubic_host_split": (None, [u32, u32, u32p, u32p]),
        "bicubic_host_taps": (u32, [u32, u32]),
        "bicubic_host_first": (u32, [u32, u32, u32]),
        "bicubic_host_weight": (i64, [u32, u32, u32, u32]),
        "bicubic_host_norm": (None, [u32, u32, u32, u32, cintp]),
        "bicubic_host_tiles": (ull, [u32, u32, u32])})


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes, a fifth of them transparent, one run of transparent pixels and some of 0 and of 255 throughout (hard
    edges: the lobes overshoot): as dwords for the core, as uint8[rows, w, 4] for the model"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    px[:, :, 3][rng.integers(0, 5, size=(rows, w)) == 0] = 0
    px[rows // 2:, : w // 2, 3] = 0
    hard = rng.integers(0, 6, size=(rows, w))
    px[hard == 0] = 0
    px[hard == 1] = 255
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, x, y, cw, rh, ow, oh, flags, och, mode, a):
    """one item written at BASE + BAND + a; returns (tiles walked, loads, output bytes); asserts guards, write counts and the normalisations"""
    band = hostbuild.Banded(ow * oh * och, a)
    tiles, norm = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    loads = lib.bicubic_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, och, mode, *band.args,
                                 ctypes.byref(tiles), ctypes.byref(norm))
    what = (och, mode, a, flags, cw, rh, ow, oh)
    assert loads >= ow * oh, (what, loads)                          # (negative: a load outside the staged rows, a store out of bounds or misaligned, a table not written exactly)
    assert tiles.value == bicubic.tiles(cw, ow, oh) == lib.bicubic_host_tiles(cw, ow, oh), what
    assert norm.value == sum(len(c) + len(r) for c, r in (bicubic.tile(t, cw, ow, oh) for t in range(tiles.value))), what
    return tiles.value, loads, band.inside(what)


def check(lib, cw, rh, ow, oh, och, mode, alignments=range(16), flag_values=range(4), x=3, y=2, seed=0):
    px, dwords = staged(cw + x + 2, y + rh, seed + cw * 1000 + rh)          # the staging ends with the item's last row
    tiles = 0
    for flags in flag_values:
        want = bicubic.bicubic(px[:, :, :och], (x, y, cw, rh), (ow, oh), flags, mode).reshape(-1)
        for a in alignments:
            tiles, loads, got = run(lib, px, dwords, x, y, cw, rh, ow, oh, flags, och, mode, a)
            assert np.array_equal(got, want), (och, mode, a, flags, cw, rh, ow, oh, int(np.argmax(got != want)))
            # every sample with a weight of every output pixel is loaded once: no two lanes share one, none is left out
            assert loads == int(np.count_nonzero(bicubic.weights(cw, ow))) * int(np.count_nonzero(bicubic.weights(rh, oh)))
    return tiles


@pytest.mark.parametrize("mode", [bicubic.PLAIN, bicubic.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_walk_against_the_model(host_lib, och, mode):
    # one pixel out of one and of many; identity; reductions with 1 to 16 lanes; enlargements; down in x with up in y and the reverse
    for (cw, rh, ow, oh) in [(1, 1, 1, 1), (11, 9, 1, 1), (11, 9, 11, 9), (12, 8, 3, 2), (11, 9, 3, 2), (11, 9, 5, 4), (5, 3, 13, 7), (1, 1, 4, 4), (3, 1, 2, 1),
                             (11, 3, 4, 9), (3, 11, 9, 4), (21, 5, 3, 2), (7, 6, 5, 4)]:
        check(host_lib, cw, rh, ow, oh, och, mode, alignments=(0, 1, 2, 3, 7, 12))
    assert {bicubic.split(cw, ow)[0] for cw, ow in ((11, 11), (7, 5), (11, 5), (21, 3), (11, 1))} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("mode", [bicubic.PLAIN, bicubic.ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_the_ratio_of_16(host_lib, och, mode):
    """128 x 64 -> 8 x 4: sixteen lanes of four columns, 64 taps in both axes under the inner pixels (the two outermost round to q = 0 and
    are not loaded); 95 -> 6 just below the cap; 23 -> 3 eight lanes"""
    assert bicubic.taps(128, 8) == 64 and bicubic.split(128, 8) == (4, 4) and int(np.count_nonzero(bicubic.kernel(128, 8)[3])) == 64
    assert bicubic.split(95, 6) == (4, 4) and bicubic.split(23, 3)[0] == 3
    check(host_lib, 128, 64, 8, 4, och, mode, alignments=(0, 5), flag_values=(0, 3))
    check(host_lib, 95, 47, 6, 3, och, mode, alignments=(1,), flag_values=(1,))
    check(host_lib, 23, 15, 3, 1, och, mode, alignments=(2,), flag_values=(2,))


@pytest.mark.parametrize("och", [3, 4])
def test_more_than_one_tile(host_lib, och):
    """130 x 70 -> 37 x 23: 851 pixels of 4 lanes, 14 tiles whose columns wrap; 37 x 23 -> 80 x 50: 4000 pixels of one lane, 16 tiles of four rows;
    1 x 300 -> 1 x 290: tiles of 256 rows of one pixel; 5 x 3 -> 300 x 2: a tile narrower than a row"""
    assert check(host_lib, 130, 70, 37, 23, och, bicubic.ALPHA_WEIGHTED, alignments=(0, 1, 7), flag_values=(0, 1, 2, 3), x=0, y=0) == 14
    assert check(host_lib, 37, 23, 80, 50, och, bicubic.PLAIN, alignments=(3,), flag_values=(2,)) == 16
    assert check(host_lib, 1, 300, 1, 290, och, bicubic.ALPHA_WEIGHTED, alignments=(1,), flag_values=(3,)) == 2
    assert check(host_lib, 5, 3, 300, 2, och, bicubic.PLAIN, alignments=(2,), flag_values=(1,)) == 3
    assert len(bicubic.tile(0, 1, 1, 290)[1]) == 256 and len(bicubic.tile(0, 5, 300, 2)[0]) == 256 and bicubic.tile(1, 5, 300, 2)[0][44] == 0
    # a tile of 256 rows of 64 taps fills the row table, sixteen pixels of 64 taps the column table
    px, dwords = staged(3, 16 * 260, 77)
    assert run(host_lib, px, dwords, 0, 0, 1, 16 * 260, 1, 260, 0, och, 0, 0)[0] == 2
    assert np.array_equal(run(host_lib, px, dwords, 0, 0, 1, 16 * 260, 1, 260, 0, och, 0, 0)[2],
                          bicubic.bicubic(px[:, :, :och], (0, 0, 1, 16 * 260), (1, 260)).reshape(-1))


def test_first_weight_norm_split_taps_and_tiles(host_lib):
    lg, c = ctypes.c_uint32(), ctypes.c_uint32()
    q = (ctypes.c_int * 64)()
    for ow in list(range(1, 9)) + [37, 224]:
        for cw in list(range(1, 16 * min(ow, 8) + 1)) + [16 * ow, 16 * ow - 1]:
            ker, w = bicubic.kernel(cw, ow), bicubic.weights(cw, ow)
            assert bicubic.taps(cw, ow) == host_lib.bicubic_host_taps(cw, ow) <= 64, (cw, ow)
            host_lib.bicubic_host_split(cw, ow, ctypes.byref(lg), ctypes.byref(c))
            assert (lg.value, c.value) == bicubic.split(cw, ow) and lg.value <= 4 and c.value <= 4 and c.value << lg.value >= bicubic.taps(cw, ow), (cw, ow)
            for X in {0, ow // 2, ow - 1}:
                k0 = host_lib.bicubic_host_first(X, cw, ow)
                assert k0 == bicubic.first(X, cw, ow), (cw, ow, X)
                for k in {0, k0, min(cw - 1, k0 + 1), cw - 1}:
                    assert host_lib.bicubic_host_weight(X, k, cw, ow) == int(ker[X, k]), (cw, ow, X, k)
                t = bicubic.taps(cw, ow)
                host_lib.bicubic_host_norm(X, cw, ow, t, q)
                assert list(q[:t]) == [int(w[X, k]) if k < cw else 0 for k in range(k0, k0 + t)], (cw, ow, X)
    for (Z, n_src, n_out) in [(0, 1, 1), (0, 16, 1), (0, 32, 2), (1, 32, 2), (0, 1, 1000), (999, 1, 1000), (1, 3, 2), (0, 3, 2), (1023, 16384, 1024), (512, 16383, 1024),
                              (16383, 3, 16384), (0, 3, 16384), (12345, 16384, 16384)]:
        assert host_lib.bicubic_host_first(Z, n_src, n_out) == bicubic.first(Z, n_src, n_out), (Z, n_src, n_out)
        t = bicubic.taps(n_src, n_out)
        host_lib.bicubic_host_norm(Z, n_src, n_out, t, q)
        k0, w = bicubic.first(Z, n_src, n_out), bicubic.weights(n_src, n_out, [Z])[0]
        assert list(q[:t]) == [int(w[k]) if k < n_src else 0 for k in range(k0, k0 + t)], (Z, n_src, n_out)
    for (cw, ow, oh) in [(1, 1, 1), (130, 37, 23), (16, 1, 1), (5, 16384, 16384), (4096, 256, 16384), (1, 16384, 16383)]:
        assert host_lib.bicubic_host_tiles(cw, ow, oh) == bicubic.tiles(cw, ow, oh), (cw, ow, oh)


def synth(i):
    z = ((i + 1) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    z ^= z >> 29
    return (z >> 16) & 0xFFFFFFFF


def int_pixel(w, x, y, cw, rh, ow, oh, X, Y, weighted):
    """(pixel as a dword, [N_r, N_g, N_b, N_a, M_r, M_g, M_b], taps loaded) in Python integers over the synthetic staged pixels"""
    cols = [(k, int(q)) for k, q in enumerate(bicubic.weights(cw, ow, [X])[0]) if q]
    rows = [(r, int(q)) for r, q in enumerate(bicubic.weights(rh, oh, [Y])[0]) if q]
    N, M = [0] * 4, [0] * 3
    for r, qy in rows:
        for k, qx in cols:
            px = synth((y + r) * w + x + k)
            ch = [(px >> (8 * c)) & 255 for c in range(4)]
            for c in range(4):
                N[c] += qy * qx * ch[c]
            for c in range(3):
                M[c] += qy * qx * ch[c] * ch[3]
    out = [min(255, max(0, (n + 2 ** 29) >> 30)) for n in N]
    if weighted and N[3] > 0:
        out[:3] = [min(255, max(0, (m + N[3] // 2) // N[3])) for m in M]
    return out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24, N + (M if weighted else [0, 0, 0]), len(cols) * len(rows)


# (cw, rh, ow, oh): the size limit with the ratio of 16 in both axes at once; the limit when enlarging; mixed axes
LIMIT = [(16384, 16384, 1024, 1024), (1, 1, 16384, 16384), (16383, 2, 1024, 16384), (3, 16384, 16384, 1024), (16384, 3, 16384, 7)]


@pytest.mark.parametrize("weighted", [0, 1])
def test_single_pixels_at_the_limits(host_lib, weighted):
    assert synth(0) == host_lib.bicubic_host_synth(0) and synth(2 ** 31 + 12345) == host_lib.bicubic_host_synth(2 ** 31 + 12345)
    largest = [0, 0]
    for (cw, rh, ow, oh) in LIMIT:
        assert max(cw, rh, ow, oh) == 16384 and cw <= 16 * ow and rh <= 16 * oh
        x, y, w = 5, 3, cw + 7
        stage_px = w * (y + rh)                                           # the staging ends with the item's last row
        for X in sorted({0, ow // 2, ow - 1}):
            for Y in sorted({0, oh - 1}):
                px, sums = ctypes.c_uint32(0), (ctypes.c_longlong * 7)()
                loads = host_lib.bicubic_host_pixel(stage_px, w, x, y, cw, rh, ow, oh, weighted, X, Y, ctypes.byref(px), sums)
                want, want_sums, taps = int_pixel(w, x, y, cw, rh, ow, oh, X, Y, weighted)
                assert loads == taps and list(sums) == want_sums and px.value == want, ((cw, rh, ow, oh), X, Y, loads, taps)
                largest = [max(a, b) for a, b in zip(largest, (max(abs(s) for s in sums[:4]), max(abs(s) for s in sums[4:7])))]
    print("largest |N| %d, |M| %d" % tuple(largest))
    assert 2 ** 36 < largest[0] < 2 ** 40 and (not weighted or 2 ** 43 < largest[1] < 2 ** 48)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "BICUBIC_HOST_MAIN", tmp_path) == "bicubic_host: 896 items ok\n"
