"""The walk warp_border_bytes makes for an item (qoi_amd/csrc/qoi_warp_border_core.h: tile -> work item -> positions -> the weights of the
item's sampling -> the first tap of each axis folded into the border's period, the others stepped from it -> the blend -> one rounding ->
store), compiled with g++ (tests/host/warp_border_host.cpp) and compared with the Python model qoi_amd/warp.py on the CPU, bit for bit:
every border, sampling, output channel count and mode, odd output addresses, rectangles of 1 x 1, 1 x 7, 7 x 1, 5 x 3 and 17 x 9, maps that
pad, turn, shear, lie hundreds of periods away and stand near +-2**56, so that the fold's ordinary path and its quotient estimate both run.
The fold alone also takes every (k, n, border) of the device sweep of tests/test_gpu_warp_fold.py (tests/warp_fold_cases.py: host_triples).
The staging outside the rectangle holds a sentinel and every load is checked to lie inside the rectangle; the loads are counted: exactly one
per tap that has a weight - none for a tap with the weight 0.  A guard band around the output stays untouched and every output byte is
written exactly once.  Items without a border flag walk warp_cubic_pixel / warp_pixel / warp_nearest through the same work item.  The same
source is also built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing
sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, cuint, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import warp

SRC = "warp_border_host.cpp"
SENTINEL = 0x5A
BORDERS = (warp.REFLECT, warp.REFLECT_101, warp.WRAP)
SAMPLINGS = (0, warp.NEAREST, warp.BICUBIC)
RECTS = ((3, 2, 1, 1), (3, 2, 1, 7), (3, 2, 7, 1), (3, 2, 5, 3), (3, 2, 17, 9))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "warp_border_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, i64p, u32, u32, cint, u64, u64, u8p, u8p, u64]),
        "warp_border_host_flags": (None, [ctypes.POINTER(cuint)]),
        "warp_border_host_fold": (cuint, [i64, u32, u32])})


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
    loads = lib.warp_border_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, m, fill, och, mode, *band.args)
    what = (rect, out_size, matrix, flags, och, mode, a)
    assert loads >= 0, (what, loads)                                  # no load outside the rectangle, no store outside the output or unaligned
    return loads, band.inside(what)


def loads_of(out_size, matrix, flags):
    """the taps that have a weight - under a folding border every one of them lies inside the rectangle: what the model says must be loaded"""
    ow, oh = out_size
    if flags & warp.NEAREST:
        return ow * oh
    a, b, c, d, e, f = matrix
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    axis = warp._cubic_axis if flags & warp.BICUBIC else warp._axis
    wx, wy = axis(a * U + b * V + c, 1, warp.WRAP)[1], axis(d * U + e * V + f, 1, warp.WRAP)[1]
    return int(((wy != 0).sum(axis=-1) * (wx != 0).sum(axis=-1)).sum())


def test_the_flags_and_the_fold_are_the_model_s(lib):
    got = (cuint * 3)()
    lib.warp_border_host_flags(got)
    assert tuple(got) == BORDERS == (64, 128, 256)
    top = 2 ** 40 - 1
    for border in BORDERS:
        for n in (1, 2, 3, 7, 640, 399_999_999):
            P = {warp.REFLECT: 2 * n, warp.REFLECT_101: max(2 * n - 2, 1), warp.WRAP: n}[border]
            ks = list(range(-40, 41)) + [top, -top, top - 1, 1 - top]
            ks += [s * (q * P + dk) for q in (1, 2, 3, 1000, top // P, top // P - 1) for dk in (-1, 0, 1, n - 1, n) for s in (1, -1)]
            ks = [k for k in ks if abs(k) <= top]
            want = warp.fold(np.array(ks, dtype=np.int64), n, border).tolist()
            for k, wk in zip(ks, want):
                assert lib.warp_border_host_fold(k, n, border) == wk, (border, n, k)


def test_the_fold_over_the_sweep_of_the_device_test(lib):
    """every (k, n, border) that tests/test_gpu_warp_fold.py folds on the device - the builder's own list -, through the host build of the same
    function: a failure there and not here is the device's code, one here is the arithmetic"""
    import warp_fold_cases
    triples = warp_fold_cases.host_triples()
    assert len(triples) == 3722 and {n for _, n, _ in triples} == set(warp_fold_cases.SIZES) and {b for _, _, b in triples} == set(BORDERS)
    assert min(k for k, _, _ in triples) < -(2 ** 39) + 64 and max(k for k, _, _ in triples) > 2 ** 39 - 64
    for border in BORDERS:
        for n in warp_fold_cases.SIZES:
            ks = [k for k, m, b in triples if m == n and b == border]
            want = warp.fold(np.array(ks, dtype=np.int64), n, border).tolist()
            for k, wk in zip(ks, want):
                assert lib.warp_border_host_fold(k, n, border) == wk, (border, n, k)


def maps_of(rect, out_size):
    _, _, cw, rh = rect
    S = warp.ONE
    return [(S, 0, -2 * S * 6, 0, S, -2 * S * 4),                                        # the rectangle padded: every position a pixel centre
            (0, -S, 2 * S * cw, S, 0, 0),                                                # a quarter turn: every tap inside
            warp.rotation((cw, rh), out_size, 30.0, 0.5), (S, 23000, -40000, -9000, S + 700, 12345),
            (S, 0, 2 * S * cw * 300 + 777, 0, S, -2 * S * rh * 500 - 999),                # hundreds of periods away
            (S, 0, 2 ** 56 - 1, 0, S, 1 - 2 ** 56), (S, 31, 1 - 2 ** 56, -17, S, 2 ** 56 - 1),   # near +-2**56
            (-2 ** 31, 2 ** 31 - 1, 2 ** 56 - 1, 3, -5, 1 - 2 ** 56)]                     # the limits


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("border", BORDERS)
def test_walk_against_the_model(lib, border, sampling):
    fill = 0x80C04020
    flags = border | sampling
    spared = 0
    for rect in RECTS:
        px, dwords = staged(rect, 2, 5)
        for out_size in ((19, 18), (33, 5)) if rect[2] == 17 else ((19, 18),):
            for matrix in maps_of(rect, out_size):
                want_loads = loads_of(out_size, matrix, flags)
                spared += want_loads < {0: 4, warp.NEAREST: 1, warp.BICUBIC: 16}[sampling] * out_size[0] * out_size[1]
                for och in (3, 4):
                    for mode in (warp.PLAIN, warp.ALPHA_WEIGHTED):
                        want = warp.warp(px[:, :, :och], rect, out_size, matrix, flags, fill, mode).reshape(-1)
                        for a in (0, 1, 3) if mode == warp.PLAIN else (7,):
                            loads, got = run(lib, px, dwords, rect, out_size, matrix, flags, fill, och, mode, a)
                            assert np.array_equal(got, want), (rect, out_size, matrix, och, mode, a, int(np.argmax(got != want)))
                            assert loads == want_loads, (rect, out_size, matrix, loads, want_loads)
    assert spared > 0 or sampling == warp.NEAREST                       # taps with the weight 0 were not read


@pytest.mark.parametrize("mode", [warp.PLAIN, warp.ALPHA_WEIGHTED])
def test_items_without_a_border_flag_walk_as_before(lib, mode):
    """the same work item serves every other item: the branch is the item's"""
    rect, fill = (3, 2, 11, 9), 0x80C04020
    px, dwords = staged(rect, 2, 9)
    m = warp.rotation((11, 9), (33, 18), 30.0)
    for och in (3, 4):
        for flags in (0, warp.REPLICATE, warp.NEAREST, warp.NEAREST | warp.REPLICATE, warp.BICUBIC, warp.BICUBIC | warp.REPLICATE):
            want = warp.warp(px[:, :, :och], rect, (33, 18), m, flags, fill, mode).reshape(-1)
            loads, got = run(lib, px, dwords, rect, (33, 18), m, flags, fill, och, mode, 1)
            assert np.array_equal(got, want), (och, flags)
            assert loads <= (1 if flags & warp.NEAREST else (16 if flags & warp.BICUBIC else 4)) * 33 * 18


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "WARP_BORDER_HOST_MAIN", tmp_path) == "warp_border_host: 3780 items ok\n"
