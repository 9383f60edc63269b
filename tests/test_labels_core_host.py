"""The walk tensor_nearest makes for an item of qoimi_decode_tensors with QOIMI_FILTER_NEAREST (qoi_amd/csrc/qoi_nearest_core.h: tile -> work
item -> (X, Y) -> (k, r) -> one load -> the sink of qoi_tensor_core.h with the integer dtypes and the one-plane layout), compiled with g++
-Wall -Werror (tests/host/nearest_host.cpp) and compared with the Python models qoi_amd/nearest.py and qoi_amd/tensors.py on the CPU: sources
of 1 x 1, 1 x 130, 37 x 29 and 70 x 45, rectangles with odd corners, outputs that enlarge, reduce by 100 and more and hit exact boundaries
(2 to 41, 14 to 23), all four flips, both output channel counts, every dtype and layout.  The output equals the model, a guard band around it
stays untouched, every output byte is written exactly once, every load is a dword of the rectangle - exactly one per output pixel -, every
store is a whole aligned one inside the output.  The same source is also built as a stand-alone program with the address and
undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import numpy as np
import pytest

import hostbuild
from hostbuild import f32p, i64, u32, u32p, u64, u8p
from qoi_amd import nearest, tensors
from qoi_amd.tensors import BF16, CHW, F16, F32, HW, HWC, I32, I64, U8

SRC = "nearest_host.cpp"
DTYPES = (U8, F16, BF16, F32, I32, I64)
LAYOUTS = (HWC, CHW, HW)
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
# (w, h) of the staged image, the rectangle, the outputs
CASES = [((1, 1), (0, 0, 1, 1), [(1, 1), (7, 5)]),
         ((1, 130), (0, 3, 1, 127), [(1, 1), (1, 127), (3, 257)]),                                  # 127 rows to one: reduced by more than 100
         ((37, 29), (3, 5, 31, 23), [(50, 41), (31, 23), (1, 1)]),                                  # 2050 pixels: nine tiles, the last partial
         ((37, 29), (1, 1, 2, 14), [(41, 23)]),                                                     # 2 to 41 and 14 to 23: centres on cell boundaries
         ((70, 45), (5, 3, 63, 41), [(3, 2), (63, 41), (126, 82)]),
         ((70, 45), (7, 1, 60, 40), [(20, 8)])]                                                     # whole factors 3 and 5


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "nearest_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, f32p, f32p, u64, u64, u8p, u8p, u64]),
        "nearest_host_tiles": (u64, [u32, u32, u32]),
        "nearest_host_index": (u32, [u32, u32, u32]),
        "nearest_host_elem": (u32, [u32]),
        "nearest_host_max_size": (u32, [])})


def staged(w, rows, seed):
    """rows x w staged pixels of 4 bytes: as dwords for the core, as uint8[rows, w, 4] for the model"""
    px = np.random.default_rng(seed).integers(0, 256, size=(rows, w, 4), dtype=np.uint8)
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def run(lib, px, dwords, rect, out_size, flags, och, f, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    dtype, layout, scale, bias = f
    elem = tensors.elem(dtype)
    B = ow * oh * (1 if layout == HW else och) * elem
    band = hostbuild.Banded(B, a)
    s, b = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(bias, np.float32)
    loads = lib.nearest_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, och, dtype, layout,
                                 s.ctypes.data_as(f32p), b.ctypes.data_as(f32p), *band.args)
    what = (rect, out_size, flags, och, dtype, layout, a)
    assert loads == ow * oh, (what, loads)                            # one load per pixel, none outside the rectangle, no bad store
    return band.inside(what)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1][2:]))
def test_walk_against_the_models(host_lib, case):
    (w, h), rect, outs = case
    x, y, cw, rh = rect
    px, dwords = staged(w, y + rh, w * 131 + h)                     # the staging ends with the rectangle's last row
    checked = 0
    for out_size in outs:
        assert host_lib.nearest_host_tiles(cw, *out_size) == nearest.tiles(*out_size)
        for och in (3, 4):
            for flags in range(4):
                P = nearest.nearest(px[:, :, :och], rect, out_size, flags)
                for dtype in DTYPES:
                    for layout in LAYOUTS:
                        f = tensors.fmt(dtype, layout) if dtype in (U8, I32, I64) else (dtype, layout, *IMAGENET)
                        want = tensors.convert(P, f).view(np.uint8).reshape(-1)
                        elem = tensors.elem(dtype)
                        for a in sorted({0, elem, (3 * elem) % 16 if elem > 1 else 7}):
                            got = run(host_lib, px, dwords, rect, out_size, flags, och, f, a)
                            assert np.array_equal(got, want), (rect, out_size, och, flags, dtype, layout, a, int(np.argmax(got != want)) // elem)
                            checked += 1
    assert checked >= 4 * 2 * 6 * 3 * 2


def test_index_tiles_and_element_sizes(host_lib):
    assert host_lib.nearest_host_max_size() == nearest.MAX_SIZE == 16384
    assert [host_lib.nearest_host_elem(d) for d in DTYPES] == [1, 2, 2, 4, 4, 8] == [tensors.elem(d) for d in DTYPES]
    for n_src, n_out in [(1, 1), (2, 41), (14, 23), (41, 2), (16384, 1), (1, 16384), (16384, 16384), (16383, 16384), (16384, 16383), (1000, 3000), (4097, 299)]:
        want = nearest.index(n_src, n_out)
        for X in sorted({0, 1, n_out // 2, n_out - 2, n_out - 1} & set(range(n_out))):
            assert host_lib.nearest_host_index(X, n_src, n_out) == want[X] < n_src, (n_src, n_out, X)
    assert (2 * 16383 + 1) * 16384 < 2 ** 29 and 2 * 16384 < 2 ** 32                   # what keeps the index in one 32-bit division
    for ow, oh in [(1, 1), (16, 16), (257, 1), (50, 41), (16384, 16384)]:
        assert host_lib.nearest_host_tiles(7, ow, oh) == -(-ow * oh // 256)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "NEAREST_HOST_MAIN", tmp_path) == "nearest_host: 5904 items ok\n"
