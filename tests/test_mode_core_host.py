"""The walk tensor_mode makes for an item of qoimi_decode_tensors with QOIMI_FILTER_MODE (qoi_amd/csrc/qoi_mode_core.h: tile -> work item ->
lane of an output pixel -> the lane's pixels of the cell -> the meetings of the lanes -> the packed word's maximum -> the sink of
qoi_tensor_core.h), compiled with g++ -Wall -Werror (tests/host/mode_host.cpp, which walks the lanes of a tile in a loop) and compared with
the Python models qoi_amd/mode.py and qoi_amd/tensors.py on the CPU, bit for bit: every lg from 0 to 6 - the split's own and forced higher
ones -, cells from 1 x 1 to 16 x 16 at ratios that are no whole numbers (cell widths alternate), outputs whose last group of lanes ends in
the middle of a tile (groups that straddle the end of an item), rectangles at odd offsets, flips, both channel counts, dtypes and layouts.
A guard band around the output stays untouched, every output byte is written exactly once, every load is a dword of the rectangle - one
per pixel of every cell -, every store a whole aligned one inside the output.  The same source is also built as a stand-alone program with
the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import numpy as np
import pytest

import hostbuild
import mode_cases as MC
from hostbuild import f32p, i64, u32, u32p, u64, u8p
from qoi_amd import mode, tensors
from qoi_amd.tensors import CHW, F16, F32, HW, HWC, I32, I64, U8

SRC = "mode_host.cpp"
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FORMATS = [(U8, HWC), (I64, HW), (I32, CHW), (F16, HWC), (F32, CHW), (U8, HW)]
# (w, h) of the staged image, classes, the rectangle, the outputs - with the lg the split chooses for each
CASES = [((1, 1), 2, (0, 0, 1, 1), [((1, 1), 0), ((7, 5), 0)]),
         ((37, 29), 3, (0, 0, 37, 29), [((9, 7), 3), ((50, 7), 1), ((37, 29), 0), ((19, 15), 0), ((13, 29), 0)]),    # cells 5 x 5, 1 x 5, 1 x 1, 2 x 2, 3 x 1
         ((37, 29), 4, (3, 5, 31, 23), [((7, 20), 2), ((4, 3), 4), ((3, 3), 5), ((2, 2), 6), ((50, 41), 0)]),       # 5 x 2, 8 x 8, 11 x 8, 16 x 12
         ((70, 45), 5, (0, 0, 70, 45), [((16, 11), 3), ((6, 4), 6)]),                                                # 5 x 5, 12 x 12
         ((70, 45), 5, (3, 1, 64, 44), [((4, 3), 6), ((7, 3), 6), ((9, 11), 3)]),                                    # 16 x 15, 10 x 15, 8 x 4
         ((70, 45), 2, (5, 0, 63, 45), [((5, 45), 2), ((63, 3), 2), ((11, 9), 3)]),                                  # 13 x 1, 1 x 15, 6 x 5
         ((64, 48), 3, (0, 0, 64, 48), [((4, 3), 6)])]                                                               # 16 x 16: L = 64, four pixels a lane


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "mode_host_run": (i64, [u32p, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, f32p, f32p, u64, u64, u8p, u8p, u64]),
        "mode_host_tiles": (u64, [u32] * 4),
        "mode_host_split": (u32, [u32] * 4),
        "mode_host_first": (u32, [u32] * 3),
        "mode_host_range": (u32, [u32] * 3),
        "mode_host_word": (u64, [u32] * 3),
        "mode_host_pick": (u32, [u64]),
        "mode_host_max_ratio": (u32, []),
        "mode_host_max_size": (u32, [])})


def staged(w, rows, classes, seed):
    """rows x w staged pixels of 4 bytes, every one a colour of the palette: as dwords for the core, as uint8[rows, w, 4] for the model"""
    px = MC.label_map(w, rows, 4, classes, seed)
    return px, np.ascontiguousarray(px).view(np.uint32).reshape(-1)


def cell_pixels(cw, rh, ow, oh):
    return sum(mode.cell(X, cw, ow)[1] for X in range(ow)) * sum(mode.cell(Y, rh, oh)[1] for Y in range(oh))


def run(lib, px, dwords, rect, out_size, flags, och, lg, f, a):
    x, y, cw, rh = rect
    ow, oh = out_size
    dtype, layout, scale, bias = f
    elem = tensors.elem(dtype)
    B = ow * oh * (1 if layout == HW else och) * elem
    band = hostbuild.Banded(B, a)
    s, b = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(bias, np.float32)
    loads = lib.mode_host_run(dwords.ctypes.data_as(u32p), dwords.size, px.shape[1], x, y, cw, rh, ow, oh, flags, och, lg, dtype, layout,
                              s.ctypes.data_as(f32p), b.ctypes.data_as(f32p), *band.args)
    what = (rect, out_size, flags, och, lg, dtype, layout, a)
    assert loads == cell_pixels(cw, rh, ow, oh), (what, loads)           # one load per pixel of every cell, none outside the rectangle, no bad store
    return band.inside(what)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[2][2:]))
def test_walk_against_the_models(host_lib, case):
    (w, h), classes, rect, outs = case
    x, y, cw, rh = rect
    px, dwords = staged(w, y + rh, classes, w * 131 + h + classes)        # the staging ends with the rectangle's last row
    checked = 0
    for out_size, want_lg in outs:
        ow, oh = out_size
        sp = host_lib.mode_host_split(cw, rh, ow, oh)
        assert (sp & 255, sp >> 8) == mode.split(cw, rh, ow, oh) and sp & 255 == want_lg, (rect, out_size, sp)
        assert host_lib.mode_host_tiles(cw, rh, ow, oh) == mode.tiles(cw, rh, ow, oh)
        for lg in sorted({want_lg, min(want_lg + 1, 6), 6}):              # the split's, and more lanes than the cell needs: lanes that hold nothing
            for k, (och, flags) in enumerate([(4, 0), (3, 3), (4, 2), (3, 1)]):
                P = mode.mode(px, rect, out_size, flags, och=och)     # (the staged alpha votes, och 3 drops it afterwards)
                assert np.array_equal(P, MC.brute(px, rect, out_size, flags, och=och))
                dtype, layout = FORMATS[(k + lg + ow) % len(FORMATS)]
                f = tensors.fmt(dtype, layout) if dtype in (U8, I32, I64) else (dtype, layout, *IMAGENET)
                want = tensors.convert(P, f).view(np.uint8).reshape(-1)
                elem = tensors.elem(dtype)
                for a in sorted({0, (3 * elem) % 16 if elem > 1 else 7}):
                    got = run(host_lib, px, dwords, rect, out_size, flags, och, lg, f, a)
                    assert np.array_equal(got, want), (rect, out_size, och, flags, lg, dtype, layout, a, int(np.argmax(got != want)) // elem)
                    checked += 1
    assert checked >= len(outs) * 4


def test_every_lg_and_groups_that_straddle_the_end_of_an_item():
    seen = set()
    straddle = 0
    for (_, _, rect, outs) in CASES:
        for (ow, oh), lg in outs:
            seen.add(lg)
            if ((ow * oh) << lg) % 256 != 0:
                straddle += 1                                            # the last tile ends with lanes behind the item's last pixel
    assert seen == set(range(7)) and straddle >= 10
    nx = {mode.cell(X, 37, 9)[1] for X in range(9)}
    assert nx == {4, 5}                                                  # a ratio that is no whole number: cell widths alternate
    assert {mode.cell(X, 64, 7)[1] for X in range(7)} == {9, 10} and mode.cell(0, 64, 4) == (0, 16)


def test_the_arithmetic_of_the_core(host_lib):
    assert host_lib.mode_host_max_ratio() == mode.MAX_RATIO == 16 and host_lib.mode_host_max_size() == mode.MAX_SIZE == 16384
    for n_src, n_out in [(1, 1), (2, 41), (14, 23), (41, 2), (16384, 1024), (1, 16384), (16384, 16384), (16383, 16384), (16384, 16383), (1000, 3000), (4097, 299), (37, 9), (64, 7)]:
        for Z in sorted({0, 1, n_out // 2, n_out - 2, n_out - 1} & set(range(n_out))):
            assert host_lib.mode_host_first(Z, n_src, n_out) == mode.first(Z, n_src, n_out)
            got = host_lib.mode_host_range(Z, n_src, n_out)
            assert (got & 0xFFFF, got >> 16) == mode.cell(Z, n_src, n_out), (n_src, n_out, Z)
        assert host_lib.mode_host_first(n_out, n_src, n_out) == n_src
    assert 2 * 16384 * 16384 + 16384 - 1 < 2 ** 32 and 2 * 16384 < 2 ** 32          # what keeps first in one 32-bit division
    # the word: the count beats the centre, the centre beats the key, a lower key beats a higher one; pick gives the pixel back
    word, pick = host_lib.mode_host_word, host_lib.mode_host_pick
    px = [0xFF000003, 0xFF07C801, 0x8006C801, 0x00000000, 0xFFFFFFFF, 0x12345678]
    for p in px:
        for count in (1, 2, 255, 256):
            for centre in (0, 1):
                wd = word(count, centre, p)
                assert pick(wd) == p and wd >> 33 == count and (wd >> 32) & 1 == centre and wd > 0
    assert word(2, 0, 0xFFFFFFFF) > word(1, 1, 0) and word(256, 0, 0xFFFFFFFF) > word(255, 1, 0)
    assert word(3, 1, 0xFFFFFFFF) > word(3, 0, 0)
    key = lambda p: MC.key([p & 255, p >> 8 & 255, p >> 16 & 255, p >> 24])       # noqa: E731
    for p in px:
        for o in px:
            if key(p) < key(o):
                assert word(5, 0, p) > word(5, 0, o), (hex(p), hex(o))
    for cw, rh, ow, oh in [(1, 1, 1, 1), (64, 48, 4, 3), (16384, 3, 1024, 3), (3, 16384, 3, 1024), (1024, 768, 224, 224), (16384, 16384, 1024, 1024), (7, 5, 16384, 16384)]:
        sp = host_lib.mode_host_split(cw, rh, ow, oh)
        assert (sp & 255, sp >> 8) == mode.split(cw, rh, ow, oh)
        assert host_lib.mode_host_tiles(cw, rh, ow, oh) == mode.tiles(cw, rh, ow, oh)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "MODE_HOST_MAIN", tmp_path) == "mode_host: 768 items ok\n"
