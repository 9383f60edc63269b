"""Label tensors as the source of qoimi_encode_tiles (QOIMI_TILE_LABELS*) in the model qoi_amd/tiles.py, no GPU: the conversion at the values
that decide it, the three properties the header states, the rejections in the order the calls look, and what stays as it was - the bits
that are still unknown, SRC_MASK, source_wrong."""
import numpy as np
import pytest

import labelimg
from qoi_amd import mode as _mode, nearest, tiles

DTYPES = (tiles.L_U8, tiles.L_I32, tiles.L_I64)
# the issue's list: the value and its byte
VALUES = [(0, 0), (1, 1), (254, 254), (255, 255), (256, 255), (-1, 0), (-100, 0), (2 ** 31 - 1, 255), (-2 ** 31, 0), (2 ** 32, 255), (2 ** 32 + 5, 255),
          (-2 ** 32 + 7, 0), (2 ** 63 - 1, 255), (-2 ** 63, 0)]


def plane(w, h, seed, dtype):
    """class indices 0..255 in regions with noise where they meet: the first channel of a label image, in the dtype's array"""
    return np.ascontiguousarray(labelimg.label_image(w, h, 4, seed)[:, :, 1].astype(tiles.LABEL_ARRAYS[dtype]))


def test_constants():
    assert (tiles.LABELS, tiles.LABELS_I32, tiles.LABELS_I64, tiles.LABELS_MASK) == (2048, 4096, 8192, 0x3800)
    assert tiles.SRC_MASK == 0x3F0 and tiles.LABELS_MASK & (tiles.SRC_MASK | tiles.FLIP_X | tiles.FLIP_Y | 4 | 8 | 1 << 10) == 0
    assert [tiles.label_flags(d) for d in DTYPES] == [2048, 2048 | 4096, 2048 | 8192]
    assert [tiles.label_bytes(5, 3, tiles.label_flags(d)) for d in DTYPES] == [15, 60, 120]
    with pytest.raises(ValueError):
        tiles.label_flags(3)


def test_the_conversion_at_the_values_that_decide_it():
    for dtype, lo, hi in ((tiles.L_U8, 0, 255), (tiles.L_I32, -2 ** 31, 2 ** 31 - 1), (tiles.L_I64, -2 ** 63, 2 ** 63 - 1)):
        mine = [(v, b) for v, b in VALUES if lo <= v <= hi]
        assert len(mine) == {tiles.L_U8: 4, tiles.L_I32: 9, tiles.L_I64: 14}[dtype]
        A = np.array([[v for v, _ in mine]], dtype=tiles.LABEL_ARRAYS[dtype])
        B = tiles.labels_to_bytes(A, tiles.label_flags(dtype))
        assert B.shape == (1, len(mine), 4) and B.dtype == np.uint8
        assert B[0, :, 0].tolist() == [b for _, b in mine], dtype
        assert np.array_equal(B[:, :, 1], B[:, :, 0]) and np.array_equal(B[:, :, 2], B[:, :, 0]) and np.all(B[:, :, 3] == 255)
    # the high dword of an int64 takes part: what an int32 view of the low dword would give is another byte
    assert np.array([2 ** 32 + 5], np.int64).astype(np.int32)[0] == 5 and dict(VALUES)[2 ** 32 + 5] == 255
    assert np.array([-2 ** 32 + 7], np.int64).astype(np.int32)[0] == 7 and dict(VALUES)[-2 ** 32 + 7] == 0
    with pytest.raises(ValueError):
        tiles.labels_to_bytes(np.zeros((2, 2), np.int32), tiles.label_flags(tiles.L_I64))          # the array of another dtype
    with pytest.raises(ValueError):
        tiles.labels_to_bytes(np.zeros((2, 2, 1), np.uint8), tiles.LABELS)                           # not one plane
    with pytest.raises(ValueError):
        tiles.labels_to_bytes(np.zeros((2, 2), np.uint8), 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_property_a_values_in_range_come_back(dtype):
    """the factor-1 tile of a whole image holds the tensor in its first channel - what decode_tensors(NEAREST, I64, HW) at the image's size
    reads (nearest.nearest at the same size is the identity)"""
    A = plane(23, 37, 3, dtype)
    assert A.min() == 0 and A.max() == 255
    T = tiles.tile(A, (0, 0, 0, 23, 37, 1, tiles.label_flags(dtype)), 4)
    back = nearest.nearest(T, (0, 0, 23, 37), (23, 37))[:, :, 0].astype(np.int64)
    assert np.array_equal(back, A.astype(np.int64))


def test_property_b_a_u8_label_tile_is_the_byte_tile_over_B():
    A = plane(37, 23, 5, tiles.L_U8)
    B = tiles.labels_to_bytes(A, tiles.LABELS)
    for och in (0, 3, 4):
        for mode, f in ((tiles.PLAIN, 1), (tiles.ALPHA_WEIGHTED, 1), (tiles.NEAREST, 1), (tiles.NEAREST, 5), (tiles.NEAREST, 64), (tiles.MODE, 1), (tiles.MODE, 3), (tiles.MODE, 16)):
            for flips in range(4):
                for rect in ((0, 0, 37, 23), (3, 5, 30, 17)):
                    t = (0,) + rect + (f,)
                    assert np.array_equal(tiles.tile(A, t + (tiles.LABELS | flips,), och, mode), tiles.tile(B, t + (flips,), och, mode)), (och, mode, f, flips, rect)
    # the other dtypes give the same tile of the same values
    for dtype in (tiles.L_I32, tiles.L_I64):
        t = (0, 3, 5, 30, 17, 3)
        assert np.array_equal(tiles.tile(A.astype(tiles.LABEL_ARRAYS[dtype]), t + (tiles.label_flags(dtype) | 1,), 3, tiles.MODE),
                              tiles.tile(B, t + (1,), 3, tiles.MODE))


@pytest.mark.parametrize("f", [2, 4, 8, 16])
def test_property_c_a_mode_tile_is_filter_mode_of_the_factor_1_image(f):
    w, h = 64, 48
    A = plane(w, h, 11, tiles.L_I64)
    B = tiles.labels_to_bytes(A, tiles.label_flags(tiles.L_I64))
    assert np.array_equal(B, tiles.tile(A, (0, 0, 0, w, h, 1, tiles.label_flags(tiles.L_I64)), 4))           # what the factor-1 pack holds
    got = tiles.tile(A, (0, 0, 0, w, h, f, tiles.label_flags(tiles.L_I64)), 4, tiles.MODE)
    assert np.array_equal(got, _mode.mode(B, (0, 0, w, h), (w // f, h // f)))
    census = {}
    assert np.array_equal(got, labelimg.loop(B, (0, 0, 0, w, h, f, 0), 4, labelimg.MODE, census))
    assert census.get("unique", 0) > 0                                                                       # votes were decided, not only constants kept


def test_the_vote_on_grey_pixels_is_the_vote_on_b():
    """4 x class 9, 4 x class 3 and a centre of class 0: the lowest b of the winners; with the centre a winner, the centre"""
    A = np.array([[9, 3, 9], [3, 0, 3], [9, 3, 9]], np.int32)
    assert tiles.tile(A, (0, 0, 0, 3, 3, 3, tiles.label_flags(tiles.L_I32)), 3, tiles.MODE).reshape(-1).tolist() == [3, 3, 3]
    A[1, 1] = 9
    assert tiles.tile(A, (0, 0, 0, 3, 3, 3, tiles.label_flags(tiles.L_I32)), 4, tiles.MODE).reshape(-1).tolist() == [9, 9, 9, 255]
    A[:] = [[9, 3, 9], [3, 400, 3], [9, 3, -7]]                                                                # saturated before the vote: 255 and 0
    assert tiles.tile(A, (0, 0, 0, 3, 3, 3, tiles.label_flags(tiles.L_I32)), 3, tiles.NEAREST).reshape(-1).tolist() == [255, 255, 255]


def test_rejections_in_order():
    I64 = tiles.label_flags(tiles.L_I64)
    cases = [
        (tiles.LABELS_I32, 1, tiles.PLAIN, "without LABELS"), (tiles.LABELS_I64 | tiles.SRC, 2, tiles.PLAIN, "without LABELS"), (12288, 1, None, "without LABELS"),
        (tiles.LABELS | 12288, 1, tiles.NEAREST, "12288"), (tiles.LABELS | 12288 | tiles.SRC_CHW, 2, tiles.PLAIN, "12288"),
        (tiles.LABELS | tiles.SRC, 1, tiles.NEAREST, "together with a SRC"), (I64 | tiles.SRC_BYTES, 2, tiles.PLAIN, "together with a SRC"),
        (I64, 2, tiles.PLAIN, "never averaged"), (tiles.LABELS, 64, tiles.ALPHA_WEIGHTED, "never averaged"),
    ]
    for flags, f, mode, cause in cases:
        assert cause in tiles.label_wrong(flags, f, mode), (flags, f, mode, tiles.label_wrong(flags, f, mode))
    for flags in (0, 3, tiles.SRC, tiles.source_flags(tiles.F32, tiles.CHW)):
        assert tiles.label_wrong(flags, 2, tiles.PLAIN) == ""                                                # no label bit: not this function's
    for dtype in DTYPES:
        for mode, f in ((tiles.PLAIN, 1), (tiles.ALPHA_WEIGHTED, 1), (tiles.NEAREST, 64), (tiles.MODE, 16), (None, 7)):
            assert tiles.label_wrong(tiles.label_flags(dtype) | 3, f, mode) == ""
    # behind the checks that exist: source_wrong comes first, and keeps its answers
    assert tiles.source_wrong(tiles.LABELS | tiles.SRC_CHW) == "a SRC_* bit without SRC" and tiles.source_wrong(tiles.LABELS | tiles.SRC, 2) == "a tensor source takes factor 1 only"
    assert tiles.source_wrong(I64, 64) == "" and tiles.source_wrong(12288) == ""
    A = np.zeros((8, 8), np.int64)
    for t, mode in (((0, 0, 0, 8, 8, 2, I64), tiles.PLAIN), ((0, 0, 0, 8, 8, 2, I64), tiles.ALPHA_WEIGHTED), ((0, 0, 0, 8, 8, 1, I64 | tiles.SRC), tiles.NEAREST),
                    ((0, 0, 0, 8, 8, 1, tiles.LABELS_I64), tiles.NEAREST), ((0, 0, 0, 8, 8, 32, I64), tiles.MODE)):
        with pytest.raises(ValueError):
            tiles.tile(A, t, 4, mode)


def test_size_with_the_bits():
    for dtype in DTYPES:
        for f in (1, 2, 16, 64):                                       # size has no mode: a label tile of any factor has a size
            for ch_in in (3, 4):
                for ch in (0, 3, 4):
                    t = (7, 3, 2, 30, 17, f, tiles.label_flags(dtype) | 2)
                    assert tiles.size(37, 23, ch_in, t, ch) == tiles.size(37, 23, ch_in, t[:6] + (2,), ch) != (0, 0, 0)       # no size changes
    for flags in (tiles.LABELS | 4, tiles.LABELS | 8, tiles.LABELS | 1 << 10, tiles.LABELS | 1 << 31, tiles.LABELS | 1 << 14,      # bits that stay unknown
                  tiles.LABELS_I32, tiles.LABELS_I64, 12288, tiles.LABELS | 12288, tiles.LABELS | tiles.SRC, tiles.label_flags(tiles.L_I32) | tiles.SRC_F16):
        assert tiles.size(4, 4, 4, (0, 0, 0, 4, 4, 1, flags), 0) == (0, 0, 0), flags
    for flags in (4, 8, 1 << 10, 1 << 31):
        assert tiles.size(4, 4, 4, (0, 0, 0, 4, 4, 1, flags), 0) == (0, 0, 0)


def test_plan_and_work_items():
    I32, I64 = tiles.label_flags(tiles.L_I32), tiles.label_flags(tiles.L_I64)
    descs = [(37, 23, 3), (64, 48, 4)]
    ts = [(0, 0, 0, 37, 23, 1, I32), (1, 0, 0, 64, 48, 2, I64 | 1), (1, 16, 16, 32, 32, 16, I64)]
    plain = [t[:6] + (t[6] & 3,) for t in ts]
    for channels in (0, 3, 4):
        assert tiles.plan(descs, ts, channels, 0) == tiles.plan(descs, plain, channels, 0)                   # the slots are the byte call's
    with pytest.raises(ValueError):
        tiles.plan(descs, ts[:2] + [plain[2]], 0, 0)                                                         # some but not all
    with pytest.raises(ValueError):
        tiles.plan(descs, ts + [(1, 0, 0, 1, 1, 1, I32)], 0, 0)                                              # one image, two dtypes
    assert tiles.label_tiles(37, 23, 1, 3, tiles.PLAIN) == tiles.ingest_tiles(37, 23) == 1 and tiles.label_tiles(1025, 3, 1, 4, tiles.MODE) == 4
    assert tiles.label_tiles(64, 48, 2, 4, tiles.MODE) == tiles.select_tiles(64, 48, 2, 4, tiles.MODE) == 3
    assert tiles.label_tiles(64, 48, 16, 3, tiles.MODE) == tiles.select_tiles(64, 48, 16, 3, tiles.MODE) == 3            # 12 pixels of 64 lanes
    assert tiles.label_tiles(37, 23, 64, 4, tiles.NEAREST) == 1
