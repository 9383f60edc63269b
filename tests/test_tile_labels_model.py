"""qoi_amd/tiles.py: tile in QOIMI_TILE_NEAREST and QOIMI_TILE_MODE against the definition as a direct loop over blocks (tests/labelimg.py:
loop): partial edge blocks, a column one pixel wide, a single pixel, 3-channel sources (alpha 255 takes part), och 3 from a 4-channel
source whose colours differ in alpha alone, the flips; the identities with mode.mode and nearest.nearest where the factor divides both
sides; factor 1 and constant blocks; what stays rejected; the work items of the kernel.  No GPU."""
import numpy as np
import pytest

from labelimg import PALETTE, label_image, loop
from qoi_amd import mode, nearest, tiles

FACTORS = (2, 3, 5, 13, 16)


def test_the_values():
    assert (tiles.NEAREST, tiles.MODE, tiles.MODE_MAX_FACTOR) == (4, 5, 16) and (tiles.PLAIN, tiles.ALPHA_WEIGHTED) == (0, 1)


@pytest.mark.parametrize("sch", [3, 4])
def test_partial_edge_blocks_and_every_way_a_vote_is_decided(sch):
    S = label_image(37, 29, sch, seed=sch)
    census = {}
    for f in FACTORS:
        assert 37 % f and 29 % f                                   # partial blocks at the right and at the bottom edge
        for k, t in enumerate([(0, 0, 0, 37, 29, f, 0), (0, 3, 5, 31, 23, f, 1), (0, 1, 2, 35, 26, f, 2), (0, 36, 0, 1, 29, f, 3)]):
            for channels in (0, 3, 4):
                for m in (tiles.NEAREST, tiles.MODE):
                    want = loop(S, t, channels, m, census if channels == 0 else None)
                    got = tiles.tile(S, t, channels, m)
                    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (sch, t, channels, m)
    # the image is built so that every way a vote is decided happens, counted by the definition
    assert census["unique"] > 100 and census["centre"] > 20 and census["lowest"] > 5, census


def test_the_planted_block_is_a_tie_the_lowest_key_decides():
    S = label_image(37, 29, 4, seed=4)
    block = S[0:3, 0:3].reshape(-1, 4)
    assert sorted(np.unique(block, axis=0, return_counts=True)[1].tolist()) == [1, 4, 4]
    a, b, c = PALETTE[6], PALETTE[3], PALETTE[0]
    assert np.array_equal(block[4], c) and mode.key(a) < mode.key(b)
    assert np.array_equal(tiles.tile(S, (0, 0, 0, 3, 3, 3), 0, tiles.MODE)[0, 0], a)
    assert np.array_equal(tiles.tile(S, (0, 0, 0, 3, 3, 3), 0, tiles.NEAREST)[0, 0], c)
    assert tiles.tile(S, (0, 0, 0, 3, 3, 3), 0, tiles.PLAIN)[0, 0].tolist() not in PALETTE.tolist()     # the box average invents a class


@pytest.mark.parametrize("sch", [3, 4])
def test_a_column_and_a_single_pixel(sch):
    col = label_image(1, 130, sch, seed=9)
    one = label_image(1, 1, sch, seed=1)
    for m in (tiles.NEAREST, tiles.MODE):
        for f in (1, 2, 3, 5, 13, 16) + ((33, 64) if m == tiles.NEAREST else ()):
            for flags in range(4):
                for channels in (0, 3, 4):
                    for t in [(0, 0, 0, 1, 130, f, flags), (0, 0, 3, 1, 127, f, flags)]:
                        assert np.array_equal(tiles.tile(col, t, channels, m), loop(col, t, channels, m)), (t, channels, m)
                    assert np.array_equal(tiles.tile(one, (0, 0, 0, 1, 1, f, flags), channels, m), loop(one, (0, 0, 0, 1, 1, f, flags), channels, m))
                    assert np.array_equal(tiles.tile(one, (0, 0, 0, 1, 1, f, flags), 4, m)[0, 0], list(one[0, 0]) + [255] * (4 - sch))


def test_colours_that_differ_in_alpha_alone_vote_apart():
    """two 2 x 2 blocks of (1, 2, 3) at alpha 255 and 128 and of (7, 0, 0): the alphas vote apart - in the second block (1, 2, 3) has two
    votes without alpha, one and one with it, so (7, 0, 0) wins alone - and och 3 drops alpha only after the vote"""
    S = np.zeros((2, 4, 4), dtype=np.uint8)
    S[0, 0], S[0, 1], S[1, 0], S[1, 1] = PALETTE[1], PALETTE[2], PALETTE[2], PALETTE[3]
    S[0, 2], S[0, 3], S[1, 2], S[1, 3] = PALETTE[1], PALETTE[2], PALETTE[3], PALETTE[3]       # (1,2,3) twice if alpha is ignored, class 7 twice: class 7 wins alone
    t = (0, 0, 0, 4, 2, 2)
    assert tiles.tile(S, t, 4, tiles.MODE).tolist() == [[PALETTE[2].tolist(), PALETTE[3].tolist()]]
    assert tiles.tile(S, t, 3, tiles.MODE).tolist() == [[[1, 2, 3], [7, 0, 0]]]
    assert np.array_equal(tiles.tile(S, t, 3, tiles.MODE), loop(S, t, 3, tiles.MODE))
    # a 3-channel source: alpha 255 everywhere takes part and changes nothing
    assert tiles.tile(np.ascontiguousarray(S[:, :, :3]), t, 4, tiles.MODE).tolist() == [[[1, 2, 3, 255], [7, 0, 0, 255]]]


@pytest.mark.parametrize("f", [2, 4, 8, 16])
def test_where_the_factor_divides_both_sides_the_tile_is_the_serving_sides_filter(f):
    S = label_image(70, 45, 4, seed=f)
    x, y, cw, ch = 3, 5, 64, 32
    assert cw % f == 0 and ch % f == 0
    for flags in range(4):
        t = (0, x, y, cw, ch, f, flags)
        assert np.array_equal(tiles.tile(S, t, 0, tiles.MODE), mode.mode(S, (x, y, cw, ch), (cw // f, ch // f), flags))
        assert np.array_equal(tiles.tile(S, t, 0, tiles.NEAREST), nearest.nearest(S, (x, y, cw, ch), (cw // f, ch // f), flags))
    assert not np.array_equal(tiles.tile(S, (0, x, y, cw, ch, f, 0), 0, tiles.MODE), tiles.tile(S, (0, x, y, cw, ch, f, 0), 0, tiles.NEAREST))


def test_factor_1_is_the_rectangle_and_a_constant_block_gives_the_constant():
    S = label_image(37, 29, 4, seed=2)
    for m in (tiles.NEAREST, tiles.MODE):
        assert np.array_equal(tiles.tile(S, (0, 3, 5, 30, 20, 1), 0, m), S[5:25, 3:33])
        assert np.array_equal(tiles.tile(S, (0, 3, 5, 30, 20, 1, 3), 3, m), S[5:25, 3:33][::-1, ::-1, :3])
        C = np.empty((29, 37, 4), dtype=np.uint8)
        C[:] = PALETTE[2]
        for f in FACTORS:
            got = tiles.tile(C, (0, 0, 0, 37, 29, f), 0, m)
            assert got.shape == (-(-29 // f), -(-37 // f), 4) and (got == PALETTE[2]).all()


def test_what_the_model_rejects():
    S = label_image(70, 45, 4, seed=3)
    for f in (17, 33, 64):
        with pytest.raises(ValueError):
            tiles.tile(S, (0, 0, 0, 70, 45, f), 0, tiles.MODE)
        assert tiles.tile(S, (0, 0, 0, 70, 45, f), 0, tiles.NEAREST).shape == (-(-45 // f), -(-70 // f), 4)
    for m in (2, 3, 6, -1):
        with pytest.raises(ValueError):
            tiles.tile(S, (0, 0, 0, 70, 45, 2), 0, m)
    assert tiles.size(70, 45, 4, (0, 0, 0, 70, 45, 64), 0) == (2 * 1 * 4, 2, 1)                  # the modes change no size


def test_the_work_items_of_tile_select():
    for f in range(1, 65):
        assert tiles.select_split(f, tiles.NEAREST) == (0, 1)
    assert [tiles.select_split(f, tiles.MODE) for f in (1, 2, 3, 4, 5, 8, 13, 16)] == [(0, 1), (0, 4), (2, 3), (2, 4), (3, 4), (4, 4), (6, 3), (6, 4)]
    for f in range(1, 17):
        lg, c = tiles.select_split(f, tiles.MODE)
        assert (lg, c) == mode.split(f, f, 1, 1) and c << lg >= f * f and (lg == 0 or 4 << (lg - 1) < f * f)
        # the lanes of a block hold every pixel of it once, whatever is left of the block at an edge
        for nx, ny in [(f, f), (1, f), (f, 1), (f - 1 or 1, f), (1, 1)]:
            held = [p for l in range(1 << lg) for p in mode.held(l, lg, nx, ny)]
            assert sorted(held) == sorted((k, r) for r in range(ny) for k in range(nx))
    with pytest.raises(ValueError):
        tiles.select_split(17, tiles.MODE)
    with pytest.raises(ValueError):
        tiles.select_split(2, tiles.PLAIN)
    for m in (tiles.NEAREST, tiles.MODE):
        for och in (3, 4):
            assert tiles.select_tiles(37, 29, 1, och, m) == -(-(-(-37 * 29 * och // 16)) // 256)
    assert tiles.select_tiles(1024, 1024, 2, 4, tiles.MODE) == 1024 and tiles.select_tiles(1024, 1024, 3, 4, tiles.MODE) == -(-342 * 342 * 4 // 256)
    assert tiles.select_tiles(1024, 1024, 16, 4, tiles.MODE) == 64 * 64 * 64 // 256 and tiles.select_tiles(1024, 1024, 64, 4, tiles.NEAREST) == 1
    assert tiles.select_tiles(37, 29, 13, 3, tiles.MODE) == 3 and tiles.select_tiles(37, 29, 13, 3, tiles.NEAREST) == 1
