"""tests/resize_window.py - the windowed statement of the area filter that the device tests of large rectangles use (tests/test_gpu_resize_wide.py)
- held byte-equal to the normative model, qoi_amd/resize.py: resize; its lane sums against resize.share; the box reduction beside it against
thumbs.thumbnail; and the `wide` items of the device module reach the sums they are there for.  No GPU, no library."""
import numpy as np
import pytest

import resize_window as rw
from qoi_amd import resize, thumbs
from qoi_amd.resize import ALPHA_WEIGHTED, PLAIN
from gpu_calls import standard
from gpu_pack import MIXED_SHAPES
from model_cases import gradient_image as image


def same(D, rect, out, flags, mode):
    got, want = rw.resized(D, rect, out, flags, mode), resize.resize(D, rect, out, flags, mode)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (D.shape, rect, out, flags, mode)


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_standard_items_over_the_mixed_shapes(och, mode):
    """the items of the device tests of the small pack: identities, 64 taps, odd rectangles, upscales, down in x with up in y"""
    seen = set()
    for i, (w, h, _) in enumerate(MIXED_SHAPES):
        D = image(w, h, och, i)
        for (_, x, y, cw, rh, ow, oh, flags) in standard(i, w, h, i):
            same(D, (x, y, cw, rh), (ow, oh), flags, mode)
            seen.add(flags)
    assert seen == {0, 1, 2, 3}


def test_random_items():
    rng = np.random.default_rng(65)
    count = {(och, mode, flags): 0 for och in (3, 4) for mode in (PLAIN, ALPHA_WEIGHTED) for flags in range(4)}
    up = down = 0
    for n in range(400):
        och, mode, flags = (3, 4)[n & 1], (PLAIN, ALPHA_WEIGHTED)[(n >> 1) & 1], (n >> 2) & 3
        w, h = int(rng.integers(1, 48)), int(rng.integers(1, 40))
        D = image(w, h, och, 1000 + n)
        cw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        x, y = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - rh + 1))
        ow, oh = int(rng.integers(-(-cw // 64), 60)), int(rng.integers(-(-rh // 64), 50))
        same(D, (x, y, cw, rh), (ow, oh), flags, mode)
        count[(och, mode, flags)] += 1
        up += ow > cw or oh > rh
        down += ow < cw or oh < rh
    assert min(count.values()) >= 20 and up >= 50 and down >= 50


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_65_taps_and_upscales(mode):
    """191 -> 3: a middle output column really overlaps 65 source columns, both axes; 127 -> 2 has the bound of 65 and overlaps 64;
    upscales by whole and by odd ratios, and by 1 in 300"""
    assert np.count_nonzero(resize.weights(191, 3), axis=1).max() == 65 and resize.taps(127, 2) == 65
    D = image(200, 195, 4, 7)
    for rect, out in [((3, 2, 191, 191), (3, 3)), ((0, 1, 191, 127), (3, 2)), ((5, 5, 127, 127), (2, 2)), ((5, 5, 127, 64), (2, 1)), ((0, 0, 191, 7), (3, 20))]:
        win = rw.Window(D, rect[:4], out)
        assert win.colN.shape[2] == (65 if rect[2] > 127 else 64) and resize.split(rect[2], out[0]) == (4, 5)
        for flags in range(4):
            same(D, rect, out, flags, mode)
        same(np.ascontiguousarray(D[..., :3]), rect, out, 1, mode)
    for rect, out in [((7, 9, 5, 3), (13, 7)), ((0, 0, 1, 1), (9, 9)), ((1, 1, 20, 20), (40, 60)), ((2, 3, 100, 90), (101, 93)), ((0, 0, 200, 2), (7, 64))]:
        for flags in range(4):
            same(D, rect, out, flags, mode)


def test_lane_sums_are_the_shares():
    """lane l's partial sums are the sums over the columns and rows resize.share gives work item (Y * ow + X) * L + l; the levels add up"""
    D = image(140, 30, 4, 11)
    for rect, out in [((1, 2, 130, 25), (37, 9)), ((0, 0, 127, 30), (2, 3)), ((3, 3, 64, 8), (1, 1)), ((0, 0, 9, 9), (20, 4)), ((4, 0, 100, 30), (9, 7))]:
        x, y, cw, rh = rect
        ow, oh = out
        win = rw.Window(D, rect, out)
        lg, c = resize.split(cw, ow)
        for col, val in ((win.colN, D.astype(np.int64)), (win.colM, D[..., :3].astype(np.int64) * D[..., 3:4])):
            lv = win.levels(col)
            assert len(lv) == lg + 1 and lv[0].shape[2] == 1 << lg and np.array_equal(lv[-1][:, :, 0], col.sum(axis=2))
            for s in range(1, lg + 1):
                assert np.array_equal(lv[s], lv[0].reshape(oh, ow, (1 << lg) >> s, 1 << s, -1).sum(axis=3))
            for item in range(0, (ow * oh) << lg, 7):
                X, Y, cols, rows = resize.share(item, cw, rh, ow, oh)
                want = sum(wy * wx * val[y + r, x + k] for r, wy in rows for k, wx in cols) if cols else 0
                assert np.array_equal(lv[0][Y, X, item & ((1 << lg) - 1)], want + np.zeros(col.shape[3], dtype=np.int64)), (rect, out, item)
        n, d = win.divisions(ALPHA_WEIGHTED)
        assert n.size == d.size == 4 * ow * oh and d.min() >= 1
        n, d = win.divisions(PLAIN)
        assert n.size == d.size == 4 * ow * oh and np.all(d == cw * rh)


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_box_thumbnail_is_the_thumbnail(mode):
    for f, (w, h) in [(1, (5, 3)), (2, (12, 6)), (3, (9, 12)), (64, (128, 64)), (5, (35, 5))]:
        for och in (3, 4):
            D = image(w, h, och, f)
            assert np.array_equal(rw.box_thumbnail(D, f, mode), thumbs.thumbnail(D, f, mode)), (f, w, h, och)
    white = np.full((64, 128, 4), 255, dtype=np.uint8)
    assert np.array_equal(rw.box_thumbnail(white, 64, ALPHA_WEIGHTED), thumbs.thumbnail(white, 64, ALPHA_WEIGHTED))
    with pytest.raises(ValueError):
        rw.box_thumbnail(white, 3)


def test_the_wide_items_reach_their_sums():
    """(the same is asserted over `huge` by the device module, where that image is built anyway)"""
    D = rw.wide_image()
    assert 0.005 < np.mean(np.any(D != 255, axis=2)) < 0.02
    wins = [rw.Window(D, r[:4], r[4:]) for r in rw.wide_rects()]
    assert [resize.split(r[2], r[4]) for r in rw.wide_rects()] == [(2, 3), (4, 4), (0, 2), (3, 4)]
    lane, late, inner = zip(*[rw.high_half_classes(w) for w in wins])
    assert lane[0] and lane[2] and late[1] and inner[1] and not lane[1]
    for w, r in zip(wins, rw.wide_rects()):
        assert w.N.max() < rw.B32 <= w.M.max()
        if r[4] * r[5] <= 2000:
            for mode in (PLAIN, ALPHA_WEIGHTED):
                assert np.array_equal(w.pixels(3, mode), resize.resize(D, r[:4], r[4:], 3, mode))
