"""qoi_amd/resize.py - the normative statement of qoimi_decode_resized - against an independent brute-force statement of the definition
(nested loops over Python integers, written here), its identities with the two calls it generalises (out == rect is crops.crop; rect = f * out
is thumbs.thumbnail, both modes), the flip symmetry, the plan and the size arithmetic.  No GPU, no library."""
import numpy as np
import pytest

from qoi_amd import crops, resize, thumbs
from qoi_amd.packplan import slot
from qoi_amd.resize import ALPHA_WEIGHTED, FLIP_X, FLIP_Y, PLAIN
from model_cases import gradient_image as image


def brute(D, rect, out_size, flags, mode):
    """the definition, tap by tap"""
    x, y, cw, rh = rect
    ow, oh = out_size
    och = D.shape[2]
    T = cw * rh
    out = [[None] * ow for _ in range(oh)]
    for Y in range(oh):
        for X in range(ow):
            N, M = [0] * och, [0] * 3
            for r in range(rh):
                wy = max(0, min((Y + 1) * rh, (r + 1) * oh) - max(Y * rh, r * oh))
                for k in range(cw):
                    wx = max(0, min((X + 1) * cw, (k + 1) * ow) - max(X * cw, k * ow))
                    p = [int(v) for v in D[y + r, x + k]]
                    for c in range(och):
                        N[c] += wy * wx * p[c]
                    if och == 4:
                        for c in range(3):
                            M[c] += wy * wx * p[c] * p[3]
            px = [(n + T // 2) // T for n in N]
            if mode == ALPHA_WEIGHTED and och == 4 and N[3] > 0:
                px[:3] = [(m + N[3] // 2) // N[3] for m in M]
            out[Y][X] = px
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = [row[::-1] for row in out]
    return np.array(out, dtype=np.uint8)


SIZES = [((11, 9), (3, 2)), ((11, 9), (5, 4)), ((11, 9), (13, 11)), ((11, 9), (1, 1)), ((11, 9), (4, 9)),
         ((5, 3), (13, 7)),                       # an upscale
         ((11, 3), (4, 8)), ((3, 11), (7, 2)),    # down in x with up in y, and the reverse
         ((64, 64), (1, 1)), ((128, 3), (2, 3))]  # the cap exactly


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_against_brute_force(och, mode):
    for n, ((cw, rh), (ow, oh)) in enumerate(SIZES):
        D = image(cw + 3, rh + 2, och, n)
        rect = (2, 1, cw, rh)
        flags = n & 3
        got = resize.resize(D, rect, (ow, oh), flags, mode)
        assert got.shape == (oh, ow, och) and got.dtype == np.uint8
        assert np.array_equal(got, brute(D, rect, (ow, oh), flags, mode)), (cw, rh, ow, oh)


def test_the_cap():
    D = image(130, 66, 4, 1)
    assert resize.resize(D, (0, 0, 64, 64), (1, 1)).shape == (1, 1, 4) and resize.resize(D, (0, 0, 128, 3), (2, 3)).shape == (3, 2, 4)
    for rect, out in [((0, 0, 65, 1), (1, 1)), ((0, 0, 1, 65), (1, 1)), ((0, 0, 129, 3), (2, 3)), ((1, 0, 130, 1), (2, 1)), ((0, 0, 4, 4), (0, 1)), ((0, 0, 4, 4), (1, 0)),
                      ((0, 0, 0, 4), (1, 1)), ((127, 0, 4, 4), (1, 1)), ((0, 63, 4, 4), (1, 1))]:
        with pytest.raises(ValueError):
            resize.resize(D, rect, out)
        assert resize.size(130, 66, rect, out, 0, 4) == 0
    with pytest.raises(ValueError):
        resize.resize(D, (0, 0, 4, 4), (2, 2), 4)
    with pytest.raises(ValueError):
        resize.resize(D, (0, 0, 4, 4), (2, 2), 0, 2)


def test_weights_sum_to_the_source_size():
    for n_src in list(range(1, 40)) + [64, 127, 128, 130]:
        for n_out in range(1, 45):
            w = resize.weights(n_src, n_out)
            assert w.shape == (n_out, n_src) and np.all(w.sum(axis=1) == n_src) and np.all(w.sum(axis=0) == n_out) and w.min() >= 0, (n_src, n_out)
            assert np.array_equal(w, w[::-1, ::-1])                                      # symmetric under mirroring both
            if n_src <= 64 * n_out:
                assert np.count_nonzero(w, axis=1).max() <= resize.taps(n_src, n_out) <= 65
    for ow in range(1, 9):                                                               # at most 65 taps under the cap
        for cw in range(max(1, 60 * ow), 64 * ow + 1):
            assert np.count_nonzero(resize.weights(cw, ow), axis=1).max() <= resize.taps(cw, ow) <= 65


@pytest.mark.parametrize("och", [3, 4])
def test_identity_is_the_crop(och):
    D = image(23, 17, och, 3)
    for rect in [(0, 0, 23, 17), (3, 5, 7, 9), (22, 16, 1, 1), (0, 4, 23, 1)]:
        for flags in range(4):
            for mode in (PLAIN, ALPHA_WEIGHTED):
                assert np.array_equal(resize.resize(D, rect, rect[2:], flags, mode), crops.crop(D, rect, flags)), (rect, flags, mode)


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_whole_multiples_are_the_thumbnail(och, mode):
    for f in (1, 2, 3, 5, 7):
        ow, oh = 6, 4
        D = image(ow * f + 5, oh * f + 3, och, f)
        rect = (4, 2, ow * f, oh * f)
        R = crops.crop(D, rect)
        if och == 4:
            assert (R[:, :, 3] == 0).any() and (R[oh * f // 2:, :f, 3] == 0).all()       # alpha-0 pixels and an all-alpha-0 block
        want = thumbs.thumbnail(R, f, mode)
        assert want.shape == (oh, ow, och)
        assert np.array_equal(resize.resize(D, rect, (ow, oh), 0, mode), want), (f, och, mode)
    # an all-transparent block: the colours are the PLAIN value in both modes
    D = image(16, 16, 4, 9)
    D[:, :, 3] = 0
    assert np.array_equal(resize.resize(D, (0, 0, 16, 16), (4, 4), 0, ALPHA_WEIGHTED), resize.resize(D, (0, 0, 16, 16), (4, 4), 0, PLAIN))


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_flipping_is_resampling_the_mirrored_source(mode):
    D = image(29, 19, 4, 4)
    for rect, out in [((2, 1, 25, 17), (7, 5)), ((0, 0, 5, 3), (13, 7)), ((3, 3, 11, 4), (4, 9))]:
        R = crops.crop(D, rect)
        whole = (0, 0, rect[2], rect[3])
        for flags in range(4):
            assert np.array_equal(resize.resize(D, rect, out, flags, mode), resize.resize(crops.crop(R, whole, flags), whole, out, 0, mode)), (rect, out, flags)


def test_plan_is_the_crop_plan():
    descs = [(130, 70), (64, 48), (37, 23), (333, 7)]
    items = [(3, 0, 0, 333, 7, 5, 1, 0), (0, 5, 1, 121, 2, 224, 224, 1), (0, 0, 0, 130, 40, 37, 23, 2), (2, 1, 3, 35, 19, 7, 7, 3)]
    projected = [(3, 0, 0, 333, 7, 0), (0, 5, 1, 121, 2, 1), (0, 0, 0, 130, 40, 2), (2, 1, 3, 35, 19, 3)]
    assert [resize.as_crop(it) for it in items] == projected
    for staging in (0, 1, 10000, 22000, 1 << 20):
        assert resize.plan(descs, items, staging) == crops.plan(descs, projected, staging)
    images, slots, subs, largest = resize.plan(descs, items, 1)
    assert images == [0, 2, 3] and slots == [slot(130 * 40 * 4), slot(37 * 22 * 4), slot(333 * 7 * 4)] and len(subs) == 3 and largest == max(slots)


def test_size():
    assert resize.size(130, 70, (0, 0, 130, 70), (224, 224), 3, 3) == 224 * 224 * 3
    assert resize.size(130, 70, (129, 69, 1, 1), (100000, 100000), 0, 4) == 4 * 10 ** 10
    assert resize.size(130, 70, (0, 0, 128, 64), (2, 1), 0, 4) == 8
    for rect, out, flags, och in [((0, 0, 129, 64), (2, 1), 0, 4), ((0, 0, 128, 65), (2, 1), 0, 4), ((0, 0, 0, 1), (1, 1), 0, 4), ((0, 0, 1, 0), (1, 1), 0, 4),
                                  ((0, 0, 1, 1), (0, 1), 0, 4), ((0, 0, 1, 1), (1, 0), 0, 4), ((130, 0, 1, 1), (1, 1), 0, 4), ((0, 70, 1, 1), (1, 1), 0, 4),
                                  ((1, 0, 130, 1), (130, 1), 0, 4), ((0, 1, 1, 70), (1, 70), 0, 4), ((0, 0, 1, 1), (1, 1), 4, 4), ((0, 0, 1, 1), (1, 1), 0, 0),
                                  ((0, 0, 1, 1), (1, 1), 0, 5), ((0, 0, 1, 1), (2 ** 32 - 1, 2 ** 32 - 1), 0, 4)]:
        assert resize.size(130, 70, rect, out, flags, och) == 0, (rect, out, flags, och)


def test_work_items_cover_every_tap_once():
    """the kernel's split: the lanes of an output pixel hold each of its columns with a weight exactly once, and all of its rows"""
    for (cw, rh, ow, oh) in [(11, 9, 3, 2), (5, 3, 13, 7), (127, 70, 2, 3), (128, 64, 2, 1), (130, 70, 37, 23), (7, 7, 7, 7)]:
        lg, c = resize.split(cw, ow)
        wx, wy = resize.weights(cw, ow), resize.weights(rh, oh)
        assert resize.tiles(cw, ow, oh) == -(-(ow * oh << lg) // 256)
        for o in range(ow * oh):
            cols = []
            for l in range(1 << lg):
                X, Y, lane_cols, rows = resize.share((o << lg) | l, cw, rh, ow, oh)
                assert (Y, X) == divmod(o, ow) and len(lane_cols) <= c <= 5
                cols += lane_cols
                assert rows == [(r, int(wy[Y, r])) for r in np.nonzero(wy[Y])[0]]
            assert cols == [(k, int(wx[X, k])) for k in np.nonzero(wx[X])[0]], (cw, ow, o)
