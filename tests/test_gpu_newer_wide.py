"""The newer tensor filters and warp samplings on the GPU (-m gpu) where the small fixtures of their own modules cannot reach - the sibling of
tests/test_gpu_resize_wide.py for tensor_cubic, tensor_lanczos, tensor_nearest, tensor_mode, warp_bicubic_bytes, warp_bicubic_tensor and the
nearest branch of warp_gather: staged pixel indices beyond 2**24, and a workgroup of the shared tile walk (qoi_dev.h: walk_tiles) that takes
many tiles inside one table entry and steps out of it.  The pack is that module's: the 17.7 Mpx image of tests/resize_window.py (`huge`)
between small ones, encoded by the oracle and decoded by it for the expectation - with two plantings in its last rows, where every pixel
index is at least 2**24: a block of noise (the flat pieces of the image would forgive a misplaced sample) and a label map of five classes
(ordinary image content has no majority for FILTER_MODE).  Every expectation is the existing definition - the oracle's decode at the call's
output channel count, the model of qoi_amd/, tensors.convert -, every comparison is exact and covers the whole output, and every byte around
the outputs is a guard (0xA5) checked after every call (tests/gpu_calls.py: run_label_tensors, run_warp).
Part 3 holds the kernels of the folding borders and of supersampling to the same two regimes: warp_border_bytes and warp_border_tensor walk
border_walk_table - more tiles than workgroups, a map that spans six and a half periods of the rectangle, so that tiles take either branch of
warp_fold_position and some both (test_warp_border_walks_many_tiles_per_workgroup, test_warp_border_and_super_tensor_kernels_walk_many_tiles)
- and border_items_beyond (test_border_items_beyond_2_24); warp_super_tensor walks super_walk_table, the table tests/test_gpu_warp_super.py
runs through warp_super_bytes."""
import numpy as np
import pytest

import resize_window as rw
from qoi_amd import mode, nearest, tensors, warp
from qoi_amd.tensors import CHW, F16, F32, FILTER_BICUBIC, FILTER_LANCZOS, FILTER_MODE, FILTER_NEAREST, HW, HWC, I32, I64, U8
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, WRAP
from gpu_calls import run_label_tensors as run_tensors, run_warp
from gpu_pack import IMAGENET, KINDS, OraclePack, image
from gpu_pack import api, ctx, cus, oracle  # noqa: F401  (fixtures)
from wide_cases import DOT, FILL, FIRST_ROW, HH, HUGE, HW_, LABELS_AT, NOISE_AT, NOISE_RECT, ODD, SPRITE, huge_with_plantings, past_2_24, super_walk_table, super_windows, walk_shape, window_of

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 4), (37, 23, 3), rw.HUGE + (4,), (130, 70, 4)]
assert FIRST_ROW * HW_ >= 1 << 24 > (FIRST_ROW - 1) * HW_ and all(y >= FIRST_ROW and y + h <= HH and x + w <= HW_ for x, y, w, h in (NOISE_AT, LABELS_AT))


@pytest.fixture(scope="module")
def pack(api, oracle):
    pixels = [huge_with_plantings() if i == HUGE else image(KINDS[(i + 2) % 5], w, h, ch, frame=i) for i, (w, h, ch) in enumerate(SHAPES)]
    p = OraclePack(api, oracle, SHAPES, pixels)
    assert np.array_equal(p.decoded(HUGE, 4).reshape(-1), p.px[HUGE])      # the oracle gives back what it was given
    return p


def u8_of(p, filt, it, och, alpha_mode):
    """the u8 result of one item of qoimi_decode_tensors by the definition"""
    if filt == FILTER_MODE:                                            # the vote is over the 4-channel decode
        return mode.mode(p.decoded(it[0], 4), it[1:5], it[5:7], it[7], och=och)
    return tensors.tensors(p.decoded(it[0], och), it[1:5], it[5:7], it[7], filt, alpha_mode)


def warped(p, it, och, alpha_mode):
    i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
    return warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, alpha_mode)


def assert_equal(got, want, what):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size and np.array_equal(got, want), (what, "first difference at byte", int(np.argmax(got != want)), "of", want.size)


# ------------------------------------------------------------------ 1: staged pixel indices beyond 2**24
# per filter: two rectangles of the last rows of `huge` - the first in a planting, the second the image's bottom right corner -, a format
# and an alpha mode; small items of the small images stand in front of, between and behind them
BIG_ITEMS = {FILTER_BICUBIC: ([(HUGE, 100, 3652, 400, 180, 64, 48, 1), (HUGE, HW_ - 37, HH - 29, 37, 29, 50, 41, 2)], (F32, CHW), ALPHA_WEIGHTED),
             FILTER_LANCZOS: ([(HUGE, 110, 3655, 390, 170, 60, 44, 2), (HUGE, HW_ - 37, HH - 29, 37, 29, 41, 33, 1)], (F16, HWC), PLAIN),
             FILTER_NEAREST: ([(HUGE, 1010, 3650, 1100, 180, 64, 64, 3), (HUGE, HW_ - 3, HH - 3, 3, 3, 7, 5, 0)], (I64, HW), PLAIN),
             FILTER_MODE: ([(HUGE, 1003, 3645, 1000, 190, 64, 48, 0), (HUGE, 1100, 3650, 300, 150, 60, 50, 2), (HUGE, HW_ - 33, HH - 9, 33, 9, 5, 3, 1)], (I32, HWC), PLAIN)}


@pytest.mark.parametrize("filt", list(BIG_ITEMS), ids=["bicubic", "lanczos", "nearest", "mode"])
def test_tensor_filters_beyond_2_24(ctx, pack, filt):
    """qoimi_decode_tensors with each of the four newer filters over rectangles whose every staged pixel index is at least 2**24 (mem.px[...] of
    the core headers, behind `stage + e.src_off`)"""
    p = pack
    big, (dtype, order), alpha_mode = BIG_ITEMS[filt]
    items = [(DOT, 0, 0, 1, 1, 3, 2, 0), (ODD, 2, 3, 30, 17, 20, 11, 1), big[0], (HUGE, 7, 5, 40, 30, 16, 12, 3)] + big[1:] + [(SPRITE, 5, 7, 100, 50, 33, 21, 2)]
    assert past_2_24(big) and sorted(items, key=lambda it: it[0]) == items
    if filt == FILTER_MODE:
        assert [mode.split(*it[3:7])[0] for it in big] == [4, 2, 3]                   # 16, 4 and 8 lanes a pixel
    f = tensors.fmt(dtype, order) if dtype in (U8, I32, I64) else (dtype, order, *IMAGENET)
    got = run_tensors(ctx, p, filt, 4, items, alpha_mode, f)
    assert ctx.tensor_stats()[:2] == (1, 1) and ctx.tensor_stats()[3] == 4
    for j, it in enumerate(items):
        assert_equal(got[j], tensors.convert(u8_of(p, filt, it, 4, alpha_mode), f), (filt, j, it))


def warp_items(cubic):
    """rectangles of the last rows of `huge` under a turn that reduces and a turn that enlarges across the image's corner; `cubic`: bicubic,
    bilinear and nearest items in one call (warp_bicubic_bytes / _tensor), else nearest and bilinear items (warp_gather / tensor_warp)"""
    a, b = (100, 3652, 400, 180), (HW_ - 37, HH - 29, 37, 29)
    ma, mb = warp.rotation(a[2:], (64, 64), 30.0, 0.2), warp.rotation(b[2:], (50, 41), -20.0, 1.7)
    first, second = (BICUBIC, BICUBIC | REPLICATE) if cubic else (NEAREST, NEAREST | REPLICATE)
    return [warp.item(ODD, (2, 3, 30, 17), (20, 11), warp.rotation((30, 17), (20, 11), 10.0, 0.7), first, FILL), warp.item(HUGE, a, (64, 64), ma, first, FILL),
            warp.item(HUGE, b, (50, 41), mb, second, 0), warp.item(HUGE, a, (64, 64), ma, NEAREST if cubic else 0, FILL), warp.item(HUGE, b, (50, 41), mb, REPLICATE, 0),
            warp.item(SPRITE, (5, 7, 100, 50), (33, 21), warp.rotation((100, 50), (33, 21), 45.0, 0.4), NEAREST | REPLICATE if cubic else 0, FILL)]


@pytest.mark.parametrize("cubic", [True, False], ids=["with bicubic items", "nearest and bilinear"])
def test_warp_samplings_beyond_2_24(ctx, pack, cubic):
    """qoimi_decode_warped and qoimi_decode_warped_tensors over rectangles whose every staged pixel index is at least 2**24"""
    p = pack
    items = warp_items(cubic)
    assert past_2_24(items) and any(it[7] & BICUBIC for it in items) == cubic and any(it[7] & NEAREST for it in items)
    for channels, alpha_mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run_warp(ctx, p, channels, items, alpha_mode, front=64 + 1)
        assert ctx.warp_stats()[:2] == (1, 1)
        for j, it in enumerate(items):
            assert_equal(got[j], warped(p, it, channels, alpha_mode), ("warped", cubic, channels, j))
    f = (F16, CHW, *IMAGENET)
    got = run_tensors(ctx, p, "warp", 4, items, ALPHA_WEIGHTED, f)
    assert ctx.tensor_stats()[:2] == (1, 1)
    for j, it in enumerate(items):
        assert_equal(got[j], tensors.convert(warped(p, it, 4, ALPHA_WEIGHTED), f), ("warped tensors", cubic, j))


# ------------------------------------------------------------------ 2: the tile walk with many tiles per workgroup
def mode_by_rows(D4, rect, out_size):
    """mode.mode of an item that ENLARGES in y, one source row at a time: there every cell of rows is one row, the nearest one (qoi_amd/mode.py:
    "a cell of one sample is the nearest sample"), so output row Y is the vote over source row nearest.index(rh, oh)[Y] alone - the model's
    own result for the rectangle of that one row and an output of one row.  uint8[oh, ow, 4], unflipped."""
    x, y, cw, rh = rect
    ow, oh = out_size
    assert rh < oh
    rows = np.stack([mode.mode(D4, (x, y + r, cw, 1), (ow, 1), 0, och=4)[0] for r in range(rh)])
    return rows[nearest.index(rh, oh)]


def test_mode_walks_many_tiles_per_workgroup(ctx, pack, cus):
    """One sub-batch whose table reads [small, big, small x 5, small]: big reduces 1000 x 50 labels of the last rows of `huge` by 5 in x - cells
    of 5 x 1 pixels, two lanes a pixel - and enlarges them in y until the entry holds more than 3 * 8 * cu tiles; the five behind it are
    one-tile votes over `huge` itself.  With at most 8 * cu workgroups each takes several tiles: they start inside the big entry, end inside
    it, and step out of it across the small ones.  The expectation is the model's, computed once - for the big item row by row
    (mode_by_rows; that this is mode.mode of a whole item is asserted here on the rectangle's first 8 rows at 20 output rows)."""
    p = pack
    x, y, cw, rh, ow = 1000, 3644, 1000, 50, 200
    oh = (3 * 8 * cus * mode.THREADS) // (2 * ow) + 2
    big = (HUGE, x, y, cw, rh, ow, oh, 0)
    inner = [(HUGE, 1000 + 7 * j, 3700 + j, 20, 12, 5, 4, j & 3) for j in range(5)]
    items = [(DOT, 0, 0, 1, 1, 1, 1, 0), big] + inner + [(SPRITE, 129, 69, 1, 1, 1, 1, 2)]
    tiles = [mode.tiles(*it[3:7]) for it in items]
    assert mode.split(cw, rh, ow, oh) == (1, 3) and oh <= mode.MAX_SIZE
    assert tiles[1] > 3 * 8 * cus and tiles[:1] + tiles[2:] == [1] * 7 and past_2_24(items)
    D4 = p.decoded(HUGE, 4)
    assert np.array_equal(mode_by_rows(D4, (x, y, cw, 8), (ow, 20)), mode.mode(D4, (x, y, cw, 8), (ow, 20), 0, och=4))
    f = tensors.fmt(U8, HWC)
    got = run_tensors(ctx, p, FILTER_MODE, 4, items, PLAIN, f)
    assert ctx.tensor_stats()[:2] == (1, 1)
    assert_equal(got[1], mode_by_rows(D4, (x, y, cw, rh), (ow, oh)), "the big entry")
    for j in (0, 2, 3, 4, 5, 6, 7):
        assert_equal(got[j], u8_of(p, FILTER_MODE, items[j], 4, PLAIN), ("a one-tile entry", j))


def rows_of(it, first, step):
    """the item whose output is rows first, first + step, ... of `it`'s: V = 2 * (first + step * j) + 1 = step * (2j + 1) + (2 * first + 1 - step)"""
    i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
    shift = 2 * first + 1 - step
    return warp.item(i, (x, y, cw, rh), (ow, len(range(first, oh, step))), (a, b * step, c + b * shift, d, e * step, f + e * shift), flags, fill)


def test_warp_bicubic_walks_many_tiles_per_workgroup(ctx, pack, cus):
    """[small, big, small x 5, small] in one launch of warp_bicubic_bytes: big turns and enlarges a rectangle of the last rows of `huge` to more
    than 3 * 8 * cu tiles of 16 x 16 (the last column and row of tiles partial), the five behind it are one-tile items of `huge` of every
    sampling.  The model would take long over 1.5 Mpx of 4 x 4 taps: the big output is compared WHOLE with the same item alone in its own
    call, and every 17th row of it - rows 5, 22, 39 ..., every phase of a tile's 16 rows - with the model (rows_of: the same map sampled at
    those rows; that it is those rows is asserted on a small output).  The small items are compared with the model."""
    p = pack
    across = 80
    down = (3 * 8 * cus) // across + 1
    ow, oh = 16 * across - 3, 16 * down - 5
    rect = (100, 3652, 400, 180)
    a, b, d, e = round(ONE * 1.1 * rect[2] / ow), round(ONE * 0.12 * rect[2] / oh), round(-ONE * 0.1 * rect[3] / ow), round(ONE * 1.1 * rect[3] / oh)
    big = warp.item(HUGE, rect, (ow, oh), (a, b, rect[2] * ONE - a * ow - b * oh, d, e, rect[3] * ONE - d * ow - e * oh), BICUBIC, FILL)     # a shear about the centre
    samplings = (BICUBIC | REPLICATE, NEAREST, 0, BICUBIC, NEAREST | REPLICATE)
    inner = [warp.item(HUGE, (HW_ - 9 - j, HH - 7 - j, 9, 7), (11 + j, 5), warp.rotation((9, 7), (11 + j, 5), 25.0 * j, 1.3), s, FILL) for j, s in enumerate(samplings)]
    items = [warp.item(DOT, (0, 0, 1, 1), (5, 4), (ONE // 3, 0, 0, 0, ONE // 3, 0), BICUBIC, FILL), big] + inner + [warp.item(SPRITE, (120, 60, 10, 10), (7, 7), flags=NEAREST)]
    tiles = [warp.tiles(it[5], it[6]) for it in items]
    assert tiles[1] == across * down > 3 * 8 * cus and tiles[:1] + tiles[2:] == [1] * 7 and past_2_24(items) and ow * oh < warp.MAX_AREA
    small = warp.item(HUGE, rect, (40, 60), warp.rotation(rect[2:], (40, 60), 30.0, 0.1), BICUBIC, FILL)
    assert np.array_equal(warped(p, rows_of(small, 5, 17), 4, ALPHA_WEIGHTED), warped(p, small, 4, ALPHA_WEIGHTED)[5::17])
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 3)
    assert ctx.warp_stats()[:2] == (1, 1)
    alone = run_warp(ctx, p, 4, [big], ALPHA_WEIGHTED)
    assert np.array_equal(got[1], alone[0]), ("the big entry differs from its own call", int(np.argmax(got[1] != alone[0])))
    assert_equal(np.ascontiguousarray(got[1].reshape(oh, ow, 4)[5::17]).reshape(-1), warped(p, rows_of(big, 5, 17), 4, ALPHA_WEIGHTED), "every 17th row of the big entry")
    for j in (0, 2, 3, 4, 5, 6, 7):
        assert_equal(got[j], warped(p, items[j], 4, ALPHA_WEIGHTED), ("a one-tile entry", j))


# ------------------------------------------------------------------ 3: the border kernels and the super tensor kernel in both regimes
_WARPED = {}
F16_CHW = (F16, CHW, *IMAGENET)


def warped_once(p, it, och, alpha_mode):
    """`warped`, computed once per item and shared between the tests below; never changed"""
    key = (tuple(it), och, alpha_mode)
    if key not in _WARPED:
        P = warped(p, it, och, alpha_mode)
        P.setflags(write=False)
        _WARPED[key] = P
    return _WARPED[key]


BIG_BORDERS = {"bilinear, reflect": REFLECT, "bicubic, wrap": BICUBIC | WRAP}


def period_of(n, flags):
    return {REFLECT: 2 * n, REFLECT_101: max(2 * n - 2, 1), WRAP: n}[flags & warp.BORDERS]


def border_walk_table(cus, flags):
    """[small, big, small x 5, small] for one launch of warp_border_bytes / warp_border_tensor: big samples the planted noise under the border
    of `flags` and a shear about the rectangle's centre that spans six and a half periods of the rectangle on either axis, into more than
    3 * 8 * cus tiles of 16 x 16 (the last column and row of tiles partial); the five behind it are one-tile items of the last rows of `huge`
    that cover the three borders and the three samplings; a one-tile item of a small image stands on either side"""
    ow, oh, _, _ = walk_shape(cus)
    rect = NOISE_RECT
    Px, Py = period_of(rect[2], flags), period_of(rect[3], flags)
    a, b, d, e = round(ONE * 6.5 * Px / ow), round(ONE * 0.4 * Px / oh), round(-ONE * 0.4 * Py / ow), round(ONE * 6.5 * Py / oh)
    big = warp.item(HUGE, rect, (ow, oh), (a, b, rect[2] * ONE - a * ow - b * oh, d, e, rect[3] * ONE - d * ow - e * oh), flags, FILL)
    kinds = (REFLECT | NEAREST, REFLECT_101 | BICUBIC, WRAP, REFLECT_101 | NEAREST, REFLECT | BICUBIC)
    inner = [warp.item(HUGE, (HW_ - 9 - j, HH - 7 - j, 9, 7), (11 + j, 5), warp.rotation((9, 7), (11 + j, 5), 25.0 * j, 0.3), s, FILL) for j, s in enumerate(kinds)]
    items = [warp.item(DOT, (0, 0, 1, 1), (5, 4), (ONE // 3, 0, 0, 0, ONE // 3, 0), WRAP | BICUBIC, FILL), big] + inner
    items.append(warp.item(SPRITE, (120, 60, 10, 10), (7, 7), (3 * ONE, 0, -40 * ONE, 0, 3 * ONE, 55 * ONE), REFLECT_101 | NEAREST))
    assert {s & warp.BORDERS for s in kinds} == {REFLECT, REFLECT_101, WRAP} and {s & ~warp.BORDERS for s in kinds} == {0, NEAREST, BICUBIC}
    assert not any(it[7] & (SUPER2 | SUPER4) for it in items)
    return items


def first_taps(it, X, Y):
    """(kx, ky): the first tap index of each axis that warp_fold_position folds for the output pixels (X, Y) (arrays) of a bilinear or bicubic
    item - the bicubic one a sample before the bilinear one"""
    _, _, _, _, _, _, _, flags, a, b, d, e, _, _, c, f = it
    U, V = 2 * np.asarray(X, dtype=np.int64) + 1, 2 * np.asarray(Y, dtype=np.int64) + 1
    back = 1 if flags & BICUBIC else 0
    return ((a * U + b * V + c - ONE) >> 17) - back, ((d * U + e * V + f - ONE) >> 17) - back


def assert_the_fold_takes_both_branches(big):
    """from the item's coefficients, at the corner pixels of every tile: on either axis the map spans at least five periods; the first and the
    last tile lie wholly in the estimate branch of warp_fold_position (k < -P or k >= 2P), a tile in the middle wholly in the conditional
    one, and there are tiles whose corners lie on either side of k = -P and of k = 2P - lanes of one workgroup in different branches"""
    _, _, _, cw, rh, ow, oh, flags = big[:8]
    x0, y0 = np.arange(0, ow, 16), np.arange(0, oh, 16)
    x1, y1 = np.minimum(x0 + 15, ow - 1), np.minimum(y0 + 15, oh - 1)
    corners = [first_taps(big, X[None, :], Y[:, None]) for X in (x0, x1) for Y in (y0, y1)]             # [corner][axis][tile row, tile column]
    for axis, n in ((0, cw), (1, rh)):
        P = period_of(n, flags)
        k = np.stack([c[axis] for c in corners])
        assert int(k.max()) - int(k.min()) >= 5 * P, (axis, int(k.min()), int(k.max()), P)
        estimate = (k < -P) | (k >= 2 * P)
        assert estimate[:, 0, 0].all() and estimate[:, -1, -1].all()                                     # the first and the last tile
        assert (~estimate).all(axis=0)[len(y0) // 2, len(x0) // 2]                                       # the tile in the middle
        for edge in (-P, 2 * P):
            across = (k < edge).any(axis=0) & (k >= edge).any(axis=0)
            assert across.any(), (axis, edge)
        assert estimate.all(axis=0).sum() > 10 and (~estimate).all(axis=0).sum() > 10


@pytest.mark.parametrize("flags", list(BIG_BORDERS.values()), ids=list(BIG_BORDERS))
def test_warp_border_walks_many_tiles_per_workgroup(ctx, pack, cus, flags):
    """[small, big, small x 5, small] in one launch of warp_border_bytes (border_walk_table).  big's map reaches three periods to either side
    of the rectangle, so whole tiles take the conditional branch of the fold, whole tiles its quotient estimate, and tiles between them both
    (assert_the_fold_takes_both_branches, on the CPU); the bicubic big folds its first tap at k - 1.  The big output is compared WHOLE with
    the same item alone in its own call, every 17th row of it - every phase of a tile's 16 rows - with the model (rows_of), the small items
    with the model."""
    p = pack
    ow, oh, across, down = walk_shape(cus)
    items = border_walk_table(cus, flags)
    big = items[1]
    tiles = [warp.tiles(it[5], it[6]) for it in items]
    assert tiles[1] == across * down > 3 * 8 * cus and tiles[:1] + tiles[2:] == [1] * 7 and past_2_24(items) and ow * oh < warp.MAX_AREA
    assert ow % 16 and oh % 16
    assert_the_fold_takes_both_branches(big)
    small = warp.item(HUGE, NOISE_RECT, (40, 60), warp.rotation(NOISE_RECT[2:], (40, 60), 30.0, 0.05), flags, FILL)
    assert np.array_equal(warped(p, rows_of(small, 5, 17), 4, ALPHA_WEIGHTED), warped(p, small, 4, ALPHA_WEIGHTED)[5::17])
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 3)
    assert ctx.warp_stats()[:2] == (1, 1)
    alone = run_warp(ctx, p, 4, [big], ALPHA_WEIGHTED)
    assert np.array_equal(got[1], alone[0]), ("the big entry differs from its own call", int(np.argmax(got[1] != alone[0])))
    assert_equal(np.ascontiguousarray(got[1].reshape(oh, ow, 4)[5::17]).reshape(-1), warped_once(p, rows_of(big, 5, 17), 4, ALPHA_WEIGHTED), "every 17th row of the big entry")
    for j in (0, 2, 3, 4, 5, 6, 7):
        assert_equal(got[j], warped_once(p, items[j], 4, ALPHA_WEIGHTED), ("a one-tile entry", j))


@pytest.mark.parametrize("table", list(BIG_BORDERS) + ["super2, reflect"])
def test_warp_border_and_super_tensor_kernels_walk_many_tiles(ctx, pack, cus, table):
    """The tables of the test above and of tests/test_gpu_warp_super.py: test_many_tiles_per_workgroup_beyond_2_24 as f16 CHW tensors: one launch
    of warp_border_tensor or warp_super_tensor over more tiles than it has workgroups and staged pixel indices from 2**24 on.  The small
    items, and the rows (border) or windows (super) of big that the u8 tests compare with the model, are tensors.convert of the model; the
    whole of big is what the item alone gives in its own tensor call."""
    p = pack
    ow, oh, across, down = walk_shape(cus)
    items = super_walk_table(cus) if table.startswith("super") else border_walk_table(cus, BIG_BORDERS[table])
    big = items[1]
    assert warp.tiles(ow, oh) == across * down > 3 * 8 * cus and big[5:7] == (ow, oh) and past_2_24(items)
    assert any(it[7] & (SUPER2 | SUPER4) for it in items) == table.startswith("super")
    got = run_tensors(ctx, p, "warp", 4, items, ALPHA_WEIGHTED, F16_CHW)
    assert ctx.tensor_stats()[:2] == (1, 1)
    alone = run_tensors(ctx, p, "warp", 4, [big], ALPHA_WEIGHTED, F16_CHW)
    assert ctx.tensor_stats()[:2] == (1, 1)
    assert np.array_equal(got[1], alone[0]), ("the big entry differs from its own call", int(np.argmax(got[1] != alone[0])) // 2)
    whole = got[1].view(np.uint16).reshape(4, oh, ow)

    def halves(u8):
        return tensors.convert(u8, F16_CHW).view(np.uint16)

    if table.startswith("super"):
        for X0, Y0 in super_windows(ow, oh):
            want = halves(warped_once(p, window_of(big, X0, Y0, 45, 27), 4, ALPHA_WEIGHTED))
            assert np.array_equal(whole[:, Y0:Y0 + 27, X0:X0 + 45], want), ("a window of the big entry", X0, Y0)
    else:
        assert np.array_equal(whole[:, 5::17], halves(warped_once(p, rows_of(big, 5, 17), 4, ALPHA_WEIGHTED))), "every 17th row of the big entry"
    for j in (0, 2, 3, 4, 5, 6, 7):
        assert_equal(got[j], tensors.convert(warped_once(p, items[j], 4, ALPHA_WEIGHTED), F16_CHW), ("a one-tile entry", j))
    # A consistency check only, not an expectation: the tensor of big is the conversion of what the u8 kernel writes for the same item.  The
    # sampling is shared, so a failure here and not above localises to the sink, not to the sampling.
    u8 = run_warp(ctx, p, 4, [big], ALPHA_WEIGHTED)[0].reshape(oh, ow, 4)
    assert np.array_equal(whole, halves(u8)), "consistency: the tensor sink and the byte sink disagree on the big entry"


def border_items_beyond():
    """warp_items with a border on every item over `huge`: the planted noise turned and reduced by 10 - the output reaches about a period to either
    side of the rectangle - and the image's bottom right corner turned and reduced by 2 - about two periods -, each border with each sampling
    between them; a bordered item of a small image in front, an item without a border behind"""
    a, b = NOISE_RECT, (HW_ - 37, HH - 29, 37, 29)
    ma, mb = warp.rotation(a[2:], (64, 64), 30.0, 0.1), warp.rotation(b[2:], (50, 41), -20.0, 0.5)
    flags = (REFLECT, REFLECT_101 | BICUBIC, WRAP | NEAREST, WRAP, REFLECT | BICUBIC, REFLECT_101 | NEAREST, REFLECT_101, WRAP | BICUBIC, REFLECT | NEAREST)
    over = [warp.item(HUGE, r, s, m, fl, FILL) for fl, (r, s, m) in zip(flags, [(a, (64, 64), ma), (b, (50, 41), mb)] * 5)]
    return [warp.item(ODD, (2, 3, 30, 17), (20, 11), warp.rotation((30, 17), (20, 11), 10.0, 0.3), REFLECT | BICUBIC, FILL)] + over + \
           [warp.item(SPRITE, (5, 7, 100, 50), (33, 21), warp.rotation((100, 50), (33, 21), 45.0, 0.4), 0, FILL)]


def test_border_items_beyond_2_24(ctx, pack):
    """qoimi_decode_warped and qoimi_decode_warped_tensors with REFLECT, REFLECT_101 and WRAP in every sampling over rectangles whose every staged
    pixel index is at least 2**24 (warp_border_bytes, warp_border_tensor)"""
    p = pack
    items = border_items_beyond()
    over = [it for it in items if it[0] == HUGE]
    assert past_2_24(items) and len(over) == 9 and {(it[7] & warp.BORDERS, it[7] & ~warp.BORDERS) for it in over} == {(b, s) for b in (REFLECT, REFLECT_101, WRAP) for s in (0, NEAREST, BICUBIC)}
    assert not any(it[7] & (SUPER2 | SUPER4) for it in items)
    for channels, alpha_mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run_warp(ctx, p, channels, items, alpha_mode, front=64 + 1)
        assert ctx.warp_stats()[:2] == (1, 1)
        for j, it in enumerate(items):
            assert_equal(got[j], warped_once(p, it, channels, alpha_mode), ("warped", channels, j))
    got = run_tensors(ctx, p, "warp", 4, items, ALPHA_WEIGHTED, F16_CHW)
    assert ctx.tensor_stats()[:2] == (1, 1)
    for j, it in enumerate(items):
        assert_equal(got[j], tensors.convert(warped_once(p, it, 4, ALPHA_WEIGHTED), F16_CHW), ("warped tensors", j))
