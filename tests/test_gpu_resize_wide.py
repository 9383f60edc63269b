"""qoimi_decode_resized and its siblings on the GPU (-m gpu) where the small fixtures of the sibling modules cannot reach: sums whose high
halves are not zero (inside a lane and across the butterfly of resize_xor_add), every path of resize_div_round / resize_div, 65 taps (five
columns per lane), a workgroup of the shared tile walk (qoi_dev.h: walk_tiles; the copy in cmp_pixels) that takes many tiles inside one table
entry and steps out of it, and staged pixel indices beyond 2**24.  One image of 17.7 Mpx (`huge`) and one of 1040 x 260 (`wide`) stand between
small ones in one pack; the images are built with numpy, encoded by the oracle and decoded by it for the expectation.  The expectation of a
resampled large rectangle is tests/resize_window.py (held equal to qoi_amd/resize.py: resize by tests/test_resize_window.py), whose sums also
PROVE that an item reaches the magnitudes it is there for: a test that does not reach them fails.  Every comparison is exact and covers the
whole output; every byte around the outputs is a guard (0xA5) checked after every call."""
import numpy as np
import pytest

import resize_window as rw
from qoi_amd import crops, resize, thumbs
from qoi_amd.imagediff import DIFF_DTYPE, DIFF_PIXELS, NONE, pixel_word
from qoi_amd.packplan import slot
from qoi_amd.resize import ALPHA_WEIGHTED, PLAIN
from gpu_calls import run_resized as run, run_thumbnails, standard
from gpu_pack import GUARD, KINDS, MIXED_SHAPES, OraclePack, dev, filled, image
from gpu_pack import api, ctx, cus, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
B32 = rw.B32
SHAPES = [(1, 1, 4), (37, 23, 3), rw.HUGE + (4,), (1, 97, 4), (131, 1, 3), (257, 9, 4), (64, 48, 3), (333, 7, 4), rw.WIDE + (4,), (130, 70, 4), (127, 127, 4)]
HUGE, WIDE, T127, SPRITE = 2, 8, 10, 9
LARGE = (HUGE, WIDE)                   # resampled rectangles of these are expected from windows; the others from the model itself
HW, HH = rw.HUGE
CMP_TILE_PX = 4096                     # qoi_compare.hip: kCmpTilePx


@pytest.fixture(scope="module")
def pack(api, oracle):
    built = {HUGE: rw.huge_image, WIDE: rw.wide_image, T127: lambda: np.random.default_rng(127).integers(0, 256, size=(127, 127, 4), dtype=np.uint8)}
    pixels = [built[i]() if i in built else image(KINDS[(i + 2) % 5], w, h, ch, frame=i) for i, (w, h, ch) in enumerate(SHAPES)]
    assert set(MIXED_SHAPES) <= set(SHAPES)
    p = OraclePack(api, oracle, SHAPES, pixels)
    for i in LARGE + (T127,):            # the oracle gives back what it was given; a decode at 3 channels is the colours of the one at 4
        assert np.array_equal(p.decoded(i, 4).reshape(-1), p.px[i]) and np.array_equal(p.decoded(i, 3), p.decoded(i, 4)[..., :3])
    assert p.sizes[HUGE] < 1 << 20       # mostly flat: the stream is small
    return p


def want(p, it, och, mode):
    i, x, y, cw, rh, ow, oh, flags = it
    if (cw, rh) == (ow, oh):
        return crops.crop(p.decoded(i, och), (x, y, cw, rh), flags).reshape(-1)
    if i in LARGE:
        return p.window(it).pixels(flags, mode if och == 4 else PLAIN, och).reshape(-1)
    return resize.resize(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, mode).reshape(-1)


def assert_items(p, got, items, och, mode, what):
    for j, it in enumerate(items):
        w = want(p, it, och, mode)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, it, int(np.argmax(got[j] != w)))


def smalls(p, images, first_flag=0):
    """a few items of the small images: they stand between the large ones"""
    return [it for i in images for it in standard(i, p.shapes[i][0], p.shapes[i][1], first_flag + i)[:4]]


def between(large, small):
    """large items with small ones in front of, between and behind them"""
    out, k = [], 0
    per = max(1, len(small) // (len(large) + 1))
    for it in large:
        out += small[k:k + per] + [it]
        k += per
    return out + small[k:]


# ------------------------------------------------------------------ 1: high halves inside a lane and across the butterfly
@pytest.mark.parametrize("mode", [ALPHA_WEIGHTED, PLAIN])
@pytest.mark.parametrize("channels", [4, 3])
def test_high_halves_in_a_lane_and_across_the_butterfly(ctx, pack, channels, mode):
    """`wide` is 0xFFFFFFFF with 1 % random pixels: the weighted colour sums are near 65025 * T.  1040 x 260 -> 100 x 260: four lanes of three
    columns, one lane's weight is 3 * 100 * 260 and its sums pass 2**32 before any exchange.  520 x 260 -> 9 x 5: sixteen lanes, each below
    2**32, the pixel above: the high halves appear in the later exchange steps only.  300 x 260 -> 301 x 263: one lane, no exchange.  An odd
    rectangle at an odd origin: eight lanes.  (The plain sums stay below 2**32 on this image - 255 * T = 6.9e7; test 2 takes them beyond.)"""
    p = pack
    large = [(WIDE,) + r + ((k + 1 + channels + mode) & 3,) for k, r in enumerate(rw.wide_rects())]
    assert [resize.split(it[3], it[5]) for it in large] == [(2, 3), (4, 4), (0, 2), (3, 4)]
    classes = [rw.high_half_classes(p.window(it)) for it in large]
    print("lane sum / pixel sum with every lane below / crossing at an inner step, from 2**32:", classes, [int(p.window(it).M.max()) for it in large])
    assert classes[0][0] and classes[2][0], "a lane's sum from 2**32 before any exchange"
    assert classes[1][1] and not classes[1][0], "a pixel whose lanes are all below 2**32 with a sum from it"
    assert classes[1][2] and classes[3][2], "the sum over 2**s lanes crosses 2**32 at a step 0 < s < lg"
    assert all(p.window(it).M.max() >= B32 for it in large)
    items = between(large, smalls(p, (0, 1, 3, SPRITE, 5)))
    assert {it[7] for it in large} == {0, 1, 2, 3}
    got = run(ctx, p, channels, items, mode, front=64 + (channels & 3))
    assert_items(p, got, items, channels, mode, (channels, mode))
    assert ctx.resize_stats()[:2] == (1, 1)
    if channels == 4:
        assert not np.array_equal(want(p, large[0], 4, PLAIN), want(p, large[0], 4, ALPHA_WEIGHTED))


# ------------------------------------------------------------------ 2: every division class
def huge_items(first_flag):
    return [(HUGE,) + r + ((first_flag + k) & 3,) for k, r in enumerate(rw.huge_rects())]


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_every_division_class(ctx, pack, mode):
    """The (n, d) of every division of the items over `huge`, from the windows.  The weighted mode - (W + A/2, A) beside (N + T/2, T) - reaches
    every path: both below 2**32 (the dark rows of alpha 3), n from 2**32 with d below, d from 2**32 (A of a white output pixel of the whole
    image is 255 * T = 4.5e9), d a power of two with n from 2**32 (alpha 128 over T = 2**23: A = 2**30, W up to 255 * 2**37) and A == 0 (the
    clear rows; whole output pixels of 72 x 60 and 73 x 61 lie inside them).  PLAIN divides by T alone, and T < 4e8 < 2**32 whatever the item:
    it reaches both below 2**32, n from 2**32 (N of the whole image) and the shift (T = 2**23; a power of two T with N from 2**32 would be
    2**25 pixels, more than this image's largest power-of-two rectangle).  4096 x 2048 -> 61 x 31 leaves the cap of 64; -> 65 x 33 keeps T and
    A and has 65 taps.  With 3 output channels the weighted mode is the plain one, byte for byte."""
    p = pack
    large = huge_items(1 + mode)
    assert [resize.split(it[3], it[5]) for it in large[:4]] == [(4, 4), (4, 5), (4, 4), (4, 5)] and resize.taps(HH, 61) == 64
    wins = [p.window(it) for it in large]
    assert wins[1].colN.shape[2] == 65                                # an output column that really overlaps 65 source columns
    n, d = (np.concatenate(x) for x in zip(*[w.divisions(mode) for w in wins]))
    classes = rw.division_classes(n, d)
    print(mode, classes, "largest N %d, M %d, A %d" % (max(w.N.max() for w in wins), max(w.M.max() for w in wins), max(w.A.max() for w in wins)))
    assert classes["both below 2^32"] and classes["n from 2^32, d below"] and classes["d a power of two, n below 2^32"]
    if mode == ALPHA_WEIGHTED:
        assert classes["d from 2^32"] and classes["d a power of two, n from 2^32"]
        assert all((w.A == 0).any() for w in (wins[0], wins[1], wins[5])) and (wins[5].A == 0).all()
        assert np.all(wins[2].A == 1 << 30) and np.all(wins[3].A == 1 << 30) and wins[2].T == 1 << 23 and wins[2].M.max() >= B32
        assert wins[4].A.max() < B32 and (wins[4].M + wins[4].A[..., None] // 2).max() < B32 and wins[4].A.min() > 0
    assert max(w.N[..., :3].max() for w in wins[:2]) >= B32
    items = between(large, smalls(p, (SPRITE, 0, 3, 7, 1)))
    got = run(ctx, p, 4, items, mode)
    assert_items(p, got, items, 4, mode, mode)
    assert ctx.resize_stats()[:2] == (1, 1) and ctx.resize_stats()[2] >= slot(HW * HH * 4)
    got3 = run(ctx, p, 3, items, mode, front=64 + 1)
    assert_items(p, got3, items, 3, PLAIN, ("3 channels", mode))
    if mode == ALPHA_WEIGHTED:
        assert any(not np.array_equal(want(p, it, 4, PLAIN), want(p, it, 4, ALPHA_WEIGHTED)) for it in large)


# ------------------------------------------------------------------ 3: 65 taps at the smallest size
@pytest.mark.parametrize("channels", [4, 3])
def test_65_taps_at_the_smallest_size(ctx, pack, channels):
    """127 -> 2: the bound of 65 taps, sixteen lanes of five columns; noise, so every tap counts"""
    p = pack
    assert resize.split(127, 2) == (4, 5) and resize.taps(127, 2) == 65 and resize.taps(64, 1) == 64
    for mode in (PLAIN, ALPHA_WEIGHTED):
        for shift in (0, 1, 3):
            items = [(T127, 0, 0, 127, rh, 2, oh, flags) for flags in range(4) for (rh, oh) in ((127, 2), (64, 1))]
            got = run(ctx, p, channels, items, mode, front=64 + shift)
            assert_items(p, got, items, channels, mode, (channels, mode, shift))
            for j, it in enumerate(items):                            # ... and the windows say the same
                assert np.array_equal(got[j], rw.resized(p.decoded(T127, channels), it[1:5], it[5:7], it[7], mode).reshape(-1))


# ------------------------------------------------------------------ 4: the tile walk with many tiles per workgroup
def table_order(items):
    """the items in the order of their table entries (qoi_stage_plan.h: plan_items within one sub-batch): by image, else as given"""
    return sorted(items, key=lambda it: it[0])


def test_resize_walks_many_tiles_per_workgroup(ctx, pack, cus):
    """One sub-batch whose table reads [small, small, big, small x 5, big', small]: big is the identity of `huge` (69120 tiles), big' its
    reduction to a half (17280), the five between them 1 x 1 and 3 x 3 rectangles of `huge` itself (staged pixel indices up to 17.7e6 > 2**24).
    With at most 8 * cu workgroups each takes dozens of tiles: they start inside a big entry, end inside it, and step out of it across the
    small ones."""
    p = pack
    whole, half = (HUGE, 0, 0, HW, HH, HW, HH, 0), (HUGE, 0, 0, HW, HH, HW // 2, HH // 2, 0)
    inner = [(HUGE, HW - 1, HH - 1, 1, 1, 1, 1, 1), (HUGE, HW - 3, HH - 3, 3, 3, 2, 2, 2), (HUGE, 4097, 3641, 1, 1, 3, 3, 3), (HUGE, 0, HH - 1, 3, 1, 1, 1, 0),
             (HUGE, HW - 2, 3700, 2, 2, 5, 5, 1)]
    items = [(0, 0, 0, 1, 1, 1, 1, 0), (1, 5, 5, 1, 1, 2, 2, 3), whole] + inner + [half, (SPRITE, 129, 69, 1, 1, 1, 1, 2)]
    assert table_order(items) == items and (HH - 1) * HW + HW - 1 >= 1 << 24
    tiles = [resize.tiles(it[3], it[5], it[6]) for it in items]
    assert tiles == [1, 1, 69120, 1, 1, 1, 1, 1, 17280, 1] and sum(tiles) > 3 * 8 * cus
    per_wg = -(-sum(tiles) // (8 * cus))
    print("tiles", sum(tiles), "workgroups", 8 * cus, "tiles per workgroup", per_wg)
    assert per_wg >= 4
    for channels, mode, shift in ((4, ALPHA_WEIGHTED, 0), (3, PLAIN, 7)):
        got = run(ctx, p, channels, items, mode, front=64 + shift)
        assert ctx.resize_stats()[:2] == (1, 1)
        # the identity is the slice, and what decode_crops gives on the device
        D = p.decoded(HUGE, channels)
        assert np.array_equal(got[2], D.reshape(-1))
        buf = filled(64 + got[2].size + 64, GUARD)
        ctx.decode_crops(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, [(HUGE, 0, 0, HW, HH, 0)], buf.data_ptr(), [64])
        cropped = buf.cpu().numpy()
        assert np.array_equal(got[2], cropped[64:-64]) and np.all(cropped[:64] == GUARD) and np.all(cropped[-64:] == GUARD)
        # the half is the thumbnail at 2, and what decode_thumbnails gives on the device
        assert np.array_equal(got[8], p.box(HUGE, channels, 2, mode))
        reduced, _, _ = run_thumbnails(ctx, p, channels, [2] * p.n, mode)
        assert np.array_equal(got[8], reduced[HUGE])
        for j in (0, 1, 3, 4, 5, 6, 7, 9):
            assert np.array_equal(got[j], want(p, items[j], channels, mode)), (channels, j)
        # `huge` alone in its sub-batch, the small images in others: the same bytes
        staging = slot(HW * HH * 4)
        images, slots, subs, largest = resize.plan(p.descs, items, staging)
        assert images == [0, 1, HUGE, SPRITE] and subs == [(0, 2), (2, 1), (3, 1)] and largest == staging
        again = run(ctx, p, channels, items, mode, staging=staging, front=64 + shift)
        assert ctx.resize_stats() == (3, 3, largest, 4)
        assert all(np.array_equal(a, b) for a, b in zip(again, got))


def crop_tiles(nbytes):
    """tiles of an output of nbytes at a 16-aligned address or one byte off it (qoi_crop_core.h: crop_tiles; crops.items has one item per
    aligned 16-byte word)"""
    return -(-(-(-(nbytes + 15) // 16)) // 256)


def test_crops_walk_many_tiles_per_workgroup(ctx, pack, cus):
    """[small, small, whole, small x 5, four overlapping quarters with every flip, small] in one sub-batch"""
    p = pack
    qw, qh = 2400, 2000
    quarters = [(HUGE, 0, 0, qw, qh, 0), (HUGE, HW - qw, 0, qw, qh, 1), (HUGE, 0, HH - qh, qw, qh, 2), (HUGE, HW - qw, HH - qh, qw, qh, 3)]
    assert 2 * qw > HW and 2 * qh > HH
    inner = [(HUGE, HW - 1, HH - 1, 1, 1, 1), (HUGE, HW - 5, HH - 2, 5, 2, 2), (HUGE, 4097, 3641, 1, 1, 3), (HUGE, 0, HH - 1, 7, 1, 0), (HUGE, HW - 2, 3700, 2, 3, 1)]
    cs = [(0, 0, 0, 1, 1, 0), (1, 5, 5, 3, 3, 3), (HUGE, 0, 0, HW, HH, 0)] + inner + quarters + [(SPRITE, 100, 60, 30, 10, 2)]
    assert sorted(cs, key=lambda c: c[0]) == cs
    for channels, shift in ((3, 1), (4, 0)):
        nbytes = [c[3] * c[4] * channels for c in cs]
        tiles = [crop_tiles(n) for n in nbytes]
        assert sum(tiles) > 3 * 8 * cus and tiles[2] > 8 * cus and max(tiles[3:8]) == 1
        offsets = [64 + shift + int(x) for x in np.cumsum([0] + nbytes[:-1])]
        results = []
        for staging in (0, slot(HW * HH * 4)):
            buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
            ctx.decode_crops(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, cs, buf.data_ptr(), offsets, staging)
            assert ctx.crop_stats()[:2] == ((1, 1) if staging == 0 else (3, 3))
            got = buf.cpu().numpy()
            assert np.all(got[:offsets[0]] == GUARD) and np.all(got[-64:] == GUARD)
            results.append(got)
        assert np.array_equal(results[0], results[1])
        for j, (c, o, n) in enumerate(zip(cs, offsets, nbytes)):
            assert np.array_equal(results[0][o:o + n], crops.crop(p.decoded(c[0], channels), c[1:5], c[5]).reshape(-1)), (channels, j)


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_thumbnails_walk_many_tiles_per_workgroup(ctx, pack, cus, mode):
    """Every image is an entry: [small, small, huge, small x 5, wide, small, t127].  At f = 2 and 3 `huge` alone holds more than 3 * 8 * cu tiles
    (17280 and 7680); at 64 its 72 x 60 blocks of sixteen lanes are 270 tiles, one per workgroup - that call is here for sixteen lanes over
    staged pixel indices beyond 2**24."""
    p = pack
    from qoi_amd.packplan import plan
    for f, channels in ((2, 4), (3, 3), (64, 4), (3, 4)):
        lanes = 1 if f <= 4 else 16
        tiles = [-(-(-(-w // f) * -(-h // f) * lanes) // 256) for (w, h, _) in p.shapes]
        if f < 64:
            assert sum(tiles) > 3 * 8 * cus and tiles[HUGE] == (HW // f) * (HH // f) // 256
        else:
            assert tiles[HUGE] == 270
        got, _, _ = run_thumbnails(ctx, p, channels, [f] * p.n, mode)
        assert ctx.thumbnail_stats()[:2] == (1, 1)
        for i in range(p.n):
            w = p.box(i, channels, f, mode) if i == HUGE else thumbs.thumbnail(p.decoded(i, channels), f, mode).reshape(-1)
            assert np.array_equal(got[i], w), (f, channels, mode, i)
        if f == 2:
            staging = slot(HW * HH * 4)
            assert [c for _, c in plan([w * h * 4 for (w, h, _) in p.shapes], staging)] == [2, 1, 8]
            again, _, _ = run_thumbnails(ctx, p, channels, [f] * p.n, mode, staging=staging)
            assert ctx.thumbnail_stats()[:2] == (3, 3) and all(np.array_equal(a, b) for a, b in zip(again, got))


# ------------------------------------------------------------------ 5: the walk written out in cmp_pixels
def test_verify_and_compare_at_the_range_edges(ctx, pack, cus):
    """qoimi_verify_images / qoimi_compare_images over [small, small, huge, small ...]: clean, then with single pixels of the caller's side
    changed at pixel 0 of `huge`, at its last pixel, at the last pixel of a workgroup's tile range and at the first pixel of the next one -
    the ranges as the host cuts them: per_wg = ceil(tiles / grid), grid = min(tiles, 8 * cu)."""
    p = pack
    order = [0, 1, HUGE, 3, 4, 5, SPRITE]
    shapes = [p.shapes[i] for i in order]
    descs, so, sizes = [p.descs[i] for i in order], [p.so[i] for i in order], [p.sizes[i] for i in order]
    px = [p.px[i] for i in order]
    pix_off = [int(x) + 3 for x in np.cumsum([0] + [a.size + 1 for a in px[:-1]])]
    host = np.full(pix_off[-1] + px[-1].size + 64, GUARD, dtype=np.uint8)
    for o, a in zip(pix_off, px):
        host[o:o + a.size] = a
    tiles = [-(-w * h // CMP_TILE_PX) for (w, h, _) in shapes]
    total, first_tile = sum(tiles), sum(tiles[:2])
    grid = min(total, 8 * cus)
    per_wg = -(-total // grid)
    assert per_wg >= 2 and tiles[2] == HW * HH // CMP_TILE_PX
    wg = grid // 2                                                    # a workgroup in the middle: its range lies inside `huge`
    assert first_tile < wg * per_wg and (wg + 1) * per_wg < first_tile + tiles[2]
    edge = ((wg + 1) * per_wg - first_tile) * CMP_TILE_PX             # the first pixel of workgroup wg + 1
    planted = [0, edge - 1, edge, HW * HH - 1]
    print("tiles", total, "grid", grid, "per workgroup", per_wg, "planted", planted)

    def both(side_a):
        d_a = dev(side_a)
        got_v, first_v = ctx.verify_images(d_a.data_ptr(), pix_off, descs, p.packed.data_ptr(), so, sizes)
        # side B of the comparison: the device's own decode of every image at its channel count
        b_off = [int(x) for x in np.cumsum([0] + [a.size for a in px[:-1]])]
        d_b = filled(sum(a.size for a in px), GUARD)
        for ch in (3, 4):
            idx = [k for k, s in enumerate(shapes) if s[2] == ch]
            ctx.decode_images(p.packed.data_ptr(), [so[k] for k in idx], [sizes[k] for k in idx], [descs[k] for k in idx], ch, d_b.data_ptr(), [b_off[k] for k in idx])
        got_c, first_c = ctx.compare_images(d_a.data_ptr(), pix_off, 0, d_b.data_ptr(), b_off, 0, descs)
        assert np.array_equal(d_a.cpu().numpy(), side_a)
        return (got_v, first_v), (got_c, first_c)

    for got, first in both(host):
        assert first == -1 and not got["flags"].any() and not got["mismatched"].any() and (got["first"] == NONE).all()
    o = pix_off[2]
    for plant in ([edge - 1], [edge], [HW * HH - 1], [0], planted, planted[1:]):
        changed = host.copy()
        for q in plant:
            changed[o + 4 * q + (q & 3)] ^= 0x5A
        exp = np.zeros(len(order), dtype=DIFF_DTYPE)
        exp["first"] = NONE
        f = min(plant)
        exp[2] = (len(plant), f, pixel_word(changed[o:o + 4 * HW * HH], f, 4), pixel_word(px[2], f, 4), DIFF_PIXELS, 0)
        for got, first in both(changed):
            assert first == 2 and np.array_equal(got, exp), (plant, got[2], exp[2])


# ------------------------------------------------------------------ 6: the context afterwards
def test_the_context_afterwards(ctx, pack):
    """the items of tests/test_gpu_resize.py: test_mixed_pack over the small images of this pack, on the context that has staged 71 MB"""
    p = pack
    small = [i for i, s in enumerate(p.shapes) if s in MIXED_SHAPES]
    assert len(small) == len(MIXED_SHAPES)
    items = [it for i in small for it in standard(i, p.shapes[i][0], p.shapes[i][1], i)]
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run(ctx, p, channels, items, mode)
        for j, it in enumerate(items):
            assert np.array_equal(got[j], resize.resize(p.decoded(it[0], channels), it[1:5], it[5:7], it[7], mode).reshape(-1)), (channels, j, it)
        assert ctx.resize_stats()[:2] == (1, 1) and ctx.resize_stats()[3] == len(small)
    run(ctx, p, 4, [(HUGE, 0, 0, HW, HH, 72, 60, 0)], PLAIN)
    planned = ctx.resize_stats()[2]
    assert planned == slot(HW * HH * 4) == resize.plan(p.descs, [(HUGE, 0, 0, HW, HH, 72, 60, 0)], 0)[3]
    assert ctx.workspace_bytes()["decode"] >= planned + 4096
