"""QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP on the GPU (-m gpu), through qoimi_decode_warped, qoimi_decode_warped_tensors
and qoimi_decode_warped_indexed: every output is compared bit for bit, over its whole length, with the definition - the oracle decodes the
stream at the call's output channel count, qoi_amd/warp.py samples that, qoi_amd/tensors.py: convert makes the tensor (each u8 model is
computed once and shared).  The pack is small: one 40 x 24 image with 4 channels and one with 3; the rectangles are 1 x 1, 1 x 7, 7 x 1,
5 x 3 and 17 x 9, the outputs up to 48 x 40, so that whole and partial 16 x 16 tiles occur.  Outputs stand behind, between and in front of
guard bytes (gpu_calls.py: run_warp, run_label_tensors); every guard byte is checked after every call.  Before the three flags existed
every call here with one of them was rejected with "unknown flag bit"."""
import numpy as np
import pytest

from qoi_amd import tensors, warp
from qoi_amd.tensors import CHW, F16, HW, I64
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, WRAP
from gpu_calls import assert_outputs, run_label_tensors as run_tensors, run_warp
from gpu_pack import IMAGENET, Pack, batch_of
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FILL = 0x40C08020
RGBA, RGB = 0, 1
SHAPES = [(40, 24, 4), (40, 24, 3)]
RECTS = [(39, 23, 1, 1), (11, 5, 1, 7), (2, 20, 7, 1), (30, 1, 5, 3), (20, 12, 17, 9)]
BORDERS = (REFLECT, REFLECT_101, WRAP)
SAMPLINGS = (0, NEAREST, BICUBIC)


def pixels():
    rng = np.random.default_rng(20252)
    rgba = rng.integers(0, 256, size=(24, 40, 4), dtype=np.uint8)
    rgba[:, :, 3][rng.integers(0, 3, size=(24, 40)) == 0] = 0                # a third of the pixels transparent: the modes differ
    return [rgba, rng.integers(0, 256, size=(24, 40, 3), dtype=np.uint8)]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, SHAPES, pixels()))


_MODELS = {}


def model(p, it, och, mode=PLAIN):
    """the u8 result P of one item: computed once, never changed"""
    key = (tuple(it), och, mode)
    if key not in _MODELS:
        i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
        P = warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_bytes(p, got, items, och, mode, what):
    assert_outputs(got, [model(p, it, och, mode) for it in items], (what, och, mode))


def border_items(border, samplings=SAMPLINGS):
    """per sampling: every rectangle padded by more than its own size (the identity moved: numpy.pad) and turned by 30 degrees at half size
    into 33 x 18; the 17 x 9 rectangle turned into 48 x 40 (nine tiles, the lower ones partial); a translation hundreds of periods away; a
    sheared map at offsets next to -2**56 and +2**56"""
    items = []
    for sampling in samplings:
        flags = border | sampling
        for j, rect in enumerate(RECTS):
            cw, rh = rect[2:]
            items.append(warp.item(j & 1, rect, (cw + 19, rh + 13), (ONE, 0, -2 * ONE * 8, 0, ONE, -2 * ONE * 6), flags, FILL))
            items.append(warp.item(1 - (j & 1), rect, (33, 18), warp.rotation((cw, rh), (33, 18), 30.0, 0.5), flags, FILL))
        rect = RECTS[4]
        items.append(warp.item(RGBA, rect, (48, 40), warp.rotation((17, 9), (48, 40), 30.0, 0.6), flags, FILL))
        items.append(warp.item(RGB, RECTS[3], (19, 18), (ONE, 0, 2 * ONE * 5 * 300 + 777, 0, ONE, -2 * ONE * 3 * 500 - 999), flags, FILL))
        items.append(warp.item(RGBA, rect, (17, 5), (ONE, 31, 1 - 2 ** 56, -17, ONE, 2 ** 56 - 1), flags, FILL))
    return items


@pytest.mark.parametrize("channels,mode", [(4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN), (3, ALPHA_WEIGHTED)])
@pytest.mark.parametrize("border", BORDERS)
def test_items_against_the_model(ctx, pack, border, channels, mode):
    p = pack
    items = border_items(border)
    got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
    assert_bytes(p, got, items, channels, mode, "warped")
    assert ctx.warp_stats()[:2] == (1, 1)
    # the padded rectangle is numpy.pad of the decoded pixels, in every sampling
    pad_mode = {REFLECT: "symmetric", REFLECT_101: "reflect", WRAP: "wrap"}[border]
    for j, it in enumerate(items):
        if it[8:12] == (ONE, 0, 0, ONE) and it[14] == -2 * ONE * 8:
            i, x, y, cw, rh = it[:5]
            padded = np.pad(p.decoded(i, channels)[y:y + rh, x:x + cw], ((6, 7), (8, 11), (0, 0)), mode=pad_mode)
            assert np.array_equal(got[j], padded.reshape(-1)), (j, it)
    if channels == 4 and mode == ALPHA_WEIGHTED:
        assert items[10][5:8] == (48, 40, border)                       # the bilinear turn into nine tiles: the modes differ
        assert not np.array_equal(model(p, items[10], 4, PLAIN), model(p, items[10], 4, ALPHA_WEIGHTED))


def test_a_one_pixel_wide_rectangle_under_reflect_101(ctx, pack):
    """n == 1 has no period of 2n - 2: every column is column 0, the rows reflect about the edge pixels"""
    p = pack
    rect = RECTS[1]
    items = [warp.item(RGBA, rect, (21, 23), (ONE, 0, -2 * ONE * 10, 0, ONE, -2 * ONE * 8), REFLECT_101 | s, FILL) for s in SAMPLINGS]
    got = run_warp(ctx, p, 4, items, PLAIN, front=64 + 3)
    assert_bytes(p, got, items, 4, PLAIN, "1 x 7")
    x, y, cw, rh = rect
    padded = np.pad(p.decoded(RGBA, 4)[y:y + rh, x:x + cw], ((8, 8), (10, 10), (0, 0)), mode="reflect")
    assert all(np.array_equal(g, padded.reshape(-1)) for g in got)


@pytest.mark.parametrize("border", BORDERS)
def test_tensors(ctx, pack, border):
    """f16 CHW for every sampling; int64 HW - a label plane - for the nearest items"""
    p = pack
    for f, items in (((F16, CHW, *IMAGENET), border_items(border)), (tensors.fmt(I64, HW), border_items(border, (NEAREST,)))):
        for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
            got = run_tensors(ctx, p, "warp", channels, items, mode, f)
            for j, it in enumerate(items):
                w = tensors.convert(model(p, it, channels, mode), f).view(np.uint8).reshape(-1)
                assert got[j].size == w.size and np.array_equal(got[j], w), (f[:2], channels, j, it, int(np.argmax(got[j] != w)))
            assert ctx.tensor_stats()[:2] == (1, 1)


def test_indexed(ctx, pack):
    """through a seek index: the band is what is staged, the border is the rectangle's"""
    p = pack
    items = [it for border in BORDERS for it in border_items(border)[1::4]]
    intervals = [4, 8]                                             # (interval_rows * width is at least 128)
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, intervals)
    plain = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED)
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 1, call=lambda out, offsets: ctx.decode_warped_indexed(
        p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, items, ALPHA_WEIGHTED, out, offsets, intervals, points, firsts))
    assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "indexed")
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))


def test_mixed_items_and_a_call_without_a_border_item(ctx, pack):
    """items of every border and sampling with plain fill, REPLICATE and bicubic items in one call, one launch, at odd offsets with guard
    bytes in front and between: every item has its model's bytes, and the items without a border flag have, byte for byte, what a call made
    of them alone - the kernels of before - writes"""
    p = pack
    rect = RECTS[4]
    turn = warp.rotation((17, 9), (41, 29), 30.0, 0.6)
    others = [warp.item(j & 1, rect, (41, 29), turn, flags, FILL) for j, flags in enumerate((0, REPLICATE, NEAREST, NEAREST | REPLICATE, BICUBIC, BICUBIC | REPLICATE))]
    folded = [warp.item(j & 1, rect, (41, 29), turn, border | s, FILL) for j, (border, s) in enumerate((b, s) for b in BORDERS for s in SAMPLINGS)]
    items = [it for pair in zip(folded, others + others[:3]) for it in pair]              # in turn with and without a border flag
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        nbytes = 41 * 29 * channels
        offsets = [65 + j * nbytes + 2 * j - (j & 1) for j in range(len(items))]          # 65, then gaps of 1 and 3 bytes in turn
        got = run_warp(ctx, p, channels, items, mode, offsets=offsets)
        assert_bytes(p, got, items, channels, mode, "mixed")
        assert ctx.warp_stats()[:2] == (1, 1)
        alone = run_warp(ctx, p, channels, others, mode, front=64 + 1)
        assert_bytes(p, alone, others, channels, mode, "without a border item")
        assert all(np.array_equal(a, b) for a, b in zip(alone, got[1::2]))
    assert len({g.tobytes() for g in got}) == len(folded) + len(others)
    f = (F16, CHW, *IMAGENET)
    got = run_tensors(ctx, p, "warp", 4, items, PLAIN, f)
    alone = run_tensors(ctx, p, "warp", 4, others, PLAIN, f)
    for j, it in enumerate(items):
        assert np.array_equal(got[j], tensors.convert(model(p, it, 4), f).view(np.uint8).reshape(-1)), j
    assert all(np.array_equal(a, b) for a, b in zip(alone, got[1::2]))


def test_sub_batches(api, pack):
    """a small staging_bytes forces one sub-batch per image: the same bytes, one launch of the border kernel per sub-batch"""
    p = pack
    c = api.Context(0)
    try:
        items = border_items(REFLECT_101, (0,)) + border_items(WRAP, (BICUBIC,)) + border_items(REFLECT, (NEAREST,))
        single = run_warp(c, p, 4, items, ALPHA_WEIGHTED)
        images, slots, subs, largest = warp.plan(p.descs, items, 0)
        assert len(subs) == 1 and c.warp_stats() == (1, 1, largest, len(images))
        images, slots, subs, largest = warp.plan(p.descs, items, 1)
        assert len(subs) == len(images) == 2
        got = run_warp(c, p, 4, items, ALPHA_WEIGHTED, staging=1, front=64 + 1)
        assert c.warp_stats() == (2, 2, largest, 2)
        assert all(np.array_equal(x, y) for x, y in zip(got, single))
        assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "sub-batches")
    finally:
        c.close()
