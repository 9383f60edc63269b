"""QOIMI_WARP_BICUBIC on the GPU (-m gpu), through qoimi_decode_warped, qoimi_decode_warped_tensors and qoimi_decode_warped_indexed: every
output is compared bit for bit, over its whole length, with the definition - the oracle decodes the stream at the call's output channel
count, qoi_amd/warp.py samples that, qoi_amd/tensors.py: convert makes the tensor (each u8 model is computed once and shared).  The pack is
small: 24 x 20 photographs with 4 and with 3 channels, a 12 x 12 image whose alpha is 0 except for isolated texels, a 12 x 12 checkerboard of
0 and 255, a 16 x 64 strip, a 1 x 1 image and a 130 x 70 photograph.  Outputs stand behind, between and in front of guard bytes
(gpu_calls.py: run_warp, run_label_tensors); every guard byte is checked after every call."""
import numpy as np
import pytest

from qoi_amd import tensors, warp
from qoi_amd.packplan import slot
from qoi_amd.tensors import CHW, F16, F32, HW, HWC, I32, U8
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REPLICATE
from gpu_calls import assert_outputs, assert_warp_items as assert_items, run_label_tensors as run_tensors, run_warp, want_warp
from gpu_pack import IMAGENET, Batch, Pack, batch_of
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FILL = 0x40C08020
PHOTO4, PHOTO3, SPARSE, BOARD, STRIP, DOT, BIG = range(7)
SHAPES = [(24, 20, 4), (24, 20, 3), (12, 12, 4), (12, 12, 4), (16, 64, 4), (1, 1, 4), (130, 70, 4)]
CORNER = (16, 12, 8, 8)               # the bottom-right corner of the 24 x 20 photographs: bright, its surroundings dark


def pixels():
    rng = np.random.default_rng(20251)
    photo4 = rng.integers(0, 96, size=(20, 24, 4), dtype=np.uint8)
    photo3 = rng.integers(0, 96, size=(20, 24, 3), dtype=np.uint8)
    for ph in (photo4, photo3):
        ph[12:, 16:] = rng.integers(160, 256, size=(8, 8, ph.shape[2]), dtype=np.uint8)
    sparse = rng.integers(0, 256, size=(12, 12, 4), dtype=np.uint8)
    sparse[:, :, 3] = 0
    sparse[4, 4, 3], sparse[7, 8, 3] = 255, 200
    yy, xx = np.mgrid[0:12, 0:12]
    board = np.repeat((((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)[:, :, None], 4, axis=2)
    strip = rng.integers(0, 256, size=(64, 16, 4), dtype=np.uint8)
    dot = np.array([[[200, 100, 50, 180]]], dtype=np.uint8)
    big = rng.integers(0, 256, size=(70, 130, 4), dtype=np.uint8)
    return [photo4, photo3, sparse, board, strip, dot, big]


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


def cubic_items(flag=BICUBIC):
    """a 1 x 1 and a 2 x 2 rectangle, where every tap clamps or fills; the corner rectangle into 17 x 17 and 33 x 5 (partial tiles on both
    axes); the identity; turns by 30 and 90 degrees; a shear; 3 x with REPLICATE and with fill; a 4 x reduction; positions far outside;
    the sparse-alpha image at a quarter-pixel offset; the checkerboard at half-pixel positions"""
    half = (ONE, 0, ONE, 0, ONE, ONE)
    return [warp.item(DOT, (0, 0, 1, 1), (5, 4), (ONE // 3, 0, 0, 0, ONE // 3, 0), flag, FILL),
            warp.item(DOT, (0, 0, 1, 1), (5, 4), (ONE // 3, 0, 0, 0, ONE // 3, 0), flag | REPLICATE, FILL),
            warp.item(PHOTO4, (22, 18, 2, 2), (7, 5), warp.rotation((2, 2), (7, 5), 20.0, 2.0), flag, FILL),
            warp.item(PHOTO4, (22, 18, 2, 2), (7, 5), warp.rotation((2, 2), (7, 5), 20.0, 2.0), flag | REPLICATE, FILL),
            warp.item(PHOTO4, CORNER, (17, 17), warp.rotation((8, 8), (17, 17), 0.0, 1.7), flag | REPLICATE, FILL),
            warp.item(PHOTO3, CORNER, (33, 5), warp.rotation((8, 8), (33, 5), 0.0, 1.7), flag, FILL),
            warp.item(PHOTO4, CORNER, (8, 8), flags=flag, fill=FILL),
            warp.item(BIG, (10, 8, 100, 50), (41, 29), warp.rotation((100, 50), (41, 29), 30.0, 0.6), flag, FILL),
            warp.item(BIG, (10, 8, 100, 50), (23, 40), warp.rotation((100, 50), (23, 40), 90.0, 0.4), flag | REPLICATE, 0),
            warp.item(PHOTO3, (0, 0, 24, 20), (17, 40), (ONE, 23001, -40000, -9001, ONE + 701, 12345), flag, 0x00FFFFFF),
            warp.item(PHOTO4, CORNER, (24, 24), (ONE // 3, 0, 0, 0, ONE // 3, 0), flag | REPLICATE, FILL),
            warp.item(PHOTO4, CORNER, (24, 24), (ONE // 3, 0, 0, 0, ONE // 3, 0), flag, FILL),
            warp.item(BIG, (1, 1, 128, 68), (32, 17), (4 * ONE, 0, 0, 0, 4 * ONE, 0), flag, FILL),
            warp.item(PHOTO4, CORNER, (6, 3), (ONE, 0, 900 * ONE, 0, ONE, -700 * ONE), flag, FILL),
            warp.item(SPARSE, (0, 0, 12, 12), (23, 23), (ONE // 2, 0, ONE // 4, 0, ONE // 2, ONE // 4), flag | REPLICATE, 0),
            warp.item(BOARD, (0, 0, 12, 12), (11, 11), half, flag | REPLICATE, 0)]


@pytest.mark.parametrize("channels,mode", [(4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN)])
def test_items_against_the_model(ctx, pack, channels, mode):
    p = pack
    items = cubic_items()
    got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
    assert_bytes(p, got, items, channels, mode, "warped")
    assert ctx.warp_stats()[:2] == (1, 1)
    # the identity is the rectangle, byte for byte; the far item is all fill
    assert np.array_equal(got[6].reshape(8, 8, channels), p.decoded(PHOTO4, channels)[12:, 16:])
    assert np.array_equal(got[13].reshape(-1, channels), np.tile([(FILL >> (8 * k)) & 255 for k in range(channels)], (18, 1)))
    # the checkerboard overshoots into both clamps
    assert got[15].min() == 0 and got[15].max() == 255
    if channels == 4:
        plain, wgt = model(p, items[14], 4, PLAIN), model(p, items[14], 4, ALPHA_WEIGHTED)
        assert not np.array_equal(plain, wgt) and np.array_equal(plain[..., 3], wgt[..., 3])


def test_orientations_equal_the_bilinear_call(api, ctx, pack):
    """every position is a pixel centre: the weights are (0, 2**15, 0, 0) and the device writes the bilinear call's bytes"""
    p = pack
    tent, cubic = [], []
    for i, rect in ((PHOTO4, CORNER), (PHOTO3, (3, 2, 17, 13)), (DOT, (0, 0, 1, 1))):
        for o in range(1, 9):
            w, h, ch = p.shapes[i]
            it = api.warp_orient(w, h, ch, rect, o)
            it.image = i
            tent.append(warp.fields(it))
            it.flags = BICUBIC | (REPLICATE if o & 1 else 0)
            cubic.append(warp.fields(it))
    without = run_warp(ctx, p, 4, tent, PLAIN, front=64 + 3)
    with_flag = run_warp(ctx, p, 4, cubic, ALPHA_WEIGHTED, front=64 + 3)
    for j, (a, b) in enumerate(zip(without, with_flag)):
        assert np.array_equal(a, b), j
        assert np.array_equal(b, model(p, cubic[j], 4, ALPHA_WEIGHTED).reshape(-1)), j


def test_mixed_items_and_odd_offsets(ctx, pack):
    """bilinear, nearest and bicubic items in one call, one launch: every item has its own model's bytes; the outputs stand at odd byte
    offsets with guard bytes between them"""
    p = pack
    turn = warp.rotation((100, 50), (41, 29), 30.0, 0.6)
    items = [warp.item(BIG, (10, 8, 100, 50), (41, 29), turn, flag, FILL) for flag in (0, BICUBIC, NEAREST, BICUBIC | REPLICATE, REPLICATE, NEAREST | REPLICATE)]
    nbytes = 41 * 29 * 4
    offsets = [65 + j * nbytes + 2 * j - (j & 1) for j in range(len(items))]            # 65, then gaps of 1 and 3 bytes in turn
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, offsets=offsets)
    assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "mixed")
    assert ctx.warp_stats()[:2] == (1, 1)
    assert len({g.tobytes() for g in got}) == len(items)
    got = run_warp(ctx, p, 3, items, PLAIN, front=64 + 1)
    assert_bytes(p, got, items, 3, PLAIN, "mixed")


def test_a_call_without_a_bicubic_item_is_unchanged(ctx, pack):
    """the launcher choice: a call none of whose items carries the flag runs the kernels it always ran and writes the same bytes"""
    p = pack
    items = [it[:7] + (it[7] & ~BICUBIC,) + it[8:] for it in cubic_items()[2:10]] + [it[:7] + ((it[7] & ~BICUBIC) | NEAREST,) + it[8:] for it in cubic_items()[7:9]]
    assert not any(it[7] & BICUBIC for it in items)
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        assert_bytes(p, run_warp(ctx, p, channels, items, mode, front=64 + 1), items, channels, mode, "no bicubic item")
    f = (F16, CHW, *IMAGENET)
    got = run_tensors(ctx, p, "warp", 4, items, PLAIN, f)
    for j, it in enumerate(items):
        assert np.array_equal(got[j], tensors.convert(model(p, it, 4), f).view(np.uint8).reshape(-1)), j


def test_sub_batches(api, pack):
    """a small staging_bytes forces one sub-batch per image: the same bytes, one launch of the bicubic kernel per sub-batch"""
    p = pack
    c = api.Context(0)
    try:
        items = cubic_items()
        single = run_warp(c, p, 4, items, ALPHA_WEIGHTED)
        images, slots, subs, largest = warp.plan(p.descs, items, 0)
        assert len(subs) == 1 and c.warp_stats() == (1, 1, largest, len(images))
        images, slots, subs, largest = warp.plan(p.descs, items, 1)
        assert len(subs) == len(images) == 6 and largest == slot(130 * 69 * 4)
        got = run_warp(c, p, 4, items, ALPHA_WEIGHTED, staging=1)
        assert c.warp_stats() == (6, 6, largest, 6)
        assert all(np.array_equal(x, y) for x, y in zip(got, single))
        assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "sub-batches")
    finally:
        c.close()


@pytest.mark.parametrize("dtype,layout", [(F16, CHW), (F32, HWC), (U8, HWC), (I32, HW)])
def test_tensors(ctx, pack, dtype, layout):
    p = pack
    items = cubic_items()
    f = tensors.fmt(dtype, layout) if dtype in (U8, I32) else (dtype, layout, *IMAGENET)
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run_tensors(ctx, p, "warp", channels, items, mode, f)
        for j, it in enumerate(items):
            w = tensors.convert(model(p, it, channels, mode), f).view(np.uint8).reshape(-1)
            assert got[j].size == w.size and np.array_equal(got[j], w), (dtype, layout, channels, j, int(np.argmax(got[j] != w)))
        if dtype == U8:                                                   # ... which is the byte call
            assert all(np.array_equal(a, b) for a, b in zip(got, run_warp(ctx, p, channels, items, mode)))
    assert ctx.tensor_stats()[:2] == (1, 1)


def test_indexed_band_at_the_bottom(ctx, pack):
    """a rectangle in the last rows of the 64-row strip through a seek index: the band is what is staged, the border is the rectangle's"""
    p = pack
    items = [warp.item(STRIP, (2, 50, 13, 14), (33, 18), warp.rotation((13, 14), (33, 18), 30.0, 1.8), BICUBIC | (j & 1), FILL) for j in range(2)]
    items.append(warp.item(BIG, (10, 40, 100, 30), (17, 17), warp.rotation((100, 30), (17, 17), -20.0, 0.3), BICUBIC, FILL))
    intervals = [8, 8, 12, 12, 8, 128, 16]                         # (interval_rows * width is at least 128)
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, intervals)
    plain = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED)
    plain_stats = ctx.warp_stats()
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, call=lambda out, offsets: ctx.decode_warped_indexed(
        p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, items, ALPHA_WEIGHTED, out, offsets, intervals, points, firsts))
    assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "indexed")
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert ctx.warp_stats()[2] < plain_stats[2]                          # the bands are shorter than the images' heads


# ------------------------------------------------------------------ the tile walk and positions past 2^32 (the counterparts of test_gpu_warp.py)
SAMPLINGS = (BICUBIC, BICUBIC | REPLICATE, NEAREST, 0)


def test_tile_walk_regimes(api, ctx, oracle, pack):
    """(qoi_dev.h: walk_tiles, as warp_cubic_walk calls it) a launch with ONE table entry, a bicubic one, its 12 tiles spread over as many
    workgroups; and more tiles than the grid's clamp of 8 workgroups per compute unit - 37 more items of one tile each, their samplings in
    turn bicubic with fill, bicubic with REPLICATE, nearest and bilinear - so that a workgroup takes two tiles and steps from an entry of one
    sampling to an entry of another.  The 3-byte outputs stand back to back at an odd front: neighbours share aligned words."""
    import torch
    one = warp.item(BIG, (0, 0, 130, 70), (61, 47), warp.rotation((130, 70), (61, 47), 30.0, 0.5), BICUBIC, FILL)
    assert warp.tiles(61, 47) == 12 and warp.tiles(1, 1) == 1
    assert_bytes(pack, run_warp(ctx, pack, 4, [one], ALPHA_WEIGHTED), [one], 4, ALPHA_WEIGHTED, "one entry")
    assert ctx.warp_stats()[:2] == (1, 1)
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    p = Pack(ctx, oracle, Batch(api, oracle, [(8, 8, 4)], ["noise"]))
    items = [warp.item(0, (j % 7, (j // 7) % 7, 2, 2), (1, 1), (ONE, 0, (j % 5) * 9000, 0, ONE, (j % 3) * 20000), SAMPLINGS[j & 3], FILL) for j in range(n)]
    assert all(items[j][7] != items[j + 1][7] for j in range(n - 1)) and {it[7] for it in items} == set(SAMPLINGS)
    for channels, mode in ((3, PLAIN), (4, ALPHA_WEIGHTED)):
        assert_items(p, run_warp(ctx, p, channels, items, mode, front=64 + 5), items, channels, mode, ("many", channels))
        assert ctx.warp_stats()[:2] == (1, 1)


def wide_maps():
    """the three maps of test_gpu_warp.py: test_positions_past_32_bits over the 33000 x 3 image - the 9 columns from 32990 on, the same turned
    by 180 degrees, an enlargement by 3 and 2 that begins half a row above the image - and a fourth whose 20 output columns walk a quarter
    of a pixel each across the right edge: k0 goes from 32997 to 33001, so that in turn k0 + 2, k0 + 1, k0 and k0 - 1 leave the rectangle"""
    return [((9, 3), (ONE, 0, 2 * 32990 * ONE, 0, ONE, 0)), ((9, 3), (-ONE, 0, 2 * 32999 * ONE + 777, 0, -ONE, 2 * 3 * ONE - 999)),
            ((40, 5), (ONE // 3, 0, 2 * 32985 * ONE + 4321, 0, ONE // 2, -ONE)), ((20, 3), (ONE // 4, 0, 2 * 32997 * ONE + ONE, 0, ONE, 0))]


def test_positions_past_32_bits(api, ctx, oracle):
    """an image of 33000 x 3, a rectangle over all its columns: Px passes 2**32 on the device (column 32768 lies at 2**32 + 2**16).  Every map
    with BICUBIC and with BICUBIC | REPLICATE - warp_cubic_axis tests the border on the 64-bit index before it narrows, in the fill form and
    in the clamp form - and with NEAREST; the nearest items also alone, in a call that stays with warp_gather.  As bytes and as tensors."""
    cw = 33000
    p = Pack(ctx, oracle, Batch(api, oracle, [(cw, 3, 4)], ["noise"]))
    rect = (0, 0, cw, 3)
    cubic = [warp.item(0, rect, out, m, flags, FILL) for out, m in wide_maps() for flags in (BICUBIC, BICUBIC | REPLICATE)]
    near = [warp.item(0, rect, out, m, NEAREST | (j & 1), FILL) for j, (out, m) in enumerate(wide_maps())] + [warp.item(0, rect, (20, 3), wide_maps()[3][1], NEAREST, FILL)]
    assert all(it[14] > 2 ** 32 for it in cubic + near)
    # the border item: an output column whose k0 - 1 is the last column of the rectangle while k0 + 2 lies outside, and every stage before it
    a, _, c, _, _, _ = wide_maps()[3][1]
    k0 = [(a * (2 * X + 1) + c - ONE) >> 17 for X in range(20)]
    assert sorted(set(k0)) == [32997, 32998, 32999, 33000, 33001] and any(k - 1 == cw - 1 and k + 2 >= cw for k in k0) and any(k + 2 == cw for k in k0)
    for items, what in ((cubic + near, "bicubic and nearest"), (near, "nearest alone")):
        for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
            got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
            assert_items(p, got, items, channels, mode, ("wide", what, channels))
            assert ctx.warp_stats()[:2] == (1, 1)
        f = (F16, CHW, *IMAGENET) if items is near else tensors.fmt(I32, HWC)
        got = run_tensors(ctx, p, "warp", 4, items, ALPHA_WEIGHTED, f)
        for j, it in enumerate(items):
            w = tensors.convert(want_warp(p, it, 4, ALPHA_WEIGHTED).reshape(it[6], it[5], 4), f).view(np.uint8).reshape(-1)
            assert got[j].size == w.size and np.array_equal(got[j], w), ("wide tensors", what, j)
    # the first map is a crop: the rectangle's columns from 32990 on, byte for byte, under either sampling
    crop = p.decoded(0, 4)[:, 32990:32999].reshape(-1)
    got = run_warp(ctx, p, 4, [cubic[0], cubic[1], near[0]], PLAIN)
    assert all(np.array_equal(g, crop) for g in got)
