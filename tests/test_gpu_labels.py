"""Label tensors on the GPU (-m gpu): QOIMI_FILTER_NEAREST of qoimi_decode_tensors (the kernel tensor_nearest), the integer dtypes
QOIMI_TENSOR_I32 / _I64 and the one-plane layout QOIMI_TENSOR_HW through every filter and the warp.  The expectation is always the
definition - the oracle decodes the stream at the call's output channel count, qoi_amd/nearest.py (or the model of the other filter, or
warp.py) resamples that, qoi_amd/tensors.py: convert makes the tensor; each u8 model is computed once and shared - and every comparison is of
bits and covers the whole output.  Every call lays its outputs at element-aligned but otherwise odd addresses - the first at 1 past a multiple
of 64 for u8, at 2 / 4 / 8 past one for the elements of 2 / 4 / 8 bytes - with 1 to 3 guard bytes (0xA5) between neighbours, rounded up to whole
elements; every guard byte is checked after every call."""
import ctypes

import numpy as np
import pytest

from qoi_amd import nearest, tensors, warp
from qoi_amd.tensors import (ALPHA_WEIGHTED, BF16, CHW, F16, F32, FILTER_AREA, FILTER_BICUBIC, FILTER_BILINEAR, FILTER_LANCZOS, FILTER_NEAREST, HW, HWC, I32, I64,
                             PLAIN, U8)
from gpu_calls import fmt_of, run_label_tensors as run
from gpu_pack import E_ARG, GUARD, Batch, Pack, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DOT, LINE, ODD, WIDE = 0, 1, 2, 3
SHAPES = [(1, 1, 3), (130, 1, 3), (37, 29, 3), (70, 45, 4)]
DTYPES = (U8, F16, BF16, F32, I32, I64)
LAYOUTS = (HWC, CHW, HW)

# 37 x 29 to 50 x 41 (2050 pixels: nine tiles, the last partial), 70 x 45 to 3 x 2, 1 x 1 to 7 x 5, equal size, 2 wide to 41 wide (14 to 23
# high: centres on cell boundaries), 130 to 1 and 129 to 257; the flips take turns; three items on one image
ITEMS = [(ODD, 0, 0, 37, 29, 50, 41, 0), (WIDE, 0, 0, 70, 45, 3, 2, 3), (DOT, 0, 0, 1, 1, 7, 5, 1), (ODD, 3, 5, 31, 23, 31, 23, 2), (ODD, 1, 1, 2, 14, 41, 23, 1),
         (LINE, 0, 0, 130, 1, 1, 1, 0), (LINE, 1, 0, 129, 1, 257, 1, 3), (WIDE, 5, 3, 63, 41, 20, 8, 0)]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, Batch(api, oracle, SHAPES, ["noise"] * 4))


_MODELS = {}


def model(p, filt, it, och, mode=PLAIN):
    """the u8 result P of one item: computed once, never changed"""
    key = (filt, tuple(it), och, mode)
    if key not in _MODELS:
        if filt == "warp":
            i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
            P = warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode)
        else:
            i, x, y, cw, rh, ow, oh, flags = it
            P = tensors.tensors(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, filt, mode)       # U8 HWC: the filter's bytes
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_items(p, got, filt, items, och, mode, f, what):
    for j, it in enumerate(items):
        w = tensors.convert(model(p, filt, it, och, mode), f).view(np.uint8).reshape(-1)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, filt, j, it[:8], int(np.argmax(got[j] != w)) // tensors.elem(f[0]))


# ------------------------------------------------------------------ 1: the nearest filter
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nearest_in_every_format(ctx, pack, dtype, layout):
    f = fmt_of(dtype, layout)
    for channels, mode in ((4, PLAIN), (3, ALPHA_WEIGHTED)):
        assert_items(pack, run(ctx, pack, FILTER_NEAREST, channels, ITEMS, mode, f), FILTER_NEAREST, ITEMS, channels, PLAIN, f, (dtype, layout, channels))
    assert ctx.tensor_stats()[:2] == (1, 1) and ctx.tensor_stats()[3] == 4
    assert nearest.tiles(50, 41) == 9 and 50 * 41 % 256 != 0


def test_nearest_flips_and_channel_counts(ctx, pack):
    f = tensors.fmt(I64, HW)
    for flags in range(4):
        items = [it[:7] + (flags,) for it in ITEMS]
        for channels in (3, 4):
            assert_items(pack, run(ctx, pack, FILTER_NEAREST, channels, items, PLAIN, tensors.fmt(U8, HWC)), FILTER_NEAREST, items, channels, PLAIN, tensors.fmt(U8, HWC), ("flip", flags))
        assert_items(pack, run(ctx, pack, FILTER_NEAREST, 4, items, PLAIN, f), FILTER_NEAREST, items, 4, PLAIN, f, ("flip", flags))
    # channels = 0: the output channel count is the images' - the three 3-channel images, then the 4-channel one
    for items in ([it for it in ITEMS if it[0] != WIDE], [it for it in ITEMS if it[0] == WIDE]):
        och = pack.shapes[items[0][0]][2]
        for g in (tensors.fmt(I32, CHW), f):
            assert_items(pack, run(ctx, pack, FILTER_NEAREST, 0, items, PLAIN, g), FILTER_NEAREST, items, och, PLAIN, g, ("channels 0", och))
    # the label of a pixel is its first byte: I64 HW of an equal-size item is the decoded rectangle's channel 0
    got = run(ctx, pack, FILTER_NEAREST, 0, [(ODD, 3, 5, 31, 23, 31, 23, 0)], PLAIN, f)[0].view(np.int64).reshape(23, 31)
    assert np.array_equal(got, pack.decoded(ODD, 3)[5:28, 3:34, 0])


def test_nearest_sub_batches(api, pack):
    """a staging of one byte: one image per sub-batch, three of them"""
    c = api.Context(0)
    try:
        items = [it for it in ITEMS if it[0] != DOT]
        f = tensors.fmt(I64, HW)
        single = run(c, pack, FILTER_NEAREST, 4, items, PLAIN, f)
        assert c.tensor_stats()[:2] == (1, 1) and c.tensor_stats()[3] == 3
        _, _, subs, largest = nearest.plan(pack.descs, items, 1)
        assert len(subs) == 3
        forced = run(c, pack, FILTER_NEAREST, 4, items, PLAIN, f, staging=1)
        assert c.tensor_stats() == (3, 3, largest, 3), c.tensor_stats()
        assert all(np.array_equal(x, y) for x, y in zip(forced, single))
        assert_items(pack, forced, FILTER_NEAREST, items, 4, PLAIN, f, "three sub-batches")
    finally:
        c.close()


def test_nearest_tile_walk(ctx, pack):
    """more tiles than the grid's clamp of 8 workgroups per compute unit: one item of 1 x 1 to 800 x 700 (2188 tiles) among 40 items of one
    tile each, so that a workgroup takes several tiles and steps from item to item (qoi_dev.h: walk_tiles)"""
    import torch
    assert 8 * torch.cuda.get_device_properties(0).multi_processor_count < 2188 + 40
    small = [(ODD, j % 30, j % 20, 7, 9, 5 + j % 3, 4, j & 3) for j in range(20)]
    items = small + [(WIDE, 2, 1, 1, 1, 800, 700, 0)] + [(WIDE, j, j, 40 + j % 7, 20, 16, 16, j & 3) for j in range(20)]
    f = tensors.fmt(I64, HW)
    assert_items(pack, run(ctx, pack, FILTER_NEAREST, 4, items, PLAIN, f), FILTER_NEAREST, items, 4, PLAIN, f, "many tiles")
    assert ctx.tensor_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 2: the new formats through the other kernels
@pytest.mark.parametrize("filt, f, it", [(FILTER_AREA, (I64, HW), (WIDE, 5, 3, 63, 41, 9, 7, 1)), (FILTER_BILINEAR, (I32, CHW), (ODD, 0, 0, 37, 29, 50, 41, 2)),
                                         (FILTER_BICUBIC, (I64, HWC), (WIDE, 0, 0, 70, 45, 33, 17, 3)), (FILTER_LANCZOS, (F16, HW), (ODD, 3, 5, 31, 23, 17, 40, 0))],
                         ids=["area", "tent", "bicubic", "lanczos"])
def test_the_other_filters_take_the_new_formats(ctx, pack, filt, f, it):
    f = fmt_of(*f)
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        items = [it, (DOT, 0, 0, 1, 1, 3, 3, 0)]
        assert_items(pack, run(ctx, pack, filt, channels, items, mode, f), filt, items, channels, mode, f, (channels, mode))
    g = tensors.fmt(I64, HW)
    assert_items(pack, run(ctx, pack, filt, 4, [it], PLAIN, g), filt, [it], 4, PLAIN, g, "I64 HW")


def test_warp_with_and_without_nearest_in_one_call(ctx, pack):
    m = warp.rotation((63, 41), (33, 18), 30.0, 0.9)
    items = [warp.item(WIDE, (5, 3, 63, 41), (33, 18), m, warp.NEAREST, 0x40C08020), warp.item(WIDE, (5, 3, 63, 41), (33, 18), m, warp.REPLICATE, 0),
             warp.item(ODD, (0, 0, 37, 29), (74, 58), (32768, 0, 0, 0, 32768, 0), warp.NEAREST | warp.REPLICATE, 0)]
    f = tensors.fmt(I64, HW)
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run(ctx, pack, "warp", channels, items, mode, f)
        assert_items(pack, got, "warp", items, channels, mode, f, ("warp", channels))
    assert not np.array_equal(got[0], got[1])                         # the flag is the item's: selection and interpolation differ
    # the third item's map is a scale by 2: the nearest FILTER of the same rectangle
    assert np.array_equal(got[2], tensors.convert(model(pack, FILTER_NEAREST, (ODD, 0, 0, 37, 29, 74, 58, 0), 3), f).view(np.uint8).reshape(-1))
    g = tensors.fmt(I32, CHW)
    assert_items(pack, run(ctx, pack, "warp", 4, items, PLAIN, g), "warp", items, 4, PLAIN, g, "warp I32 CHW")


# ------------------------------------------------------------------ 3: an output that begins past 2^32 in d_out
def test_an_output_past_4_gib(ctx, pack):
    """I64 HW at d_out + 2^32 + 8 * 12345: the offset's high half is not zero; the alias 2^32 lower in the same allocation stays the guard"""
    import torch
    B32, room = 1 << 32, 8 << 20
    it = (ODD, 0, 0, 37, 29, 50, 41, 3)
    f = tensors.fmt(I64, HW)
    want = tensors.convert(model(pack, FILTER_NEAREST, it, 3), f).view(np.uint8).reshape(-1)
    off = B32 + 8 * 12345
    assert off + want.size < B32 + room
    arena = filled(B32 + room, GUARD)
    try:
        ctx.decode_tensors(pack.packed.data_ptr(), pack.so, pack.sizes, pack.descs, 3, [it], FILTER_NEAREST, PLAIN, f, arena.data_ptr(), [off])
        got = arena[off:off + want.size].cpu().numpy()
        assert np.array_equal(got, want), int(np.argmax(got != want)) // 8
        arena[off:off + want.size].fill_(GUARD)
        assert bool((arena.view(torch.int64) == int.from_bytes(bytes([GUARD]) * 8, "little", signed=True)).all()), "a byte outside the output was written"
    finally:
        del arena
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4: rejections on a live context, and the context afterwards
def test_rejections_leave_the_output_untouched(api, ctx, pack):
    p = pack
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    two = [(WIDE, 0, 0, 70, 45, 10, 10, 0), (ODD, 0, 0, 8, 8, 8, 8, 1)]              # 800 and 512 bytes as I64 HW
    ok = tensors.fmt(I64, HW)
    one, zero = (1.0,) * 4, (0.0,) * 4

    def fm(f):
        return api.tensor_format(f)

    def call(items=two, offsets=(128, 128 + 800), channels=4, filter=FILTER_NEAREST, f=ok):
        arr = (api.QoimiResize * len(items))(*[api.QoimiResize(*it) for it in items])
        t = fm(f)
        return lib.qoimi_decode_tensors(ctx._h, *args, channels, arr, len(items), filter, 0, ctypes.byref(t), buf.data_ptr(), (ctypes.c_size_t * len(items))(*offsets), 0, None)

    assert call() == 0, api.last_error()                                              # side by side: accepted
    got = buf.cpu().numpy()
    for it, o, nb in ((two[0], 128, 800), (two[1], 928, 512)):
        assert np.array_equal(got[o:o + nb], tensors.convert(model(p, FILTER_NEAREST, it, 4), ok).view(np.uint8).reshape(-1))
    assert np.all(got[:128] == GUARD) and np.all(got[928 + 512:] == GUARD)
    stats = ctx.tensor_stats()
    assert stats[:2] == (1, 1) and stats[3] == 2
    buf.fill_(GUARD)
    rejected = [
        (lambda: call(filter=8), "filter"), (lambda: call(filter=10), "filter"), (lambda: call(filter=2), "filter"),
        (lambda: call(f=(4, HW, one, zero)), "dtype"), (lambda: call(f=(7, HW, one, zero)), "dtype"), (lambda: call(f=(I64, 2, one, zero)), "layout"), (lambda: call(f=(I64, 4, one, zero)), "layout"),
        (lambda: call(f=(I64, HW, (1.0, 1.0, 1.0, 2.0), zero)), "QOIMI_TENSOR_I64"), (lambda: call(f=(I32, HW, one, (0.0, 0.0, -0.0, 0.0))), "QOIMI_TENSOR_I32"),
        (lambda: call(offsets=(132, 1024)), "multiple of the element size"), (lambda: call(offsets=(128, 1028)), "multiple of the element size"),
        (lambda: call(offsets=(128, 128 + 792)), "overlap"), (lambda: call(offsets=(128, 128 + 3192), f=(I64, HWC, one, zero)), "overlap"),     # HWC: 3200 bytes
        (lambda: call(items=[(WIDE, 66, 0, 10, 10, 10, 10, 0)], offsets=(64,)), "leaves"), (lambda: call(items=[(WIDE, 0, 0, 10, 10, 10, 10, 4)], offsets=(64,)), "flag"),
        (lambda: call(items=[(WIDE, 0, 0, 1, 1, 16385, 1, 0)], offsets=(64,)), "16384"), (lambda: call(items=[(WIDE, 0, 0, 1, 1, 1, 16385, 0)], offsets=(64,)), "16384"),
        (lambda: call(items=[(WIDE, 0, 0, 70, 1, 1, 1, 0)], offsets=(64,), filter=FILTER_AREA), "64"),
        (lambda: call(items=[(ODD, 0, 0, 1, 1, 1, 1, 0), (WIDE, 0, 0, 1, 1, 1, 1, 0)], offsets=(64, 128), channels=0), "channel"),
    ]
    for c, word in rejected:
        assert c() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.tensor_stats() == stats, word
    # 70 to 1 is no fault of the nearest filter's, and the context works afterwards
    assert call(items=[(WIDE, 0, 0, 70, 45, 1, 1, 0)], offsets=(64,)) == 0, api.last_error()
    assert int(buf[64:72].cpu().numpy().view(np.int64)[0]) == int(p.decoded(WIDE, 4)[22, 35, 0])
    assert_items(p, run(ctx, p, FILTER_NEAREST, 3, ITEMS[:3], PLAIN, ok), FILTER_NEAREST, ITEMS[:3], 3, PLAIN, ok, "afterwards")
