"""qoimi_decode_tensors and qoimi_decode_warped_tensors on the GPU (-m gpu): the resampled rectangles of a pack written as u8, f16, bf16 or f32
tensors, HWC or CHW, scaled and shifted per channel.  The expectation is always the definition - the oracle decodes the stream at the call's
output channel count, qoi_amd/resize.py, bilinear.py or warp.py resample that, qoi_amd/tensors.py: convert makes the tensor (each u8 model is
computed once and shared) - and U8 with HWC is also compared with qoimi_decode_resized / _bilinear / _warped on the device.  Every comparison
is of bits and covers the whole output.
Every call lays its outputs at element-aligned but otherwise odd addresses - the first at 1 past a multiple of 64 for u8, at 2 past a multiple
of 16 for the 2-byte types, at 4 past one for f32 - with 1 to 3 guard bytes (0xA5) between neighbours, rounded up to whole elements (2, 2, 4
bytes for the 2-byte types, 4 for f32: an element-aligned neighbour cannot stand nearer); every guard byte is checked after every call.
The items make the filter tiles use 1, 2, 4, 8 and 16 lanes per pixel under both filters."""
import ctypes

import numpy as np
import pytest

from qoi_amd import bilinear, resize, tensors, warp
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_AREA, FILTER_BILINEAR, HWC, U8
from qoi_amd.warp import ALPHA_WEIGHTED, PLAIN, REPLICATE
from gpu_calls import WARP, WILD, run_tensors as run, tensor_layout as layout_of
from gpu_pack import E_ARG, GUARD, IMAGENET, Batch, Pack, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FILL = 0x40C08020
KIND_NAMES = {FILTER_AREA: "area", FILTER_BILINEAR: "bilinear", WARP: "warp"}
BIG, PHOTO, NOISE, TINY = 0, 1, 2, 3
SHAPES = [(200, 140, 4), (130, 70, 3), (64, 48, 4), (7, 5, 4)]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, Batch(api, oracle, SHAPES, ["sprite_alpha", "photo", "noise", "noise"]))


# enlarging 7 x 5 to 37 x 29 (five tiles of 256 work items), 1 : 1, reductions of about 3, 7, 12, 20 and 64 (32 under the tents) per axis
# down to 3 x 2 and 1 x 1; the flips take turns
AREA_ITEMS = [(TINY, 0, 0, 7, 5, 37, 29, 1), (NOISE, 3, 2, 40, 30, 40, 30, 2), (PHOTO, 0, 0, 130, 70, 43, 23, 3), (BIG, 0, 0, 200, 140, 28, 20, 0),
              (BIG, 5, 3, 36, 24, 3, 2, 1), (BIG, 100, 70, 60, 40, 3, 2, 2), (BIG, 4, 6, 192, 128, 3, 2, 3), (NOISE, 0, 0, 64, 48, 1, 1, 0), (PHOTO, 9, 3, 64, 64, 1, 1, 1)]
TENT_ITEMS = AREA_ITEMS[:6] + [(BIG, 4, 6, 96, 64, 3, 2, 3), (NOISE, 0, 0, 32, 32, 1, 1, 0), (PHOTO, 9, 3, 32, 32, 1, 1, 1)]
# 30 degrees to 17 x 16 and to 33 x 18 (three of the 16 x 16 tiles across, two down), a border of each kind; 1 x 1
WARP_ITEMS = [warp.item(BIG, (20, 10, 150, 100), (17, 16), warp.rotation((150, 100), (17, 16), 30.0, 0.15), 0, FILL),
              warp.item(PHOTO, (3, 5, 55, 35), (33, 18), warp.rotation((55, 35), (33, 18), 30.0, 0.9), REPLICATE, 0),
              warp.item(NOISE, (0, 0, 64, 48), (1, 1), warp.rotation((64, 48), (1, 1), 45.0), 0, 0x00FFFFFF)]
ITEMS = {FILTER_AREA: AREA_ITEMS, FILTER_BILINEAR: TENT_ITEMS, WARP: WARP_ITEMS}


def test_the_items_use_every_lane_count():
    assert {resize.split(it[3], it[5])[0] for it in AREA_ITEMS} == {0, 1, 2, 3, 4}
    assert {bilinear.split(it[3], it[5])[0] for it in TENT_ITEMS} == {0, 1, 2, 3, 4}
    assert resize.tiles(7, 37, 29) > 4 and bilinear.tiles(7, 37, 29) > 4 and warp.tiles(33, 18) == 6


_MODELS = {}


def model(p, kind, it, och, mode):
    """the u8 result P of the underlying call for one item: computed once, never changed"""
    key = (kind, tuple(it), och, mode)
    if key not in _MODELS:
        if kind == WARP:
            i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
            P = warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode)
        else:
            i, x, y, cw, rh, ow, oh, flags = it
            P = (resize.resize if kind == FILTER_AREA else bilinear.bilinear)(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, mode)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_items(p, got, kind, items, och, mode, f, what):
    for j, it in enumerate(items):
        w = tensors.convert(model(p, kind, it, och, mode), f).view(np.uint8).reshape(-1)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, KIND_NAMES[kind], j, it, int(np.argmax(got[j] != w)) // tensors.ELEM[f[0]])


# ------------------------------------------------------------------ 1: U8 + HWC is the u8 call
@pytest.mark.parametrize("kind", [FILTER_AREA, FILTER_BILINEAR, WARP])
def test_u8_hwc_is_the_u8_call(ctx, pack, kind):
    p, items = pack, ITEMS[kind]
    u8_call = {FILTER_AREA: ctx.decode_resized, FILTER_BILINEAR: ctx.decode_bilinear, WARP: ctx.decode_warped}[kind]
    for channels, mode in ((4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN), (3, ALPHA_WEIGHTED)):
        offsets, nbytes, total = layout_of(items, channels, 1)
        buf = filled(total, GUARD)
        u8_call(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, buf.data_ptr(), offsets)
        ref = buf.cpu().numpy()
        got = run(ctx, p, kind, channels, items, mode, tensors.fmt(U8, HWC))
        for j, (o, n) in enumerate(zip(offsets, nbytes)):
            assert np.array_equal(got[j], ref[o:o + n]), (KIND_NAMES[kind], channels, mode, j)
        assert_items(p, got, kind, items, channels, mode, tensors.fmt(U8, HWC), (channels, mode))
    assert ctx.tensor_stats()[:2] == (1, 1) and ctx.tensor_stats()[3] == len({it[0] for it in items})


# ------------------------------------------------------------------ 2: every dtype x layout x och x kind against the model
@pytest.mark.parametrize("layout", [HWC, CHW])
@pytest.mark.parametrize("dtype", [U8, F16, BF16, F32])
def test_formats_against_the_model(ctx, pack, dtype, layout):
    p = pack
    formats = [tensors.fmt(U8, layout)] if dtype == U8 else [(dtype, layout, *IMAGENET), (dtype, layout, *WILD)]
    for kind in (FILTER_AREA, FILTER_BILINEAR, WARP):
        for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
            for f in formats:
                got = run(ctx, p, kind, channels, ITEMS[kind], mode, f)
                assert_items(p, got, kind, ITEMS[kind], channels, mode, f, (dtype, layout, channels, f[2][0]))
    if dtype == F16:                                             # what WILD is there for really happens
        flat = tensors.convert(model(p, FILTER_AREA, AREA_ITEMS[1], 4, ALPHA_WEIGHTED), (F16, HWC, *WILD)).view(np.uint16).reshape(-1, 4)
        assert np.any(flat[:, 0] == 0x7C00) and np.any((flat[:, 2] > 0) & (flat[:, 2] < 0x0400)) and np.all(flat[:, 1] >= 0x8000)


def test_descriptor_channels(ctx, pack):
    """channels = 0: the output channel count is the images'"""
    p = pack
    f = (F16, CHW, *IMAGENET)
    for kind, items in ((FILTER_BILINEAR, [(PHOTO, 0, 0, 130, 70, 43, 23, 3)]), (FILTER_AREA, [AREA_ITEMS[3], AREA_ITEMS[7]]), (WARP, [WARP_ITEMS[1]])):
        och = p.shapes[items[0][0]][2]
        assert_items(p, run(ctx, p, kind, 0, items, PLAIN, f), kind, items, och, PLAIN, f, "channels 0")


# ------------------------------------------------------------------ 3: the tile walk and the sub-batches
def test_tile_walk_regimes(api, ctx, oracle):
    """(qoi_dev.h: walk_tiles) more tiles than the grid's clamp of 8 workgroups per compute unit - 37 more items of one tile each - so that a
    workgroup takes two tiles and steps from item to item (an item over several workgroups: the 37 x 29 and 33 x 18 outputs of the tests
    above, five and six tiles)."""
    import torch
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    p = Pack(ctx, oracle, Batch(api, oracle, [(8, 8, 4)], ["noise"]))
    f = (F16, CHW, *IMAGENET)
    rs = [(0, j % 7, (j // 7) % 7, 2, 2, 1, 1, j & 3) for j in range(n)]
    ws = [warp.item(0, (j % 7, (j // 7) % 7, 2, 2), (1, 1), (65536, 0, (j % 5) * 9000, 0, 65536, (j % 3) * 20000), j & 1, FILL) for j in range(n)]
    for kind, items in ((FILTER_AREA, rs), (FILTER_BILINEAR, rs), (WARP, ws)):
        for channels, mode in ((3, PLAIN), (4, ALPHA_WEIGHTED)):
            assert_items(p, run(ctx, p, kind, channels, items, mode, f), kind, items, channels, mode, f, ("many", channels))
            assert ctx.tensor_stats()[:2] == (1, 1)


def test_sub_batches(api, pack):
    c = api.Context(0)
    try:
        p = pack
        for kind, f in ((FILTER_AREA, (BF16, CHW, *IMAGENET)), (FILTER_BILINEAR, (F16, HWC, *IMAGENET)), (WARP, (F32, CHW, *WILD))):
            items = ITEMS[kind]
            images = len({it[0] for it in items})
            single = run(c, p, kind, 4, items, ALPHA_WEIGHTED, f)
            assert c.tensor_stats()[:2] == (1, 1) and c.tensor_stats()[3] == images
            _, _, the_plan, largest = tensors.plan(p.descs, [it[:5] + (0,) for it in items], 1)
            assert len(the_plan) == images > 1
            forced = run(c, p, kind, 4, items, ALPHA_WEIGHTED, f, staging=1)      # one image per sub-batch
            assert c.tensor_stats() == (images, images, largest, images), c.tensor_stats()
            assert all(np.array_equal(x, y) for x, y in zip(forced, single)), KIND_NAMES[kind]
    finally:
        c.close()


# ------------------------------------------------------------------ 4: rejections on a live context, and the context afterwards
def test_rejections_on_a_live_context(api, ctx, pack):
    p = pack
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    two = [(BIG, 0, 0, 100, 60, 10, 10, 0), (NOISE, 0, 0, 8, 8, 8, 8, 1)]
    two_w = [warp.item(BIG, (0, 0, 100, 60), (10, 10)), warp.item(NOISE, (0, 0, 8, 8), (8, 8))]
    ok = (F16, CHW, *IMAGENET)

    def fm(f, reserved=(0, 0)):
        t = api.tensor_format(f)
        return api.QoimiTensorFormat(t.dtype, t.layout, t.scale, t.bias, (ctypes.c_uint * 2)(*reserved))

    def call(items=two, offsets=(128, 128 + 800), channels=4, filter=FILTER_BILINEAR, mode=0, f=fm(ok), null_format=False, out=None):
        arr = (api.QoimiResize * len(items))(*[api.QoimiResize(*it) for it in items])
        return lib.qoimi_decode_tensors(ctx._h, *args, channels, arr, len(items), filter, mode, None if null_format else ctypes.byref(f),
                                        buf.data_ptr() if out is None else out, (ctypes.c_size_t * len(items))(*offsets), 0, None)

    def call_w(items=two_w, offsets=(128, 128 + 800), channels=4, mode=0, f=fm(ok), null_format=False):
        arr = (api.QoimiWarp * len(items))(*[api.QoimiWarp(*it) for it in items])
        return lib.qoimi_decode_warped_tensors(ctx._h, *args, channels, arr, len(items), mode, None if null_format else ctypes.byref(f), buf.data_ptr(),
                                               (ctypes.c_size_t * len(items))(*offsets), 0, None)

    assert call() == 0, api.last_error()                                              # side by side: accepted
    got = buf.cpu().numpy()
    for it, o, nb in ((two[0], 128, 800), (two[1], 928, 512)):
        assert np.array_equal(got[o:o + nb], tensors.convert(model(p, FILTER_BILINEAR, it, 4, PLAIN), ok).view(np.uint8).reshape(-1))
    assert np.all(got[:128] == GUARD) and np.all(got[928 + 512:] == GUARD)
    stats = ctx.tensor_stats()
    assert stats[:2] == (1, 1) and stats[3] == 2
    buf.fill_(GUARD)
    inf, nan = float("inf"), float("nan")
    one = (1.0,) * 4
    zero = (0.0,) * 4
    rejected = [
        (lambda: call(filter=2), "filter"), (lambda: call(filter=-1), "filter"),
        (lambda: call(null_format=True), "format"), (lambda: call_w(null_format=True), "format"),
        (lambda: call(f=fm((4, HWC, one, zero))), "dtype"), (lambda: call_w(f=fm((0xFFFFFFFF, HWC, one, zero))), "dtype"),
        (lambda: call(f=fm((F16, 2, one, zero))), "layout"), (lambda: call_w(f=fm((F32, 7, one, zero))), "layout"),
        (lambda: call(f=fm(ok, (1, 0))), "reserved"), (lambda: call_w(f=fm(ok, (0, 9))), "reserved"),
        (lambda: call(f=fm((F32, HWC, (1.0, inf, 1.0, 1.0), zero))), "finite"), (lambda: call(f=fm((F16, HWC, one, (0.0, 0.0, 0.0, nan)))), "finite"),
        (lambda: call_w(f=fm((BF16, CHW, (-inf, 1.0, 1.0, 1.0), zero))), "finite"),
        (lambda: call(f=fm((U8, HWC, (1.0, 1.0, 2.0, 1.0), zero))), "QOIMI_TENSOR_U8"), (lambda: call(f=fm((U8, CHW, one, (0.0, -0.0, 0.0, 0.0)))), "QOIMI_TENSOR_U8"),
        (lambda: call_w(f=fm((U8, HWC, one, (0.0, 0.0, 0.0, 1.0)))), "QOIMI_TENSOR_U8"),
        (lambda: call(offsets=(129, 1024)), "multiple of the element size"), (lambda: call(offsets=(128, 1025)), "multiple of the element size"),
        (lambda: call(offsets=(128, 2050), f=fm((F32, HWC, one, zero))), "multiple of the element size"), (lambda: call_w(offsets=(127, 1024)), "multiple of the element size"),
        (lambda: call(offsets=(128, 128 + 798)), "overlap"), (lambda: call_w(offsets=(128, 128 + 798)), "overlap"),      # f16: 800 bytes, not the 400 of u8
        (lambda: call(offsets=(128, 128 + 1596), f=fm((F32, CHW, one, zero))), "overlap"), (lambda: call(offsets=(500, 128)), "overlap"),
        (lambda: call(items=[(BIG, 0, 0, 1, 1, 32767, 32767, 0)], offsets=(0,), filter=FILTER_AREA, out=2 ** 64 - 2 ** 32), "address space"),   # fits as u8
        (lambda: call(items=[(BIG, 0, 0, 130, 1, 4, 1, 0)], offsets=(64,)), "32"), (lambda: call(items=[(BIG, 0, 0, 130, 1, 2, 1, 0)], offsets=(64,), filter=FILTER_AREA), "64"),
        (lambda: call(items=[(BIG, 191, 0, 10, 10, 10, 10, 0)], offsets=(64,)), "leaves"), (lambda: call(items=[(BIG, 0, 0, 10, 10, 10, 10, 4)], offsets=(64,)), "flag"),
        (lambda: call_w(items=[warp.item(BIG, (0, 0, 10, 10), (1 << 20, 1))], offsets=(64,)), "2^20"),
        (lambda: call(mode=2), "mode"), (lambda: call_w(mode=-1), "mode"), (lambda: call(channels=5), "channels"),
        (lambda: call(items=[(PHOTO, 0, 0, 1, 1, 1, 1, 0), (BIG, 0, 0, 1, 1, 1, 1, 0)], offsets=(64, 128), channels=0), "channel"),
        # the order: the filter in front of the format, the format in front of the items, the items in front of the alignment
        (lambda: call(filter=5, null_format=True), "filter"), (lambda: call(items=[(BIG, 191, 0, 10, 10, 10, 10, 0)], offsets=(63,), f=fm((4, HWC, one, zero))), "dtype"),
        (lambda: call(items=[(BIG, 191, 0, 10, 10, 10, 10, 0)], offsets=(63,)), "leaves"), (lambda: call(offsets=(129, 130)), "overlap"),
    ]
    for f, word in rejected:
        assert f() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.tensor_stats() == stats, word
    with pytest.raises(api.QoiError):
        ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, two, FILTER_AREA, PLAIN, ok, buf.data_ptr(), [129, 1024])
    assert bool((buf == GUARD).all()) and ctx.tensor_stats() == stats
    # the context works afterwards
    assert call_w() == 0, api.last_error()
    got = buf.cpu().numpy()
    for it, o, nb in ((two_w[0], 128, 800), (two_w[1], 928, 512)):
        assert np.array_equal(got[o:o + nb], tensors.convert(model(p, WARP, it, 4, PLAIN), ok).view(np.uint8).reshape(-1))
    assert_items(p, run(ctx, p, FILTER_AREA, 3, AREA_ITEMS[:3], PLAIN, ok), FILTER_AREA, AREA_ITEMS[:3], 3, PLAIN, ok, "afterwards")
