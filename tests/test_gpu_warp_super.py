"""QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 on the GPU (-m gpu), through qoimi_decode_warped, qoimi_decode_warped_tensors and
qoimi_decode_warped_indexed: every output is compared bit for bit, over its whole length, with the definition - the oracle decodes the stream
at the call's output channel count, qoi_amd/warp.py samples that, qoi_amd/tensors.py: convert makes the tensor (each u8 model is computed
once and shared).  The pack is small: 33 x 21 x 4, 64 x 48 x 3 and 5 x 1 x 4; the outputs run from 1 x 1 to 17 x 9 (edge tiles) and one of
40 x 24 (six tiles).  Outputs stand behind, between and in front of guard bytes (gpu_calls.py: run_warp, run_label_tensors); every guard
byte is checked after every call.  The box identity is also compared with qoimi_decode_thumbnails and qoimi_decode_resized on the device.  The
last test takes the pack of tests/wide_cases.py: huge_with_plantings - a 17.7 Mpx image between small ones - for a call with more tiles than the launch
has workgroups over staged pixel indices from 2**24 on.  Before the two flags existed every call here with one of them was rejected with
"unknown flag bit"."""
import ctypes

import numpy as np
import pytest

import resize_window as rw
from qoi_amd import tensors, thumbs, warp
from qoi_amd.tensors import CHW, F16, F32, HWC
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, WRAP
from gpu_calls import assert_outputs, run_label_tensors as run_tensors, run_warp
from gpu_pack import E_ARG, GUARD, IMAGENET, KINDS, OraclePack, Pack, batch_of, filled, image
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from wide_cases import huge_with_plantings, past_2_24, super_walk_table, super_windows, walk_shape, window_of

pytestmark = pytest.mark.gpu
FILL = 0x40C08020
RGBA, RGB, STRIP = 0, 1, 2
SHAPES = [(33, 21, 4), (64, 48, 3), (5, 1, 4)]
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
SUPERS = (SUPER2, SUPER4)


def pixels():
    rng = np.random.default_rng(20261)
    out = []
    for w, h, ch in SHAPES:
        D = rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8)
        if ch == 4:
            D[:, :, 3][rng.integers(0, 3, size=(h, w)) == 0] = 0                # a third of the pixels transparent: the modes differ
        out.append(D)
    return out


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, SHAPES, pixels()))


_MODELS = {}


def model(p, it, och, mode=PLAIN):
    """the u8 result P of one item: computed once, never changed"""
    key = (id(p), tuple(it), och, mode)
    if key not in _MODELS:
        i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
        P = warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_bytes(p, got, items, och, mode, what):
    assert_outputs(got, [model(p, it, och, mode) for it in items], (what, och, mode))


def super_items(flag, borders=BORDERS):
    """per border: the 33 x 21 image turned by 30 degrees and reduced by 2.5 into 17 x 9; the strip reduced by 4 into 1 x 1 and turned into
    3 x 7; a rectangle of the 64 x 48 image turned by 17 degrees and reduced by 1.7 into 40 x 24 (six tiles); a 2 x 2 rectangle sheared into
    3 x 2; a 1 x 7 rectangle reduced by 3 into 16 x 16 (one whole tile); a reducing map hundreds of periods away; a sheared map at offsets
    next to -2**56 and +2**56"""
    items = []
    for border in borders:
        flags = border | flag
        items.append(warp.item(RGBA, (0, 0, 33, 21), (17, 9), warp.rotation((33, 21), (17, 9), 30.0, 1 / 2.5), flags, FILL))
        items.append(warp.item(STRIP, (0, 0, 5, 1), (1, 1), warp.rotation((5, 1), (1, 1), 0.0, 1 / 4), flags, FILL))
        items.append(warp.item(STRIP, (0, 0, 5, 1), (3, 7), warp.rotation((5, 1), (3, 7), 60.0, 1 / 1.5), flags, FILL))
        items.append(warp.item(RGB, (3, 5, 40, 30), (40, 24), warp.rotation((40, 30), (40, 24), 17.0, 1 / 1.7), flags, FILL))
        items.append(warp.item(RGBA, (10, 7, 2, 2), (3, 2), (ONE, 23000, -40000, -9000, ONE + 700, 12345), flags, FILL))
        items.append(warp.item(RGB, (11, 5, 1, 7), (16, 16), warp.rotation((1, 7), (16, 16), 0.0, 1 / 3), flags, FILL))
        items.append(warp.item(RGB, (30, 1, 5, 3), (7, 5), (3 * ONE, 0, 2 * ONE * 5 * 300 + 777, 0, 3 * ONE, -2 * ONE * 3 * 500 - 999), flags, FILL))
        items.append(warp.item(RGBA, (8, 6, 17, 9), (17, 5), (ONE, 31, 1 - 2 ** 56, -17, ONE, 2 ** 56 - 1), flags, FILL))
    return items


@pytest.mark.parametrize("channels,mode", [(4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN), (3, ALPHA_WEIGHTED)])
@pytest.mark.parametrize("flag", SUPERS)
def test_items_against_the_model(ctx, pack, flag, channels, mode):
    p = pack
    items = super_items(flag)
    got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
    assert_bytes(p, got, items, channels, mode, "warped")
    assert ctx.warp_stats()[:2] == (1, 1)
    if channels == 4 and mode == ALPHA_WEIGHTED:
        assert not np.array_equal(model(p, items[0], 4, PLAIN), model(p, items[0], 4, ALPHA_WEIGHTED))      # the modes differ
        # ... and so do the flag and its absence, and the two flags
        plain = items[0][:7] + (items[0][7] & ~flag,) + items[0][8:]
        other = items[0][:7] + (items[0][7] ^ (SUPER2 | SUPER4),) + items[0][8:]
        assert len({model(p, it, 4, mode).tobytes() for it in (items[0], plain, other)}) == 3


@pytest.mark.parametrize("flag", SUPERS)
def test_tensors(ctx, pack, flag):
    """f16 CHW and f32 HWC, guard bytes between the outputs"""
    p = pack
    items = super_items(flag)
    for f in ((F16, CHW, *IMAGENET), (F32, HWC, *IMAGENET)):
        for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
            got = run_tensors(ctx, p, "warp", channels, items, mode, f)
            for j, it in enumerate(items):
                w = tensors.convert(model(p, it, channels, mode), f).view(np.uint8).reshape(-1)
                assert got[j].size == w.size and np.array_equal(got[j], w), (f[:2], channels, j, it, int(np.argmax(got[j] != w)))
            assert ctx.tensor_stats()[:2] == (1, 1)


def test_indexed(ctx, pack):
    """through a seek index: the band is what is staged, the border is the rectangle's"""
    p = pack
    items = super_items(SUPER2)[::3] + super_items(SUPER4)[1::3]
    intervals = [4, 2, 26]                                         # (interval_rows * width is at least 128)
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, intervals)
    plain = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED)
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 1, call=lambda out, offsets: ctx.decode_warped_indexed(
        p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, items, ALPHA_WEIGHTED, out, offsets, intervals, points, firsts))
    assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "indexed")
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("flag,s", [(SUPER2, 2), (SUPER4, 4)])
def test_the_box_identity_on_the_device(ctx, pack, flag, s):
    """a = e = s * ONE into 1 / s of the rectangle: qoimi_decode_thumbnails at factor s and qoimi_decode_resized of the same rectangle, byte
    for byte, in both modes"""
    p = pack
    box = (s * ONE, 0, 0, 0, s * ONE, 0)
    rect = (1, 1, 32, 20)
    for channels, mode in ((4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN)):
        items = [warp.item(RGB, (0, 0, 64, 48), (64 // s, 48 // s), box, flag | border, FILL) for border in (0, WRAP)]
        items.append(warp.item(RGBA, rect, (32 // s, 20 // s), box, flag | REFLECT, FILL))
        got = run_warp(ctx, p, channels, items, mode, front=64 + 3)
        assert_bytes(p, got, items, channels, mode, "box")
        # the whole 64 x 48 image as a thumbnail (the other images at factor 1)
        factors = [1, s, 1]
        tw = [thumbs.size(w, h, f) for (w, h, _), f in zip(SHAPES, factors)]
        nbytes = [a * b * channels for a, b in tw]
        offsets = [64 + int(v) for v in np.cumsum([0] + nbytes[:-1])]
        buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
        ctx.decode_thumbnails(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, factors, mode, buf.data_ptr(), offsets)
        thumb = buf.cpu().numpy()[offsets[1]:offsets[1] + nbytes[1]]
        assert thumb.size == got[0].size and np.array_equal(thumb, got[0]) and np.array_equal(thumb, got[1]), (channels, mode)
        # the rectangle through qoimi_decode_resized
        n = (32 // s) * (20 // s) * channels
        buf = filled(64 + n + 64, GUARD)
        ctx.decode_resized(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, [(RGBA,) + rect + (32 // s, 20 // s, 0)], mode, buf.data_ptr(), [64])
        back = buf.cpu().numpy()
        assert np.array_equal(back[64:64 + n], got[2]) and np.all(back[:64] == GUARD) and np.all(back[64 + n:] == GUARD), (channels, mode)


def test_mixed_items_keep_the_bytes_of_a_call_without_a_super_item(ctx, pack):
    """items of both flags and every border with nearest, bilinear and bicubic items of every border in one call, one launch, at odd
    offsets with guard bytes in front and between: every item has its model's bytes, and the items without a SUPER flag have, byte for byte,
    what a call made of them alone - the kernels of before - writes"""
    p = pack
    rect = (8, 6, 17, 9)
    turn = warp.rotation((17, 9), (41, 29), 30.0, 0.6)
    older = [(s, b) for s in (0, NEAREST, BICUBIC) for b in BORDERS]
    others = [warp.item(RGBA if j & 1 else RGB, rect, (41, 29), turn, s | b, FILL) for j, (s, b) in enumerate(older)]
    supers = [warp.item(RGB if j & 1 else RGBA, rect, (19, 13), warp.rotation((17, 9), (19, 13), 30.0, 0.5), flag | b, FILL)
              for j, (flag, b) in enumerate((f, b) for f in SUPERS for b in BORDERS)]
    items = [it for pair in zip(supers + supers[:5], others) for it in pair]                # in turn with and without a SUPER flag
    assert len(others) == 15 and len(items) == 30
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        nbytes = [it[5] * it[6] * channels for it in items]
        offsets = [65 + int(v) + 2 * j - (j & 1) for j, v in enumerate(np.cumsum([0] + nbytes[:-1]))]     # 65, then gaps of 1 and 3 bytes in turn
        got = run_warp(ctx, p, channels, items, mode, offsets=offsets)
        assert_bytes(p, got, items, channels, mode, "mixed")
        assert ctx.warp_stats()[:2] == (1, 1)
        alone = run_warp(ctx, p, channels, others, mode, front=64 + 1)
        assert_bytes(p, alone, others, channels, mode, "without a SUPER item")
        assert all(np.array_equal(a, b) for a, b in zip(alone, got[1::2]))
    f = (F16, CHW, *IMAGENET)
    got = run_tensors(ctx, p, "warp", 4, items, PLAIN, f)
    alone = run_tensors(ctx, p, "warp", 4, others, PLAIN, f)
    for j, it in enumerate(items):
        assert np.array_equal(got[j], tensors.convert(model(p, it, 4), f).view(np.uint8).reshape(-1)), j
    assert all(np.array_equal(a, b) for a, b in zip(alone, got[1::2]))


def test_sub_batches(api, pack):
    """a small staging_bytes forces one sub-batch per image: the same bytes, one launch of the kernel per sub-batch"""
    p = pack
    c = api.Context(0)
    try:
        items = super_items(SUPER2, (REFLECT_101, 0)) + super_items(SUPER4, (WRAP, REPLICATE))
        single = run_warp(c, p, 4, items, ALPHA_WEIGHTED)
        images, slots, subs, largest = warp.plan(p.descs, items, 0)
        assert len(subs) == 1 and c.warp_stats() == (1, 1, largest, len(images))
        images, slots, subs, largest = warp.plan(p.descs, items, 1)
        assert len(subs) == len(images) == 3
        got = run_warp(c, p, 4, items, ALPHA_WEIGHTED, staging=1, front=64 + 1)
        assert c.warp_stats() == (3, 3, largest, 3)
        assert all(np.array_equal(x, y) for x, y in zip(got, single))
        assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "sub-batches")
    finally:
        c.close()


def test_the_new_rejections_leave_the_output_untouched(api, ctx, pack):
    p = pack
    lib = api.load_library()
    n = p.n
    buf = filled(8192, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    fmt = api.tensor_format((F16, CHW, *IMAGENET))
    good = warp.item(RGBA, (0, 0, 33, 21), (8, 5), warp.rotation((33, 21), (8, 5), 30.0, 0.25), SUPER4 | REPLICATE, FILL)

    def call(items, tensor):
        arr = (api.QoimiWarp * len(items))(*[api.QoimiWarp(*it) for it in items])
        offsets = (ctypes.c_size_t * len(items))(*[64 + 1024 * j for j in range(len(items))])
        if tensor:
            return lib.qoimi_decode_warped_tensors(ctx._h, *args, 4, arr, len(items), 0, ctypes.byref(fmt), buf.data_ptr(), offsets, 0, None)
        return lib.qoimi_decode_warped(ctx._h, *args, 4, arr, len(items), 0, buf.data_ptr(), offsets, 0, None)

    for tensor in (False, True):
        stats = ctx.tensor_stats() if tensor else ctx.warp_stats()
        for flags, word in ((SUPER2 | SUPER4, "item 1: QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 together"), (SUPER2 | SUPER4 | WRAP, "item 1: QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 together"),
                            (SUPER2 | NEAREST, "item 1: supersampling is defined for the bilinear sampling only"),
                            (SUPER4 | BICUBIC | REFLECT, "item 1: supersampling is defined for the bilinear sampling only"), (512 | SUPER2, "item 1: unknown flag bit")):
            bad = good[:7] + (flags,) + good[8:]
            assert call([good, bad], tensor) == E_ARG and word in api.last_error(), (flags, api.last_error())
            assert bool((buf == GUARD).all()) and (ctx.tensor_stats() if tensor else ctx.warp_stats()) == stats, flags
    assert call([good], False) == 0, api.last_error()                                       # the context serves the next call
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:64 + 160], model(p, good, 4).reshape(-1)) and np.all(got[:64] == GUARD) and np.all(got[64 + 160:] == GUARD)


# ------------------------------------------------------------------ the tile walk with many tiles per workgroup, staged pixel indices from 2**24 on
WIDE_SHAPES = [(1, 1, 4), (37, 23, 3), rw.HUGE + (4,), (130, 70, 4)]
DOT, ODD, HUGE, SPRITE = range(4)
HW_, HH = rw.HUGE


@pytest.fixture(scope="module")
def wide(api, oracle):
    px = [huge_with_plantings() if i == HUGE else image(KINDS[(i + 2) % 5], w, h, ch, frame=i) for i, (w, h, ch) in enumerate(WIDE_SHAPES)]
    return OraclePack(api, oracle, WIDE_SHAPES, px)


def test_many_tiles_per_workgroup_beyond_2_24(ctx, wide):
    """[small, big, small x 5, small] in one launch of warp_super_bytes: big shears a rectangle of the last rows of the 17.7 Mpx image - every
    staged pixel index at least 2**24 - under SUPER2 into more than 3 * 8 * cu tiles of 16 x 16 (the last column and row of tiles partial),
    the five behind it are one-tile items of that image of both flags and the older samplings.  The model would take long over 1.5 Mpx of
    sixteen taps: the big output is compared WHOLE with the same item alone in its own call, and four windows of it - the corners of the
    walk, partial tiles among them - with the model (window_of; that it is that window is asserted on a small output)."""
    import torch
    p = wide
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ow, oh, across, down = walk_shape(cus)
    rect = (100, 3652, 400, 180)
    items = super_walk_table(cus)                                  # (tests/test_gpu_newer_wide.py runs the same table through warp_super_tensor)
    big = items[1]
    assert big[:8] == (HUGE,) + rect + (ow, oh, SUPER2 | REFLECT)
    tiles = [warp.tiles(it[5], it[6]) for it in items]
    assert tiles[1] == across * down > 3 * 8 * cus and tiles[:1] + tiles[2:] == [1] * 7 and past_2_24(items) and ow * oh < warp.MAX_AREA
    small = warp.item(HUGE, rect, (40, 60), warp.rotation(rect[2:], (40, 60), 30.0, 0.1), SUPER4 | REFLECT, FILL)
    assert np.array_equal(model(p, window_of(small, 7, 22, 30, 17), 4, ALPHA_WEIGHTED), model(p, small, 4, ALPHA_WEIGHTED)[22:39, 7:37])
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 3)
    assert ctx.warp_stats()[:2] == (1, 1)
    alone = run_warp(ctx, p, 4, [big], ALPHA_WEIGHTED)
    assert np.array_equal(got[1], alone[0]), ("the big entry differs from its own call", int(np.argmax(got[1] != alone[0])))
    whole = got[1].reshape(oh, ow, 4)
    for X0, Y0 in super_windows(ow, oh):
        want = model(p, window_of(big, X0, Y0, 45, 27), 4, ALPHA_WEIGHTED)
        assert np.array_equal(whole[Y0:Y0 + 27, X0:X0 + 45], want), ("a window of the big entry", X0, Y0)
    for j in (0, 2, 3, 4, 5, 6, 7):
        assert np.array_equal(got[j], model(p, items[j], 4, ALPHA_WEIGHTED).reshape(-1)), ("a one-tile entry", j)
