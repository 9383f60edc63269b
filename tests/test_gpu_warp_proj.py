"""QOIMI_WARP_PROJECTIVE on the GPU (-m gpu), through qoimi_decode_warped, qoimi_decode_warped_tensors and qoimi_decode_warped_indexed: every
output is compared bit for bit, over its whole length, with the definition - the oracle decodes the stream, qoi_amd/warp.py divides the
positions and samples, qoi_amd/tensors.py: convert makes the tensor (each u8 model is computed once and shared).  The pack is small: noise
with alpha of 33 x 21 x 4, 64 x 48 x 3 and 5 x 1 x 4 and a strip of 33000 x 3 x 3, on which a position passes 2**32; the outputs run from
1 x 1 over 17 x 9 to 33 x 40 (nine tiles, ragged edges) and 70000 x 3 (F = 31).  Outputs stand behind, between and in front of guard bytes
(gpu_calls.py: run_warp, run_label_tensors); every guard byte is checked after every call.  With g = h = 0 the flagged call is compared
with the unflagged call on the device; in a mixed call the older items keep the bytes of a call without a projective item.  Before the
flag existed every call here with it was rejected with "unknown flag bit"."""
import ctypes

import numpy as np
import pytest

from qoi_amd import tensors, warp
from qoi_amd.tensors import CHW, F16, HW, I64
from qoi_amd.warp import (ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, PROJECTIVE, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4,
                          WRAP)
from gpu_calls import assert_outputs, run_label_tensors as run_tensors, run_warp
from gpu_pack import E_ARG, GUARD, IMAGENET, Pack, batch_of, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FILL = 0x80FF4007
RGBA, RGB, STRIP, LONG = 0, 1, 2, 3
SHAPES = [(33, 21, 4), (64, 48, 3), (5, 1, 4), (33000, 3, 3)]
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
SAMPLINGS = (0, NEAREST, BICUBIC)


def pixels():
    out = []
    for j, (w, h, ch) in enumerate(SHAPES):
        D = np.random.default_rng(20280 + j).integers(0, 256, (h, w, ch), dtype=np.uint8)
        if ch == 4:
            D[::2, ::3, 3] = 0
            D[::2, 1::3, 3] = 255
        if w > 1000:                                                   # compressible, so that the stream stays small: runs of a few pixels
            D = np.repeat(D[:, ::8], 8, axis=1)[:, :w]
        out.append(np.ascontiguousarray(D))
    return out


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, SHAPES, pixels()))


_MODELS = {}


def model(p, it, och, mode=PLAIN):
    """the u8 result of one item: computed once, never changed.  An item with a VOTE flag votes over the 4-channel decode whatever och is"""
    key = (id(p), tuple(it), och, mode)
    if key not in _MODELS:
        i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, reserved, c, f = it
        voted = flags & warp.VOTES
        P = warp.warp(p.decoded(i, 4 if voted else och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode, och=och if voted else 0, reserved=reserved)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_bytes(p, got, items, och, mode, what):
    assert_outputs(got, [model(p, it, och, mode) for it in items], (what, och, mode))


def tilt(out_size, share_x, share_y):
    """(g, h) that use the given shares (-1 .. 1) of the room the limit 2**F - |g| (ow - 1) - |h| (oh - 1) >= 2**(F - 3) leaves"""
    ow, oh = out_size
    room = 7 * 2 ** (warp.proj_bits(ow, oh) - 3)
    g = int(share_x * room / max(ow - 1, 1))
    h = int(share_y * room / max(oh - 1, 1))
    return max(-32768, min(32767, g)), max(-32768, min(32767, h))


def proj_items(sampling, borders=BORDERS):
    """per border: the 33 x 21 image turned by 30 degrees into 17 x 9 with a moderate tilt; the strip into 1 x 1 (W = 2**14 whatever g and h
    are) and turned into 3 x 7; a rectangle of the 64 x 48 image through four corner points into 33 x 40 (nine tiles, ragged edges); a 2 x 2
    rectangle sheared into 3 x 2 with the denominator at its limit; a 1 x 7 rectangle into 16 x 16 (one whole tile); a map hundreds of
    periods away; a sheared map at offsets next to -2**53 and +2**53"""
    items = []
    for border in borders:
        flags = border | sampling
        items.append(warp.item(RGBA, (0, 0, 33, 21), (17, 9), warp.rotation((33, 21), (17, 9), 30.0, 0.6), flags, FILL, proj=tilt((17, 9), 0.4, -0.3)))
        items.append(warp.item(STRIP, (0, 0, 5, 1), (1, 1), warp.rotation((5, 1), (1, 1), 0.0, 1 / 4), flags, FILL, proj=(32767, -32768)))
        items.append(warp.item(STRIP, (0, 0, 5, 1), (3, 7), warp.rotation((5, 1), (3, 7), 60.0, 1 / 1.5), flags, FILL, proj=tilt((3, 7), -0.5, 0.5)))
        m, gh, _ = warp.perspective((40, 30), (33, 40), [(4.0, 2.0), (36.5, 6.0), (39.0, 28.0), (1.0, 24.5)])
        items.append(warp.item(RGB, (3, 5, 40, 30), (33, 40), m, flags, FILL, proj=gh))
        items.append(warp.item(RGBA, (10, 7, 2, 2), (3, 2), (ONE, 23000, -40000, -9000, ONE + 700, 12345), flags, FILL, proj=tilt((3, 2), -1.0, 0.0)))
        items.append(warp.item(RGB, (11, 5, 1, 7), (16, 16), warp.rotation((1, 7), (16, 16), 0.0, 1 / 3), flags, FILL, proj=tilt((16, 16), 0.5, 0.5)))
        items.append(warp.item(RGB, (30, 1, 5, 3), (7, 5), (3 * ONE, 0, 2 * ONE * 5 * 300 + 777, 0, 3 * ONE, -2 * ONE * 3 * 500 - 999), flags, FILL, proj=tilt((7, 5), 0.2, 0.7)))
        items.append(warp.item(RGBA, (8, 6, 17, 9), (17, 5), (ONE, 31, 1 - 2 ** 53, -17, ONE, 2 ** 53 - 1), flags, FILL, proj=tilt((17, 5), -0.6, -0.4)))
    for it in items:
        assert it[7] & PROJECTIVE and warp._wrong(10 ** 6, 10 ** 6, it[1:5], it[5:7], (it[8], it[9], it[14], it[10], it[11], it[15]), it[7], it[13]) == "", it
    return items


@pytest.mark.parametrize("channels,mode", [(4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN), (3, ALPHA_WEIGHTED)])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_items_against_the_model(ctx, pack, sampling, channels, mode):
    p = pack
    items = proj_items(sampling)
    assert warp.tiles(33, 40) == 9                                   # 3 x 3, the last column and row partial
    got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
    assert_bytes(p, got, items, channels, mode, "warped")
    assert ctx.warp_stats()[:2] == (1, 1)
    if channels == 4 and mode == PLAIN:
        # the tilt shows: the same item without it differs
        flat = items[0][:13] + (0,) + items[0][14:]
        assert not np.array_equal(model(p, items[0], 4), model(p, flat, 4))


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_tensors(ctx, pack, sampling):
    """f16 CHW - what a training loader takes - and I64 HW, guard bytes between the outputs"""
    p = pack
    items = proj_items(sampling)
    for f in ((F16, CHW, *IMAGENET), tensors.fmt(I64, HW)):
        for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
            got = run_tensors(ctx, p, "warp", channels, items, mode, f)
            for j, it in enumerate(items):
                w = tensors.convert(model(p, it, channels, mode), f).view(np.uint8).reshape(-1)
                assert got[j].size == w.size and np.array_equal(got[j], w), (f[:2], channels, j, it, int(np.argmax(got[j] != w)))
            assert ctx.tensor_stats()[:2] == (1, 1)


def test_indexed(ctx, pack):
    """through a seek index: the band is what is staged, the items pass through with their g and h"""
    p = pack
    items = proj_items(0)[::3] + proj_items(NEAREST)[1::3] + proj_items(BICUBIC)[2::3]
    intervals = [4, 2, 26, 1]                                        # (interval_rows * width is at least 128)
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, intervals)
    plain = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED)
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 1, call=lambda out, offsets: ctx.decode_warped_indexed(
        p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, items, ALPHA_WEIGHTED, out, offsets, intervals, points, firsts))
    assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "indexed")
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))


def test_zero_coefficients_are_the_unflagged_call_on_the_device(ctx, pack):
    """g = h = 0: W = 2**F and Px = Nx - the new kernel against the kernels of before, byte for byte, in every sampling, border, mode, channel
    count and as tensors"""
    p = pack
    older = [(s, b) for s in SAMPLINGS for b in BORDERS]
    turn = warp.rotation((17, 9), (41, 29), 30.0, 0.6)
    unflagged = [warp.item(RGBA if j & 1 else RGB, (8, 6, 17, 9), (41, 29), turn, s | b, FILL) for j, (s, b) in enumerate(older)]
    unflagged.append(warp.item(STRIP, (0, 0, 5, 1), (1, 1), warp.IDENTITY, 0, FILL))
    unflagged.append(warp.item(RGBA, (8, 6, 17, 9), (17, 5), (ONE, 31, 1 - 2 ** 53, -17, ONE, 2 ** 53 - 1), WRAP, FILL))
    flagged = [it[:7] + (it[7] | PROJECTIVE,) + it[8:] for it in unflagged]
    for channels, mode in ((4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN)):
        a = run_warp(ctx, p, channels, unflagged, mode, front=64 + 1)
        b = run_warp(ctx, p, channels, flagged, mode, front=64 + 3)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (channels, mode)
        assert_bytes(p, b, flagged, channels, mode, "g = h = 0")
    f = (F16, CHW, *IMAGENET)
    a = run_tensors(ctx, p, "warp", 3, unflagged, PLAIN, f)
    b = run_tensors(ctx, p, "warp", 3, flagged, PLAIN, f)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_mixed_items_keep_the_bytes_of_a_call_without_a_projective_item(ctx, pack):
    """projective items of every sampling and border with nearest, bilinear, bicubic, supersampled and voted items of every border in one
    call, one launch, at odd offsets with guard bytes in front and between: every item has its model's bytes, and the items without the
    flag have, byte for byte, what a call made of them alone - the kernels of before - writes"""
    p = pack
    rect = (8, 6, 17, 9)
    turn = warp.rotation((17, 9), (41, 29), 30.0, 0.6)
    older = [(s, b) for s in (0, NEAREST, BICUBIC, SUPER2, SUPER4, VOTE2, VOTE4) for b in BORDERS]
    others = [warp.item(RGBA if j & 1 else RGB, rect, (41, 29), turn, s | b, FILL) for j, (s, b) in enumerate(older)]
    projs = [warp.item(RGB if j & 1 else RGBA, rect, (19, 13), warp.rotation((17, 9), (19, 13), 30.0, 0.8), s | b, FILL, proj=tilt((19, 13), 0.3 + 0.02 * j, -0.4))
             for j, (s, b) in enumerate((s, b) for s in SAMPLINGS for b in BORDERS)]
    items = [it for pair in zip((projs * 3)[:35], others) for it in pair]                    # in turn with and without the flag
    assert len(others) == 35 and len(items) == 70
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        nbytes = [it[5] * it[6] * channels for it in items]
        offsets = [65 + int(v) + 2 * j - (j & 1) for j, v in enumerate(np.cumsum([0] + nbytes[:-1]))]     # 65, then gaps of 1 and 3 bytes in turn
        got = run_warp(ctx, p, channels, items, mode, offsets=offsets)
        assert_bytes(p, got, items, channels, mode, "mixed")
        assert ctx.warp_stats()[:2] == (1, 1)
        alone = run_warp(ctx, p, channels, others, mode, front=64 + 1)
        assert all(np.array_equal(a, b) for a, b in zip(alone, got[1::2]))
    f = (F16, CHW, *IMAGENET)
    got = run_tensors(ctx, p, "warp", 4, items, PLAIN, f)
    alone = run_tensors(ctx, p, "warp", 4, others, PLAIN, f)
    for j, it in enumerate(items):
        assert np.array_equal(got[j], tensors.convert(model(p, it, 4), f).view(np.uint8).reshape(-1)), j
    assert all(np.array_equal(a, b) for a, b in zip(alone, got[1::2]))


def test_a_wide_output_and_a_wide_source(ctx, pack):
    """an output of 70000 x 3 has F = 31: the quotient comes down in two chunks and W passes 2**31; on the 33000 x 3 strip the position of
    column 32768 and beyond is 2**32 or more"""
    p = pack
    assert warp.proj_bits(70000, 3) == 31
    wide = warp.item(RGBA, (0, 0, 33, 21), (70000, 3), (31, 0, 0, 0, 7 * ONE, 0), REFLECT, FILL, proj=(-26843, 9000))        # 33 columns over 70000, rows by 7
    wide_n = warp.item(RGB, (3, 5, 40, 30), (70000, 3), (75, 40000, 0, 9, 9 * ONE, 0), NEAREST, FILL, proj=(20000, -32768))
    src = (0, 0, 33000, 3)
    long_ = warp.item(LONG, src, (33, 40), (1000 * ONE, 3000, 0, 50, ONE // 16, 0), REPLICATE, FILL, proj=tilt((33, 40), -0.05, 0.3))         # 1000 columns a pixel
    long_c = warp.item(LONG, src, (17, 9), (3800 * ONE, 0, 0, 0, ONE // 3, 0), BICUBIC | WRAP, FILL, proj=tilt((17, 9), -0.7, 0.1))
    items = [wide, long_, wide_n, long_c]
    for it in items:
        assert warp._wrong(33000, 48, it[1:5], it[5:7], (it[8], it[9], it[14], it[10], it[11], it[15]), it[7], it[13]) == "", it
    for it in (long_, long_c):
        Px, _ = warp.positions(it[5:7], (it[8], it[9], it[14], it[10], it[11], it[15]), it[7], it[13])
        assert int(Px.max()) >= 2 ** 32 and int(Px.min()) < 2 ** 32
    g, h = warp.proj_of(wide[13])
    assert 2 ** 31 + abs(g) * 69999 - abs(h) * 2 > 2 ** 31 > 2 ** 31 - abs(g) * 69999 - abs(h) * 2 >= 2 ** 28        # W on both sides of 2**31
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
        assert_bytes(p, got, items, channels, mode, "wide")


def test_more_tiles_than_workgroups(ctx, pack):
    """[small, big, small, small] in one launch of warp_proj_bytes: big takes more than 8 * cu tiles of 16 x 16 - what a launch has
    workgroups for - with the last column and row of tiles partial, so every workgroup walks several tiles and some walk across entries"""
    import torch
    p = pack
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    across = 40
    down = (8 * cus) // across + 2
    ow, oh = 16 * across - 3, 16 * down - 5
    m, gh, _ = warp.perspective((64, 48), (ow, oh), [(6.0, 3.0), (60.0, 8.5), (57.0, 45.0), (2.0, 40.0)])
    big = warp.item(RGB, (0, 0, 64, 48), (ow, oh), m, REPLICATE, FILL, proj=gh)
    small = proj_items(BICUBIC, (REFLECT_101,))
    items = [small[0], big, small[3], warp.item(RGBA, (0, 0, 33, 21), (9, 9), warp.rotation((33, 21), (9, 9), 10.0, 0.3), SUPER2 | WRAP, FILL)]
    assert warp.tiles(ow, oh) == across * down > 8 * cus and gh != (0, 0)
    got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED, front=64 + 3)
    assert ctx.warp_stats()[:2] == (1, 1)
    assert_bytes(p, got, items, 4, ALPHA_WEIGHTED, "many tiles")


def test_sub_batches(api, pack):
    """a small staging_bytes forces one sub-batch per image: the same bytes, one launch of the kernel per sub-batch"""
    p = pack
    c = api.Context(0)
    try:
        items = proj_items(0, (REFLECT_101, 0)) + proj_items(BICUBIC, (WRAP,))
        single = run_warp(c, p, 4, items, ALPHA_WEIGHTED)
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
    turn = warp.rotation((33, 21), (8, 5), 30.0, 0.25)
    good = warp.item(RGBA, (0, 0, 33, 21), (8, 5), turn, REPLICATE, FILL, proj=tilt((8, 5), 0.5, 0.4))

    def call(items, tensor):
        arr = (api.QoimiWarp * len(items))(*[api.QoimiWarp(*it) for it in items])
        offsets = (ctypes.c_size_t * len(items))(*[64 + 1024 * j for j in range(len(items))])
        if tensor:
            return lib.qoimi_decode_warped_tensors(ctx._h, *args, 4, arr, len(items), 0, ctypes.byref(fmt), buf.data_ptr(), offsets, 0, None)
        return lib.qoimi_decode_warped(ctx._h, *args, 4, arr, len(items), 0, buf.data_ptr(), offsets, 0, None)

    far = turn[:2] + (2 ** 53,) + turn[3:]
    bad_items = [(good[:7] + (good[7] | SUPER2,) + good[8:], "item 1: the projective map is defined for the bilinear, nearest and bicubic samplings"),
                 (good[:7] + (PROJECTIVE | VOTE4,) + good[8:], "item 1: the projective map is defined for the bilinear, nearest and bicubic samplings"),
                 (warp.item(RGBA, (0, 0, 33, 21), (8, 5), far, REPLICATE, FILL, proj=(0, 0)), "item 1: |c| or |f| is 2^53 or more with QOIMI_WARP_PROJECTIVE"),
                 (good[:13] + (warp.proj_reserved(*tilt((8, 5), 0.7, 0.4)),) + good[14:], "item 1: the denominator of QOIMI_WARP_PROJECTIVE falls below 1/8 inside the output"),
                 (good[:7] + (good[7] | 32768,) + good[8:], "item 1: unknown flag bit"), (good[:7] + (good[7] | 65536,) + good[8:], "item 1: unknown flag bit"),
                 (good[:7] + (REPLICATE,) + good[8:], "item 1: reserved is not 0")]
    for tensor in (False, True):
        stats = ctx.tensor_stats() if tensor else ctx.warp_stats()
        for bad, word in bad_items:
            assert call([good, bad], tensor) == E_ARG and word in api.last_error(), (bad, api.last_error())
            assert bool((buf == GUARD).all()) and (ctx.tensor_stats() if tensor else ctx.warp_stats()) == stats, bad
    assert call([good], False) == 0, api.last_error()                                       # the context serves the next call
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:64 + 160], model(p, good, 4).reshape(-1)) and np.all(got[:64] == GUARD) and np.all(got[64 + 160:] == GUARD)
