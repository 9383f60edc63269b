"""qoimi_decode_warped and qoimi_decode_warped_indexed on the GPU (-m gpu): rectangles of a pack's images sampled through affine maps through
bounded staging.  The expectation is always the definition: the oracle decodes the stream at the call's output channel count, and
qoi_amd/warp.py: warp samples that; the identity is also compared with qoimi_decode_crops and the power-of-two enlargement with
qoimi_decode_bilinear on the device.  Every comparison is exact and covers the whole output.  Outputs stand behind, between and in front of
guard bytes (0xA5); every guard byte is checked after every call.  Sub-batch boundaries are forced through staging_bytes by
qoi_amd/warp.py: plan (qoimi_warp_stats says that the call really ran that many sub-batches over that much staging)."""
import ctypes

import numpy as np
import pytest

from qoi_amd import warp
from qoi_amd.packplan import slot
from qoi_amd.warp import ALPHA_WEIGHTED, ONE, PLAIN, REPLICATE
from gpu_calls import assert_warp_items as assert_items, run_warp as run, sizes_of, want_warp as want
from gpu_pack import E_ARG, GUARD, KINDS, MIXED_SHAPES, Batch, Pack, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BIG = 7                               # 130 x 70 x 4, sprite_alpha
FILL = 0x40C08020


@pytest.fixture(scope="module")
def mixed(api, ctx, oracle):
    """the mixed pack of tests/test_gpu_resize.py: shapes from 1 x 1 and 1 x 97 to 130 x 70, 3 and 4 channels, all content classes"""
    kinds = [KINDS[(i + 2) % 5] for i in range(len(MIXED_SHAPES))]
    assert set(kinds) == set(KINDS) and MIXED_SHAPES[BIG] == (130, 70, 4)
    return Pack(ctx, oracle, Batch(api, oracle, MIXED_SHAPES, kinds))


@pytest.fixture(scope="module")
def equal(api, ctx, oracle):
    return Pack(ctx, oracle, Batch(api, oracle, [(64, 48, 4)] * 7, [KINDS[i % 5] for i in range(7)]))


def general(i, rect, k=0):
    """a 30 degree turn, a shear, scales of about 0.37 and 3.1, a quarter turn by the general formula: borders and fills take turns"""
    cw, rh = rect[2:]
    outs = [(41, 29), (33, 18), (17, 1), (1, 17), (23, 40)]
    maps = [warp.rotation((cw, rh), outs[0], 30.0), (ONE, 23000, cw * ONE - ONE * 33 - 23000 * 18, -9000, ONE + 700, rh * ONE + 9000 * 33 - (ONE + 700) * 18),
            warp.rotation((cw, rh), outs[2], 0.0, 0.37), warp.rotation((cw, rh), outs[3], 0.0, 3.1), warp.rotation((cw, rh), outs[4], 90.0, 0.8)]
    return [warp.item(i, rect, o, m, (k + j) & 1, (FILL, 0x00FFFFFF, 0)[(k + j) % 3]) for j, (o, m) in enumerate(zip(outs, maps))]


# ------------------------------------------------------------------ 1: the identities on the device
@pytest.mark.parametrize("channels", [4, 3])
def test_identity_items_are_the_crops(ctx, mixed, channels):
    p = mixed
    cs = [(BIG, 0, 0, 130, 70, 0), (BIG, 17, 11, 31, 7, 0), (3, 1, 3, 35, 19, 0), (4, 250, 0, 7, 9, 0), (0, 0, 0, 1, 1, 0), (2, 120, 0, 11, 1, 0), (1, 0, 90, 1, 7, 0)]
    items = [warp.item(i, (x, y, cw, ch), (cw, ch), flags=j & 1, fill=FILL) for j, (i, x, y, cw, ch, _) in enumerate(cs)]
    nbytes = [c[3] * c[4] * channels for c in cs]
    offsets = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
    ctx.decode_crops(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, cs, buf.data_ptr(), offsets)
    cropped = buf.cpu().numpy()
    for mode in (PLAIN, ALPHA_WEIGHTED):
        got = run(ctx, p, channels, items, mode)
        for j, (o, n) in enumerate(zip(offsets, nbytes)):
            assert np.array_equal(got[j], cropped[o:o + n]), (channels, mode, j)
    assert ctx.warp_stats()[:2] == (1, 1)


def oriented(R, orientation):
    return {1: R, 2: R[:, ::-1], 3: R[::-1, ::-1], 4: R[::-1], 5: R.transpose(1, 0, 2), 6: np.rot90(R, -1), 7: R[::-1, ::-1].transpose(1, 0, 2),
            8: np.rot90(R, 1)}[orientation]


@pytest.mark.parametrize("channels", [4, 3])
def test_the_eight_orientations(api, ctx, mixed, channels):
    p = mixed
    items, rects = [], []
    for i, rect in ((BIG, (0, 0, 130, 70)), (BIG, (17, 11, 31, 7)), (3, (1, 3, 35, 19)), (1, (0, 90, 1, 7)), (0, (0, 0, 1, 1))):
        for o in range(1, 9):
            w, h, ch = p.shapes[i]
            it = api.warp_orient(w, h, ch, rect, o)
            it.image = i
            items.append(warp.fields(it)); rects.append((i, rect, o))
    got = run(ctx, p, channels, items, PLAIN, front=64 + 3)
    for g, (i, (x, y, cw, rh), o) in zip(got, rects):
        assert np.array_equal(g, np.ascontiguousarray(oriented(p.decoded(i, channels)[y:y + rh, x:x + cw], o)).reshape(-1)), (i, o)


@pytest.mark.parametrize("channels,mode", [(4, ALPHA_WEIGHTED), (3, PLAIN)])
def test_power_of_two_enlargement_is_decode_bilinear(ctx, mixed, channels, mode):
    p = mixed
    rs = [(BIG, 17, 11, 31, 7, 62, 14, 0), (BIG, 0, 0, 13, 9, 104, 72, 0), (3, 1, 3, 35, 19, 70, 76, 0), (0, 0, 0, 1, 1, 4, 8, 0), (1, 0, 90, 1, 7, 2, 28, 0)]
    items = [warp.item(i, (x, y, cw, rh), (ow, oh), (ONE * cw // ow, 0, 0, 0, ONE * rh // oh, 0), REPLICATE) for (i, x, y, cw, rh, ow, oh, _) in rs]
    nbytes = sizes_of(items, channels)
    offsets = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
    ctx.decode_bilinear(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, rs, mode, buf.data_ptr(), offsets)
    ref = buf.cpu().numpy()
    got = run(ctx, p, channels, items, mode)
    for j, (o, n) in enumerate(zip(offsets, nbytes)):
        assert np.array_equal(got[j], ref[o:o + n]), (channels, mode, j)


# ------------------------------------------------------------------ 2: general maps against the model
@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("channels", [4, 3])
def test_general_maps(ctx, mixed, channels, mode):
    p = mixed
    items = general(BIG, (0, 0, 130, 70)) + general(BIG, (9, 5, 101, 33), 1) + general(3, (1, 3, 35, 19), 2) + general(5, (0, 0, 64, 48), 3) + general(0, (0, 0, 1, 1), 4)
    # an opaque image turned by 45 degrees over a transparent white fill: in the alpha-weighted mode the border keeps the image's colours
    items.append(warp.item(5, (0, 0, 64, 48), (30, 30), warp.rotation((64, 48), (30, 30), 45.0, 0.3), 0, 0x00FFFFFF))
    assert {it[7] for it in items} == {0, REPLICATE} and {it[12] for it in items} == {FILL, 0x00FFFFFF, 0}
    got = run(ctx, p, channels, items, mode)
    assert_items(p, got, items, channels, mode, (channels, mode))
    assert ctx.warp_stats()[:2] == (1, 1) and ctx.warp_stats()[3] == 4
    if channels == 4 and mode == ALPHA_WEIGHTED:
        assert not np.array_equal(want(p, items[-1], 4, PLAIN), got[-1]) and np.any(got[-1].reshape(-1, 4)[:, 3] == 0)


def test_positions_past_32_bits(api, ctx, oracle):
    """an image of 33000 x 3: a rectangle over all its columns, the output the 9 columns from 32990 on, turned by 180 degrees and not - Px
    passes 2**32 on the device (column 32768 lies at 2**32 + 2**16)"""
    p = Pack(ctx, oracle, Batch(api, oracle, [(33000, 3, 4)], ["noise"]))
    rect = (0, 0, 33000, 3)
    items = [warp.item(0, rect, (9, 3), (ONE, 0, 2 * 32990 * ONE, 0, ONE, 0), 0, FILL),
             warp.item(0, rect, (9, 3), (-ONE, 0, 2 * 32999 * ONE + 777, 0, -ONE, 2 * 3 * ONE - 999), REPLICATE),
             warp.item(0, rect, (40, 5), (ONE // 3, 0, 2 * 32985 * ONE + 4321, 0, ONE // 2, -ONE), 0, FILL)]
    assert all(it[14] > 2 ** 32 for it in items)
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run(ctx, p, channels, items, mode, front=64 + 1)
        assert_items(p, got, items, channels, mode, ("wide", channels))
    assert np.array_equal(got[0], p.decoded(0, 3)[:, 32990:32999].reshape(-1))


# ------------------------------------------------------------------ 3: placement
@pytest.mark.parametrize("channels", [3, 4])
def test_every_alignment_with_guards(ctx, mixed, channels):
    """outputs of 1, 2, 5 pixels, a row, a column and 33 x 18, back to back: neighbours share aligned words; every alignment of the first"""
    p = mixed
    outs = [(1, 1), (2, 1), (5, 1), (17, 1), (1, 17), (33, 18), (1, 1)]
    items = [warp.item(BIG, (3, 5, 55, 35), o, warp.rotation((55, 35), o, 30.0 + 50 * j, 0.9), j & 1, FILL) for j, o in enumerate(outs)]
    for shift in (0, 1, 2, 3):
        got = run(ctx, p, channels, items, ALPHA_WEIGHTED, front=64 + shift)
        assert_items(p, got, items, channels, ALPHA_WEIGHTED, (channels, shift))
    # gaps of one byte between outputs in descending order keep their guards
    nbytes = sizes_of(items, channels)
    offsets, pos = [0] * len(items), 33
    for j in reversed(range(len(items))):
        offsets[j] = pos
        pos += nbytes[j] + (6, 1, 3, 0)[j % 4]
    got = run(ctx, p, channels, items, PLAIN, offsets=offsets, total=pos + 77)
    assert_items(p, got, items, channels, PLAIN, ("order", channels))


def test_tile_walk_regimes(api, ctx, oracle, mixed):
    """(qoi_dev.h: walk_tiles) a launch with ONE table entry, its 12 tiles spread over as many workgroups; and more tiles than the grid's
    clamp of 8 workgroups per compute unit - 37 more items of one tile each - so that a workgroup takes two tiles and steps from item to item.
    The 3-byte outputs stand back to back: neighbours share aligned words."""
    import torch
    one = warp.item(BIG, (0, 0, 130, 70), (61, 47), warp.rotation((130, 70), (61, 47), 30.0, 0.5), 0, FILL)
    assert warp.tiles(61, 47) == 12 and warp.tiles(1, 1) == 1
    assert_items(mixed, run(ctx, mixed, 4, [one], ALPHA_WEIGHTED), [one], 4, ALPHA_WEIGHTED, "one entry")
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    p = Pack(ctx, oracle, Batch(api, oracle, [(8, 8, 4)], ["noise"]))
    items = [warp.item(0, (j % 7, (j // 7) % 7, 2, 2), (1, 1), (ONE, 0, (j % 5) * 9000, 0, ONE, (j % 3) * 20000), j & 1, FILL) for j in range(n)]
    for channels, mode in ((3, PLAIN), (4, ALPHA_WEIGHTED)):
        assert_items(p, run(ctx, p, channels, items, mode, front=64 + 5), items, channels, mode, ("many", channels))
        assert ctx.warp_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 4: sub-batches
def test_sub_batches(api, equal):
    c = api.Context(0)
    try:
        p = equal
        items = [x for i in range(6) for x in general(i, (3, 2, 55, 46), i)]          # image 6 has no item
        one = slot(64 * 48 * 4)
        single = run(c, p, 4, items, ALPHA_WEIGHTED)
        assert c.warp_stats() == (1, 1, 6 * one, 6)
        assert_items(p, single, items, 4, ALPHA_WEIGHTED, "single")
        for staging, subs, per in ((1, 6, 1), (2 * one, 3, 2), (3 * one + 255, 2, 3), (0, 1, 6)):
            images, slots, the_plan, largest = warp.plan(p.descs, items, staging)
            assert images == list(range(6)) and len(the_plan) == subs and all(count == per for _, count in the_plan) and largest == per * one
            got = run(c, p, 4, items, ALPHA_WEIGHTED, staging=staging)
            assert c.warp_stats() == (subs, subs, largest, 6), (staging, c.warp_stats())
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        # rows_i is the largest y + height of the image's items: a rectangle of the upper rows stages only those
        top = [warp.item(2, (0, 0, 64, 10), (20, 20), warp.rotation((64, 10), (20, 20), 45.0), 0, FILL)]
        assert_items(p, run(c, p, 3, top), top, 3, PLAIN, "top")
        assert c.warp_stats() == (1, 1, slot(64 * 10 * 4), 1)
    finally:
        c.close()


# ------------------------------------------------------------------ 5: through a seek index
def test_indexed_equals_the_plain_call(ctx, equal):
    """an index from qoimi_build_seek_index at 8 rows per interval; items in the top, a middle and the last band, several per image; image 6
    has none"""
    p = equal
    K = 8
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, K)
    rects = [(0, 0, 1, 64, 5), (0, 10, 19, 40, 22), (1, 3, 41, 33, 7), (2, 0, 30, 64, 18), (3, 63, 47, 1, 1), (4, 5, 17, 12, 3), (5, 0, 24, 64, 24), (5, 7, 40, 9, 8)]
    outs = [(13, 2), (50, 30), (2, 7), (18, 64), (3, 2), (12, 3), (33, 5), (20, 20)]
    items = [warp.item(r[0], r[1:], o, warp.rotation(r[3:], o, 25.0 * j, 1.2), j & 1, FILL) for j, (r, o) in enumerate(zip(rects, outs))]
    for channels, mode, staging in ((4, ALPHA_WEIGHTED, 0), (3, PLAIN, 1), (0, PLAIN, 0)):
        plain = run(ctx, p, channels, items, mode, staging=staging)
        plain_stats = ctx.warp_stats()
        indexed = run(ctx, p, channels, items, mode, call=lambda out, offsets: ctx.decode_warped_indexed(
            p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, out, offsets, [K] * p.n, points, firsts, staging_bytes=staging))
        stats, seek = ctx.warp_stats(), ctx.seek_stats()
        assert all(np.array_equal(a, b) for a, b in zip(plain, indexed)), (channels, mode)
        assert_items(p, indexed, items, channels or 4, mode, ("indexed", channels))
        assert stats[:2] == plain_stats[:2] and stats[3] == 6 and stats[2] <= plain_stats[2]                     # (a band is no longer than its image)
        assert staging != 0 or stats[2] < plain_stats[2]
        assert seek[1] == 6 and seek[2] > 0


# ------------------------------------------------------------------ 6: rejections on a live context, and the context afterwards
def test_rejections_on_a_live_context(api, ctx, mixed):
    p = mixed
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)

    def call(items, offsets, channels=4, mode=0):
        arr = (api.QoimiWarp * len(items))(*[api.QoimiWarp(*it) for it in items])
        return lib.qoimi_decode_warped(ctx._h, *args, channels, arr, len(items), mode, buf.data_ptr(), (ctypes.c_size_t * len(items))(*offsets), 0, None)

    def one(rect=(0, 0, 10, 10), out=(10, 10), m=warp.IDENTITY, flags=0, reserved=0, image=BIG):
        t = warp.item(image, rect, out, m, flags, FILL)
        return t[:13] + (reserved,) + t[14:]

    two = [warp.item(BIG, (0, 0, 100, 60), (10, 10), warp.rotation((100, 60), (10, 10), 30.0, 0.1), 0, FILL), warp.item(5, (0, 0, 8, 8), (8, 8), flags=REPLICATE)]
    assert call(two, [100, 100 + 400]) == 0                                           # side by side: accepted
    got = buf.cpu().numpy()
    assert np.array_equal(got[100:500], want(p, two[0], 4, PLAIN)) and np.array_equal(got[500:756], want(p, two[1], 4, PLAIN))
    assert np.all(got[:100] == GUARD) and np.all(got[756:] == GUARD)
    stats = ctx.warp_stats()
    assert stats == (1, 1, slot(130 * 60 * 4) + slot(64 * 8 * 4), 2)
    buf.fill_(GUARD)
    rejected = [
        (lambda: call(two, [100, 100 + 399]), "overlap"), (lambda: call(two, [100 + 255, 100]), "overlap"),
        (lambda: call([one(rect=(121, 0, 10, 10))], [64]), "leaves"), (lambda: call([one(rect=(0, 61, 10, 10))], [64]), "leaves"),
        (lambda: call([one(out=(1 << 20, 1))], [64]), "2^20"), (lambda: call([one(out=(20000, 20000))], [64]), "400 000 000"),
        (lambda: call([one(m=(ONE, 0, 1 << 56, 0, ONE, 0))], [64]), "2^56"), (lambda: call([one(flags=2)], [64]), "flag"), (lambda: call([one(reserved=1)], [64]), "reserved"),
        (lambda: call(two, [100, 600], mode=2), "mode"), (lambda: call(two, [100, 600], mode=-1), "mode"),
        (lambda: call([one(rect=(0, 0, 1, 1), out=(1, 1), image=2), one(rect=(0, 0, 1, 1), out=(1, 1))], [64, 128], channels=0), "channel"),
    ]
    for f, word in rejected:
        assert f() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.warp_stats() == stats, word
    with pytest.raises(api.QoiError):
        ctx.decode_warped(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, two, PLAIN, buf.data_ptr(), [100, 100 + 399])
    assert bool((buf == GUARD).all()) and ctx.warp_stats() == stats
    # the context works afterwards: the same call and a decode_images give their exact results
    got = run(ctx, p, 4, two, ALPHA_WEIGHTED)
    assert_items(p, got, two, 4, ALPHA_WEIGHTED, "afterwards")
    nbytes = [w * h * 4 for (w, h, _) in p.shapes]
    offsets = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    out = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
    ctx.decode_images(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, out.data_ptr(), offsets)
    got = out.cpu().numpy()
    for i, (o, nb) in enumerate(zip(offsets, nbytes)):
        assert np.array_equal(got[o:o + nb], p.decoded(i, 4).reshape(-1)), i
    assert np.all(got[:64] == GUARD) and np.all(got[-64:] == GUARD)
