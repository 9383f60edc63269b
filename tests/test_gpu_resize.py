"""qoimi_decode_resized on the GPU (-m gpu): rectangles of a pack's images resampled to fixed sizes through bounded staging.  The expectation is
always the definition: the oracle decodes the stream as it is given (whole, cut, with a foreign end marker) at the call's output channel
count, and qoi_amd/resize.py: resize resamples that.  Every comparison is exact.  Outputs stand behind, between and in front of guard bytes
(0xA5); every guard byte is checked after every call.  Sub-batch boundaries are forced through staging_bytes by qoi_amd/resize.py: plan
(qoimi_resize_stats says that the call really ran that many sub-batches over that much staging)."""
import ctypes

import numpy as np
import pytest

from qoi_amd import crops, resize, thumbs
from qoi_amd.packplan import slot
from qoi_amd.resize import ALPHA_WEIGHTED, PLAIN
from gpu_calls import run_resized as run, sizes_of, standard
from gpu_pack import E_ARG, GUARD, KINDS, MIXED_SHAPES, Batch, Pack, dev, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BIG = 7                               # 130 x 70 x 4, sprite_alpha


@pytest.fixture(scope="module")
def mixed(api, ctx, oracle):
    """3 and 4 channels, all content classes"""
    kinds = [KINDS[(i + 2) % 5] for i in range(len(MIXED_SHAPES))]
    assert set(kinds) == set(KINDS) and MIXED_SHAPES[BIG] == (130, 70, 4)
    return Pack(ctx, oracle, Batch(api, oracle, MIXED_SHAPES, kinds))


@pytest.fixture(scope="module")
def equal(api, ctx, oracle):
    return Pack(ctx, oracle, Batch(api, oracle, [(64, 48, 4)] * 7, [KINDS[i % 5] for i in range(7)]))


def want(p, it, och, mode, **how):
    i, x, y, cw, rh, ow, oh, flags = it
    return resize.resize(p.decoded(i, och, **how), (x, y, cw, rh), (ow, oh), flags, mode).reshape(-1)


def assert_items(p, got, items, och, mode, what):
    for j, it in enumerate(items):
        w = want(p, it, och, mode)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, it, int(np.argmax(got[j] != w)))


# ------------------------------------------------------------------ 1: the mixed pack
@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("channels", [4, 3])
def test_mixed_pack(ctx, mixed, channels, mode):
    p = mixed
    items = [it for i, (w, h, _) in enumerate(p.shapes) for it in standard(i, w, h, i)]
    assert {it[7] for it in items} == {0, 1, 2, 3} and (BIG, 0, 0, 130, 70, 37, 23, 1) in items and (BIG, 0, 0, 130, 70, 3, 2, 0) in items
    assert (0, 0, 0, 1, 1, 1, 1, 1) in items and (5, 0, 0, 64, 48, 1, 1, 2) in items                # 64 x 48 to 1 x 1: 64 taps in x
    assert any(it[1] % 2 and it[2] % 2 and it[3] % 2 and it[4] % 2 and it[5] % 2 and it[6] % 2 for it in items)
    assert any(it[3] > it[5] and it[4] < it[6] for it in items)                                       # down in x with up in y
    assert {resize.split(it[3], it[5])[0] for it in items} == {0, 1, 2, 3, 4}                         # every number of lanes per pixel
    got = run(ctx, p, channels, items, mode)
    assert_items(p, got, items, channels, mode, (channels, mode))
    assert ctx.resize_stats()[:2] == (1, 1) and ctx.resize_stats()[3] == p.n


@pytest.mark.parametrize("och", [4, 3])
def test_the_images_own_channels(api, ctx, mixed, och):
    """channels 0: the referenced images share a channel count, the others of the pack need not; mixing them is rejected"""
    p = mixed
    images = [i for i, s in enumerate(p.shapes) if s[2] == och]
    assert 3 <= len(images) < p.n
    items = [it for i in images for it in standard(i, p.shapes[i][0], p.shapes[i][1], i + 1)]
    got = run(ctx, p, 0, items, ALPHA_WEIGHTED)
    assert [g.size for g in got] == sizes_of(items, och)
    assert_items(p, got, items, och, ALPHA_WEIGHTED, ("own", och))
    stats = ctx.resize_stats()
    assert stats[3] == len(images)
    other = [i for i, s in enumerate(p.shapes) if s[2] != och][0]
    buf = filled(4096, GUARD)
    with pytest.raises(api.QoiError):
        ctx.decode_resized(p.packed.data_ptr(), p.so, p.sizes, p.descs, 0, [(images[0], 0, 0, 1, 1, 2, 2, 0), (other, 0, 0, 1, 1, 2, 2, 0)], PLAIN, buf.data_ptr(), [64, 128])
    assert "channel" in api.last_error() and bool((buf == GUARD).all()) and ctx.resize_stats() == stats


# ------------------------------------------------------------------ 2: agreement with the siblings on the device
@pytest.mark.parametrize("channels", [4, 3])
def test_identity_items_are_the_crops(ctx, mixed, channels):
    p = mixed
    cs = [(BIG, 0, 0, 130, 70, 1), (BIG, 17, 11, 31, 7, 2), (3, 1, 3, 35, 19, 3), (4, 250, 0, 7, 9, 0), (0, 0, 0, 1, 1, 1), (2, 120, 0, 11, 1, 2), (1, 0, 90, 1, 7, 3)]
    items = [(i, x, y, cw, ch, cw, ch, flags) for (i, x, y, cw, ch, flags) in cs]
    nbytes = [c[3] * c[4] * channels for c in cs]
    offsets = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
    ctx.decode_crops(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, cs, buf.data_ptr(), offsets)
    cropped = buf.cpu().numpy()
    for mode in (PLAIN, ALPHA_WEIGHTED):
        got = run(ctx, p, channels, items, mode)
        for j, (o, n) in enumerate(zip(offsets, nbytes)):
            assert np.array_equal(got[j], cropped[o:o + n]), (channels, mode, j)
            assert np.array_equal(got[j], crops.crop(p.decoded(cs[j][0], channels), cs[j][1:5], cs[j][5]).reshape(-1))


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_whole_multiples_are_the_thumbnails(ctx, equal, mode):
    p = equal
    for channels in (4, 3):
        for f in (2, 4, 16):
            tw, th = 64 // f, 48 // f
            nbytes = [tw * th * channels] * p.n
            offsets = [64 + i * nbytes[0] for i in range(p.n)]
            buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
            ctx.decode_thumbnails(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, f, mode, buf.data_ptr(), offsets)
            reduced = buf.cpu().numpy()
            items = [(i, 0, 0, 64, 48, tw, th, 0) for i in range(p.n)]
            got = run(ctx, p, channels, items, mode)
            for i in range(p.n):
                assert np.array_equal(got[i], reduced[offsets[i]:offsets[i] + nbytes[i]]), (channels, f, mode, i)
                assert np.array_equal(got[i], thumbs.thumbnail(p.decoded(i, channels), f, mode).reshape(-1))


# ------------------------------------------------------------------ 3: placement
PLACED = [(3, 4, 5, 1, 1, 1, 1, 0), (3, 7, 2, 9, 5, 2, 1, 1), (5, 9, 9, 20, 7, 5, 1, 2), (3, 30, 3, 1, 6, 1, 6, 3), (5, 1, 1, 3, 2, 3, 2, 1), (BIG, 17, 11, 1, 1, 1, 1, 0),
          (BIG, 3, 5, 55, 35, 11, 7, 3), (4, 250, 0, 7, 9, 7, 9, 2), (0, 0, 0, 1, 1, 1, 1, 1), (1, 0, 90, 1, 7, 1, 7, 2), (2, 120, 0, 11, 1, 11, 1, 1), (6, 1, 1, 331, 5, 33, 5, 3),
          (3, 0, 0, 4, 4, 2, 1, 0), (3, 36, 22, 1, 1, 1, 1, 0)]


@pytest.mark.parametrize("channels", [3, 4])
def test_outputs_back_to_back_at_odd_offsets(ctx, mixed, channels):
    """1, 2, 5 and 6 pixels (3 to 18 bytes at 3 channels: outputs inside one aligned 16-byte word, outputs that straddle one), rows, columns,
    rectangles; neighbours share aligned words"""
    p = mixed
    for shift in (0, 1, 3, 5, 15):
        got = run(ctx, p, channels, PLACED, ALPHA_WEIGHTED, front=64 + shift)
        assert_items(p, got, PLACED, channels, ALPHA_WEIGHTED, (channels, shift))


def test_reverse_order_and_one_byte_gaps(ctx, mixed):
    """output offsets descend while the item order ascends; the items are not sorted by image; gaps of 6, 1, 3 and 0 bytes keep their guards"""
    p = mixed
    items = [(5, 3, 3, 31, 17, 13, 5, 1), (BIG, 1, 1, 99, 33, 40, 9, 2), (0, 0, 0, 1, 1, 3, 3, 0), (5, 0, 40, 64, 8, 7, 3, 3), (2, 7, 0, 101, 1, 9, 2, 1), (BIG, 100, 60, 30, 10, 30, 10, 0),
             (1, 0, 5, 1, 77, 1, 11, 2)]
    for channels in (4, 3):
        nbytes = sizes_of(items, channels)
        offsets, pos = [0] * len(items), 33
        for j in reversed(range(len(items))):
            offsets[j] = pos
            pos += nbytes[j] + (6, 1, 3, 0)[j % 4]
        assert all(offsets[j] > offsets[j + 1] for j in range(len(items) - 1))
        got = run(ctx, p, channels, items, PLAIN, offsets=offsets, total=pos + 77)
        assert_items(p, got, items, channels, PLAIN, ("order", channels))


# ------------------------------------------------------------------ 4: more than one tile, stepping from item to item
def test_large_items_between_small_ones(ctx, mixed):
    p = mixed
    big = (BIG, 0, 0, 130, 70, 61, 47, 1)                              # 2867 pixels of one lane: 12 tiles
    up = (3, 2, 1, 30, 20, 71, 43, 2)                                  # 3053 pixels of one lane: 12 tiles
    assert resize.tiles(130, 61, 47) == 12 and resize.tiles(30, 71, 43) == 12
    items = [(0, 0, 0, 1, 1, 1, 1, 0), (3, 5, 5, 1, 1, 2, 2, 0), big, (3, 36, 22, 1, 1, 1, 1, 0), up, (BIG, 129, 69, 1, 1, 1, 1, 3), big[:7] + (2,), (0, 0, 0, 1, 1, 1, 1, 2)]
    for channels, shift in ((4, 0), (3, 7)):
        got = run(ctx, p, channels, items, ALPHA_WEIGHTED, front=64 + shift)
        assert_items(p, got, items, channels, ALPHA_WEIGHTED, ("large", channels, shift))


def test_tile_walk_regimes(api, ctx, oracle, mixed):
    """(qoi_dev.h: walk_tiles) a launch with ONE table entry, its 12 tiles spread over as many workgroups; and more tiles than the grid's
    clamp of 8 workgroups per compute unit - 37 more items of one tile each - so that a workgroup takes two tiles and steps from item to item.
    The 3-byte outputs stand back to back: neighbours share aligned words."""
    import torch
    one = (BIG, 0, 0, 130, 70, 61, 47, 3)
    assert resize.tiles(130, 61, 47) == 12 and resize.tiles(1, 1, 1) == 1
    assert_items(mixed, run(ctx, mixed, 4, [one], ALPHA_WEIGHTED), [one], 4, ALPHA_WEIGHTED, "one entry")
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    p = Pack(ctx, oracle, Batch(api, oracle, [(8, 8, 4)], ["noise"]))
    items = [(0, j % 8, (j // 8) % 8, 1, 1, 1, 1, j & 3) for j in range(n)]
    for channels, mode in ((3, PLAIN), (4, ALPHA_WEIGHTED)):
        assert_items(p, run(ctx, p, channels, items, mode, front=64 + 5), items, channels, mode, ("many", channels))
        assert ctx.resize_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 5: sub-batches
def test_sub_batches(api, mixed, equal):
    c = api.Context(0)
    try:
        p = equal
        items = [x for i in range(6) for x in standard(i, 64, 48, i)]                # image 6 has no item
        one = slot(64 * 48 * 4)
        single = run(c, p, 4, items, ALPHA_WEIGHTED)
        assert c.resize_stats() == (1, 1, 6 * one, 6)
        assert_items(p, single, items, 4, ALPHA_WEIGHTED, "single")
        for staging, subs, per in ((1, 6, 1), (one, 6, 1), (2 * one, 3, 2), (3 * one + 255, 2, 3), (0, 1, 6)):
            images, slots, the_plan, largest = resize.plan(p.descs, items, staging)
            assert images == list(range(6)) and len(the_plan) == subs and all(count == per for _, count in the_plan) and largest == per * one
            got = run(c, p, 4, items, ALPHA_WEIGHTED, staging=staging)
            assert c.resize_stats() == (subs, subs, largest, 6), (staging, c.resize_stats())
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        # the arena is allocated as the largest sub-batch of a call plus a page: what the context holds covers the largest plan so far
        assert c.workspace_bytes()["decode"] >= 6 * one + 4096
        # the mixed pack, items in any order of image, one, two to three and all images per sub-batch
        p = mixed
        items = [x for i in (5, 0, 7, 2, 6, 1, 4, 3) for x in standard(i, p.shapes[i][0], p.shapes[i][1], i)]
        single = run(c, p, 3, items)
        assert_items(p, single, items, 3, PLAIN, "mixed single")
        for staging in (1, 13000, 40000):
            images, slots, the_plan, largest = resize.plan(p.descs, items, staging)
            got = run(c, p, 3, items, staging=staging)
            assert c.resize_stats() == (len(the_plan), len(the_plan), largest, 8), (staging, c.resize_stats(), the_plan)
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        assert len(resize.plan(p.descs, items, 1)[2]) == 8 and 2 <= len(resize.plan(p.descs, items, 13000)[2]) < 8
    finally:
        c.close()


def test_workspace_is_consistent_with_the_plan(api, mixed):
    """a fresh context: after one call qoimi_workspace_bytes [1] has grown by at least the staging the call planned for ([2]) plus a page"""
    p = mixed
    c = api.Context(0)
    try:
        before = c.workspace_bytes()["decode"]
        items = [(BIG, 0, 0, 130, 70, 37, 23, 0), (5, 0, 0, 64, 48, 224, 224, 1)]
        run(c, p, 4, items)
        planned = c.resize_stats()[2]
        assert planned == slot(130 * 70 * 4) + slot(64 * 48 * 4) == resize.plan(p.descs, items, 0)[3]
        grown = c.workspace_bytes()["decode"] - before
        assert grown >= planned + 4096, (planned, grown)                 # (the table and the decoder's own workspace for two small images are in there too)
    finally:
        c.close()


# ------------------------------------------------------------------ 6: only the rows an item needs are staged; unreferenced images
def test_row_truncation_and_unreferenced_images(api, ctx, mixed):
    p = mixed
    items = [(BIG, 0, 0, 130, 1, 13, 2, 0), (BIG, 5, 1, 121, 2, 224, 5, 1), (BIG, 129, 2, 1, 1, 3, 3, 2), (BIG, 0, 0, 130, 3, 3, 1, 3)]
    assert crops.rows_needed(p.descs, [resize.as_crop(it) for it in items]) == {BIG: 3}
    sizes = list(p.sizes)
    descs = list(p.descs)
    for i in range(p.n - 1):                                            # nobody names these: garbage sizes and descriptors
        sizes[i] = (0, -5, 7)[i % 3]
        descs[i] = api.QoiDesc(0, 0, 9, 9)
    for channels in (4, 3):
        got = run(ctx, p, channels, items, ALPHA_WEIGHTED, sizes=sizes, descs=descs)
        assert_items(p, got, items, channels, ALPHA_WEIGHTED, ("rows", channels))
        assert ctx.resize_stats() == (1, 1, slot(130 * 3 * 4), 1)
    w, h, _ = p.shapes[3]
    for r in (1, 2, h - 1, h):                                          # the decode down to row r is the prefix of the full decode
        got = run(ctx, p, 3, [(3, 0, r - 1, w, 1, 5, 2, 0), (3, 0, 0, w, r, w, r, 0)])
        assert np.array_equal(got[1].reshape(r, w, 3), p.decoded(3, 3)[:r]), r
        assert ctx.resize_stats()[2:] == (slot(w * r * 4), 1)


# ------------------------------------------------------------------ 7: leniency
def test_leniency(ctx, mixed):
    """a stream cut in the middle repeats its last pixel, a foreign end marker is ignored: as the oracle decodes them"""
    p = mixed
    cut, marker = 5, 3
    sizes = list(p.sizes)
    sizes[cut] = p.sizes[cut] // 2
    host = p.host.copy()
    end = p.so[marker] + p.sizes[marker]
    host[end - 8:end] = 0xEE
    damaged = dev(host)
    assert not np.array_equal(p.decoded(cut, 4, size=sizes[cut]), p.decoded(cut, 4))
    items = [(cut, 3, 31, 55, 17, 20, 20, 1), (cut, 0, 0, 64, 48, 9, 7, 0), (marker, 1, 12, 35, 11, 5, 30, 2), (marker, 0, 0, 37, 23, 1, 1, 3), (BIG, 0, 35, 130, 35, 65, 7, 0)]
    for channels in (4, 3):
        got = run(ctx, p, channels, items, ALPHA_WEIGHTED, sizes=sizes, packed=damaged)
        for j, it in enumerate(items):
            how = {"size": sizes[cut]} if it[0] == cut else {"host": host} if it[0] == marker else {}
            assert np.array_equal(got[j], want(p, it, channels, ALPHA_WEIGHTED, **how)), (channels, j)
    assert np.array_equal(damaged.cpu().numpy(), host)


# ------------------------------------------------------------------ 8: rejections on a live context, and the context afterwards
def test_rejections_on_a_live_context(api, ctx, mixed):
    p = mixed
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)

    def call(items, offsets, channels=4, mode=0):
        arr = (api.QoimiResize * len(items))(*[api.QoimiResize(*it) for it in items])
        return lib.qoimi_decode_resized(ctx._h, *args, channels, arr, len(items), mode, buf.data_ptr(), (ctypes.c_size_t * len(items))(*offsets), 0, None)

    two = [(BIG, 0, 0, 100, 60, 10, 10, 0), (5, 0, 0, 8, 8, 8, 8, 1)]
    assert call(two, [100, 100 + 400]) == 0                                           # side by side: accepted
    got = buf.cpu().numpy()
    assert np.array_equal(got[100:500], want(p, two[0], 4, PLAIN)) and np.array_equal(got[500:756], want(p, two[1], 4, PLAIN))
    assert np.all(got[:100] == GUARD) and np.all(got[756:] == GUARD)
    stats = ctx.resize_stats()
    assert stats == (1, 1, slot(130 * 60 * 4) + slot(64 * 8 * 4), 2)
    buf.fill_(GUARD)
    rejected = [
        (lambda: call(two, [100, 100 + 399]), "overlap"), (lambda: call(two, [100 + 255, 100]), "overlap"),
        (lambda: call([(BIG, 0, 0, 130, 1, 2, 1, 0)], [64]), "64"), (lambda: call([(BIG, 0, 0, 1, 66, 1, 1, 0)], [64]), "64"),
        (lambda: call([(BIG, 121, 0, 10, 10, 10, 10, 0)], [64]), "leaves"), (lambda: call([(BIG, 0, 61, 10, 10, 10, 10, 0)], [64]), "leaves"),
        (lambda: call([(BIG, 0, 0, 10, 10, 10, 10, 4)], [64]), "flag"), (lambda: call(two, [100, 600], mode=2), "mode"), (lambda: call(two, [100, 600], mode=-1), "mode"),
        (lambda: call([(2, 0, 0, 1, 1, 1, 1, 0), (BIG, 0, 0, 1, 1, 1, 1, 0)], [64, 128], channels=0), "channel"),
    ]
    for f, word in rejected:
        assert f() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.resize_stats() == stats, word
    with pytest.raises(api.QoiError):
        ctx.decode_resized(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, two, PLAIN, buf.data_ptr(), [100, 100 + 399])
    assert bool((buf == GUARD).all()) and ctx.resize_stats() == stats


def test_the_context_afterwards(ctx, mixed):
    """a plain decode_images and a decode_crops on the context that has resampled still give their exact results"""
    p = mixed
    run(ctx, p, 4, standard(BIG, 130, 70), ALPHA_WEIGHTED, staging=1)
    nbytes = [w * h * 4 for (w, h, _) in p.shapes]
    offsets = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    buf = filled(offsets[-1] + nbytes[-1] + 64, GUARD)
    ctx.decode_images(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, buf.data_ptr(), offsets)
    got = buf.cpu().numpy()
    for i, (o, n) in enumerate(zip(offsets, nbytes)):
        assert np.array_equal(got[o:o + n], p.decoded(i, 4).reshape(-1)), i
    assert np.all(got[:64] == GUARD) and np.all(got[-64:] == GUARD)
    cs = [(BIG, 3, 5, 11, 7, 3), (3, 1, 3, 35, 19, 1)]
    cb = [c[3] * c[4] * 3 for c in cs]
    buf = filled(64 + sum(cb) + 64, GUARD)
    ctx.decode_crops(p.packed.data_ptr(), p.so, p.sizes, p.descs, 3, cs, buf.data_ptr(), [64, 64 + cb[0]])
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:64 + cb[0]], crops.crop(p.decoded(BIG, 3), cs[0][1:5], 3).reshape(-1))
    assert np.array_equal(got[64 + cb[0]:64 + sum(cb)], crops.crop(p.decoded(3, 3), cs[1][1:5], 1).reshape(-1))
    assert np.all(got[:64] == GUARD) and np.all(got[-64:] == GUARD)
