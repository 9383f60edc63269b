"""qoimi_decode_bilinear and qoimi_decode_bilinear_indexed on the GPU (-m gpu): rectangles of a pack's images resampled by the antialiased
bilinear filter through bounded staging.  The expectation is always the definition: the oracle decodes the stream at the call's output channel
count, and qoi_amd/bilinear.py: bilinear resamples that.  Every comparison is exact and covers the whole output.  Outputs stand behind,
between and in front of guard bytes (0xA5); every guard byte is checked after every call.  Sub-batch boundaries are forced through
staging_bytes by qoi_amd/bilinear.py: plan (qoimi_bilinear_stats says that the call really ran that many sub-batches over that much staging)."""
import ctypes

import numpy as np
import pytest

from qoi_amd import bilinear, crops
from qoi_amd.bilinear import ALPHA_WEIGHTED, PLAIN
from qoi_amd.packplan import slot
from gpu_calls import sizes_of
from gpu_pack import E_ARG, GUARD, KINDS, MIXED_SHAPES, Batch, Pack, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BIG = 7                               # 130 x 70 x 4, sprite_alpha


@pytest.fixture(scope="module")
def mixed(api, ctx, oracle):
    """the mixed pack of tests/test_gpu_resize.py: shapes from 1 x 1 and 1 x 97 to 130 x 70, 3 and 4 channels, all content classes"""
    kinds = [KINDS[(i + 2) % 5] for i in range(len(MIXED_SHAPES))]
    assert set(kinds) == set(KINDS) and MIXED_SHAPES[BIG] == (130, 70, 4)
    return Pack(ctx, oracle, Batch(api, oracle, MIXED_SHAPES, kinds))


@pytest.fixture(scope="module")
def equal(api, ctx, oracle):
    return Pack(ctx, oracle, Batch(api, oracle, [(64, 48, 4)] * 7, [KINDS[i % 5] for i in range(7)]))


def standard(i, w, h, first_flag=0):
    """identity; the whole image to ceil(w/32) x ceil(h/32) - the cap; a non-integer reduction (130 x 70 -> 37 x 23, smaller images in that
    proportion); an interior rectangle with odd origin and odd size to an odd size; an enlargement of a 1 x 1 and of a (up to) 5 x 3
    rectangle; down in x with up in y; the flag values take turns"""
    out = [(0, 0, w, h, w, h), (0, 0, w, h, -(-w // 32), -(-h // 32)), (0, 0, w, h, max(1, w * 37 // 130), max(1, h * 23 // 70))]
    if w >= 3 and h >= 4:
        out.append((1, 3, min(223, w - 1 if (w - 1) % 2 else w - 2), min(159, h - 3 if (h - 3) % 2 else h - 4), 7, 5))   # (at most 32 to 1)
    out.append((w - 1, h - 1, 1, 1, 4, 3))
    out.append((w // 3, h // 3, min(5, w - w // 3), min(3, h - h // 3), 13, 7))
    out.append((0, 0, w, min(h, 3), max(1, w // 3), 8))
    return [(i, x, y, cw, rh, ow, oh, (first_flag + k) & 3) for k, (x, y, cw, rh, ow, oh) in enumerate(out)]


def run(ctx, p, channels, items, mode=PLAIN, staging=0, offsets=None, total=None, front=64, call=None):
    """One call; outputs back to back behind `front` guard bytes unless offsets are given.  Returns the outputs."""
    och = channels or p.shapes[items[0][0]][2]
    nbytes = sizes_of(items, och)
    if offsets is None:
        offsets = [front + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    if total is None:
        total = max(o + n for o, n in zip(offsets, nbytes)) + 64
    buf = filled(total, GUARD)
    if call is None:
        ctx.decode_bilinear(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, buf.data_ptr(), offsets, staging)
    else:
        call(buf.data_ptr(), offsets)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)]


def want(p, it, och, mode):
    i, x, y, cw, rh, ow, oh, flags = it
    return bilinear.bilinear(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, mode).reshape(-1)


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
    assert {it[7] for it in items} == {0, 1, 2, 3} and (BIG, 0, 0, 130, 70, 37, 23, 1) in items and (5, 0, 0, 64, 48, 2, 2, 2) in items
    assert any(it[1] % 2 and it[2] % 2 and it[3] % 2 and it[4] % 2 and it[5] % 2 and it[6] % 2 for it in items)
    assert any(it[3] > it[5] and it[4] < it[6] for it in items)                                       # down in x with up in y
    assert {bilinear.split(it[3], it[5])[0] for it in items} == {0, 1, 2, 3, 4}                       # every number of lanes per pixel
    got = run(ctx, p, channels, items, mode)
    assert_items(p, got, items, channels, mode, (channels, mode))
    assert ctx.bilinear_stats()[:2] == (1, 1) and ctx.bilinear_stats()[3] == p.n
    if channels == 4 and mode == ALPHA_WEIGHTED:
        assert any(not np.array_equal(want(p, it, 4, PLAIN), want(p, it, 4, ALPHA_WEIGHTED)) for it in items)


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
    stats = ctx.bilinear_stats()
    assert stats[3] == len(images)
    other = [i for i, s in enumerate(p.shapes) if s[2] != och][0]
    buf = filled(4096, GUARD)
    with pytest.raises(api.QoiError):
        ctx.decode_bilinear(p.packed.data_ptr(), p.so, p.sizes, p.descs, 0, [(images[0], 0, 0, 1, 1, 2, 2, 0), (other, 0, 0, 1, 1, 2, 2, 0)], PLAIN, buf.data_ptr(), [64, 128])
    assert "channel" in api.last_error() and bool((buf == GUARD).all()) and ctx.bilinear_stats() == stats


# ------------------------------------------------------------------ 2: placement
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


# ------------------------------------------------------------------ 3: every lane-split regime in one call
REGIMES = [
    (0, 0, 0, 1, 1, 4, 4, 0),             # L = 1, enlarging: one source pixel
    (2, 5, 0, 3, 1, 2, 1, 1),             # L = 1: 3 x 1 -> 2 x 1
    (0, 0, 0, 1, 1, 1, 1, 2),             # one work item ...
    (3, 0, 0, 37, 23, 80, 50, 3),         # ... next to 4000 of one lane, 16 tiles: the rectangle touches all four borders
    (BIG, 3, 5, 99, 60, 33, 20, 0),       # L = 2: ratio 3; the rectangle touches no border
    (6, 1, 1, 331, 5, 47, 1, 1),          # L = 4: ratio about 7
    (4, 0, 0, 257, 9, 17, 2, 2),          # L = 8: ratio about 15
    (BIG, 1, 3, 128, 64, 4, 2, 3),        # L = 16: the ratio of exactly 32 in both axes
    (BIG, 0, 0, 130, 70, 130, 70, 0),     # the identity: 9100 work items
]


@pytest.mark.parametrize("channels,mode,shift", [(4, ALPHA_WEIGHTED, 0), (3, PLAIN, 7), (4, PLAIN, 1)])
def test_every_regime_in_one_call(ctx, mixed, channels, mode, shift):
    p = mixed
    assert [bilinear.split(it[3], it[5])[0] for it in REGIMES] == [0, 0, 0, 0, 1, 2, 3, 4, 0]
    assert bilinear.taps(128, 4) == 64 and bilinear.tiles(1, 1, 1) == 1 and bilinear.tiles(37, 80, 50) == 16
    got = run(ctx, p, channels, REGIMES, mode, front=64 + shift)
    assert_items(p, got, REGIMES, channels, mode, (channels, mode, shift))
    assert ctx.bilinear_stats()[:2] == (1, 1)
    # enlarging is smooth where the area filter repeats pixels: the 80 x 50 enlargement has more distinct rows than its source
    assert len(np.unique(got[3].reshape(50, -1), axis=0)) > 23


# ------------------------------------------------------------------ 4: agreement with qoimi_decode_crops on the device
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


# ------------------------------------------------------------------ 5: sub-batches
def test_sub_batches(api, mixed, equal):
    c = api.Context(0)
    try:
        p = equal
        items = [x for i in range(6) for x in standard(i, 64, 48, i)]                # image 6 has no item
        one = slot(64 * 48 * 4)
        single = run(c, p, 4, items, ALPHA_WEIGHTED)
        assert c.bilinear_stats() == (1, 1, 6 * one, 6)
        assert_items(p, single, items, 4, ALPHA_WEIGHTED, "single")
        for staging, subs, per in ((1, 6, 1), (2 * one, 3, 2), (3 * one + 255, 2, 3), (0, 1, 6)):
            images, slots, the_plan, largest = bilinear.plan(p.descs, items, staging)
            assert images == list(range(6)) and len(the_plan) == subs and all(count == per for _, count in the_plan) and largest == per * one
            got = run(c, p, 4, items, ALPHA_WEIGHTED, staging=staging)
            assert c.bilinear_stats() == (subs, subs, largest, 6), (staging, c.bilinear_stats())
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        p = mixed                                                                     # items in any order of image
        items = [x for i in (5, 0, 7, 2, 6, 1, 4, 3) for x in standard(i, p.shapes[i][0], p.shapes[i][1], i)]
        single = run(c, p, 3, items)
        assert_items(p, single, items, 3, PLAIN, "mixed single")
        for staging in (1, 13000):
            images, slots, the_plan, largest = bilinear.plan(p.descs, items, staging)
            got = run(c, p, 3, items, staging=staging)
            assert c.bilinear_stats() == (len(the_plan), len(the_plan), largest, 8), (staging, c.bilinear_stats(), the_plan)
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        assert len(bilinear.plan(p.descs, items, 1)[2]) == 8 and 2 <= len(bilinear.plan(p.descs, items, 13000)[2]) < 8
    finally:
        c.close()


# ------------------------------------------------------------------ 6: through a seek index
def test_indexed_equals_the_plain_call(ctx, equal):
    """an index from qoimi_build_seek_index at 8 rows per interval; items in the top, a middle and the last band, several per image; image 6
    has none.  qoimi_seek_stats [1..3] are what qoimi_decode_resized_indexed leaves for the same items."""
    p = equal
    K = 8
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, K)
    rects = [(0, 0, 1, 64, 5), (0, 10, 19, 40, 22), (1, 3, 41, 33, 7), (2, 0, 30, 64, 18), (3, 63, 47, 1, 1), (4, 5, 17, 12, 3), (5, 0, 24, 64, 24), (5, 7, 40, 9, 8)]
    outs = [(13, 2, 0), (90, 50, 1), (2, 7, 2), (2, 1, 3), (3, 2, 0), (12, 3, 1), (33, 5, 2), (20, 20, 3)]
    items = [r + o for r, o in zip(rects, outs)]
    for channels, mode, staging in ((4, ALPHA_WEIGHTED, 0), (3, PLAIN, 1), (0, PLAIN, 0)):
        plain = run(ctx, p, channels, items, mode, staging=staging)
        plain_stats = ctx.bilinear_stats()
        indexed = run(ctx, p, channels, items, mode, call=lambda out, offsets: ctx.decode_bilinear_indexed(
            p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, out, offsets, [K] * p.n, points, firsts, staging_bytes=staging))
        stats, seek = ctx.bilinear_stats(), ctx.seek_stats()
        assert all(np.array_equal(a, b) for a, b in zip(plain, indexed)), (channels, mode)
        assert_items(p, indexed, items, channels or 4, mode, ("indexed", channels))
        assert stats[:2] == plain_stats[:2] and stats[3] == 6 and stats[2] <= plain_stats[2]                     # (a band is no longer than its image)
        assert staging != 0 or stats[2] < plain_stats[2]
        run(ctx, p, channels, items, mode, call=lambda out, offsets: ctx.decode_resized_indexed(
            p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, out, offsets, [K] * p.n, points, firsts, staging_bytes=staging))
        assert seek[1] == 6 and seek[2] > 0 and seek[1:] == ctx.seek_stats()[1:]


# ------------------------------------------------------------------ 7: 64-bit sums and weights past 2**31 on the device
def test_sums_past_32_bits(api, ctx, oracle):
    """one 1024 x 768 photograph to 224 x 224 x 3: D is about 5e7 and N_c passes 2**32"""
    p = Pack(ctx, oracle, Batch(api, oracle, [(1024, 768, 3)], ["photo"]))
    item = (0, 0, 0, 1024, 768, 224, 224, 0)
    D = bilinear.weights(768, 224).sum(axis=1)[:, None] * bilinear.weights(1024, 224).sum(axis=1)[None, :]
    w = want(p, item, 3, PLAIN)
    least = int(((w.reshape(224, 224, 3).astype(np.int64) - 1) * D[:, :, None]).max())       # N_c >= (value - 1/2) * D
    print("D from %d to %d; the largest N_c at least %d" % (D.min(), D.max(), least))
    assert 3e7 < D.min() and 4e7 < D.max() < 6e7 and least >= 2 ** 32
    assert bilinear.split(1024, 224) == (2, 3)
    for channels, mode, shift in ((3, PLAIN, 1), (4, ALPHA_WEIGHTED, 0)):
        got = run(ctx, p, channels, [item], mode, front=64 + shift)
        assert_items(p, got, [item], channels, mode, ("photo", channels))


def test_weights_past_2_31(api, ctx, oracle):
    """24000 x 1 at 3 channels to 750 x 24000: 54 MB of output, the ratio of exactly 32 in x with sixteen lanes, an enlargement by 24000 in
    y; ty * tx reaches about 2.3e9, between 2**31 and 2**32.  Compared whole."""
    p = Pack(ctx, oracle, Batch(api, oracle, [(24000, 1, 3)], ["noise"]))
    item = (0, 0, 0, 24000, 1, 750, 24000, 0)
    largest = int(bilinear.weights(24000, 750).max()) * int(bilinear.weights(1, 24000).max())
    print("largest ty * tx %d" % largest)
    assert 2 ** 31 < largest < 2 ** 32 and bilinear.split(24000, 750) == (4, 4) and bilinear.size(24000, 1, item[1:5], item[5:7], 0, 3) == 54000000
    got = run(ctx, p, 3, [item], PLAIN, front=64 + 1)
    w = want(p, item, 3, PLAIN)
    assert got[0].size == w.size and np.array_equal(got[0], w), int(np.argmax(got[0] != w))
    assert ctx.bilinear_stats() == (1, 1, slot(24000 * 4), 1)


# ------------------------------------------------------------------ 8: rejections on a live context, and the context afterwards
def test_rejections_on_a_live_context(api, ctx, mixed):
    p = mixed
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)

    def call(items, offsets, channels=4, mode=0):
        arr = (api.QoimiResize * len(items))(*[api.QoimiResize(*it) for it in items])
        return lib.qoimi_decode_bilinear(ctx._h, *args, channels, arr, len(items), mode, buf.data_ptr(), (ctypes.c_size_t * len(items))(*offsets), 0, None)

    two = [(BIG, 0, 0, 100, 60, 10, 10, 0), (5, 0, 0, 8, 8, 8, 8, 1)]
    assert call(two, [100, 100 + 400]) == 0                                           # side by side: accepted
    got = buf.cpu().numpy()
    assert np.array_equal(got[100:500], want(p, two[0], 4, PLAIN)) and np.array_equal(got[500:756], want(p, two[1], 4, PLAIN))
    assert np.all(got[:100] == GUARD) and np.all(got[756:] == GUARD)
    stats = ctx.bilinear_stats()
    assert stats == (1, 1, slot(130 * 60 * 4) + slot(64 * 8 * 4), 2)
    buf.fill_(GUARD)
    rejected = [
        (lambda: call(two, [100, 100 + 399]), "overlap"), (lambda: call(two, [100 + 255, 100]), "overlap"),
        (lambda: call([(BIG, 0, 0, 130, 1, 4, 1, 0)], [64]), "32"), (lambda: call([(BIG, 0, 0, 1, 33, 1, 1, 0)], [64]), "32"),
        (lambda: call([(BIG, 0, 0, 1, 1, 32768, 32768, 0)], [64]), "2^30"), (lambda: call([(BIG, 0, 0, 130, 1, 1 << 23, 128, 0)], [64]), "2^30"),
        (lambda: call([(BIG, 121, 0, 10, 10, 10, 10, 0)], [64]), "leaves"), (lambda: call([(BIG, 0, 61, 10, 10, 10, 10, 0)], [64]), "leaves"),
        (lambda: call([(BIG, 0, 0, 10, 10, 10, 10, 4)], [64]), "flag"), (lambda: call(two, [100, 600], mode=2), "mode"), (lambda: call(two, [100, 600], mode=-1), "mode"),
        (lambda: call([(2, 0, 0, 1, 1, 1, 1, 0), (BIG, 0, 0, 1, 1, 1, 1, 0)], [64, 128], channels=0), "channel"),
    ]
    for f, word in rejected:
        assert f() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.bilinear_stats() == stats, word
    with pytest.raises(api.QoiError):
        ctx.decode_bilinear(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, two, PLAIN, buf.data_ptr(), [100, 100 + 399])
    assert bool((buf == GUARD).all()) and ctx.bilinear_stats() == stats
    # the context works afterwards: the same call, a decode_images and a decode_crops give their exact results
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
