"""qoimi_decode_resized_indexed and qoimi_pixel_stats_indexed on the GPU (-m gpu), on the pack of tests/seek_cases.py with its model index: byte
for byte qoimi_decode_resized (both modes, channels 0 / 3 / 4, flips, items in the top, middle and last band, several per image, a 3 : 1
reduction and an enlargement) and field for field qoimi_pixel_stats (with and without histograms); staging forced to several sub-batches; the
staging the inner call plans for a band at the bottom of a 256 x 2048 image is the band's; unreferenced images with garbage sizes and
descriptors; an index of another stream is accepted or rejected exactly as qoimi_band_plan says."""
import numpy as np
import pytest

from qoi_amd import crops
from qoi_amd import seekindex as si
from seek_cases import DevicePack, cases
from gpu_pack import GUARD, Batch, Pack, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pack(api, oracle):
    return DevicePack(api, cases(oracle))


def rects(p, images):
    """(image, x, y, width, height) in the top, the middle and the last band of every image, and its last pixel"""
    out = []
    for i in images:
        c = p.cases[i]
        cw, rh = min(c.w, 12), min(c.h, 3)
        out += [(i, 0, 0, cw, rh), (i, c.w - cw, c.h // 2, cw, min(rh, c.h - c.h // 2)), (i, 0, c.h - rh, cw, rh), (i, c.w - 1, c.h - 1, 1, 1)]
    return out


def items_of(p, images):
    """a 3 : 1 reduction, an enlargement with FLIP_X, one more row with FLIP_Y, a pixel blown up with both"""
    out = []
    for k, (i, x, y, cw, rh) in enumerate(rects(p, images)):
        ow, oh, flags = [(max(1, cw // 3), max(1, rh // 3), 0), (cw * 2, 5, 1), (cw, rh + 1, 2), (3, 2, 3)][k % 4]
        out.append((i, x, y, cw, rh, ow, oh, flags))
    return out


def resized_both(ctx, p, channels, items, mode, staging=0, descs=None, sizes=None, intervals=None, firsts=None):
    och = channels or p.cases[items[0][0]].ch
    nbytes = [it[5] * it[6] * och for it in items]
    offsets = [64 + int(x) + 3 * j for j, x in enumerate(np.cumsum([0] + nbytes[:-1]))]
    total = offsets[-1] + nbytes[-1] + 64
    plain, indexed = filled(total, GUARD), filled(total, GUARD)
    ctx.decode_resized(p.dev.data_ptr(), p.offsets, p.sizes, p.descs, channels, items, mode, plain.data_ptr(), offsets, staging)
    plain_stats = ctx.resize_stats()
    ctx.decode_resized_indexed(p.dev.data_ptr(), p.offsets, sizes or p.sizes, descs or p.descs, channels, items, mode, indexed.data_ptr(), offsets,
                               intervals or p.intervals, p.points, firsts or p.point_firsts, staging_bytes=staging)
    return plain.cpu().numpy(), indexed.cpu().numpy(), plain_stats, ctx.resize_stats(), offsets, nbytes


def stat_bytes(stats):
    return [bytes(s) for s in stats]


def with_ch(p, ch):
    return [i for i, c in enumerate(p.cases) if c.ch == ch]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("channels", [4, 3])
def test_resized_identical_to_decode_resized(ctx, pack, channels, mode):
    items = items_of(pack, range(len(pack.cases)))
    plain, indexed, _, _, _, _ = resized_both(ctx, pack, channels, items, mode)
    assert np.array_equal(plain, indexed), int(np.argmax(plain != indexed))
    assert not np.all(plain[64:-64] == GUARD) and ctx.seek_stats()[1] == len(pack.cases)


@pytest.mark.parametrize("och", [4, 3])
def test_resized_the_images_own_channels_and_unreferenced_garbage(api, ctx, pack, och):
    images = with_ch(pack, och)
    items = items_of(pack, images)
    descs = [d if i in images else api.QoiDesc(0, 7, 9, 3) for i, d in enumerate(pack.descs)]
    sizes = [s if i in images else 0 for i, s in enumerate(pack.sizes)]
    intervals = [k if i in images else 0 for i, k in enumerate(pack.intervals)]
    for mode in (0, 1):
        plain, indexed, _, stats, _, _ = resized_both(ctx, pack, 0, items, mode, descs=descs, sizes=sizes, intervals=intervals)
        assert np.array_equal(plain, indexed) and stats[3] == len(images) == ctx.seek_stats()[1]


@pytest.mark.parametrize("hist", [False, True])
def test_stats_identical_to_pixel_stats(api, ctx, pack, hist):
    import torch
    images = list(range(len(pack.cases)))
    regions = [r + (k % 4,) for k, r in enumerate(rects(pack, images))]
    descs = list(pack.descs)
    h1 = torch.full((len(regions), 4, 256), 7, dtype=torch.int32, device="cuda") if hist else None
    h2 = torch.full((len(regions), 4, 256), 9, dtype=torch.int32, device="cuda") if hist else None
    plain = ctx.pixel_stats(pack.dev.data_ptr(), pack.offsets, pack.sizes, descs, regions, d_hist=h1.data_ptr() if hist else 0)
    indexed = ctx.pixel_stats_indexed(pack.dev.data_ptr(), pack.offsets, pack.sizes, descs, regions, pack.intervals, pack.points, pack.point_firsts,
                                      d_hist=h2.data_ptr() if hist else 0)
    assert stat_bytes(plain) == stat_bytes(indexed) and len(indexed) == len(regions)
    assert ctx.pixel_stats_counters()[3] == len(images) == ctx.seek_stats()[1]
    c = pack.cases[regions[2][0]]                                            # `first` is pixel (0, 0) of the flipped rectangle of the FULL decode
    _, x, y, cw, rh, flags = regions[2]
    assert indexed[2].first == int(crops.crop(c.full[4], (x, y, cw, rh), flags).reshape(-1, 4)[0].view("<u4")[0])
    if hist:
        assert bool((h1 == h2).all()) and int(h2.sum()) == 4 * sum(r[3] * r[4] for r in regions)
    # unreferenced images with garbage sizes and descriptors are not looked at
    some = with_ch(pack, 3)[:3]
    regions = [r + (0,) for r in rects(pack, some)]
    bad_descs = [d if i in some else api.QoiDesc(0, 7, 9, 3) for i, d in enumerate(pack.descs)]
    bad_sizes = [s if i in some else 0 for i, s in enumerate(pack.sizes)]
    bad_ks = [k if i in some else 0 for i, k in enumerate(pack.intervals)]
    plain = ctx.pixel_stats(pack.dev.data_ptr(), pack.offsets, bad_sizes, bad_descs, regions)
    indexed = ctx.pixel_stats_indexed(pack.dev.data_ptr(), pack.offsets, bad_sizes, bad_descs, regions, bad_ks, pack.points, pack.point_firsts)
    assert stat_bytes(plain) == stat_bytes(indexed) and ctx.pixel_stats_counters()[3] == 3


def test_sub_batches_of_the_inner_call(ctx, pack):
    images = list(range(len(pack.cases)))
    items = items_of(pack, images)
    plain, indexed, plain_stats, stats, _, _ = resized_both(ctx, pack, 4, items, 1, staging=1)
    # (every image has an item in its top band: the bands start at row 0 and are the images, the plan is the plain call's)
    assert np.array_equal(plain, indexed) and stats[0] == stats[1] == len(images) == plain_stats[0] and stats[2] == plain_stats[2]
    low = [it for k, it in enumerate(items) if k % 4 >= 2]                   # the items of the last band only: the largest slot is a band's
    plain, indexed, plain_stats, stats, _, _ = resized_both(ctx, pack, 4, low, 1, staging=1)
    assert np.array_equal(plain, indexed) and stats[0] == stats[1] == len(images) == plain_stats[0] and stats[2] < plain_stats[2]
    regions = [r + (0,) for k, r in enumerate(rects(pack, images)) if k % 4 >= 2]
    a = ctx.pixel_stats(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, regions, staging_bytes=1)
    plain_counters = ctx.pixel_stats_counters()
    b = ctx.pixel_stats_indexed(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, regions, pack.intervals, pack.points, pack.point_firsts, staging_bytes=1)
    counters = ctx.pixel_stats_counters()
    assert stat_bytes(a) == stat_bytes(b) and counters[0] == counters[1] == len(images) == plain_counters[0] and counters[2] < plain_counters[2]


def test_a_band_at_the_bottom_stages_the_band(api, ctx, oracle):
    """256 x 2048, K = 128, one item in the rows 1920 to 2047: the inner call stages pad_rows + 128 rows, not 2048.  The index is built from the
    pixels the pack was encoded from."""
    w, h, K = 256, 2048, 128
    p = Pack(ctx, oracle, Batch(api, oracle, [(w, h, 4)], ["photo"]))
    points, firsts = ctx.seek_index_from_pixels(p.b.d_px.data_ptr(), p.b.pix_off, p.packed.data_ptr(), p.so, p.sizes, p.descs, [K])
    assert len(points) == 15
    region = (0, 3, 1920, 250, 128, 1)
    bands, rebased = si.bands_for_crops(p.descs, [region], [K], [points])
    assert bands == [(0, 1920, 128)]
    pad = si.pad_rows_of(points[14], w)
    want_staging = crops.plan([(w, pad + 128)], rebased, 0)[3]
    assert want_staging == (pad + 128) * w * 4 and 1 <= pad <= K
    arena = -(-si.band_info(p.sizes[0], w, h, 4, 0, K, points, 1920, 128)["size"] // 16) * 16
    item = region[:5] + (83, 43, 1)
    out1, out2 = filled(64 + 83 * 43 * 4 + 64, GUARD), filled(64 + 83 * 43 * 4 + 64, GUARD)
    ctx.decode_resized_indexed(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [item], 0, out1.data_ptr(), [64], [K], points, firsts)
    assert ctx.resize_stats() == (1, 1, want_staging, 1) and ctx.seek_stats()[1:3] == (1, arena)
    ctx.decode_resized(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [item], 0, out2.data_ptr(), [64])
    assert ctx.resize_stats()[2] == h * w * 4 and bool((out1 == out2).all())
    got = ctx.pixel_stats_indexed(p.packed.data_ptr(), p.so, p.sizes, p.descs, [region], [K], points, firsts)
    assert ctx.pixel_stats_counters() == (1, 1, want_staging, 1) and ctx.seek_stats()[1:3] == (1, arena)
    want = ctx.pixel_stats(p.packed.data_ptr(), p.so, p.sizes, p.descs, [region])
    assert ctx.pixel_stats_counters()[2] == h * w * 4 and stat_bytes(got) == stat_bytes(want)


def test_an_index_of_another_stream(api, ctx, pack):
    """the points of `cut` handed in for `noise96` and the other way round: the call is rejected where qoimi_band_plan rejects the band it
    makes, else it succeeds with some pixels; the pack stays as it is, nothing beside the outputs is written, the context goes on working"""
    names = [c.name for c in pack.cases]
    i, j = names.index("noise96"), names.index("cut")
    swapped = list(pack.point_firsts)
    swapped[i], swapped[j] = pack.point_firsts[j], pack.point_firsts[i]
    items = [(i, 0, 60, 96, 10, 32, 5, 0), (j, 0, 90, 96, 6, 96, 6, 0)]

    def accepted(item):
        image, _, y, _, rh = item[:5]
        K = pack.intervals[image]
        first = y // K * K
        return api.band_plan(pack.descs[image], pack.sizes[image], K, pack.points[swapped[image]:], first, y + rh - first) is not None

    want_ok = all(accepted(it) for it in items)
    nbytes = [it[5] * it[6] * 4 for it in items]
    offsets = [64, 64 + nbytes[0] + 1]
    out = filled(offsets[1] + nbytes[1] + 64, GUARD)
    try:
        ctx.decode_resized_indexed(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, 4, items, 0, out.data_ptr(), offsets, pack.intervals, pack.points, swapped)
        ok = True
    except api.QoiError:
        ok = False
        assert bool((out == GUARD).all())
    assert ok == want_ok
    got = out.cpu().numpy()
    mask = np.ones(got.size, dtype=bool)
    for o, nb in zip(offsets, nbytes):
        mask[o:o + nb] = False
    assert np.all(got[mask] == GUARD)
    regions = [it[:5] + (0,) for it in items]
    try:
        ctx.pixel_stats_indexed(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, regions, pack.intervals, pack.points, swapped)
        ok = True
    except api.QoiError:
        ok = False
    assert ok == want_ok and np.array_equal(pack.dev.cpu().numpy(), pack.host)
    plain, indexed, _, _, _, _ = resized_both(ctx, pack, 4, items, 0)
    assert np.array_equal(plain, indexed)
