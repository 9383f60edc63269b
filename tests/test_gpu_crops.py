"""qoimi_decode_crops on the GPU (-m gpu): rectangles of a pack's images through bounded staging.  The expectation is always the definition:
the oracle decodes the stream as it is given (whole, cut, with a foreign end marker) at the call's output channel count, and
qoi_amd/crops.py: crop cuts that.  Every comparison is exact.  Outputs stand behind, between and in front of guard bytes (0xA5); every guard
byte is checked after every call.  Sub-batch boundaries are forced through staging_bytes by qoi_amd/crops.py: plan (qoimi_crop_stats says that
the call really ran that many sub-batches over that much staging)."""
import ctypes
import os

import numpy as np
import pytest

from qoi_amd import crops
from qoi_amd.packplan import slot
from gpu_calls import standard_crops as standard
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


def sizes_of(cs, och):
    return [c[3] * c[4] * och for c in cs]


def run(ctx, p, channels, cs, staging=0, offsets=None, total=None, sizes=None, packed=None, front=64):
    """One call; outputs back to back behind `front` guard bytes unless offsets are given.  Returns the outputs."""
    och = channels or p.shapes[cs[0][0]][2]
    nbytes = sizes_of(cs, och)
    if offsets is None:
        offsets = [front + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    if total is None:
        total = max(o + n for o, n in zip(offsets, nbytes)) + 64
    buf = filled(total, GUARD)
    ctx.decode_crops((p.packed if packed is None else packed).data_ptr(), p.so, p.sizes if sizes is None else sizes, p.descs, channels, cs,
                     buf.data_ptr(), offsets, staging)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)]


def want(p, c, och, **how):
    i, x, y, cw, ch, flags = c
    return crops.crop(p.decoded(i, och, **how), (x, y, cw, ch), flags).reshape(-1)


def assert_crops(p, got, cs, och, what):
    for j, c in enumerate(cs):
        w = want(p, c, och)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, c, int(np.argmax(got[j] != w)))


# ------------------------------------------------------------------ 1: the mixed pack
@pytest.mark.parametrize("channels", [4, 3])
def test_mixed_pack(ctx, mixed, channels):
    p = mixed
    cs = [c for i, (w, h, _) in enumerate(p.shapes) for c in standard(i, w, h, i)]
    assert {c[5] for c in cs} == {0, 1, 2, 3} and any(c[1] % 2 and c[2] % 2 and c[3] % 2 and c[4] % 2 for c in cs)
    got = run(ctx, p, channels, cs)
    assert_crops(p, got, cs, channels, channels)
    assert ctx.crop_stats()[:2] == (1, 1) and ctx.crop_stats()[3] == p.n


@pytest.mark.parametrize("och", [4, 3])
def test_the_images_own_channels(ctx, mixed, och):
    """channels 0: the referenced images share a channel count, the others of the pack need not"""
    p = mixed
    images = [i for i, s in enumerate(p.shapes) if s[2] == och]
    assert 3 <= len(images) < p.n
    cs = [c for i in images for c in standard(i, p.shapes[i][0], p.shapes[i][1], i + 1)]
    got = run(ctx, p, 0, cs)
    assert [g.size for g in got] == sizes_of(cs, och)
    assert_crops(p, got, cs, och, ("own", och))
    assert ctx.crop_stats()[3] == len(images)


# ------------------------------------------------------------------ 2: every alignment, neighbours sharing aligned words
@pytest.mark.parametrize("channels", [3, 4])
def test_output_alignment(ctx, mixed, channels):
    p = mixed
    # 1, 2, 5 and 6 pixels (3 to 18 bytes at 3 channels: crops inside one word, crops that straddle one), rows, columns, rectangles
    cs = [(3, 4, 5, 1, 1, 0), (3, 7, 2, 2, 1, 1), (5, 9, 9, 5, 1, 2), (3, 30, 3, 1, 6, 3), (5, 1, 1, 3, 2, 1), (BIG, 17, 11, 1, 1, 0), (BIG, 3, 5, 11, 7, 3),
          (4, 250, 0, 7, 9, 2), (0, 0, 0, 1, 1, 1), (1, 0, 90, 1, 7, 2), (2, 120, 0, 11, 1, 1), (6, 1, 1, 331, 5, 3), (3, 0, 0, 2, 1, 0), (3, 36, 22, 1, 1, 0)]
    for shift in (0, 1, 3, 5, 15):
        got = run(ctx, p, channels, cs, front=64 + shift)
        assert_crops(p, got, cs, channels, (channels, shift))


# ------------------------------------------------------------------ 3: order
def test_order(ctx, mixed):
    """output offsets descend while the crop order ascends; the crops are not sorted by image"""
    p = mixed
    cs = [(5, 3, 3, 31, 17, 1), (BIG, 1, 1, 99, 33, 2), (0, 0, 0, 1, 1, 0), (5, 0, 40, 64, 8, 3), (2, 7, 0, 101, 1, 1), (BIG, 100, 60, 30, 10, 0), (1, 0, 5, 1, 77, 2)]
    for channels in (4, 3):
        nbytes = sizes_of(cs, channels)
        offsets, pos = [0] * len(cs), 33
        for j in reversed(range(len(cs))):
            offsets[j] = pos
            pos += nbytes[j] + (6, 1, 3, 0)[j % 4]
        assert all(offsets[j] > offsets[j + 1] for j in range(len(cs) - 1))
        got = run(ctx, p, channels, cs, offsets=offsets, total=pos + 77)
        assert_crops(p, got, cs, channels, ("order", channels))


# ------------------------------------------------------------------ 4: many crops of one image
@pytest.mark.parametrize("channels", [4, 3])
def test_tiles_of_one_image_reassemble(ctx, mixed, channels):
    from tools.qoitile_mi355x import tile_grid
    p = mixed
    grid = tile_grid(130, 70, 32)
    assert len(grid) == 15
    cs = [(BIG, x, y, tw, th, 0) for (_, _, x, y, tw, th) in grid]
    got = run(ctx, p, channels, cs)
    whole = np.zeros((70, 130, channels), dtype=np.uint8)
    for g, (_, _, x, y, tw, th) in zip(got, grid):
        whole[y:y + th, x:x + tw] = g.reshape(th, tw, channels)
    assert np.array_equal(whole, p.decoded(BIG, channels))
    assert ctx.crop_stats() == (1, 1, slot(130 * 70 * 4), 1)


# ------------------------------------------------------------------ 5: more than one tile, stepping from crop to crop
def test_large_crops_between_small_ones(ctx, mixed):
    p = mixed
    for channels, big in ((4, (BIG, 0, 0, 130, 70, 1)), (3, (4, 0, 0, 257, 9, 2))):
        assert big[3] * big[4] * channels > 4096
        cs = [(0, 0, 0, 1, 1, 0), (3, 5, 5, 1, 1, 0), big, (3, 36, 22, 1, 1, 0), (BIG, 129, 69, 1, 1, 3), big[:5] + (3,), (0, 0, 0, 1, 1, 2)]
        for shift in (0, 7):
            got = run(ctx, p, channels, cs, front=64 + shift)
            assert_crops(p, got, cs, channels, ("large", channels, shift))


def test_tile_walk_regimes(api, ctx, oracle, mixed):
    """(qoi_dev.h: walk_tiles) a launch with ONE table entry, its 9 tiles spread over as many workgroups; and more tiles than the grid's clamp
    of 8 workgroups per compute unit - 37 more crops of one tile each - so that a workgroup takes two tiles and steps from crop to crop.
    The 3-byte outputs stand back to back: neighbours share aligned words."""
    import torch
    one = (BIG, 0, 0, 130, 70, 3)
    assert -(-len(crops.items(64, 130 * 70 * 4)) // 256) == 9                        # (run: 64 bytes behind an aligned buffer)
    assert_crops(mixed, run(ctx, mixed, 4, [one]), [one], 4, "one entry")
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    p = Pack(ctx, oracle, Batch(api, oracle, [(8, 8, 4)], ["noise"]))
    cs = [(0, j % 8, (j // 8) % 8, 1, 1, j & 3) for j in range(n)]
    for channels in (3, 4):
        assert_crops(p, run(ctx, p, channels, cs, front=64 + 5), cs, channels, ("many", channels))
        assert ctx.crop_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 6: sub-batches
def test_sub_batches(api, mixed, equal):
    c = api.Context(0)
    try:
        p = equal
        cs = [x for i in range(6) for x in standard(i, 64, 48, i)]                   # image 6 has no crop
        one = slot(64 * 48 * 4)
        single = run(c, p, 4, cs)
        assert c.crop_stats() == (1, 1, 6 * one, 6)
        assert_crops(p, single, cs, 4, "single")
        for staging, subs, per in ((1, 6, 1), (one, 6, 1), (2 * one, 3, 2), (3 * one + 255, 2, 3)):
            images, slots, the_plan, largest = crops.plan(p.descs, cs, staging)
            assert images == list(range(6)) and len(the_plan) == subs and all(count == per for _, count in the_plan) and largest == per * one
            got = run(c, p, 4, cs, staging=staging)
            assert c.crop_stats() == (subs, subs, largest, 6), (staging, c.crop_stats())
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        # the mixed pack, crops in any order of image, two to three images per sub-batch
        p = mixed
        cs = [x for i in (5, 0, 7, 2, 6, 1, 4, 3) for x in standard(i, p.shapes[i][0], p.shapes[i][1], i)]
        single = run(c, p, 3, cs)
        assert_crops(p, single, cs, 3, "mixed single")
        for staging in (1, 13000, 40000):
            images, slots, the_plan, largest = crops.plan(p.descs, cs, staging)
            got = run(c, p, 3, cs, staging=staging)
            assert c.crop_stats() == (len(the_plan), len(the_plan), largest, 8), (staging, c.crop_stats(), the_plan)
            assert all(np.array_equal(x, y) for x, y in zip(got, single)), staging
        assert len(crops.plan(p.descs, cs, 1)[2]) == 8 and 2 <= len(crops.plan(p.descs, cs, 13000)[2]) < 8
    finally:
        c.close()


# ------------------------------------------------------------------ 7: unreferenced images
def test_unreferenced_images_are_not_looked_at(ctx, mixed):
    p = mixed
    sizes = list(p.sizes)
    sizes[1] = sizes[4] = 0
    cs = [x for i in (0, 2, 3, 5, 6, 7) for x in standard(i, p.shapes[i][0], p.shapes[i][1], i)]
    got = run(ctx, p, 4, cs, sizes=sizes)
    assert_crops(p, got, cs, 4, "unreferenced")
    assert ctx.crop_stats()[3] == 6


# ------------------------------------------------------------------ 8: only the rows a crop needs are staged
def test_row_shortening(ctx, mixed):
    p = mixed
    cs = [(BIG, 0, 0, 130, 1, 0), (BIG, 5, 1, 121, 2, 1), (BIG, 129, 2, 1, 1, 2), (BIG, 0, 0, 130, 3, 3)]
    assert crops.rows_needed(p.descs, cs) == {BIG: 3}
    for channels in (4, 3):
        got = run(ctx, p, channels, cs)
        assert_crops(p, got, cs, channels, ("rows", channels))
        assert ctx.crop_stats() == (1, 1, slot(130 * 3 * 4), 1)
    # every number of rows of a small image: the decode down to row r is the prefix of the full decode
    w, h, _ = p.shapes[3]
    for r in range(1, h + 1):
        got = run(ctx, p, 3, [(3, 0, r - 1, w, 1, 0), (3, 0, 0, w, r, 0)])
        assert np.array_equal(got[1].reshape(r, w, 3), p.decoded(3, 3)[:r]), r
        assert ctx.crop_stats()[2] == slot(w * r * 4)


# ------------------------------------------------------------------ 9: leniency
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
    cs = [(cut, 3, 31, 55, 17, 1), (cut, 0, 0, 64, 48, 0), (marker, 1, 12, 35, 11, 2), (marker, 0, 0, 37, 23, 3), (BIG, 0, 35, 130, 35, 0)]
    for channels in (4, 3):
        got = run(ctx, p, channels, cs, sizes=sizes, packed=damaged)
        for j, c in enumerate(cs):
            how = {"size": sizes[cut]} if c[0] == cut else {"host": host} if c[0] == marker else {}
            assert np.array_equal(got[j], want(p, c, channels, **how)), (channels, j)
    assert np.array_equal(damaged.cpu().numpy(), host)


# ------------------------------------------------------------------ 10: rejections on a live context
def test_rejections_on_a_live_context(api, ctx, mixed):
    p = mixed
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)

    def call(cs, offsets, channels=4):
        arr = (api.QoimiCrop * len(cs))(*[api.QoimiCrop(*c) for c in cs])
        return lib.qoimi_decode_crops(ctx._h, *args, channels, arr, len(cs), buf.data_ptr(), (ctypes.c_size_t * len(cs))(*offsets), 0, None)

    two = [(BIG, 0, 0, 10, 10, 0), (5, 0, 0, 8, 8, 1)]
    assert call(two, [100, 100 + 399]) == E_ARG and "overlap" in api.last_error()
    assert call(two, [100 + 255, 100]) == E_ARG and "overlap" in api.last_error()
    assert call([(BIG, 121, 0, 10, 10, 0)], [64]) == E_ARG and "leaves" in api.last_error()
    assert call([(BIG, 0, 61, 10, 10, 0)], [64]) == E_ARG
    assert call([(2, 0, 0, 1, 1, 0), (BIG, 0, 0, 1, 1, 0)], [64, 128], channels=0) == E_ARG and "channel" in api.last_error()
    with pytest.raises(api.QoiError):
        ctx.decode_crops(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, two, buf.data_ptr(), [100, 100 + 399])
    assert bool((buf == GUARD).all())
    assert call(two, [100, 100 + 400]) == 0                                           # side by side: accepted
    got = buf.cpu().numpy()
    assert np.array_equal(got[100:500], want(p, two[0], 4)) and np.array_equal(got[500:756], want(p, two[1], 4))
    assert np.all(got[:100] == GUARD) and np.all(got[756:] == GUARD)


# ------------------------------------------------------------------ 11: the tool
def test_tool(api, oracle, tmp_path):
    from qoi_amd import synth
    from tools import qoitile_mi355x
    for name, px, ch in (("rgba", synth.frame_rgba("sprite_alpha", 70, 50, 0), 4), ("rgb", synth.frame_rgb("photo", 70, 50, 1), 3)):
        src = tmp_path / (name + ".qoi")
        assert api.qoi_write(str(src), px.reshape(-1), api.QoiDesc(70, 50, ch, 0)) > 0
        decoded, _ = oracle.decode(src.read_bytes(), ch)
        decoded = decoded.reshape(50, 70, ch)
        out_dir = tmp_path / name
        lines = []
        assert qoitile_mi355x.main([str(src), "--tile", "32", "-o", str(out_dir)], out=lines.append) == 0
        grid = qoitile_mi355x.tile_grid(70, 50, 32)
        assert sorted(os.listdir(out_dir)) == sorted(f"tile_{r}_{c}.qoi" for (r, c, _, _, _, _) in grid) and len(grid) == 6
        for (r, c, x, y, tw, th) in grid:
            tile, desc = oracle.decode((out_dir / f"tile_{r}_{c}.qoi").read_bytes(), ch)
            assert tile is not None and (desc.width, desc.height, desc.channels) == (tw, th, ch)
            assert np.array_equal(tile.reshape(th, tw, ch), decoded[y:y + th, x:x + tw]), (name, r, c)
        assert any("6 tiles" in l for l in lines)
    (tmp_path / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)
    assert qoitile_mi355x.main([str(tmp_path / "junk.qoi"), "--tile", "32", "-o", str(tmp_path / "junk")], out=lambda s: None) == 1
