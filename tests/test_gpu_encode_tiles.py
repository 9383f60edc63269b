"""qoimi_encode_tiles on the GPU (-m gpu): tiles and pyramid levels of device images as a pack.  The pixels of a tile are those of
qoi_amd/tiles.py: tile, its stream is the reference encoder's stream of them, byte for byte, and the pack is laid out by the numpy model of
tests/model_cases.py (pack_offsets) - every stream, both device tables, both host tables, the descriptors, the fill byte everywhere else."""
import ctypes

import numpy as np
import pytest

from qoi_amd import tiles
from gpu_calls import TILE_FILL as FILL, Sources, run_tiles as run, tile_model as model
from gpu_pack import dev
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets as offsets

pytestmark = pytest.mark.gpu
FACTORS = (1, 2, 3, 4, 5, 8, 13, 16, 33, 64)


@pytest.fixture(scope="module")
def small(api):
    # 1x1, 1x130, 37x29x3 at byte offset 1, 70x45x4 at byte offset 3, 128x64x4 at an aligned offset (the 16-byte paths), and an image that
    # no tile names - its descriptor is replaced by one that would be rejected
    s = Sources(api, [(1, 1, 4, 0), (1, 130, 3, 40), (37, 29, 3, 513), (70, 45, 4, 4099), (128, 64, 4, 17408), (9, 9, 4, 50300)])
    s.descs[5] = api.QoiDesc(0, 0, 9, 9)
    return s


def mixed_tiles():
    ts = [(0, 0, 0, 1, 1, 1, 0), (0, 0, 0, 1, 1, 64, 3), (1, 0, 0, 1, 130, 1, 2), (1, 0, 3, 1, 127, 5, 1), (1, 0, 0, 1, 130, 64, 0)]
    for k, f in enumerate(FACTORS):
        ts.append((2, 0, 0, 37, 29, f, k & 3))
        ts.append((2, 3, 5, 30, 20, f, (k + 1) & 3))
        ts.append((3, 0, 0, 70, 45, f, (k + 2) & 3))
        ts.append((3, 3, 5, 63, 36, f, (k + 3) & 3))
        ts.append((4, 4 * (k % 3), k, 128 - 4 * (k % 3), 64 - k, f, k & 3))
    ts += [(4, 0, 0, 128, 64, 1, 0), (4, 0, 0, 128, 64, 1, 1), (4, 8, 1, 64, 32, 1, 3), (4, 1, 0, 127, 64, 1, 0), (3, 69, 44, 1, 1, 1, 0), (2, 36, 0, 1, 29, 2, 0)]
    return ts


# ------------------------------------------------------------------ 1: byte identity
@pytest.mark.parametrize("mode", [tiles.PLAIN, tiles.ALPHA_WEIGHTED])
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_byte_identity(ctx, oracle, small, channels, mode):
    ts = mixed_tiles()
    assert 55 <= len(ts) <= 70 and not any(t[0] == 5 for t in ts)
    before = small.host.copy()
    px, streams = model(oracle, small, ts, channels, mode)
    retries = ctx.encode_retries()
    for align in (1, 64):
        run(ctx, small, ts, channels, mode, align, streams, shift=0 if align == 64 else 3)
    assert ctx.tile_stats()[3] == 5 and ctx.encode_retries() == retries
    assert np.array_equal(small.d.cpu().numpy(), before)       # the source is only read


def test_whole_image_tiles_are_encode_images(ctx, oracle, small):
    """a tile that is a whole image, factor 1, no flip, its own channel count: the stream of the image"""
    ts = [(i, 0, 0, w, h, 1, 0) for i, (w, h, ch, _) in enumerate(small.shapes[:5])]
    streams = [oracle.encode(small.img[i].reshape(-1), w, h, ch, small.descs[i].colorspace) for i, (w, h, ch, _) in enumerate(small.shapes[:5])]
    run(ctx, small, ts, 0, tiles.PLAIN, 1, streams)


# ------------------------------------------------------------------ 2: sum extremes
def test_sum_extremes(api, ctx, oracle):
    """64 x 64 blocks at factor 64: all 0xFF - the sums reach the 32-bit limit qoi_thumb_core.h documents - and alpha 0 everywhere"""
    src = Sources(api, [(64, 64, 4, 0), (64, 64, 4, 16384 + 5)])
    src.img[0][:] = 255
    src.img[1][:, :, 3] = 0
    src.d = dev(src.host)
    ts = [(0, 0, 0, 64, 64, 64, 0), (1, 0, 0, 64, 64, 64, 0), (0, 0, 0, 64, 64, 32, 3), (1, 1, 1, 63, 63, 64, 0)]
    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED):
        for channels in (0, 3):
            px, streams = model(oracle, src, ts, channels, mode)
            assert px[0].reshape(-1).tolist() == [255] * (channels or 4)
            run(ctx, src, ts, channels, mode, 1, streams)


# ------------------------------------------------------------------ 3: sub-batches
def test_sub_batches(ctx, oracle, small):
    ts = mixed_tiles()
    px, streams = model(oracle, small, ts, 0, tiles.ALPHA_WEIGHTED)
    slots, _, _, _ = tiles.plan([(w, h, ch) for (w, h, ch, _) in small.shapes], ts, 0, 0)
    mid = sum(slots[:7]) + slots[7] // 2
    results = []
    for staging in (1, mid, 0):
        _, subs, largest, referenced = tiles.plan([(w, h, ch) for (w, h, ch, _) in small.shapes], ts, 0, staging)
        results.append(run(ctx, small, ts, 0, tiles.ALPHA_WEIGHTED, 16, streams, staging=staging)[:2])
        assert ctx.tile_stats() == (len(subs), len(subs), largest, referenced) and referenced == 5, (staging, ctx.tile_stats())
        assert ctx.workspace_bytes()["encode"] >= largest
        ctx.encode_status(0)
    assert len(tiles.plan([(w, h, ch) for (w, h, ch, _) in small.shapes], ts, 0, 1)[1]) == len(ts)
    assert 1 < len(tiles.plan([(w, h, ch) for (w, h, ch, _) in small.shapes], ts, 0, mid)[1]) < len(ts)
    assert len(tiles.plan([(w, h, ch) for (w, h, ch, _) in small.shapes], ts, 0, 0)[1]) == 1
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1])


# ------------------------------------------------------------------ 4: memory contract
def test_memory_contract(ctx, oracle, small):
    ts = mixed_tiles()
    before = small.host.copy()
    px, streams = model(oracle, small, ts, 0, tiles.PLAIN)
    lens = [len(s) for s in streams]
    want_off = offsets(lens, 4)
    k = len(ts) // 2
    cap = int(want_off[k]) + lens[k] // 2                       # cuts the list in the middle: whole streams are missing, nothing is partial
    got_off, _, _ = run(ctx, small, ts, 0, tiles.PLAIN, 4, streams, capacity=cap, shift=5, staging=sum(tiles.plan(
        [(w, h, c) for (w, h, c, _) in small.shapes], ts, 0, 0)[0][:9]))
    assert int(got_off[-1]) > cap
    run(ctx, small, ts, 0, tiles.PLAIN, 4, streams, capacity=0, null_dest=True)
    run(ctx, small, ts, 0, tiles.PLAIN, 4, streams, capacity=0)
    assert np.array_equal(small.d.cpu().numpy(), before)


# ------------------------------------------------------------------ 5: serving what was ingested
@pytest.mark.parametrize("shape", [(300, 200, 3), (257, 129, 4)])
def test_pyramid_is_served_by_decode_images(api, ctx, shape):
    import torch
    w, h, ch = shape
    src = Sources(api, [(w, h, ch, 7)], seed=w)
    pyr = api.tile_pyramid(w, h, ch, 64, 48, 4)
    ts = [tiles.fields(t) for t in pyr]
    assert ts == tiles.pyramid(w, h, 64, 48, 4)
    n = len(ts)
    bound = sum(tiles.encode_bound(*tiles.size(w, h, ch, t)[1:], ch) for t in ts)
    pack = torch.full((bound,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    mode = tiles.ALPHA_WEIGHTED
    off, sizes, descs = ctx.encode_tiles(src.d.data_ptr(), src.off, src.descs, 0, pyr, mode, 1, pack.data_ptr(), bound, d_off.data_ptr(), d_len.data_ptr())
    # nothing but the call's three host tables from here on
    nbytes = [d.width * d.height * d.channels for d in descs]
    out_off = [int(v) for v in np.cumsum([0] + nbytes[:-1])]
    out = torch.full((sum(nbytes),), FILL, dtype=torch.uint8, device="cuda")
    ctx.decode_images(pack.data_ptr(), [int(o) for o in off[:n]], sizes, descs, 0, out.data_ptr(), out_off)
    got = out.cpu().numpy()
    again = np.zeros((h, w, ch), dtype=np.uint8)
    for k, (t, d) in enumerate(zip(ts, descs)):
        want = tiles.tile(src.img[0], t, 0, mode)
        g = got[out_off[k]:out_off[k] + nbytes[k]].reshape(d.height, d.width, d.channels)
        assert np.array_equal(g, want), (shape, k, t)
        if t[5] == 1:
            again[t[2]:t[2] + t[4], t[1]:t[1] + t[3]] = g
    assert np.array_equal(again, src.img[0])                   # level 0 reassembles the source
