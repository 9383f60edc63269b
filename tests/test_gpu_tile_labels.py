"""qoimi_encode_tiles in QOIMI_TILE_NEAREST / QOIMI_TILE_MODE on the GPU (-m gpu): the kernel tile_select.  The harness is that of
tests/test_gpu_encode_tiles.py - sources at odd byte offsets, a guarded region, the reference encoder's streams of the model's pixels
(qoi_amd/tiles.py: tile) byte for byte, both device tables, both host tables, the descriptors, the fill byte everywhere else - over label
images (tests/labelimg.py), whose blocks hold unique winners, ties the centre wins and ties the lowest key decides."""
import numpy as np
import pytest

from labelimg import label_image, loop
from qoi_amd import tensors, tiles
from gpu_calls import TILE_FILL, Sources, run_tiles, tile_model
from gpu_pack import dev
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets

pytestmark = pytest.mark.gpu
FILL = TILE_FILL
FACTORS = {tiles.NEAREST: (1, 2, 3, 4, 5, 8, 13, 16, 33, 64), tiles.MODE: (1, 2, 3, 4, 5, 8, 13, 16)}
MODES = (tiles.NEAREST, tiles.MODE)


def label_sources(api, shapes, seed=11, cell=5, noise=True):
    """Sources whose images are label images; the buffer between them keeps its random bytes"""
    s = Sources(api, shapes, seed)
    for i, (w, h, ch, _) in enumerate(shapes):
        s.img[i][:] = label_image(w, h, ch, seed + i, cell, noise)
    s.d = dev(s.host)
    assert s.d.data_ptr() % 256 == 0
    return s


@pytest.fixture(scope="module")
def small(api):
    # 1x1, 1x130, 37x29x3 at byte offset 1, 70x45x4 at byte offset 3, 128x64x4 at an aligned offset (the 16-byte loads of the copy)
    return label_sources(api, [(1, 1, 4, 0), (1, 130, 3, 40), (37, 29, 3, 513), (70, 45, 4, 4099), (128, 64, 4, 17408)])


def mixed_tiles(mode):
    """every factor of the mode - entries of every lg - in one table, all four flips, rectangles at odd corners"""
    top = FACTORS[mode][-1]
    ts = [(0, 0, 0, 1, 1, 1, 0), (0, 0, 0, 1, 1, top, 3), (1, 0, 0, 1, 130, 1, 2), (1, 0, 3, 1, 127, 5, 1), (1, 0, 0, 1, 130, top, 0)]
    for k, f in enumerate(FACTORS[mode]):
        ts.append((2, 0, 0, 37, 29, f, k & 3))
        ts.append((2, 3, 5, 30, 20, f, (k + 1) & 3))
        ts.append((3, 0, 0, 70, 45, f, (k + 2) & 3))
        ts.append((3, 3, 5, 63, 36, f, (k + 3) & 3))
        ts.append((4, 4 * (k % 3), k, 128 - 4 * (k % 3), 64 - k, f, k & 3))
    ts += [(4, 0, 0, 128, 64, 1, 1), (4, 1, 0, 127, 64, 1, 0), (3, 69, 44, 1, 1, 1, 0), (2, 36, 0, 1, 29, 2, 0), (3, 0, 0, 64, 32, 16 if mode == tiles.MODE else 32, 3)]
    return ts


def shapes_of(src):
    return [(w, h, ch) for (w, h, ch, _) in src.shapes]


# ------------------------------------------------------------------ 1: byte identity
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_byte_identity(ctx, oracle, small, channels, mode):
    ts = mixed_tiles(mode)
    before = small.host.copy()
    px, streams = tile_model(oracle, small, ts, channels, mode)
    if mode == tiles.MODE and channels == 0:
        # the images hold every way a vote is decided, counted by the definition as a loop (and the model agrees with the loop)
        census = {}
        for t, p in zip(ts, px):
            assert np.array_equal(p, loop(small.img[t[0]], t, channels, mode, census)), t
        assert census["unique"] > 100 and census["centre"] > 20 and census["lowest"] > 5, census
    retries = ctx.encode_retries()
    run_tiles(ctx, small, ts, channels, mode, 1, streams, shift=3)
    run_tiles(ctx, small, ts, channels, mode, 64, streams)
    subs = tiles.plan(shapes_of(small), ts, channels, 0)[1]
    assert ctx.tile_stats()[:2] == (len(subs), len(subs)) and ctx.tile_stats()[3] == 5 and ctx.encode_retries() == retries
    assert np.array_equal(small.d.cpu().numpy(), before)       # the source is only read


# ------------------------------------------------------------------ 2: sub-batches and a capacity cut
@pytest.mark.parametrize("mode", MODES)
def test_sub_batches_and_a_capacity_cut(ctx, oracle, small, mode):
    ts = mixed_tiles(mode)
    px, streams = tile_model(oracle, small, ts, 0, mode)
    slots = tiles.plan(shapes_of(small), ts, 0, 0)[0]
    mid = sum(slots[:7]) + slots[7] // 2
    results = []
    for staging in (1, mid, 0):
        _, subs, largest, referenced = tiles.plan(shapes_of(small), ts, 0, staging)
        results.append(run_tiles(ctx, small, ts, 0, mode, 16, streams, staging=staging)[:2])
        assert ctx.tile_stats() == (len(subs), len(subs), largest, referenced) and referenced == 5, (staging, ctx.tile_stats())     # [1]: launches of tile_select
    assert len(tiles.plan(shapes_of(small), ts, 0, 1)[1]) == len(ts) and 1 < len(tiles.plan(shapes_of(small), ts, 0, mid)[1]) < len(ts)
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1])
    lens = [len(s) for s in streams]
    want_off = pack_offsets(lens, 4)
    k = len(ts) // 2
    cap = int(want_off[k]) + lens[k] // 2                       # cuts the list in the middle: whole streams are missing, nothing is partial
    got_off, _, _ = run_tiles(ctx, small, ts, 0, mode, 4, streams, capacity=cap, shift=5, staging=sum(slots[:9]))
    assert int(got_off[-1]) > cap
    run_tiles(ctx, small, ts, 0, mode, 4, streams, capacity=0, null_dest=True)


# ------------------------------------------------------------------ 3: the walk
def test_a_workgroup_walks_tiles_of_entries_with_different_lane_splits(api, ctx, oracle):
    """more tiles of work items than the launch has workgroups (8 per CU): a workgroup takes several, of entries whose lg differ"""
    import torch
    src = label_sources(api, [(1024, 1024, 4, 0)], seed=3, cell=64, noise=False)
    S = src.img[0]
    S[:, 336:352] = label_image(16, 1024, 4, 5, cell=2)          # noise in a narrow band only: most blocks are constant, the model stays quick
    S[500:508, :] = label_image(1024, 8, 4, 6, cell=3)
    src.d = dev(src.host)
    workgroups = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    calls = {tiles.MODE: [(0, 0, 0, 1024, 1024, f, k & 3) for k, f in enumerate((2, 3, 4, 16))],
             tiles.NEAREST: [(0, 0, 0, 1024, 1024, 1, 0), (0, 0, 0, 1024, 1024, 64, 3), (0, 0, 0, 1024, 1024, 1, 1), (0, 0, 0, 1024, 1024, 2, 2), (0, 0, 0, 1024, 1024, 1, 2)]}
    for mode, ts in calls.items():
        count = sum(tiles.select_tiles(t[3], t[4], t[5], 4, mode) for t in ts)
        assert count > workgroups + 2, (mode, count, workgroups)
        assert len({tiles.select_split(t[5], mode)[0] for t in ts}) == (3 if mode == tiles.MODE else 1)
        px, streams = tile_model(oracle, src, ts, 0, mode)
        run_tiles(ctx, src, ts, 0, mode, 1, streams)
        assert ctx.tile_stats()[:2] == (1, 1)
    census = {}
    band = (0, 0, 495, 1023, 15, 3, 0)                          # blocks of the MODE call's f = 3 entry, counted by the definition as a loop
    assert np.array_equal(tiles.tile(S, band, 0, tiles.MODE), loop(S, band, 0, tiles.MODE, census))
    assert min(census.get(k, 0) for k in ("unique", "centre", "lowest")) > 0, census


# ------------------------------------------------------------------ 4: what is ingested is what the serving side computes
@pytest.mark.parametrize("mode,filt", [(tiles.MODE, tensors.FILTER_MODE), (tiles.NEAREST, tensors.FILTER_NEAREST)])
def test_round_trip_with_the_serving_side(api, ctx, mode, filt):
    import torch
    w = h = 256
    src = label_sources(api, [(w, h, 4, 7)], seed=21)
    pyr = api.tile_pyramid(w, h, 4, 256, 256, 5)                 # level l: the whole image at f = 2^l, every f divides the sides
    ts = [tiles.fields(t) for t in pyr]
    assert ts == tiles.pyramid(w, h, 256, 256, 5) and [t[5] for t in ts] == [1, 2, 4, 8, 16]
    ts += [(0, 64, 32, 128, 64, f, k & 3, 0) for k, f in enumerate((2, 4, 8, 16))] + [(0, 16, 240, 240, 16, 16, 3, 0), (0, 3, 5, 96, 48, 3, 1, 0)]
    assert all(t[3] % t[5] == 0 and t[4] % t[5] == 0 for t in ts)
    n = len(ts)
    bound = sum(tiles.encode_bound(*tiles.size(w, h, 4, t)[1:], 4) for t in ts)
    pack = torch.full((bound,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    off, sizes, descs = ctx.encode_tiles(src.d.data_ptr(), src.off, src.descs, 0, ts, mode, 1, pack.data_ptr(), bound, d_off.data_ptr(), d_len.data_ptr())
    # nothing but the call's three host tables from here on
    nbytes = [d.width * d.height * d.channels for d in descs]
    out_off = [int(v) for v in np.cumsum([0] + nbytes[:-1])]
    out = torch.full((sum(nbytes),), FILL, dtype=torch.uint8, device="cuda")
    ctx.decode_images(pack.data_ptr(), [int(o) for o in off[:n]], sizes, descs, 0, out.data_ptr(), out_off)
    ingested = out.cpu().numpy()
    assert np.array_equal(ingested[:nbytes[0]].reshape(h, w, 4), src.img[0])                       # level 0 is the source
    # the serving side: the same rectangles of level 0 - stream 0 of the pack - at the tiles' sizes
    items = [(0, t[1], t[2], t[3], t[4], t[3] // t[5], t[4] // t[5], t[6]) for t in ts]
    served = torch.full((sum(nbytes),), FILL, dtype=torch.uint8, device="cuda")
    ctx.decode_tensors(pack.data_ptr(), [int(off[0])], [int(sizes[0])], [descs[0]], 4, items, filt, 0, tensors.fmt(tensors.U8, tensors.HWC), served.data_ptr(), out_off)
    assert np.array_equal(served.cpu().numpy(), ingested)
    for k, t in enumerate(ts):
        assert np.array_equal(ingested[out_off[k]:out_off[k] + nbytes[k]].reshape(descs[k].height, descs[k].width, 4), tiles.tile(src.img[0], t, 0, mode)), t


# ------------------------------------------------------------------ 5: the box filter after a label call
def test_the_box_filter_after_a_label_call_gives_its_bytes(ctx, oracle, small):
    ts = mixed_tiles(tiles.MODE)
    for first in MODES:
        _, streams = tile_model(oracle, small, ts, 0, first)
        run_tiles(ctx, small, ts, 0, first, 1, streams)
        for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED):
            _, want = tile_model(oracle, small, ts, 0, mode)
            assert want != streams
            run_tiles(ctx, small, ts, 0, mode, 1, want)
            subs = tiles.plan(shapes_of(small), ts, 0, 0)[1]
            assert ctx.tile_stats()[:2] == (len(subs), len(subs))


def test_rejections_on_a_live_context_launch_nothing(ctx, small):
    import torch
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.full((3,), -1, dtype=torch.int64, device="cuda"), torch.full((2,), -1, dtype=torch.int32, device="cuda")
    stats = ctx.tile_stats()
    for mode, ts, word in [(tiles.MODE, [(3, 0, 0, 70, 45, 2, 0), (3, 0, 0, 70, 45, 17, 0)], "tile 1: factor above 16"), (6, [(3, 0, 0, 70, 45, 2, 0)] * 2, "mode"),
                           (2, [(3, 0, 0, 70, 45, 2, 0)] * 2, "mode")]:
        with pytest.raises(Exception) as e:
            ctx.encode_tiles(small.d.data_ptr(), small.off, small.descs, 0, ts, mode, 1, buf.data_ptr(), 4096, d_off.data_ptr(), d_len.data_ptr())
        assert word in str(e.value), (mode, str(e.value))
        assert (buf.cpu().numpy() == FILL).all() and (d_off.cpu().numpy() == -1).all() and (d_len.cpu().numpy() == -1).all()
    assert ctx.tile_stats() == stats


# ------------------------------------------------------------------ 6: the command-line tool
@pytest.mark.parametrize("name,mode", [("nearest", tiles.NEAREST), ("mode", tiles.MODE)])
def test_the_pyramid_tool_with_a_label_filter(api, oracle, tmp_path, name, mode):
    from tools import qoipyramid_mi355x as tool
    w, h = 150, 90
    px = label_image(w, h, 4, seed=8)
    src = tmp_path / "mask.qoi"
    assert api.qoi_write(str(src), px.reshape(-1), api.QoiDesc(w, h, 4, 0)) > 0
    lines = []
    assert tool.main([str(src), "--tile", "64", "--levels", "3", "--filter", name, "-o", str(tmp_path / "p")], out=lines.append) == 0
    assert "9 tiles" in lines[-1] and "3 levels" in lines[-1]
    classes = {tuple(c) for c in px.reshape(-1, 4).tolist()}
    for (level, row, col, tl) in tool.pyramid_grid(w, h, 64, 3):
        blob = (tmp_path / "p" / str(level) / f"tile_{row}_{col}.qoi").read_bytes()
        want = tiles.tile(px, tl, 0, mode)
        assert blob == oracle.encode(want.reshape(-1), want.shape[1], want.shape[0], 4), (level, row, col)
        assert {tuple(c) for c in want.reshape(-1, 4).tolist()} <= classes                       # no class is invented on any level
