"""Tensors as the source of qoimi_encode_tiles on the GPU (-m gpu): u8 / f16 / bf16 / f32 tensors, interleaved or planar, converted by the
kernel tensor_ingest on their way into the encoder.  A tile's pixels are those of qoi_amd/tiles.py: convert and tile, its stream is the
reference encoder's stream of them, byte for byte, and the pack is laid out by the numpy model of tests/test_packed_api.py - the checks of
tests/test_gpu_encode_tiles.py: run, which this file reuses as it is.  The tensors stand at two placements: 1 or 3 elements behind a
16-byte boundary (the element-by-element loads), and at multiples of 256, where torch hands a tensor over (the 8- and 16-byte loads of a
four-element HWC pixel and of a CHW run).  The shapes, formats, placements and tiles are those of tests/ingest_cases.py, which
tests/test_ingest_paths.py replays on the CPU."""
import numpy as np
import pytest

import ingest_cases
from ingest_cases import ALIGNED, FORMATS
from qoi_amd import tensors, tiles
from gpu_calls import TILE_FILL as FILL, Sources, Tensors, ingest_model as model, run_tiles as run
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
SPECIALS = [np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 65504.0]


def tiles_of(src, k0=0):
    """every image whole, and where it is wide enough a rectangle at x = 1 and one at the right edge; the four flips go round"""
    return ingest_cases.tiles_of(src.specs, k0)


@pytest.fixture(scope="module", params=[0, 1])
def mixed(request, api):
    """every legal dtype x layout x range with sch 3 and 4: 40 tensors of the five shapes in one buffer"""
    src = Tensors(api, ingest_cases.mixed_specs(request.param), seed=7 + request.param)
    assert all(o % 16 != 0 for o in src.off)
    return request.param, src


@pytest.fixture(scope="module", params=[0, 1])
def mixed_aligned(request, api):
    """the same 40 tensors, each at a multiple of 256"""
    src = Tensors(api, ingest_cases.mixed_specs(request.param), seed=7 + request.param, how=ALIGNED)
    assert all(o % 256 == 0 for o in src.off)
    return request.param, src


# ------------------------------------------------------------------ 1: byte identity
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_byte_identity(ctx, oracle, mixed, channels):
    byte_identity(ctx, oracle, mixed, channels)


@pytest.mark.parametrize("channels", ingest_cases.MIXED_CHANNELS)
def test_byte_identity_aligned(ctx, oracle, mixed_aligned, channels):
    byte_identity(ctx, oracle, mixed_aligned, channels)


def byte_identity(ctx, oracle, mixed, channels):
    k0, src = mixed
    ts = tiles_of(src, k0)
    assert {t[6] & 3 for t in ts} == {0, 1, 2, 3} and {src.flags[t[0]] for t in ts} == {tiles.source_flags(*f) for f in FORMATS}
    big = [b for b in src.bytes if b.size > 2000]
    assert all(b.min() == 0 and b.max() == 255 for b in big)           # both clamps occur
    before = src.host.copy()
    px, streams = model(oracle, src, ts, channels)
    run(ctx, src, ts, channels, tiles.PLAIN, 1, streams, shift=3)
    run(ctx, src, ts, channels, tiles.MODE, 64, streams)               # at factor 1 every mode gives the same bytes
    assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == 40
    assert np.array_equal(src.d.cpu().numpy(), before)                 # the source is only read


# ------------------------------------------------------------------ 2: special values
def test_special_values(api, ctx, oracle):
    specs, want = [], []
    for dtype in (tiles.F16, tiles.BF16, tiles.F32):
        sub = {tiles.F16: np.array([1], np.uint16).view(np.float16), tiles.BF16: np.array([1], np.uint16), tiles.F32: np.array([1], np.uint32).view(np.float32)}[dtype]
        with np.errstate(over="ignore"):
            v = np.asarray(SPECIALS, np.float32)
            a = v if dtype == tiles.F32 else v.astype(np.float16) if dtype == tiles.F16 else tensors.bf16_bits(v)
        a = np.tile(np.concatenate([a, sub]), 3)                       # 8 pixels of 3 elements: one row
        for rng in (tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES):
            specs.append((8, 1, 3, (dtype, tiles.HWC, rng), a))
            mid = 128 if rng == tiles.SYMMETRIC else 0                 # -0.0 and the smallest subnormal: t = 127.5, a tie, to even
            want.append([0, 255, 0, mid, 255, 0, 255, mid] * 3)
    src = Tensors(api, specs, seed=3)
    for b, w in zip(src.bytes, want):
        assert b.reshape(-1).tolist() == w                             # the model, against the list written out
    ts = [(i, 0, 0, 8, 1, 1, src.flags[i]) for i in range(9)]
    px, streams = model(oracle, src, ts, 0)
    run(ctx, src, ts, 0, tiles.PLAIN, 1, streams)


# ------------------------------------------------------------------ 3: round trip on the device (no model)
ROUND_TRIPS = ((tensors.F16, tensors.CHW, 1.0 / 255.0, 0.0, tiles.UNIT), (tensors.F32, tensors.HWC, 2.0 / 255.0, -1.0, tiles.SYMMETRIC))


@pytest.mark.parametrize("ch", [3, 4])
def test_round_trip_on_the_device(api, ctx, ch):
    round_trip(api, ctx, ch, False)


@pytest.mark.parametrize("ch", [3, 4])
def test_round_trip_on_the_device_aligned(api, ctx, ch):
    """decode_tensors writes to 256-aligned out_offsets, which the second encode reads: the wide loads"""
    round_trip(api, ctx, ch, True)


def round_trip(api, ctx, ch, aligned):
    import torch
    assert ingest_cases.ROUND_TRIP_SHAPES == [(37, 23), (70, 9), (300, 17)]
    u8 = Sources(api, [(37, 23, ch, 0), (70, 9, ch, 4096 + 3), (300, 17, ch, 8192 + 1)], seed=9)       # (a tensor call decodes to one channel count)
    n = 3
    whole = [(i, 0, 0, w, h, 1, i & 3) for i, (w, h, _, _) in enumerate(u8.shapes)]

    def encode(d_pixels, offs, ts):
        pack = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
        d_off, d_len = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        off, sizes, descs = ctx.encode_tiles(d_pixels, offs, u8.descs, 0, ts, tiles.PLAIN, 1, pack.data_ptr(), 1 << 16, d_off.data_ptr(), d_len.data_ptr())
        return pack, off, sizes, descs

    pack, off, sizes, descs = encode(u8.d.data_ptr(), u8.off, whole)
    want = pack[:int(off[-1])].cpu().numpy()
    assert [(d, l, r) for d, l, _, _, r in ROUND_TRIPS] == ingest_cases.ROUND_TRIP_FORMATS
    for dtype, layout, scale, bias, rng in ROUND_TRIPS:
        elem = tensors.ELEM[dtype]
        nbytes = [d.width * d.height * d.channels * elem for d in u8.descs]
        out_off = ingest_cases.round_trip_offsets(nbytes, aligned)             # element-aligned and not 16-aligned, or multiples of 256
        assert all(o % 256 == 0 for o in out_off) if aligned else all(o % elem == 0 and o % 16 != 0 for o in out_off)
        out = torch.zeros(out_off[-1] + nbytes[-1] + 64, dtype=torch.uint8, device="cuda")
        items = [(i, 0, 0, d.width, d.height, d.width, d.height, 0) for i, d in enumerate(u8.descs)]
        ctx.decode_tensors(pack.data_ptr(), [int(o) for o in off[:n]], sizes, descs, 0, items, tensors.FILTER_AREA, tensors.PLAIN,
                           tensors.fmt(dtype, layout, (scale,) * 4, (bias,) * 4), out.data_ptr(), out_off)
        src_flags = tiles.source_flags(dtype, layout, rng)
        # (the pack holds the mirrored images, the tensors are those: encoded again as they are they give the pack)
        again, off2, sizes2, _ = encode(out.data_ptr(), out_off, [t[:6] + (src_flags,) for t in whole])
        assert np.array_equal(off2, off) and sizes2.tolist() == sizes.tolist()
        assert out.data_ptr() % 256 == 0
        assert np.array_equal(again[:int(off[-1])].cpu().numpy(), want), (dtype, layout)
        assert ctx.tile_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 4: SRC alone
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_src_alone_is_the_unflagged_call(api, ctx, oracle, channels):
    src = Sources(api, [(1, 1, 4, 0), (5, 3, 3, 40), (37, 23, 3, 513), (70, 9, 4, 4099), (300, 17, 4, 17408), (300, 17, 3, 50301)])
    ts = []
    for i, (w, h, ch, _) in enumerate(src.shapes):
        ts.append((i, 0, 0, w, h, 1, i & 3))
        if w > 4:
            ts += [(i, 1, 0, w - 2, h, 1, (i + 1) & 3), (i, w - 4, 1, 4, h - 1, 1, (i + 2) & 3)]
    px = [tiles.tile(src.img[t[0]], t, channels) for t in ts]
    streams = [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], src.descs[t[0]].colorspace) for p, t in zip(px, ts)]
    a = run(ctx, src, ts, channels, tiles.PLAIN, 4, streams)
    b = run(ctx, src, [t[:6] + (t[6] | tiles.SRC,) for t in ts], channels, tiles.PLAIN, 4, streams)      # the same streams at the same offsets
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ 5: memory contract and sub-batches
def test_memory_contract_and_sub_batches(ctx, oracle, mixed):
    from model_cases import pack_offsets as offsets
    k0, src = mixed
    ts = tiles_of(src, k0)
    shapes = [(d.width, d.height, d.channels) for d in src.descs]
    before = src.host.copy()
    px, streams = model(oracle, src, ts, 0)
    slots, _, _, _ = tiles.plan(shapes, ts, 0, 0)
    mid = sum(slots[:7]) + slots[7] // 2
    for staging in (1, mid, 0):
        _, subs, largest, referenced = tiles.plan(shapes, ts, 0, staging)
        run(ctx, src, ts, 0, tiles.PLAIN, 16, streams, staging=staging)
        assert ctx.tile_stats() == (len(subs), len(subs), largest, referenced) and referenced == 40, (staging, ctx.tile_stats())
    assert len(tiles.plan(shapes, ts, 0, 1)[1]) == len(ts) and 3 <= len(tiles.plan(shapes, ts, 0, mid)[1]) < len(ts)
    lens = [len(s) for s in streams]
    want_off = offsets(lens, 4)
    k = len(ts) // 2
    cap = int(want_off[k]) + lens[k] // 2                              # cuts the list in the middle: whole streams are missing, nothing is partial
    got_off, _, _ = run(ctx, src, ts, 0, tiles.PLAIN, 4, streams, capacity=cap, shift=5, staging=mid)
    assert int(got_off[-1]) > cap and ctx.tile_stats()[0] == ctx.tile_stats()[1] >= 3
    run(ctx, src, ts, 0, tiles.PLAIN, 4, streams, capacity=0, null_dest=True)
    assert np.array_equal(src.d.cpu().numpy(), before)


# ------------------------------------------------------------------ 6: more tiles than workgroups
def test_a_workgroup_walks_three_tiles_or_more(api, ctx, oracle):
    import torch
    w, h = 2200, 2000
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles.ingest_tiles(w, h) > 2 * n_cus * 8                    # (a launch has n_cus * 8 workgroups at the most)
    rng = np.random.default_rng(21)
    low = rng.uniform(-0.1, 1.1, size=(3, h // 8, w // 8)).astype(np.float32)              # blocks of 8 x 8: streams of every chunk kind
    a = np.repeat(np.repeat(low, 8, axis=1), 8, axis=2) + rng.uniform(-0.01, 0.01, size=(3, h, w)).astype(np.float32)
    src = Tensors(api, [(w, h, 3, (tiles.F16, tiles.CHW, tiles.UNIT), a.astype(np.float16))])
    assert src.bytes[0].min() == 0 and src.bytes[0].max() == 255
    ts = [(0, 0, 0, w, h, 1, src.flags[0] | 1)]
    px, streams = model(oracle, src, ts, 0)
    run(ctx, src, ts, 0, tiles.PLAIN, 1, streams)


# ------------------------------------------------------------------ the command-line tool
def test_the_tool_writes_the_model_s_streams(oracle, tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import qoifromtensor_mi355x as tool
    a = np.random.default_rng(4).uniform(-1.5, 1.5, size=(3, 4, 9, 37)).astype(np.float16)
    np.save(tmp_path / "batch.npy", a)
    said = []
    assert tool.main([str(tmp_path / "batch.npy"), "-o", str(tmp_path / "out"), "--range", "symmetric", "--channels", "3"], out=said.append) == 0
    flags = tiles.source_flags(tiles.F16, tiles.CHW, tiles.SYMMETRIC)
    for i in range(3):
        B = tiles.convert(a[i], flags)[:, :, :3]
        assert (tmp_path / "out" / ("%04d.qoi" % i)).read_bytes() == oracle.encode(np.ascontiguousarray(B).reshape(-1), 37, 9, 3, 0), i
    assert "3 files of 3 channels" in said[0]
