"""Label tensors as the source of qoimi_encode_tiles on the GPU (-m gpu): one-plane u8 / int32 / int64 tensors of class indices, saturated
and replicated by the kernel label_ingest on their way into the encoder.  A tile's pixels are those of qoi_amd/tiles.py: labels_to_bytes and
tile, its stream is the reference encoder's stream of them, byte for byte, and the pack is laid out by the numpy model - the checks of
tests/gpu_calls.py: run_tiles, which this file uses as it is.  The planes share one device buffer at the offsets at which the kernel takes
its different loads: every residue of 16 an int32 or int64 plane can have, odd byte offsets for u8."""
import numpy as np
import pytest

from gpu_calls import TILE_FILL as FILL, run_tiles as run
from gpu_pack import dev
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from labelimg import label_image
from qoi_amd import tensors, tiles

pytestmark = pytest.mark.gpu
DTYPES = (tiles.L_U8, tiles.L_I32, tiles.L_I64)
SHAPES = [(37, 23), (5, 1), (1, 9), (1025, 3), (300, 17)]
# the plane's address modulo 16, by dtype: 16-byte loads and their fallbacks (i32, i64), both dwords of a run (u8: odd offsets)
RESIDUES = {tiles.L_U8: (1, 3, 5, 7, 11), tiles.L_I32: (0, 4, 8, 12, 4), tiles.L_I64: (0, 8, 8, 0, 8)}
VALUES = [0, 1, 254, 255, 256, -1, -100, 2 ** 31 - 1, -2 ** 31, 2 ** 32, 2 ** 32 + 5, -2 ** 32 + 7, 2 ** 63 - 1, -2 ** 63]
RANGE = {tiles.L_U8: (0, 255), tiles.L_I32: (-2 ** 31, 2 ** 31 - 1), tiles.L_I64: (-2 ** 63, 2 ** 63 - 1)}


class Planes:
    """Label planes in one device buffer, plane i at a byte offset that is residues[i] modulo 16; the interface of gpu_calls.Sources as far
    as run_tiles looks at it (d, off, descs).  specs: (w, h, dtype, residue, channels of the descriptor, array [h, w])."""

    def __init__(self, api, specs, seed=5):
        rng = np.random.default_rng(seed)
        self.off, self.flags, self.arrays, self.descs, parts = [], [], [], [], []
        cur = 256
        for i, (w, h, dtype, res, ch, a) in enumerate(specs):
            off = -(-cur // 16) * 16 + res
            a = np.ascontiguousarray(a, dtype=tiles.LABEL_ARRAYS[dtype])
            assert a.shape == (h, w) and off % tiles.LABEL_ELEM[dtype] == 0, (i, a.shape, off)
            self.off.append(off)
            self.flags.append(tiles.label_flags(dtype))
            self.arrays.append(a)
            self.descs.append(api.QoiDesc(w, h, ch, i & 1))
            parts.append((off, a.view(np.uint8).reshape(-1)))
            cur = off + a.nbytes + 3
        self.host = rng.integers(0, 256, size=cur + 64, dtype=np.uint8)
        for off, b in parts:
            self.host[off:off + b.size] = b
        self.d = dev(self.host)
        assert self.d.data_ptr() % 256 == 0, ("the source buffer's base is no multiple of 256", self.d.data_ptr())
        self.shapes = [(w, h, ch) for (w, h, _, _, ch, _) in specs]


def values(w, h, dtype, seed):
    """classes in short runs - streams of every chunk kind - and, where the dtype holds them, the listed values"""
    rng = np.random.default_rng(seed)
    v = np.repeat(rng.integers(0, 256, size=w * h), rng.integers(1, 6, size=w * h))[:w * h].astype(np.int64)
    lo, hi = RANGE[dtype]
    mine = np.array([x for x in VALUES if lo <= x <= hi], dtype=np.int64)
    at = rng.permutation(w * h)[:min(mine.size * 3, w * h)]
    v[at] = mine[np.arange(at.size) % mine.size]
    return v.reshape(h, w).astype(tiles.LABEL_ARRAYS[dtype])


def model(oracle, src, ts, channels, mode):
    """the model's pixels of every tile - och is the call's channels, or the descriptor's - and the reference encoder's streams of them"""
    px = [tiles.tile(src.arrays[t[0]], t, channels or src.descs[t[0]].channels, mode) for t in ts]
    return px, [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], src.descs[t[0]].colorspace) for p, t in zip(px, ts)]


@pytest.fixture(scope="module", params=DTYPES, ids=["u8", "i32", "i64"])
def planes(request, api):
    dtype = request.param
    src = Planes(api, [(w, h, dtype, res, 3 + (i & 1), values(w, h, dtype, 40 + i)) for i, ((w, h), res) in enumerate(zip(SHAPES, RESIDUES[dtype]))], seed=dtype)
    assert [o % 16 for o in src.off] == list(RESIDUES[dtype])
    return dtype, src


def stream_tiles(src):
    """every plane whole, and where it is wide enough an interior rectangle at odd x; the four flips go round"""
    ts, k = [], 0
    for i, (w, h, _) in enumerate(src.shapes):
        ts.append((i, 0, 0, w, h, 1, src.flags[i] | (k & 3)))
        k += 1
        if w > 6:
            ts.append((i, 1, h // 3, w - 4, h - h // 3, 1, src.flags[i] | (k & 3)))
            ts.append((i, 3, 0, w - 3, max(h - 1, 1), 1, src.flags[i] | ((k + 1) & 3)))
            k += 2
    return ts


# ------------------------------------------------------------------ 1: streams
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_streams(ctx, oracle, planes, channels):
    dtype, src = planes
    ts = stream_tiles(src)
    assert {t[6] & 3 for t in ts} == {0, 1, 2, 3}
    lo, hi = RANGE[dtype]
    held = set(np.concatenate([a.reshape(-1) for a in src.arrays]).tolist())
    assert {v for v in VALUES if lo <= v <= hi} <= held                 # the listed values stand in the planes
    before = src.host.copy()
    px, streams = model(oracle, src, ts, channels, tiles.PLAIN)
    run(ctx, src, ts, channels, tiles.PLAIN, 1, streams, shift=3)
    run(ctx, src, ts, channels, tiles.MODE, 64, streams)               # at factor 1 every mode gives the same bytes
    assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == len(SHAPES)
    assert np.array_equal(src.d.cpu().numpy(), before)                 # the source is only read


# ------------------------------------------------------------------ 2: reductions
@pytest.fixture(scope="module")
def maps(api):
    """label images of tests/labelimg.py as planes: (37 x 23) as int64 and (64 x 48) as u8 and as int32, class indices of their green channel"""
    a, b = label_image(37, 23, 4, 31)[:, :, 1], label_image(64, 48, 4, 32)[:, :, 1]
    assert len(np.unique(a)) >= 3 and len(np.unique(b)) >= 3
    return Planes(api, [(37, 23, tiles.L_I64, 8, 4, a), (64, 48, tiles.L_U8, 3, 3, b), (64, 48, tiles.L_I32, 4, 4, b)], seed=9)


@pytest.mark.parametrize("mode,factors", [(tiles.MODE, (2, 3, 16)), (tiles.NEAREST, (2, 64))], ids=["mode", "nearest"])
@pytest.mark.parametrize("channels", [0, 3])
def test_reductions(ctx, oracle, maps, mode, factors, channels):
    ts = []
    for k, f in enumerate(factors):
        for i, (w, h, _) in enumerate(maps.shapes):
            ts.append((i, 0, 0, w, h, f, maps.flags[i] | (k & 3)))
            ts.append((i, 3, 1, w - 5, h - 2, f, maps.flags[i] | ((k + i + 1) & 3)))      # partial edge blocks
    ts.append((0, 0, 0, 37, 23, 1, maps.flags[0]))                     # the copy and the reductions in one table
    px, streams = model(oracle, maps, ts, channels, mode)
    if mode == tiles.MODE:
        assert any(not np.array_equal(p, q) for p, q in zip(px, model(oracle, maps, ts, channels, tiles.NEAREST)[0]))    # a vote is not the centre
    run(ctx, maps, ts, channels, mode, 1, streams, shift=1)
    assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == 3


def test_a_label_pyramid(api, ctx, oracle, maps):
    w, h, ch = maps.shapes[2]
    pyr = [tiles.fields(t) for t in api.tile_pyramid(w, h, ch, 16, 16, 3)]
    assert pyr == tiles.pyramid(w, h, 16, 16, 3) and len(pyr) == 12 + 4 + 1
    for mode in (tiles.MODE, tiles.NEAREST):
        ts = [(2,) + t[1:6] + (maps.flags[2],) for t in pyr]
        px, streams = model(oracle, maps, ts, 0, mode)
        run(ctx, maps, ts, 0, mode, 4, streams)
        assert ctx.tile_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 3: round trip (property a)
@pytest.mark.parametrize("dtype,out", [(tiles.L_I64, tensors.I64), (tiles.L_I32, tensors.I32)], ids=["i64", "i32"])
def test_round_trip(api, ctx, dtype, out):
    import torch
    w, h = 23, 37
    a = np.random.default_rng(17).integers(0, 256, size=(h, w)).astype(tiles.LABEL_ARRAYS[dtype])
    assert a.min() == 0 and a.max() == 255
    t_in = torch.from_numpy(a).cuda()
    cap = tiles.encode_bound(w, h, 4)
    pack = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    off, sizes, descs = ctx.encode_tiles(t_in.data_ptr(), [0], [api.QoiDesc(w, h, 4, 0)], 0, [(0, 0, 0, w, h, 1, tiles.label_flags(dtype))], tiles.NEAREST, 1,
                                         pack.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())
    t_out = torch.full((h, w), -7, dtype=t_in.dtype, device="cuda")
    ctx.decode_tensors(pack.data_ptr(), [int(off[0])], sizes, descs, 0, [(0, 0, 0, w, h, w, h, 0)], tensors.FILTER_NEAREST, tensors.PLAIN, tensors.fmt(out, tensors.HW),
                       t_out.data_ptr(), [0])
    assert torch.equal(t_out, t_in)


# ------------------------------------------------------------------ 4: sub-batches
def test_sub_batches(ctx, oracle, planes):
    dtype, src = planes
    ts = stream_tiles(src) + [(0, 0, 0, 37, 23, 2, src.flags[0]), (4, 1, 1, 298, 15, 3, src.flags[4] | 1)]
    px, streams = model(oracle, src, ts, 0, tiles.MODE)
    slots = tiles.plan(src.shapes, ts, 0, 0)[0]
    three = [s for s in sorted({sum(slots[:k]) for k in range(1, len(slots) + 1)} | {max(slots)}) if s >= max(slots) and len(tiles.plan(src.shapes, ts, 0, s)[1]) == 3]
    assert three, slots
    whole = run(ctx, src, ts, 0, tiles.MODE, 16, streams)
    assert ctx.tile_stats()[:2] == (1, 1)
    _, subs, largest, referenced = tiles.plan(src.shapes, ts, 0, three[0])
    cut = run(ctx, src, ts, 0, tiles.MODE, 16, streams, staging=three[0], shift=5)
    assert ctx.tile_stats() == (3, 3, largest, referenced) and referenced == len(SHAPES), ctx.tile_stats()
    assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1])


# ------------------------------------------------------------------ 5: a non-blocking stream
def test_stream_order_on_a_non_blocking_stream(api, ctx, oracle):
    """one label call behind a kernel that writes the planes, on a stream that does not synchronise with stream 0: the harness of
    tests/stream_order.py.  The stale planes hold other classes, which give other streams."""
    from model_cases import pack_offsets
    from stream_order import Case, Harness, Inp, Out
    shapes = [(160, 120), (97, 61)]
    flags = tiles.label_flags(tiles.L_I64)
    true = [label_image(w, h, 4, 50 + i)[:, :, 1].astype(np.int64) for i, (w, h) in enumerate(shapes)]
    stale = [label_image(w, h, 4, 60 + i)[:, :, 0].astype(np.int64) + 2 ** 32 for i, (w, h) in enumerate(shapes)]
    ts = [(0, 0, 0, 160, 120, 1, flags), (1, 1, 2, 90, 51, 3, flags | 2), (0, 3, 5, 120, 64, 16, flags | 1), (1, 0, 0, 97, 61, 1, flags | 3)]
    px = [tiles.tile(true[t[0]], t, 4, tiles.MODE) for t in ts]
    assert all(not np.array_equal(tiles.tile(stale[t[0]], t, 4, tiles.MODE), p) for t, p in zip(ts, px))
    want = [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], 4) for p in px]
    lens = [len(s) for s in want]
    po = [0, true[0].nbytes + 8]
    blob = lambda planes_: np.concatenate([planes_[0].view(np.uint8).reshape(-1), np.zeros(8, np.uint8), planes_[1].view(np.uint8).reshape(-1)])  # noqa: E731
    inp = Inp(blob(true), blob(stale))
    off = pack_offsets(lens, 1)
    outs = [Out(int(off[-1]), [(int(off[i]), s) for i, s in enumerate(want)]), Out(8 * (len(ts) + 1), [(0, off)]), Out(4 * len(ts), [(0, np.array(lens, dtype=np.int32))])]
    descs = [api.QoiDesc(w, h, 4, 0) for w, h in shapes]
    desc_shapes = [(w, h, 4) for w, h in shapes]
    staging = max(tiles.plan(desc_shapes, ts, 0, 0)[0])
    subs = tiles.plan(desc_shapes, ts, 0, staging)[1]
    assert len(subs) >= 2

    def ok(result):
        assert np.array_equal(result[0], off) and result[1].tolist() == lens, (result[0], off, result[1], lens)
        assert ctx.tile_stats()[:2] == (len(subs), len(subs))

    H = Harness()
    H.run(Case("encode_tiles, labels", True, [inp], outs,
               lambda st: ctx.encode_tiles(inp.ptr, po, descs, 0, ts, tiles.MODE, 1, outs[0].ptr, int(off[-1]), outs[1].ptr, outs[2].ptr, staging, st), ok))
    assert H.met == [("encode_tiles, labels", H.met[0][1])]


# ------------------------------------------------------------------ 6: no rejected call launches anything
def test_rejections_on_a_live_context_launch_nothing(ctx, oracle, planes):
    import torch
    dtype, src = planes
    good = stream_tiles(src)[:3]
    _, streams = model(oracle, src, good, 0, tiles.PLAIN)
    run(ctx, src, good, 0, tiles.PLAIN, 1, streams)
    stats = ctx.tile_stats()
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.full((4,), -1, dtype=torch.int64, device="cuda"), torch.full((3,), -1, dtype=torch.int32, device="cuda")
    before = src.host.copy()
    lab, other = src.flags[0], tiles.label_flags((dtype + 1) % 3)
    elem = tiles.LABEL_ELEM[dtype]
    odd = [o + (1 if elem > 1 else 0) for o in src.off]
    inside = src.d.data_ptr() + src.off[0] + 37 * 23 * elem - 1           # the pack would begin on the last byte of plane 0, counted in elements
    cases = [(tiles.PLAIN, [(0, 0, 0, 37, 23, 1, lab), (0, 0, 0, 37, 23, 2, lab)], src.off, None, "tile 1: a label source is never averaged"),
             (tiles.ALPHA_WEIGHTED, [(0, 0, 0, 37, 23, 64, lab)], src.off, None, "never averaged"),
             (tiles.MODE, [(0, 0, 0, 37, 23, 17, lab)], src.off, None, "factor above 16"),
             (tiles.NEAREST, [(0, 0, 0, 37, 23, 2, tiles.LABELS | 12288)], src.off, None, "12288 is not a dtype"),
             (tiles.NEAREST, [(0, 0, 0, 37, 23, 2, lab | tiles.SRC_CHW | tiles.SRC)], src.off, None, "factor 1 only"),
             (tiles.NEAREST, [(0, 0, 0, 37, 23, 1, lab | tiles.SRC)], src.off, None, "together with a QOIMI_TILE_SRC"),
             (tiles.NEAREST, [(0, 0, 0, 37, 23, 2, lab), (1, 0, 0, 5, 1, 1, 0)], src.off, None, "a byte call, a tensor call or a label call"),
             (tiles.NEAREST, [(0, 0, 0, 37, 23, 2, lab), (0, 0, 0, 1, 1, 1, other)], src.off, None, "two different label dtypes"),
             (tiles.NEAREST, [(0, 0, 0, 37, 23, 2, lab)], src.off, inside, "overlap")]
    if elem > 1:
        cases.append((tiles.NEAREST, [(0, 0, 0, 37, 23, 2, lab)], odd, None, "multiple of the element size"))
    for mode, ts, offs, dest, word in cases:
        with pytest.raises(Exception) as e:
            ctx.encode_tiles(src.d.data_ptr(), offs, src.descs, 0, ts, mode, 1, buf.data_ptr() if dest is None else dest, 4096, d_off.data_ptr(), d_len.data_ptr())
        assert word in str(e.value), (mode, ts, str(e.value))
        assert (buf.cpu().numpy() == FILL).all() and (d_off.cpu().numpy() == -1).all() and (d_len.cpu().numpy() == -1).all()
        assert ctx.tile_stats() == stats, word
    assert np.array_equal(src.d.cpu().numpy(), before)
