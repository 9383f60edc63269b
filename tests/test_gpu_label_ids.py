"""24-bit label ids on the GPU (-m gpu): QOIMI_TILE_LABELS_ID24 in qoimi_encode_tiles - one-plane u8 / int32 / int64 maps of ids, saturated
to 0..2^24 - 1 and spread over r, g and b by the kernel label_ingest - and QOIMI_TENSOR_HW_ID24 in qoimi_decode_tensors and
qoimi_decode_warped_tensors, which puts the three bytes together again.  A tile's pixels are those of qoi_amd/tiles.py: label_ids_to_bytes
and tile, its stream is the reference encoder's stream of them byte for byte, the pack is laid out by the numpy model (the checks of
tests/gpu_calls.py: run_tiles, as it is); a tensor is qoi_amd/tensors.py: convert of the underlying call's pixels, bit for bit, with guard
bytes between the outputs.  The planes share one device buffer at the offsets at which the kernel takes its different loads."""
import numpy as np
import pytest

from gpu_calls import TILE_FILL as FILL, run_tiles as run
from gpu_pack import GUARD, OraclePack, dev, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from qoi_amd import tensors, tiles, warp

pytestmark = pytest.mark.gpu
DTYPES = (tiles.L_U8, tiles.L_I32, tiles.L_I64)
SHAPES = [(1, 1), (3, 2), (4, 1), (5, 3), (8, 2), (37, 29), (64, 48)]
# the plane's address modulo 16, by dtype: 0, the element size E, 8 and (i32) 12 among them - the aligned 16-byte runs and the element-wise loads
RESIDUES = {tiles.L_U8: (0, 1, 8, 3, 5, 7, 11), tiles.L_I32: (0, 4, 8, 12, 4, 12, 0), tiles.L_I64: (0, 8, 8, 0, 8, 0, 8)}
BOUNDARY = [-2 ** 63, -2 ** 31, -1, 0, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 - 1]
RANGE = {tiles.L_U8: (0, 255), tiles.L_I32: (-2 ** 31, 2 ** 31 - 1), tiles.L_I64: (-2 ** 63, 2 ** 63 - 1)}
ID_MAX = 2 ** 24 - 1


class Planes:
    """Label planes in one device buffer, plane i at a byte offset that is its residue modulo 16; the interface of gpu_calls.Sources as far
    as run_tiles looks at it (d, off, descs).  specs: (w, h, dtype, residue, channels of the descriptor, ids or class indices, array [h, w])."""

    def __init__(self, api, specs, seed=5):
        rng = np.random.default_rng(seed)
        self.off, self.flags, self.arrays, self.descs, parts = [], [], [], [], []
        cur = 256
        for i, (w, h, dtype, res, ch, ids, a) in enumerate(specs):
            off = -(-cur // 16) * 16 + res
            a = np.ascontiguousarray(a, dtype=tiles.LABEL_ARRAYS[dtype])
            assert a.shape == (h, w) and off % tiles.LABEL_ELEM[dtype] == 0, (i, a.shape, off)
            self.off.append(off)
            self.flags.append(tiles.label_flags(dtype, ids))
            self.arrays.append(a)
            self.descs.append(api.QoiDesc(w, h, ch, i & 1))
            parts.append((off, a.view(np.uint8).reshape(-1)))
            cur = off + a.nbytes + 3
        self.host = rng.integers(0, 256, size=cur + 64, dtype=np.uint8)
        for off, b in parts:
            self.host[off:off + b.size] = b
        self.d = dev(self.host)
        assert self.d.data_ptr() % 256 == 0, ("the source buffer's base is no multiple of 256", self.d.data_ptr())
        self.shapes = [(w, h, ch) for (w, h, _, _, ch, _, _) in specs]


def values(w, h, dtype, seed):
    """the boundary list cycled through (where the dtype holds the value), random ids below 2^24, and constant regions for the vote"""
    rng = np.random.default_rng(seed)
    lo, hi = RANGE[dtype]
    top = min(hi, ID_MAX)
    mine = np.array([x for x in BOUNDARY if lo <= x <= hi], dtype=np.int64)
    v = rng.integers(0, top + 1, size=w * h).astype(np.int64)
    v[::3] = mine[np.arange(len(v[::3])) % mine.size]
    v = v.reshape(h, w)
    if w >= 8 and h >= 8:                                               # regions of one id, each wider than a block of the smaller factors
        few = np.array([1, 256, 65536, 70000, top, 0])
        few = few[few <= top]
        for k in range(6):
            x, y = int(rng.integers(0, w - 6)), int(rng.integers(0, h - 6))
            v[y:y + int(rng.integers(3, 9)), x:x + int(rng.integers(3, 12))] = few[k % few.size]
    return v.astype(tiles.LABEL_ARRAYS[dtype])


def model(oracle, src, ts, channels, mode):
    """the model's pixels of every tile - och is the call's channels, or the descriptor's - and the reference encoder's streams of them"""
    px = [tiles.tile(src.arrays[t[0]], t, channels or src.descs[t[0]].channels, mode) for t in ts]
    return px, [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], src.descs[t[0]].colorspace) for p, t in zip(px, ts)]


@pytest.fixture(scope="module", params=DTYPES, ids=["u8", "i32", "i64"])
def planes(request, api):
    dtype = request.param
    src = Planes(api, [(w, h, dtype, res, 3 + (i & 1), True, values(w, h, dtype, 40 + i)) for i, ((w, h), res) in enumerate(zip(SHAPES, RESIDUES[dtype]))], seed=dtype)
    assert [o % 16 for o in src.off] == list(RESIDUES[dtype])
    E = tiles.LABEL_ELEM[dtype]
    assert {0, E % 16, 8} <= set(RESIDUES[dtype]) and (dtype != tiles.L_I32 or 12 in RESIDUES[dtype])
    return dtype, src


def copy_tiles(src):
    """every plane whole, and of the larger ones an inner rectangle of odd size at odd x and y; the four flips go round"""
    ts, k = [], 0
    for i, (w, h, _) in enumerate(src.shapes):
        ts.append((i, 0, 0, w, h, 1, src.flags[i] | (k & 3)))
        k += 1
        if w > 6 and h > 6:
            ts.append((i, 3, 1, w - 6 - (w & 1 ^ 1), h - 4 - (h & 1 ^ 1), 1, src.flags[i] | (k & 3)))
            ts.append((i, 1, 5, w - 2, h - 6, 1, src.flags[i] | ((k + 1) & 3)))
            k += 2
    return ts


# ------------------------------------------------------------------ 1: ingest, factor 1
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_streams(ctx, oracle, planes, channels):
    dtype, src = planes
    ts = copy_tiles(src)
    assert {t[6] & 3 for t in ts} == {0, 1, 2, 3} and any(t[3] & 1 and t[4] & 1 and t[1] & 1 and t[2] & 1 for t in ts)
    lo, hi = RANGE[dtype]
    held = set(np.concatenate([a.reshape(-1) for a in src.arrays]).tolist())
    assert {v for v in BOUNDARY if lo <= v <= hi} <= held               # the listed values stand in the planes
    before = src.host.copy()
    px, streams = model(oracle, src, ts, channels, tiles.PLAIN)
    if dtype != tiles.L_U8:
        assert any((p[:, :, 0] != p[:, :, 1]).any() and (p[:, :, 1] != p[:, :, 2]).any() for p in px)     # the pixels are not grey
    run(ctx, src, ts, channels, tiles.PLAIN, 1, streams, shift=3)
    run(ctx, src, ts, channels, tiles.MODE, 64, streams)               # at factor 1 every mode gives the same bytes
    assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == len(SHAPES)
    assert np.array_equal(src.d.cpu().numpy(), before)                 # the source is only read


# ------------------------------------------------------------------ 2: ingest, the reductions
def vote_factors():
    """every factor 2..16 at which tile_select splits a block over its lanes in another way"""
    seen, out = set(), []
    for f in range(2, 17):
        s = tiles.select_split(f, tiles.MODE)
        if s not in seen:
            seen.add(s)
            out.append(f)
    return out


@pytest.mark.parametrize("mode,factors", [(tiles.MODE, tuple(vote_factors())), (tiles.NEAREST, (2, 3, 64))], ids=["mode", "nearest"])
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_reductions(ctx, oracle, planes, mode, factors, channels):
    dtype, src = planes
    assert 2 in factors and (mode == tiles.NEAREST or len({tiles.select_split(f, mode) for f in factors}) == len(factors) >= 4), factors
    ts = []
    for k, f in enumerate(factors):
        for i in (1, 4, 5, 6):
            w, h, _ = src.shapes[i]
            ts.append((i, 0, 0, w, h, f, src.flags[i] | (k & 3)))
            if w > 6 and h > 6:
                ts.append((i, 3, 1, w - 5, h - 2, f, src.flags[i] | ((k + i + 1) & 3)))      # partial edge blocks
    ts.append((5, 0, 0, 37, 29, 1, src.flags[5]))                      # the copy and the reductions in one table
    px, streams = model(oracle, src, ts, channels, mode)
    if mode == tiles.MODE:
        assert any(not np.array_equal(p, q) for p, q in zip(px, model(oracle, src, ts, channels, tiles.NEAREST)[0]))    # a vote is not the centre
    run(ctx, src, ts, channels, mode, 1, streams, shift=1)
    assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == 4


# ------------------------------------------------------------------ 3: ids and class indices in one call; sub-batches
@pytest.fixture(scope="module")
def mixed(api):
    """the 37 x 29 and 64 x 48 planes twice: as ids and as class indices, the dtypes taking turns"""
    specs = []
    for i, (dtype, ids, (w, h), res) in enumerate([(tiles.L_I32, True, (37, 29), 4), (tiles.L_I32, False, (37, 29), 12), (tiles.L_I64, True, (64, 48), 8),
                                                    (tiles.L_I64, False, (64, 48), 0), (tiles.L_U8, True, (37, 29), 1), (tiles.L_U8, False, (8, 2), 3)]):
        specs.append((w, h, dtype, res, 3 + (i & 1), ids, values(w, h, dtype, 70 + i // 2)))
    return Planes(api, specs, seed=12)


def mixed_tiles(src):
    ts = []
    for i, (w, h, _) in enumerate(src.shapes):
        ts.append((i, 0, 0, w, h, 1, src.flags[i] | (i & 3)))
        ts.append((i, 1, 0, w - 1, h, 2, src.flags[i] | ((i + 1) & 3)))
        ts.append((i, 0, 1, w, h - 1, 3, src.flags[i]))
    return ts


def test_id_and_plain_images_mix_in_one_call(ctx, oracle, mixed):
    ts = mixed_tiles(mixed)
    assert {t[6] & tiles.LABELS_ID24 for t in ts} == {0, tiles.LABELS_ID24}
    for mode in (tiles.MODE, tiles.NEAREST):
        px, streams = model(oracle, mixed, ts, 0, mode)
        # the same values as ids and as class indices give other pixels: the bit is the image's, not the call's
        assert not np.array_equal(px[0], px[3]) and np.all(px[3][:, :, 0] == px[3][:, :, 1])
        run(ctx, mixed, ts, 0, mode, 4, streams, shift=2)
        assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == 6


def test_sub_batches(ctx, oracle, mixed):
    ts = mixed_tiles(mixed)
    px, streams = model(oracle, mixed, ts, 4, tiles.MODE)
    slots = tiles.plan(mixed.shapes, ts, 4, 0)[0]
    sums = sorted({sum(slots[:k]) for k in range(1, len(slots) + 1)} | {max(slots)})
    three = [s for s in sums if s >= max(slots) and len(tiles.plan(mixed.shapes, ts, 4, s)[1]) >= 3]
    assert three, slots
    whole = run(ctx, mixed, ts, 4, tiles.MODE, 16, streams)
    assert ctx.tile_stats()[:2] == (1, 1)
    _, subs, largest, referenced = tiles.plan(mixed.shapes, ts, 4, three[-1])
    assert len(subs) >= 3
    cut = run(ctx, mixed, ts, 4, tiles.MODE, 16, streams, staging=three[-1], shift=5)
    assert ctx.tile_stats() == (len(subs), len(subs), largest, referenced) and referenced == 6, ctx.tile_stats()
    assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1])


# ------------------------------------------------------------------ 4: decode
def layout(items, elem, front):
    """(offsets, byte sizes, total): one element per pixel; the first output at `front`, one to three guard elements between the outputs"""
    nbytes = [it[5] * it[6] * elem for it in items]
    pos, offsets = front, []
    for j, n in enumerate(nbytes):
        offsets.append(pos)
        pos += n + (1 + j % 3) * elem
    return offsets, nbytes, pos + 64


def run_ids(ctx, p, filt, channels, items, td, staging=0, front=None):
    """One call with QOIMI_TENSOR_HW_ID24; returns the outputs as arrays [oh, ow].  The buffer's base is a multiple of 256, so the offsets
    are the alignment: I32 outputs begin at 4 modulo 8."""
    elem = tensors.INT_ELEM[td]
    offsets, nbytes, total = layout(items, elem, 64 + elem if front is None else front)
    buf = filled(total, GUARD)
    assert buf.data_ptr() % 256 == 0, ("the output buffer's base is no multiple of 256", buf.data_ptr())
    f = tensors.fmt(td, tensors.HW_ID24)
    if filt == "warp":
        ctx.decode_warped_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, tensors.PLAIN, f, buf.data_ptr(), offsets, staging)
    else:
        ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, filt, tensors.PLAIN, f, buf.data_ptr(), offsets, staging)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n].view(tensors.numpy_dtype(td)).reshape(it[6], it[5]) for o, n, it in zip(offsets, nbytes, items)]


@pytest.mark.parametrize("td", [tensors.I64, tensors.I32], ids=["i64", "i32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "i32", "i64"])
def test_property_a_the_round_trip(api, ctx, dtype, td):
    """encode_tiles with the bit, whole images at factor 1, then NEAREST at the image's size with HW_ID24: the planes widened"""
    import torch
    rng = np.random.default_rng(17 + dtype)
    shapes = [(37, 29), (5, 3), (64, 48), (1, 1)]
    top = 255 if dtype == tiles.L_U8 else ID_MAX
    planes_ = [rng.integers(0, top + 1, size=(h, w)).astype(tiles.LABEL_ARRAYS[dtype]) for w, h in shapes]
    planes_[0].flat[:4] = [0, top, min(256, top), min(65536, top)]
    E = tiles.LABEL_ELEM[dtype]
    po = [int(x) for x in np.cumsum([0] + [-(-a.nbytes // 8) * 8 for a in planes_[:-1]])]
    host = np.zeros(po[-1] + planes_[-1].nbytes, np.uint8)
    for o, a in zip(po, planes_):
        host[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
    d_in = dev(host)
    assert d_in.data_ptr() % 16 == 0 and all(o % E == 0 for o in po)
    flags = tiles.label_flags(dtype, ids=True)
    ts = [(i, 0, 0, w, h, 1, flags) for i, (w, h) in enumerate(shapes)]
    cap = sum(tiles.encode_bound(w, h, 4) + 16 for w, h in shapes)
    pack = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(len(ts) + 1, dtype=torch.int64, device="cuda"), torch.zeros(len(ts), dtype=torch.int32, device="cuda")
    off, sizes, descs = ctx.encode_tiles(d_in.data_ptr(), po, [api.QoiDesc(w, h, 4, 0) for w, h in shapes], 0, ts, tiles.NEAREST, 1, pack.data_ptr(), cap,
                                         d_off.data_ptr(), d_len.data_ptr())

    class P:
        pass
    p = P()
    p.packed, p.so, p.sizes, p.descs = pack, [int(o) for o in off[:len(ts)]], [int(s) for s in sizes], descs
    items = [(i, 0, 0, w, h, w, h, 0) for i, (w, h) in enumerate(shapes)]
    for channels in (0, 3):
        got = run_ids(ctx, p, tensors.FILTER_NEAREST, channels, items, td)
        for g, a in zip(got, planes_):
            assert g.dtype == tensors.numpy_dtype(td) and np.array_equal(g, a.astype(np.int64)), (dtype, td, channels, a.shape)


@pytest.fixture(scope="module")
def idpack(api, oracle):
    """ids as the pixels label_ids_to_bytes gives them, encoded by the reference encoder: a 48 x 32 map of regions (image 0, 4 channels), the same
    as a 3-channel stream (image 1), and a hand-made RGBA image whose alpha is not 255 (image 2)"""
    rng = np.random.default_rng(33)
    few = np.array([0, 1, 256, 65536, 65537, ID_MAX, 300000, 513])
    ids = few[np.repeat(rng.integers(0, few.size, size=48 * 32), rng.integers(1, 5, size=48 * 32))[:48 * 32]].reshape(32, 48).astype(np.int64)
    ids[8:20, 10:30] = 70000
    B = tiles.label_ids_to_bytes(ids, tiles.label_flags(tiles.L_I64, ids=True))
    A = rng.integers(0, 256, size=(11, 13, 4), dtype=np.uint8)
    A[:, :, 3] = rng.choice(np.array([0, 1, 128, 254], dtype=np.uint8), size=(11, 13))
    p = OraclePack(api, oracle, [(48, 32, 4), (48, 32, 3), (13, 11, 4)], [B, B[:, :, :3], A])
    p.ids, p.B, p.A = ids, B, A
    return p


def test_property_c_filter_mode_of_the_factor_1_pack(ctx, idpack):
    """with f dividing w and h, an ID24 MODE tile decodes to what FILTER_MODE gives from the factor-1 pack at w/f x h/f"""
    p = idpack
    flags = tiles.label_flags(tiles.L_I64, ids=True)
    items = [(0, 0, 0, 48, 32, 48 // f, 32 // f, 0) for f in (2, 4, 8, 16)]
    got = run_ids(ctx, p, tensors.FILTER_MODE, 4, items, tensors.I64)
    for f, g in zip((2, 4, 8, 16), got):
        T = tiles.tile(p.ids, (0, 0, 0, 48, 32, f, flags), 4, tiles.MODE)
        want = tensors.convert(T, tensors.fmt(tensors.I64, tensors.HW_ID24))
        assert np.array_equal(g, want), f
        assert np.array_equal(g, tensors.tensors(p.B, (0, 0, 48, 32), (48 // f, 32 // f), 0, tensors.FILTER_MODE, tensors.PLAIN, tensors.fmt(tensors.I64, tensors.HW_ID24)))
        assert set(np.unique(g)) <= set(np.unique(p.ids))               # no id is invented
    # ... flipped, from a rectangle, as I32, through sub-batches of the decode
    items = [(0, 4, 2, 40, 28, 10, 7, 3), (1, 0, 0, 48, 32, 24, 16, 1), (0, 1, 1, 45, 30, 15, 10, 2)]
    f32 = tensors.fmt(tensors.I32, tensors.HW_ID24)
    for filt in (tensors.FILTER_MODE, tensors.FILTER_NEAREST):
        got = run_ids(ctx, p, filt, 0, [items[0], items[2]], tensors.I32)
        for it, g in zip([items[0], items[2]], got):
            assert np.array_equal(g, tensors.tensors(p.B, it[1:5], it[5:7], it[7], filt, tensors.PLAIN, f32)), (filt, it)
        got = run_ids(ctx, p, filt, 0, [items[1]], tensors.I32)
        assert np.array_equal(got[0], tensors.tensors(p.B[:, :, :3], items[1][1:5], items[1][5:7], items[1][7], filt, tensors.PLAIN, f32)), filt


def warp_model(D, it, td):
    it = warp.fields(it)
    return tensors.warped_tensors(D, it[1:5], it[5:7], (it[8], it[9], it[14], it[10], it[11], it[15]), it[7], it[12], tensors.PLAIN, tensors.fmt(td, tensors.HW_ID24))


def test_the_warp_with_nearest_and_vote2(api, ctx, idpack):
    p = idpack
    rect = (3, 2, 41, 27)
    items = []
    for o in range(1, 9):
        it = warp.fields(api.warp_orient(48, 32, 4, rect, o))
        assert it == warp.orient(48, 32, rect, o)
        items.append(it[:7] + (it[7] | warp.NEAREST,) + it[8:])
    got = run_ids(ctx, p, "warp", 4, items, tensors.I64)
    upright = p.ids[2:29, 3:44]
    for o, (it, g) in enumerate(zip(items, got), start=1):
        assert np.array_equal(g, warp_model(p.B, it, tensors.I64)), o
        assert g.shape == ((41, 27) if o >= 5 else (27, 41)) and np.array_equal(np.unique(g), np.unique(upright)), o
    assert np.array_equal(got[0], upright) and np.array_equal(got[2], upright[::-1, ::-1]) and np.array_equal(got[4], upright.T)
    # the vote over 2 x 2 sub-samples of a reducing, turned map; and as I32
    m = warp.rotation((41, 27), (20, 14), 30.0, 0.5)
    votes = [warp.item(0, rect, (20, 14), m, warp.VOTE2), warp.item(0, (0, 0, 48, 32), (24, 16), (2 * warp.ONE, 0, 0, 0, 2 * warp.ONE, 0), warp.VOTE2)]
    for td in (tensors.I64, tensors.I32):
        got = run_ids(ctx, p, "warp", 4, votes, td)
        for it, g in zip(votes, got):
            assert np.array_equal(g, warp_model(p.B, it, td)), (td, it)
    assert set(np.unique(got[1])) <= set(np.unique(p.ids))


def test_a_bilinear_case_is_a_pure_function_of_the_bytes(ctx, idpack):
    """an averaged id is no id - but the element is r | g << 8 | b << 16 of whatever pixel the underlying call gives"""
    p = idpack
    items = [(0, 1, 1, 45, 30, 17, 11, 1), (2, 0, 0, 13, 11, 20, 9, 0)]
    for td in (tensors.I64, tensors.I32):
        got = run_ids(ctx, p, tensors.FILTER_BILINEAR, 4, items, td)
        for it, g in zip(items, got):
            D = p.B if it[0] == 0 else p.A
            P = tensors.tensors(D, it[1:5], it[5:7], it[7], tensors.FILTER_BILINEAR, tensors.PLAIN, tensors.fmt())
            want = P[:, :, 0].astype(np.int64) | P[:, :, 1].astype(np.int64) << 8 | P[:, :, 2].astype(np.int64) << 16
            assert np.array_equal(g, want) and np.array_equal(g, tensors.convert(P, tensors.fmt(td, tensors.HW_ID24))), (td, it)


def test_alpha_is_ignored(ctx, idpack):
    p = idpack
    assert (p.A[:, :, 3] != 255).all()
    want = p.A[:, :, 0].astype(np.int64) | p.A[:, :, 1].astype(np.int64) << 8 | p.A[:, :, 2].astype(np.int64) << 16
    items = [(2, 0, 0, 13, 11, 13, 11, 0)]
    for channels in (3, 4):
        for td in (tensors.I64, tensors.I32):
            assert np.array_equal(run_ids(ctx, p, tensors.FILTER_NEAREST, channels, items, td)[0], want), (channels, td)
    it = warp.item(2, (0, 0, 13, 11), (13, 11), flags=warp.NEAREST)
    for channels in (3, 4):
        assert np.array_equal(run_ids(ctx, p, "warp", channels, [it], tensors.I64)[0], want), channels


# ------------------------------------------------------------------ 5: no rejected call launches anything
def test_rejections_on_a_live_context_launch_nothing(ctx, oracle, planes, idpack):
    import torch
    dtype, src = planes
    good = copy_tiles(src)[:3]
    _, streams = model(oracle, src, good, 0, tiles.PLAIN)
    run(ctx, src, good, 0, tiles.PLAIN, 1, streams)
    stats = ctx.tile_stats()
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.full((4,), -1, dtype=torch.int64, device="cuda"), torch.full((3,), -1, dtype=torch.int32, device="cuda")
    before = src.host.copy()
    lab = src.flags[5]
    cases = [(tiles.NEAREST, [(5, 0, 0, 37, 29, 2, tiles.LABELS_ID24)], "without QOIMI_TILE_LABELS"),                               # bit 15 without LABELS
             (tiles.NEAREST, [(5, 0, 0, 37, 29, 2, lab & ~tiles.LABELS)], "without QOIMI_TILE_LABELS"),
             (tiles.NEAREST, [(5, 0, 0, 37, 29, 2, lab), (5, 0, 0, 1, 1, 1, lab & ~tiles.LABELS_ID24)], "two different label"),     # one image, with and without the bit
             (tiles.NEAREST, [(5, 0, 0, 1, 1, 1, lab & ~tiles.LABELS_ID24), (6, 0, 0, 8, 8, 1, src.flags[6]), (5, 0, 0, 37, 29, 2, lab)], "two different label"),
             (tiles.PLAIN, [(5, 0, 0, 37, 29, 2, lab)], "never averaged"),
             (tiles.NEAREST, [(5, 0, 0, 37, 29, 2, lab | 1 << 14)], "unknown flag bit")]
    for mode, ts, word in cases:
        with pytest.raises(Exception) as e:
            ctx.encode_tiles(src.d.data_ptr(), src.off, src.descs, 0, ts, mode, 1, buf.data_ptr(), 4096, d_off.data_ptr(), d_len.data_ptr())
        assert word in str(e.value), (mode, ts, str(e.value))
        assert (buf.cpu().numpy() == FILL).all() and (d_off.cpu().numpy() == -1).all() and (d_len.cpu().numpy() == -1).all()
        assert ctx.tile_stats() == stats, word
    assert np.array_equal(src.d.cpu().numpy(), before)
    # the layout with each float dtype and with U8
    p = idpack
    out = filled(4096, GUARD)
    item = [(0, 0, 0, 48, 32, 4, 4, 0)]
    run_ids(ctx, p, tensors.FILTER_NEAREST, 4, item, tensors.I64)
    tstats = ctx.tensor_stats()
    for td in (tensors.U8, tensors.F16, tensors.BF16, tensors.F32):
        for warped in (False, True):
            with pytest.raises(Exception) as e:
                if warped:
                    ctx.decode_warped_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [warp.item(0, (0, 0, 48, 32), (4, 4), flags=warp.NEAREST)], tensors.PLAIN,
                                              (td, tensors.HW_ID24, np.ones(4, np.float32), np.zeros(4, np.float32)), out.data_ptr(), [0], 0)
                else:
                    ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, item, tensors.FILTER_NEAREST, tensors.PLAIN,
                                       (td, tensors.HW_ID24, np.ones(4, np.float32), np.zeros(4, np.float32)), out.data_ptr(), [0], 0)
            assert "ID24" in str(e.value), (td, warped, str(e.value))
            assert (out.cpu().numpy() == GUARD).all() and ctx.tensor_stats() == tstats, (td, warped)


# ------------------------------------------------------------------ 6: the tools
def test_the_two_tool_options(ref, port, tmp_path):
    from tools import qoifromlabels_mi355x as fromlabels, qoitensor_mi355x as totensor
    enc = ref or port
    rng = np.random.default_rng(91)
    a = rng.integers(0, ID_MAX + 1, size=(11, 16)).astype(np.int32)
    a[2:6, 3:9] = 70000
    a[0, 0], a[10, 15], a[5, 5] = -3, 2 ** 24, 2 ** 31 - 1
    np.save(tmp_path / "ids.npy", a)
    said = []
    assert fromlabels.main([str(tmp_path / "ids.npy"), "-o", str(tmp_path / "q"), "--ids"], out=said.append) == 0, said
    want = tiles.tile(a, (0, 0, 0, 16, 11, 1, tiles.label_flags(tiles.L_I32, ids=True)), 3)
    assert (tmp_path / "q" / "0000.qoi").read_bytes() == enc.encode(want.reshape(-1), 16, 11, 3, 0)
    assert "3 elements outside 0..16777215 saturated" in said[-1], said[-1]
    assert fromlabels.main([str(tmp_path / "ids.npy"), "-o", str(tmp_path / "g")], out=said.append) == 0 and "outside 0..255 saturated" in said[-1]
    assert totensor.main([str(tmp_path / "q"), "--size", "16x11", "-o", str(tmp_path / "back.npy"), "--filter", "nearest", "--dtype", "i64", "--layout", "id24"], out=said.append) == 0, said
    back = np.load(tmp_path / "back.npy")
    assert back.shape == (1, 11, 16) and back.dtype == np.int64 and np.array_equal(back[0], np.clip(a, 0, ID_MAX).astype(np.int64))
    assert totensor.main([str(tmp_path / "q"), "--size", "8x5", "-o", str(tmp_path / "small.npy"), "--filter", "mode", "--dtype", "i32", "--layout", "id24", "--fit", "crop"], out=said.append) == 0
    small = np.load(tmp_path / "small.npy")
    assert small.shape == (1, 5, 8) and small.dtype == np.int32 and set(np.unique(small)) <= set(np.unique(np.clip(a, 0, ID_MAX)))
    assert totensor.main([str(tmp_path / "q"), "--size", "8x5", "-o", str(tmp_path / "no.npy"), "--dtype", "f32", "--layout", "id24"], out=said.append) == 2 and "i32 or i64" in said[-1]
    assert not (tmp_path / "no.npy").exists()
