"""qoimi_pixel_stats on the GPU (-m gpu): per-rectangle pixel statistics of a pack's images through bounded staging.  The expectation is always
the definition: the oracle decodes the stream as it is given (whole, cut, with a foreign end marker) at 4 channels, and qoi_amd/pixelstats.py:
stats / hist reduce that.  Every comparison is exact.  The histograms stand between guard bytes (0xA5) that are checked after every call.
Sub-batch boundaries are forced through staging_bytes by qoi_amd/pixelstats.py: plan (qoimi_pixel_stats_counters says that the call really ran
that many sub-batches over that much staging)."""
import numpy as np
import pytest

from qoi_amd import pixelstats as ps
from gpu_calls import standard_crops as standard
from gpu_pack import GUARD, KINDS, MIXED_SHAPES, Batch, Pack, dev, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BIG = 7                               # 130 x 70 x 4, sprite_alpha
T = ps.TILE_PX


@pytest.fixture(scope="module")
def mixed(api, ctx, oracle):
    """3 and 4 channels, all content classes"""
    kinds = [KINDS[(i + 2) % 5] for i in range(len(MIXED_SHAPES))]
    assert set(kinds) == set(KINDS) and MIXED_SHAPES[BIG] == (130, 70, 4) and {s[2] for s in MIXED_SHAPES} == {3, 4}
    return Pack(ctx, oracle, Batch(api, oracle, MIXED_SHAPES, kinds))


class OraclePack(Pack):
    """Given pixels as the oracle's streams, one behind the other in one device buffer; decoded(): tests/gpu_pack.py: Pack."""

    def __init__(self, api, oracle, shapes, pixels):
        self.oracle, self.n, self.shapes = oracle, len(shapes), shapes
        streams = [oracle.encode(np.ascontiguousarray(p, dtype=np.uint8).reshape(-1), w, h, ch) for p, (w, h, ch) in zip(pixels, shapes)]
        self.descs = [api.QoiDesc(w, h, ch, 0) for (w, h, ch) in shapes]
        self.sizes = [len(s) for s in streams]
        self.so = [int(x) for x in np.cumsum([3] + [n + 1 for n in self.sizes[:-1]])]
        self.host = np.zeros(self.so[-1] + self.sizes[-1] + 64, dtype=np.uint8)
        for o, s in zip(self.so, streams):
            self.host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.packed = dev(self.host)
        self._decoded = {}


def run(ctx, p, regions, hist=False, staging=0, sizes=None, packed=None, descs=None):
    """One call -> (the results as pixelstats.stats gives them, uint32[n, 4, 256] or None).  The histograms stand behind 64 and in front of
    64 guard bytes."""
    n = len(regions)
    buf = filled(64 + n * 4096 + 64, GUARD) if hist else None
    got = ctx.pixel_stats((p.packed if packed is None else packed).data_ptr(), p.so, p.sizes if sizes is None else sizes,
                          p.descs if descs is None else descs, regions, buf.data_ptr() + 64 if hist else 0, staging)
    assert len(got) == n and all(list(s.reserved) == [0, 0, 0, 0] for s in got)
    if not hist:
        return [ps.of_struct(s) for s in got], None
    host = buf.cpu().numpy()
    assert np.all(host[:64] == GUARD) and np.all(host[-64:] == GUARD), "a byte beside the histograms was written"
    return [ps.of_struct(s) for s in got], host[64:-64].view(np.uint32).reshape(n, 4, 256)


def want(p, r, **how):
    return ps.stats(p.decoded(r[0], 4, **how), r)


def assert_stats(p, got, hists, regions, what, **how):
    for j, r in enumerate(regions):
        w = want(p, r, **how)
        assert got[j] == w, (what, j, r, {k: (got[j][k], w[k]) for k in w if got[j][k] != w[k]})
        if hists is not None:
            assert np.array_equal(hists[j], ps.hist(p.decoded(r[0], 4, **how), r)), (what, j, r)


def staging_for(p, regions, subs):
    """a staging_bytes with which the plan has `subs` sub-batches"""
    slots = ps.plan(p.descs, regions, 0)[1]
    for s in sorted({int(x) for x in np.cumsum(slots)} | set(slots)):
        if len(ps.plan(p.descs, regions, s)[2]) == subs:
            return s
    raise AssertionError("no such staging")


# ------------------------------------------------------------------ 1: the mixed pack
@pytest.mark.parametrize("hist", [False, True])
def test_mixed_pack(ctx, mixed, hist):
    p = mixed
    regions = [r for i, (w, h, _) in enumerate(p.shapes) for r in standard(i, w, h, i)]
    assert {r[5] for r in regions} == {0, 1, 2, 3} and any(r[1] % 2 and r[2] % 2 and r[3] % 2 and r[4] % 2 for r in regions)
    single, hists = run(ctx, p, regions, hist)
    assert_stats(p, single, hists, regions, ("mixed", hist))
    images, slots, subs, largest = ps.plan(p.descs, regions, 0)
    assert ctx.pixel_stats_counters() == (1, 1, largest, p.n) and largest == sum(slots)
    # a 3-channel stream is opaque: alpha 255 everywhere
    for j, r in enumerate(regions):
        if p.shapes[r[0]][2] == 3:
            assert single[j]["flags"] & ps.OPAQUE and single[j]["sum"][3] == 255 * single[j]["pixels"] and single[j]["min"][3] == 255
    assert any(not s["flags"] & ps.OPAQUE for s in single) and any(s["transparent_pixels"] for s in single)
    for staging in (staging_for(p, regions, 2), 1):
        images, slots, subs, largest = ps.plan(p.descs, regions, staging)
        assert len(subs) == (2 if staging > 1 else p.n)
        got, h2 = run(ctx, p, regions, hist, staging=staging)
        assert ctx.pixel_stats_counters() == (len(subs), len(subs), largest, p.n), (staging, ctx.pixel_stats_counters())
        assert got == single and (hists is None or np.array_equal(h2, hists)), staging


# ------------------------------------------------------------------ 2: tile edges
def rect_of(n, w, h):
    """(cw, ch) with cw * ch == n inside w x h"""
    return next((cw, n // cw) for cw in range(w, 0, -1) if n % cw == 0 and n // cw <= h)


@pytest.mark.parametrize("hist", [False, True])
def test_tile_edges(ctx, mixed, hist):
    """regions of exactly TILE_PX - 1, TILE_PX and TILE_PX + 1 pixels, and the whole image: several tiles, so several workgroups add into one
    result"""
    p = mixed
    shapes = [rect_of(n, 130, 70) for n in (T - 1, T, T + 1)]
    assert [cw * ch for cw, ch in shapes] == [T - 1, T, T + 1] and ps.tiles(130, 70) >= 3
    regions = [(BIG, 130 - cw - k, 70 - ch, cw, ch, k) for k, (cw, ch) in enumerate(shapes)] + [(BIG, 0, 0, 130, 70, 3)]
    assert [ps.tiles(r[3], r[4]) for r in regions[:3]] == [1, 1, 2]
    got, hists = run(ctx, p, regions, hist)
    assert_stats(p, got, hists, regions, ("edges", hist))
    alone, h1 = run(ctx, p, regions[3:], hist)                      # one table entry, one workgroup per tile
    assert alone == got[3:] and (hists is None or np.array_equal(h1[0], hists[3]))


# ------------------------------------------------------------------ 3: many entries per workgroup
def test_many_small_regions(api, ctx, oracle):
    """640 regions of 1 x 1 and 2 x 1 over a 64 x 48 image in one call: every tile is another region, a workgroup flushes at every step"""
    import torch
    p = Pack(ctx, oracle, Batch(api, oracle, [(64, 48, 4)], ["noise"]))
    n = max(640, 8 * torch.cuda.get_device_properties(0).multi_processor_count * 2 + 37)
    regions = [(0, j % 63, (j // 63) % 48, 1 + (j & 1), 1, j & 3) for j in range(n)]
    assert n >= 600 and {r[3] for r in regions} == {1, 2}
    for hist in (False, True):
        got, hists = run(ctx, p, regions, hist)
        assert_stats(p, got, hists, regions, ("many", hist))
        assert ctx.pixel_stats_counters()[:2] == (1, 1)
        if hist:
            assert all(int(hists[j, c].sum()) == regions[j][3] for j in range(n) for c in range(4))


# ------------------------------------------------------------------ 4: regions that share pixels
def test_coinciding_and_overlapping_regions(ctx, mixed):
    p = mixed
    same = (BIG, 10, 5, 101, 37)
    regions = [same + (0,), (BIG, 0, 0, 130, 70, 0), same + (0,), (BIG, 50, 20, 80, 50, 1), same + (3,), (BIG, 10, 5, 100, 37, 0), (BIG, 11, 5, 101, 37, 2)]
    got, hists = run(ctx, p, regions, True)
    assert_stats(p, got, hists, regions, "shared")
    assert got[0] == got[2] and {k: v for k, v in got[4].items() if k != "first"} == {k: v for k, v in got[0].items() if k != "first"}
    assert np.array_equal(hists[0], hists[2]) and np.array_equal(hists[0], hists[4])
    assert len({g["pixels"] for g in (got[0], got[1], got[3], got[5])}) == 4 and got[1]["sum"] != got[0]["sum"]


# ------------------------------------------------------------------ 5: the flags
def test_flags(api, ctx, oracle):
    """40 x 30: a full tile and a partial one whose last lane holds the image's last pixel"""
    rng = np.random.default_rng(3)
    w, h = 40, 30
    assert T < w * h < 2 * T and (w * h) % 4 == 0
    constant = np.tile(np.array([7, 200, 31, 128], dtype=np.uint8), (h, w, 1))
    last = constant.copy(); last[-1, -1, 2] = 32
    clear = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8); clear[..., 3] = 0
    opaque1 = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8); opaque1[..., 3] = 255; opaque1[h // 2, w // 2, 3] = 254
    grey1 = np.repeat(rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8), 4, axis=2); grey1[..., 3] = rng.integers(1, 255, size=(h, w)); grey1[7, 9, 1] ^= 1
    white = np.full((h, w, 4), 255, dtype=np.uint8)
    pixels = [constant, last, clear, opaque1, grey1, white]
    p = OraclePack(api, oracle, [(w, h, 4)] * len(pixels), pixels)
    for i, px in enumerate(pixels):
        assert np.array_equal(p.decoded(i, 4), px)
    regions = [(i, 0, 0, w, h, i & 3) for i in range(len(pixels))]
    got, hists = run(ctx, p, regions, True)
    assert_stats(p, got, hists, regions, "flags")
    assert [g["flags"] for g in got] == [ps.CONSTANT, 0, ps.TRANSPARENT, 0, 0, ps.CONSTANT | ps.OPAQUE | ps.GREY]
    assert got[3]["opaque_pixels"] == w * h - 1 and got[4]["grey_pixels"] == w * h - 1 and got[1]["max"][2] == 32 and got[1]["min"][2] == 31
    # without the one pixel each flag holds
    regions = [(1, 0, 0, w, h - 1, 0), (3, 0, 0, w, h // 2, 0), (4, 0, 8, w, h - 8, 0)]
    got, _ = run(ctx, p, regions)
    assert_stats(p, got, None, regions, "flags without the pixel")
    assert [g["flags"] for g in got] == [ps.CONSTANT, ps.OPAQUE, ps.GREY]


# ------------------------------------------------------------------ 6: leniency
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
    regions = [(cut, 3, 31, 55, 17, 1), (cut, 0, 0, 64, 48, 0), (marker, 1, 12, 35, 11, 2), (marker, 0, 0, 37, 23, 3), (BIG, 0, 35, 130, 35, 0)]
    got, hists = run(ctx, p, regions, True, sizes=sizes, packed=damaged)
    for j, r in enumerate(regions):
        how = {"size": sizes[cut]} if r[0] == cut else {"host": host} if r[0] == marker else {}
        assert got[j] == want(p, r, **how), j
        assert np.array_equal(hists[j], ps.hist(p.decoded(r[0], 4, **how), r)), j
    assert np.array_equal(damaged.cpu().numpy(), host)


# ------------------------------------------------------------------ 7: a rejected call, then a good one
def test_the_context_stays_usable(api, ctx, mixed):
    p = mixed
    good = [(BIG, 3, 5, 11, 7, 3), (0, 0, 0, 1, 1, 0)]
    with pytest.raises(api.QoiError):
        ctx.pixel_stats(p.packed.data_ptr(), p.so, p.sizes, p.descs, good + [(BIG, 121, 0, 10, 10, 0)])
    assert "leaves" in api.last_error()
    with pytest.raises(api.QoiError):
        ctx.pixel_stats(p.packed.data_ptr(), p.so, p.sizes, p.descs, [(BIG, 0, 0, 1, 1, 4)])
    got, hists = run(ctx, p, good, True)
    assert_stats(p, got, hists, good, "after a rejection")


# ------------------------------------------------------------------ 8: unreferenced images
def test_unreferenced_images_are_not_looked_at(api, ctx, mixed):
    p = mixed
    sizes, descs = list(p.sizes), list(p.descs)
    for i in (1, 4):
        sizes[i] = 0
        descs[i] = api.QoiDesc(0, 0, 9, 9)
    regions = [r for i in (0, 2, 3, 5, 6, 7) for r in standard(i, p.shapes[i][0], p.shapes[i][1], i)]
    got, _ = run(ctx, p, regions, sizes=sizes, descs=descs)
    assert_stats(p, got, None, regions, "unreferenced")
    assert ctx.pixel_stats_counters()[3] == 6
