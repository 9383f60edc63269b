"""qoimi_seek_index_from_pixels on the GPU (-m gpu): one call over oracle-encoded images - packed at odd offsets, their pixels between fill bytes
at offsets congruent to 0, 1, 2 and 3 mod 4 for both channel counts - gives the points of qoi_amd/seekindex.py: points_from_pixels field for
field and those of qoimi_build_seek_index byte for byte, leaves pixels and pack as they were, and its index decodes crops in every image's last
band.  Intervals of two tiles and a tail, of less than a tile, equal neighbours across lane 63, the 256-thread step and the interval edge, a
colour last seen many intervals back, an image without a point in the middle.  A stream of other pixels; rejections; the workspace."""
import ctypes

import numpy as np
import pytest

from qoi_amd import seekindex as si
from seek_cases import Case, DevicePack, cases
from gpu_pack import E_ARG, GUARD, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
PIXEL_FILL = 0xC3


def my_cases(oracle):
    shared = {c.name: c for c in cases(oracle)}
    rng = np.random.default_rng(77)
    wide = rng.integers(0, 256, size=129 * 40 * 3, dtype=np.uint8)           # an interval of 2064 pixels: two tiles and a tail; 40 = 2 * 16 + 8
    alpha = rng.integers(0, 4, size=77 * 23 * 4, dtype=np.uint8) * 85          # few values per channel: INDEX chunks, short runs, alpha changes
    stripes = np.repeat((np.arange(-(-300 * 30 // 70)) % 5 * 50 + 3).astype(np.uint8), 70)[:300 * 30, None].repeat(4, axis=1)   # constant stripes 70 pixels wide
    out = [shared["noise96"],
           Case("wide129", oracle.encode(wide, 129, 40, 3), 129, 40, 3, 16, oracle),
           shared["w1"], shared["w63"],
           shared["no_point"],                                              # ... in the middle of the call
           shared["w64"], shared["w65"], shared["old_colour"],
           Case("stripes", oracle.encode(stripes, 300, 30, 4), 300, 30, 4, 5, oracle),
           Case("alpha77", oracle.encode(alpha, 77, 23, 4), 77, 23, 4, 4, oracle)]  # (a fourth 4-channel image with points: every offset mod 4 is read)
    assert [len(c.points) for c in out] == [47, 2, 3, 6, 0, 6, 6, 29, 5, 5] and any(c.h % c.K for c in out)
    return out


class Pixels:
    """The cases' pixels (what their streams decode to, at their own channel count) on the device between fill bytes: the k-th image of a
    channel count THAT HAS A POINT - the kernels read no other - stands at an offset congruent to k mod 4."""

    def __init__(self, the_cases):
        import torch
        self.offsets, pos, seen = [], 64, {3: 0, 4: 0}
        for c in the_cases:
            pos += (seen[c.ch] - pos) % 4
            seen[c.ch] += 1 if len(c.points) else 0
            self.offsets.append(pos)
            pos += c.w * c.h * c.ch + 5
        for ch in (3, 4):
            assert {o % 4 for o, c in zip(self.offsets, the_cases) if c.ch == ch and len(c.points)} == {0, 1, 2, 3}
        host = np.full(pos + 64, PIXEL_FILL, dtype=np.uint8)
        for o, c in zip(self.offsets, the_cases):
            host[o:o + c.w * c.h * c.ch] = c.full[c.ch].reshape(-1)
        self.host = host
        self.dev = torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def pack(api, oracle):
    p = DevicePack(api, my_cases(oracle))
    p.pixels = Pixels(p.cases)
    return p


def from_pixels(c, p, **kw):
    return c.seek_index_from_pixels(p.pixels.dev.data_ptr(), p.pixels.offsets, p.dev.data_ptr(), p.offsets, p.sizes, p.descs, p.intervals, **kw)


def test_points_equal_the_model_and_the_decode_based_build(ctx, pack):
    got, firsts = from_pixels(ctx, pack)
    assert ctx.seek_stats()[0] == 0
    # (a) the model, field for field
    assert firsts == pack.point_firsts and got.size == pack.points.size
    for c, first in zip(pack.cases, firsts):
        want = si.points_from_pixels(c.stream, c.w, c.h, c.K, c.full[c.ch], c.ch)
        assert want.tobytes() == c.points.tobytes()                          # (the stream decodes to these pixels)
        mine = got[first:first + len(want)]
        for field in ("byte_off", "skip", "prev", "reserved", "table"):
            bad = np.flatnonzero([not np.array_equal(a[field], b[field]) for a, b in zip(mine, want)])
            assert bad.size == 0, (c.name, field, int(bad[0]), mine[int(bad[0])][field], want[int(bad[0])][field])
    # (b) qoimi_build_seek_index over the same pack, byte for byte
    built, built_firsts = ctx.build_seek_index(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, pack.intervals)
    assert built_firsts == firsts and built.tobytes() == got.tobytes() and ctx.seek_stats()[0] == 1
    # (c) nothing of the caller's was written
    assert np.array_equal(pack.pixels.dev.cpu().numpy(), pack.pixels.host) and np.array_equal(pack.dev.cpu().numpy(), pack.host)
    # (d) a crop in the last band of each image through that index
    cs = [(i, 0, len(c.points) * c.K, c.w, c.h - len(c.points) * c.K, i % 4) for i, c in enumerate(pack.cases)]
    nbytes = [c[3] * c[4] * 4 for c in cs]
    offsets = [64 + int(x) + 3 * j for j, x in enumerate(np.cumsum([0] + nbytes[:-1]))]
    plain, indexed = filled(offsets[-1] + nbytes[-1] + 64, GUARD), filled(offsets[-1] + nbytes[-1] + 64, GUARD)
    ctx.decode_crops(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, 4, cs, plain.data_ptr(), offsets)
    ctx.decode_crops_indexed(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, 4, cs, indexed.data_ptr(), offsets, pack.intervals, got, firsts)
    assert bool((plain == indexed).all()) and ctx.seek_stats()[1] == len(pack.cases)
    host = plain.cpu().numpy()
    for c, crop, o, nb in zip(pack.cases, cs, offsets, nbytes):
        want = c.full[4][crop[2]:, ::-1 if crop[5] & 1 else 1][::-1 if crop[5] & 2 else 1]
        assert np.array_equal(host[o:o + nb], want.reshape(-1)), c.name


def test_one_image_and_an_image_without_points(ctx, pack):
    i = [c.name for c in pack.cases].index("no_point")
    got, firsts = ctx.seek_index_from_pixels(pack.pixels.dev.data_ptr(), [pack.pixels.offsets[i]], pack.dev.data_ptr(), [pack.offsets[i]], [pack.sizes[i]],
                                             [pack.descs[i]], [pack.intervals[i]])
    assert got.size == 0 and firsts == [0]
    for j, c in enumerate(pack.cases):
        if c.name in ("wide129", "stripes"):
            got, _ = ctx.seek_index_from_pixels(pack.pixels.dev.data_ptr(), [pack.pixels.offsets[j]], pack.dev.data_ptr(), [pack.offsets[j]], [pack.sizes[j]],
                                                [pack.descs[j]], [c.K])
            assert got.tobytes() == c.points.tobytes(), c.name
    # another interval for the same image
    c = pack.cases[0]
    got, _ = ctx.seek_index_from_pixels(pack.pixels.dev.data_ptr(), [pack.pixels.offsets[0]], pack.dev.data_ptr(), [pack.offsets[0]], [pack.sizes[0]], [pack.descs[0]], [7])
    assert got.tobytes() == si.points(c.stream, c.w, c.h, 7, c.full[4]).tobytes() and got.size == 13


def test_a_stream_of_other_pixels(ctx, pack):
    """the stream of w63's neighbour handed in with other pixels of the same shape: byte_off / skip are the stream's, prev / table the pixels'"""
    names = [c.name for c in pack.cases]
    a = pack.cases[names.index("w65")]
    rng = np.random.default_rng(9)
    other = rng.integers(0, 256, size=(a.h, a.w, a.ch), dtype=np.uint8)
    import torch
    d_other = torch.from_numpy(np.concatenate([np.full(3, PIXEL_FILL, dtype=np.uint8), other.reshape(-1)])).cuda()
    i = names.index("w65")
    got, _ = ctx.seek_index_from_pixels(d_other.data_ptr(), [3], pack.dev.data_ptr(), [pack.offsets[i]], [pack.sizes[i]], [pack.descs[i]], [a.K])
    want = si.points_from_pixels(a.stream, a.w, a.h, a.K, other, a.ch)
    assert got.tobytes() == want.tobytes()
    for f in ("byte_off", "skip"):
        assert np.array_equal(got[f], a.points[f])
    assert not np.array_equal(got["table"], a.points["table"]) and not np.array_equal(got["prev"], a.points["prev"])
    assert np.array_equal(pack.dev.cpu().numpy(), pack.host)


def test_rejections_on_a_live_context(api, ctx, pack):
    lib = api.load_library()
    n = len(pack.cases)
    out = (api.QoimiSeekPoint * pack.points.size)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    before = bytes(out)

    def call(sizes=pack.sizes, descs=pack.descs, ks=pack.intervals, n_=n, points=out, px=pack.pixels.dev.data_ptr(), po=pack.pixels.offsets):
        return lib.qoimi_seek_index_from_pixels(ctx._h, px, (ctypes.c_size_t * n)(*po) if po is not None else None, pack.dev.data_ptr(), (ctypes.c_size_t * n)(*pack.offsets),
                                                (ctypes.c_int * n)(*sizes), (api.QoiDesc * n)(*descs), n_, (ctypes.c_uint * n)(*ks), points, None)

    assert call(sizes=[21] + pack.sizes[1:]) == E_ARG and "22" in api.last_error()
    assert call(descs=[api.QoiDesc(96, 96, 5, 0)] + pack.descs[1:]) == E_ARG
    assert call(ks=[1] + pack.intervals[1:]) == E_ARG and "128" in api.last_error()       # 1 * 96 < 128
    assert call(ks=[0] + pack.intervals[1:]) == E_ARG
    assert call(n_=0) == E_ARG and call(points=None) == E_ARG and call(px=None) == E_ARG and call(po=None) == E_ARG
    assert call(po=[2 ** 64 - pack.pixels.dev.data_ptr() - 5] + pack.pixels.offsets[1:]) == E_ARG and "pointer" in api.last_error()
    assert bytes(out) == before
    got, _ = from_pixels(ctx, pack)                                          # ... and the context goes on working
    assert got.tobytes() == pack.points.tobytes()


def test_no_staging_arena(api, oracle):
    """one 512 x 512 x 4 image on two fresh contexts: the decode-based build holds the staging arena - 512 * 512 * 4 bytes, the largest
    sub-batch plus a page, no slack - and a decoder's workspace on top of what the pixel-based build holds"""
    import torch
    w = h = 512
    rng = np.random.default_rng(3)
    px = (rng.integers(0, 6, size=(h, w, 1)) * 40 + np.arange(4)).astype(np.uint8)
    s = oracle.encode(px, w, h, 4)
    d_s, d_px = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda(), torch.from_numpy(px.reshape(-1)).cuda()
    descs = [api.QoiDesc(w, h, 4, 0)]
    a, b = api.Context(0), api.Context(0)
    try:
        got, _ = a.seek_index_from_pixels(d_px.data_ptr(), [0], d_s.data_ptr(), [0], [len(s)], descs, [16])
        built, _ = b.build_seek_index(d_s.data_ptr(), [0], [len(s)], descs, [16])
        assert got.tobytes() == built.tobytes() and got.size == 31
        print("decode workspace: from pixels", a.workspace_bytes()["decode"], "decode-based", b.workspace_bytes()["decode"])
        assert b.workspace_bytes()["decode"] - a.workspace_bytes()["decode"] >= w * h * 4
    finally:
        a.close()
        b.close()
