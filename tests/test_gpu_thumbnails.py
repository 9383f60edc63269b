"""qoimi_decode_thumbnails on the GPU (-m gpu): every image of a pack at 1/f of its size through bounded staging.  The expectation is always
the definition: the oracle decodes the stream as it is given (whole, cut, with a foreign end marker) at the call's output channel count,
and qoi_amd/thumbs.py: thumbnail reduces that.  Every comparison is exact.  Sub-batch boundaries are forced through staging_bytes by the plan
of qoi_amd/packplan.py over width * height * 4 (qoimi_thumbnail_stats says that the call really ran that many sub-batches)."""
import ctypes
import os

import numpy as np
import pytest

from qoi_amd import thumbs
from qoi_amd.thumbs import ALPHA_WEIGHTED, PLAIN
from gpu_calls import run_thumbnails as run, thumb_bytes
from gpu_pack import E_ARG, GUARD, KINDS, MIXED_SHAPES, Batch, Pack, batch_of, dev, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FACTORS = [2, 3, 4, 5, 7, 8, 16, 64]


@pytest.fixture(scope="module")
def mixed(api, ctx, oracle):
    """3 and 4 channels, all content classes (sprite_alpha at 130 x 70 x 4: transparent regions)"""
    kinds = [KINDS[(i + 2) % 5] for i in range(len(MIXED_SHAPES))]
    assert set(kinds) == set(KINDS) and kinds[7] == "sprite_alpha"
    return Pack(ctx, oracle, Batch(api, oracle, MIXED_SHAPES, kinds))


@pytest.fixture(scope="module")
def all_rgb(api, ctx, oracle):
    shapes = [(w, h, 3) for (w, h, _) in MIXED_SHAPES]
    return Pack(ctx, oracle, Batch(api, oracle, shapes, [KINDS[i % 5] for i in range(len(shapes))]))


@pytest.fixture(scope="module")
def equal(api, ctx, oracle):
    return Pack(ctx, oracle, Batch(api, oracle, [(64, 48, 4)] * 13, [KINDS[i % 5] for i in range(13)]))


def want(p, i, och, f, mode, **how):
    return thumbs.thumbnail(p.decoded(i, och, **how), f, mode).reshape(-1)


def assert_thumbs(p, got, och, factors, mode, what):
    for i in range(p.n):
        w = want(p, i, och, factors[i], mode)
        assert got[i].size == w.size and np.array_equal(got[i], w), (what, i, p.shapes[i], factors[i], int(np.argmax(got[i] != w)))


# ------------------------------------------------------------------ 1: f == 1 is the decode
@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_identity(ctx, mixed, mode):
    p = mixed
    got, _, _ = run(ctx, p, 4, 1, mode)
    sizes = [w * h * 4 for (w, h, _) in p.shapes]
    po = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    full = filled(sum(sizes), GUARD)
    ctx.decode_images(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, full.data_ptr(), po)
    full = full.cpu().numpy()
    for i in range(p.n):
        assert np.array_equal(got[i], full[po[i]:po[i] + sizes[i]]), (mode, i)
        assert np.array_equal(got[i], p.decoded(i, 4).reshape(-1)), (mode, i)
    assert ctx.thumbnail_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 2: factors and modes
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_factors_and_modes(ctx, mixed, channels, mode):
    """every image meets every factor of the cycle: partial edge blocks, w < f, h < f, 1 x 1 at 64"""
    p = mixed
    for r in range(len(FACTORS)):
        factors = [FACTORS[(i + r) % len(FACTORS)] for i in range(p.n)]
        got, _, _ = run(ctx, p, channels, factors, mode)
        assert_thumbs(p, got, channels, factors, mode, (channels, mode, r))


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_all_rgb_with_the_headers_channels(ctx, all_rgb, mode):
    p = all_rgb
    for r in (0, 3, 5):
        factors = [FACTORS[(i + r) % len(FACTORS)] for i in range(p.n)]
        got, _, _ = run(ctx, p, 0, factors, mode)
        assert [g.size for g in got] == thumb_bytes(p.shapes, factors, 3)
        assert_thumbs(p, got, 3, factors, mode, ("rgb", mode, r))


def test_the_weighted_mode_is_not_the_plain_one(ctx, mixed):
    """the sprite (alpha 0 around it) and the noise images (random alpha): the two modes differ on the device as they do in the model"""
    p = mixed
    factors = [4] * p.n
    plain, _, _ = run(ctx, p, 4, factors, PLAIN)
    weighted, _, _ = run(ctx, p, 4, factors, ALPHA_WEIGHTED)
    assert not np.array_equal(plain[7], weighted[7]) and not np.array_equal(want(p, 7, 4, 4, PLAIN), want(p, 7, 4, 4, ALPHA_WEIGHTED))
    assert_thumbs(p, plain, 4, factors, PLAIN, "plain")
    assert_thumbs(p, weighted, 4, factors, ALPHA_WEIGHTED, "weighted")
    # with 3 output channels the weighted mode IS the plain one (the staged alpha of the 4-channel streams takes no part)
    a, _, _ = run(ctx, p, 3, factors, PLAIN)
    b, _, _ = run(ctx, p, 3, factors, ALPHA_WEIGHTED)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 3: extremes
def test_extremes(api, ctx, oracle):
    """the largest sums (64 x 64 of 0xFFFFFFFF in one block) and blocks without any alpha beside opaque ones"""
    rng = np.random.default_rng(9)
    white = np.full((64, 64, 4), 255, dtype=np.uint8)
    half = rng.integers(0, 256, size=(64, 128, 4), dtype=np.uint8)
    half[:, :64, 3] = 0
    half[:, 64:, 3] = rng.choice(np.array([1, 255, 255, 200], dtype=np.uint8), size=(64, 64))
    p = Pack(ctx, oracle, batch_of(api, oracle, [(64, 64, 4), (128, 64, 4)], [white, half]))
    assert np.array_equal(p.decoded(0, 4), white) and np.array_equal(p.decoded(1, 4), half)
    for f in (64, 2):
        got, _, _ = run(ctx, p, 4, f, ALPHA_WEIGHTED)
        assert_thumbs(p, got, 4, [f, f], ALPHA_WEIGHTED, f)
        assert np.all(got[0] == 255)
    got, _, _ = run(ctx, p, 4, 64, ALPHA_WEIGHTED)
    left = got[1][:4]
    assert left[3] == 0 and np.array_equal(left, thumbs.thumbnail(half[:, :64], 64, PLAIN).reshape(-1))      # all transparent: the plain value


def test_more_tiles_than_the_grid(api, ctx, oracle):
    """(qoi_dev.h: walk_tiles) more tiles than the grid's clamp of 8 workgroups per compute unit - 37 more images of 1 x 1, one tile each - so
    that a workgroup takes two tiles and steps from image to image.  (One entry in a launch: test_sub_batches; an image of 36 tiles over as
    many workgroups: test_identity.)"""
    import torch
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    px = np.random.default_rng(11).integers(0, 256, size=(n, 4), dtype=np.uint8)
    p = Pack(ctx, oracle, batch_of(api, oracle, [(1, 1, 4)] * n, list(px)))
    for channels, mode in ((3, PLAIN), (4, ALPHA_WEIGHTED)):
        got, _, _ = run(ctx, p, channels, 1, mode)
        assert np.array_equal(np.concatenate(got), px[:, :channels].reshape(-1)), (channels, mode)
        assert_thumbs(p, got, channels, [1] * n, mode, ("many", channels))
        assert ctx.thumbnail_stats()[:2] == (1, 1)


# ------------------------------------------------------------------ 4: sub-batches
def test_sub_batches(api, ctx, equal):
    from qoi_amd.packplan import plan, slot
    p = equal
    slots4 = [w * h * 4 for (w, h, _) in p.shapes]
    one = slot(64 * 48 * 4)
    factors = [4] * p.n
    # the decoder's own workspace first: the sub-batches of every plan below as plain decode_images calls on a context of its own
    c = api.Context(0)
    try:
        stagings = (one, 3 * one, 3 * one + 1, 13 * one, 0)
        full = filled(sum(slots4), 0)
        for staging in stagings:
            for first, count in plan(slots4, staging if staging else 1 << 30):
                ctx_so, ctx_sz = p.so[first:first + count], p.sizes[first:first + count]
                c.decode_images(p.packed.data_ptr(), ctx_so, ctx_sz, p.descs[first:first + count], 4, full.data_ptr(), [k * slots4[0] for k in range(count)])
        # ... and the arena of the image tables, which the compare and verify calls share with this one: a compare_images call of as many
        # images creates it (with the arenas' slack of a quarter and 1 MiB: far more than 13 entries of 48 bytes), so that from here on the
        # staging arena is the only one that can grow
        po = [k * slots4[0] for k in range(p.n)]
        c.compare_images(full.data_ptr(), po, 4, full.data_ptr(), po, 4, p.descs)
        before = c.workspace_bytes()["decode"]
        results = []
        # (the arena never shrinks; the largest sub-batch never does from one staging to the next either, so it holds this plan's and not an earlier one's)
        assert [max(count for _, count in plan(slots4, s if s else 1 << 30)) for s in stagings] == [1, 3, 3, 13, 13]
        for staging, subs in zip(stagings, (13, 5, 5, 1, 1)):
            the_plan = plan(slots4, staging if staging else 1 << 30)
            assert len(the_plan) == subs, (staging, the_plan)
            got, _, _ = run(c, p, 4, factors, PLAIN, staging=staging)
            stats = c.thumbnail_stats()
            assert stats[0] == stats[1] == subs, (staging, stats)
            largest = max(count for _, count in the_plan) * one
            assert stats[2] == largest and stats[3] == 0, (staging, stats)
            grown = c.workspace_bytes()["decode"] - before
            print("staging", staging, "sub-batches", subs, "largest", largest, "grown", grown)
            # the staging arena is this plan's largest sub-batch plus a page, with no slack; nothing else grows
            assert largest <= grown <= largest + 4096, (staging, grown, largest)
            results.append(got)
        assert_thumbs(p, results[0], 4, factors, PLAIN, "sub-batches")
        assert all(all(np.array_equal(x, y) for x, y in zip(r, results[0])) for r in results)
    finally:
        c.close()


# ------------------------------------------------------------------ 5: placement
def test_placement(api, ctx, mixed):
    p = mixed
    factors = [FACTORS[(i + 1) % len(FACTORS)] for i in range(p.n)]
    nbytes = thumb_bytes(p.shapes, factors, 4)
    # descending order, odd offsets, gaps of different odd / even sizes
    offsets, pos = [0] * p.n, 33
    for i in reversed(range(p.n)):
        offsets[i] = pos
        pos += nbytes[i] + (6, 1, 3)[i % 3]
    assert offsets[0] > offsets[5] and any(o % 2 for o in offsets) and any(o % 4 == 2 for o in offsets)
    got, _, _ = run(ctx, p, 4, factors, ALPHA_WEIGHTED, offsets=offsets, total=pos + 77)
    assert_thumbs(p, got, 4, factors, ALPHA_WEIGHTED, "placement")
    nbytes3 = thumb_bytes(p.shapes, factors, 3)
    got, _, _ = run(ctx, p, 3, factors, PLAIN, offsets=offsets, total=pos + 77)         # 3 bytes per pixel in the same places
    assert_thumbs(p, got, 3, factors, PLAIN, "placement, 3 channels")
    assert sum(nbytes3) < sum(nbytes)
    # image 0 in front of image 5, overlapping it by one byte: rejected, nothing written
    bad = list(offsets)
    bad[0] = offsets[5] - nbytes[0] + 1
    buf = filled(pos + 77, GUARD)
    with pytest.raises(api.QoiError):
        ctx.decode_thumbnails(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, factors, PLAIN, buf.data_ptr(), bad)
    lib = api.load_library()
    n = p.n
    rc = lib.qoimi_decode_thumbnails(ctx._h, p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n, 4,
                                     (ctypes.c_uint * n)(*factors), PLAIN, buf.data_ptr(), (ctypes.c_size_t * n)(*bad), 0, None)
    assert rc == E_ARG and "overlap" in api.last_error()
    assert bool((buf == GUARD).all())
    bad[0] -= 1                                                           # side by side: accepted
    got, _, _ = run(ctx, p, 4, factors, PLAIN, offsets=bad, total=pos + 77)
    assert_thumbs(p, got, 4, factors, PLAIN, "side by side")


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
    factors = [FACTORS[(i + 2) % len(FACTORS)] for i in range(p.n)]
    assert not np.array_equal(p.decoded(cut, 4, size=sizes[cut]), p.decoded(cut, 4))
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        got, _, _ = run(ctx, p, channels, factors, mode, sizes=sizes, packed=damaged)
        for i in range(p.n):
            how = {"size": sizes[cut]} if i == cut else {"host": host} if i == marker else {}
            w = want(p, i, channels, factors[i], mode, **how)
            assert np.array_equal(got[i], w), (channels, mode, i)
    assert np.array_equal(damaged.cpu().numpy(), host)


# ------------------------------------------------------------------ 7: mixed output channel counts
def test_mixed_output_channels_are_rejected(api, ctx, mixed):
    p = mixed
    lib = api.load_library()
    n = p.n
    buf = filled(131072, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    offs = (ctypes.c_size_t * n)(*[10000 * i for i in range(n)])
    assert {d.channels for d in p.descs} == {3, 4}
    assert lib.qoimi_decode_thumbnails(ctx._h, *args, 0, (ctypes.c_uint * n)(*([2] * n)), PLAIN, buf.data_ptr(), offs, 0, None) == E_ARG
    assert "channel" in api.last_error()
    assert lib.qoimi_decode_thumbnails(ctx._h, *args, 4, (ctypes.c_uint * n)(*([2] * (n - 1) + [65])), PLAIN, buf.data_ptr(), offs, 0, None) == E_ARG
    assert lib.qoimi_decode_thumbnails(ctx._h, *args, 4, (ctypes.c_uint * n)(*([2] * n)), 2, buf.data_ptr(), offs, 0, None) == E_ARG
    assert bool((buf == GUARD).all())
    assert lib.qoimi_decode_thumbnails(ctx._h, *args, 4, (ctypes.c_uint * n)(*([2] * n)), PLAIN, buf.data_ptr(), offs, 0, None) == 0


# ------------------------------------------------------------------ 8: the tool
def test_tool(api, oracle, tmp_path):
    from qoi_amd import synth
    from tools import png_io, qoithumb_mi355x
    images = {"a": (synth.frame_rgba("sprite_alpha", 130, 70, 0), 130, 70, 4), "b": (synth.frame_rgb("photo", 257, 9, 1), 257, 9, 3),
              "c": (synth.frame_rgba("photo", 64, 48, 2), 64, 48, 4)}
    src = tmp_path / "in"
    src.mkdir()
    for name, (px, w, h, ch) in images.items():
        assert api.qoi_write(str(src / (name + ".qoi")), px.reshape(-1), api.QoiDesc(w, h, ch, 0)) > 0
    lines = []
    for mode, flag in ((PLAIN, "plain"), (ALPHA_WEIGHTED, "weighted")):
        out_dir = tmp_path / flag
        assert qoithumb_mi355x.main([str(src), "--max-side", "40", "-o", str(out_dir), "--mode", flag], out=lines.append) == 0
        assert sorted(os.listdir(out_dir)) == ["a.png", "b.png", "c.png"]
        for name, (px, w, h, ch) in images.items():
            f = thumbs.factor_for(w, h, 40)
            assert f == {"a": 4, "b": 7, "c": 2}[name]
            decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 4)      # a pack with a 4-channel file comes out at 4 channels
            got, gw, gh = png_io.read_png((out_dir / (name + ".png")).read_bytes(), 4)
            assert (gw, gh) == thumbs.size(w, h, f)
            assert np.array_equal(got, thumbs.thumbnail(decoded.reshape(h, w, 4), f, mode)), (name, flag)
    assert any("3 thumbnails" in l for l in lines)
    (src / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)
    assert qoithumb_mi355x.main([str(src), "--max-side", "40", "-o", str(tmp_path / "again")], out=lines.append) == 1
    assert sorted(os.listdir(tmp_path / "again")) == ["a.png", "b.png", "c.png"]
