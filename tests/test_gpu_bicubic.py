"""qoimi_decode_tensors with QOIMI_FILTER_BICUBIC on the GPU (-m gpu): every output is compared bit for bit, over its whole length, with the
definition - the oracle decodes the stream at the call's output channel count, qoi_amd/bicubic.py resamples that, qoi_amd/tensors.py: convert
makes the tensor (each u8 model is computed once and shared).  The pack is small: 67 x 45 with soft alpha and runs of alpha 0, 67 x 45 with 3
channels, 1 x 1, 130 x 34, a 70 x 66 checkerboard of 0 / 255 whose alpha alternates in blocks of two (it holds the 64 x 64 rectangle of the
64-tap item) - for it the model is first shown to clamp at 0, to clamp at 255 and to meet A <= 0, the paths a wrong sign or a missing clamp
would break - and a column 4 x 4160, whose reduction by 16 to one column fills the row table of a tile: 256 rows of 64 entries.  The images
of 16384 x 1 and 1 x 16384 for the far end of the size limits are a pack of their own (tests/table_tiles.py).  The outputs of a call lie at
element-aligned but otherwise odd addresses with guard bytes between them (gpu_calls.py: tensor_layout, run_tensors); every guard byte is checked
after every call.  The items use 1, 2, 4, 8 and 16 lanes per pixel, 4 to 64 taps, tiles that hold whole rows and tiles that wrap one
(assert_paths, which tests/test_table_walk.py runs without a GPU)."""
import ctypes

import numpy as np
import pytest

import table_tiles as tt
from qoi_amd import bicubic, tensors
from qoi_amd.bicubic import ALPHA_WEIGHTED, PLAIN
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_BICUBIC, HWC, U8
from gpu_calls import WILD, run_tensors as run
from gpu_pack import E_ARG, GUARD, IMAGENET, Pack, batch_of, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import BICUBIC_ITEMS as ITEMS, BICUBIC_TABLES as TABLES, CHECK, CHECK_UP, ONE, RGB, SOFT, STRIP, assert_bicubic_paths as assert_paths

pytestmark = pytest.mark.gpu
SHAPES = [(67, 45, 4), (67, 45, 3), (1, 1, 4), (130, 34, 4), (70, 66, 4), (4, 4160, 4)]


def pixels():
    rng = np.random.default_rng(20240)
    soft = rng.integers(0, 256, size=(45, 67, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:45, 0:67]
    soft[:, :, 3] = np.clip(((xx * 5 + yy * 3) % 300) - 40, 0, 255)             # ramps with runs of alpha 0 between them
    rgb = rng.integers(0, 256, size=(45, 67, 3), dtype=np.uint8)
    rgb[10:30, 20:50] = (rgb[10:30, 20:50] // 8) * 8                            # a quieter patch
    one = np.array([[[200, 100, 50, 180]]], dtype=np.uint8)
    strip = rng.integers(0, 256, size=(34, 130, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:66, 0:70]
    check = np.empty((66, 70, 4), dtype=np.uint8)
    check[:, :, :3] = (((xx + yy) % 2) * 255)[:, :, None]
    check[:, :, 3] = ((xx // 2 + yy // 2) % 2) * 255
    tall = rng.integers(0, 256, size=(4160, 4, 4), dtype=np.uint8)
    return [soft, rgb, one, strip, check, tall]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, SHAPES, pixels()))


@pytest.fixture(scope="module")
def limits(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, tt.LIMIT_SHAPES, tt.limit_pixels()))


_MODELS = {}


def model(p, it, och, mode):
    """the u8 result P of one item of pack p: computed once, never changed"""
    key = (p, tuple(it), och, mode)
    if key not in _MODELS:
        i, x, y, cw, rh, ow, oh, flags = it
        P = bicubic.bicubic(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, mode)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_items(p, got, items, och, mode, f, what):
    for j, it in enumerate(items):
        w = tensors.convert(model(p, it, och, mode), f).view(np.uint8).reshape(-1)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, it, int(np.argmax(got[j] != w)) // tensors.ELEM[f[0]])


def test_the_items_use_every_lane_count_and_the_model_every_path(pack):
    assert_paths()
    # the checkerboard enlarged, before the clamp: values below 0, above 255, and a pixel whose weighted alpha sum is not positive
    _, x, y, cw, rh, ow, oh, _ = CHECK_UP
    R = pack.decoded(CHECK, 4)[y:y + rh, x:x + cw].astype(np.int64)
    N = np.einsum("Yr,rXc->YXc", bicubic.weights(rh, oh), np.einsum("Xk,rkc->rXc", bicubic.weights(cw, ow), R))
    v = (N + (1 << 29)) >> 30
    assert v[:, :, :3].min() < 0 and v[:, :, :3].max() > 255 and v[:, :, 3].min() < 0 and v[:, :, 3].max() > 255
    assert (N[:, :, 3] < 0).any() and (N[:, :, 3] == 0).any() and (N[:, :, 3] > 0).any()
    plain, weighted = model(pack, CHECK_UP, 4, PLAIN), model(pack, CHECK_UP, 4, ALPHA_WEIGHTED)
    assert plain.min() == 0 and plain.max() == 255 and not np.array_equal(plain, weighted)
    assert np.array_equal(weighted[N[:, :, 3] <= 0], plain[N[:, :, 3] <= 0])


@pytest.mark.parametrize("layout", [HWC, CHW])
@pytest.mark.parametrize("dtype", [U8, F16, BF16, F32])
def test_formats_against_the_model(ctx, pack, dtype, layout):
    formats = [tensors.fmt(U8, layout)] if dtype == U8 else [(dtype, layout, *IMAGENET), (dtype, layout, *WILD)]
    for channels, mode in ((4, ALPHA_WEIGHTED), (4, PLAIN), (3, PLAIN)):
        for f in formats:
            got = run(ctx, pack, FILTER_BICUBIC, channels, ITEMS, mode, f)
            assert_items(pack, got, ITEMS, channels, mode, f, (dtype, layout, channels, mode, float(f[2][0])))
    assert ctx.tensor_stats()[:2] == (1, 1) and ctx.tensor_stats()[3] == len({it[0] for it in ITEMS})


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_the_tables_at_their_largest(ctx, pack, mode):
    """256 rows of 64 entries in one tile; one row of 256 pixels of 4 column entries each with 64 row entries"""
    for f in (tensors.fmt(U8, HWC), (F32, CHW, *IMAGENET)):
        got = run(ctx, pack, FILTER_BICUBIC, 4, TABLES, mode, f)
        assert_items(pack, got, TABLES, 4, mode, f, ("tables", mode, f[0]))


def test_flips_modes_and_channels(ctx, pack):
    """all four flips of one reduction and one enlargement; with 3 channels ALPHA_WEIGHTED is PLAIN; channels = 0 takes the images' count"""
    f = tensors.fmt(U8, HWC)
    items = [(SOFT, 4, 3, 37, 29, 5, 7, fl) for fl in range(4)] + [(CHECK, 5, 4, 9, 7, 13, 11, fl) for fl in range(4)]
    for channels, mode in ((4, PLAIN), (4, ALPHA_WEIGHTED), (3, ALPHA_WEIGHTED), (0, ALPHA_WEIGHTED)):
        och = channels or 4
        got = run(ctx, pack, FILTER_BICUBIC, channels, items, mode, f)
        assert_items(pack, got, items, och, mode, f, ("flips", channels, mode))
        for base in (0, 4):
            a = [g.reshape(items[base][6], items[base][5], och) for g in got[base:base + 4]]
            assert np.array_equal(a[1], a[0][:, ::-1]) and np.array_equal(a[2], a[0][::-1]) and np.array_equal(a[3], a[0][::-1, ::-1])
    three = [(RGB, 60, 0, 7, 45, 3, 50, 3), (RGB, 0, 0, 67, 45, 67, 45, 0)]
    got = run(ctx, pack, FILTER_BICUBIC, 0, three, ALPHA_WEIGHTED, (F16, CHW, *IMAGENET))
    assert_items(pack, got, three, 3, PLAIN, (F16, CHW, *IMAGENET), "channels 0 of 3")
    assert np.array_equal(model(pack, three[1], 3, PLAIN), pack.decoded(RGB, 3))          # the identity is the rectangle


def test_the_size_limit_is_accepted(ctx, pack):
    """1 x 1 -> 16384 x 1: the largest side, 64 tiles of one row"""
    items = [(ONE, 0, 0, 1, 1, 16384, 1, 1)]
    got = run(ctx, pack, FILTER_BICUBIC, 4, items, PLAIN, (F16, CHW, *IMAGENET))
    assert_items(pack, got, items, 4, PLAIN, (F16, CHW, *IMAGENET), "16384")


def test_the_other_end_of_the_limits(ctx, limits):
    """16384 x 1 -> 1024 x 1 flipped in x (exactly 16 : 1, 64 taps, sixteen lanes), 1 x 16384 -> 1 x 1024 flipped in y (four tiles of 256 rows
    of 64 entries, row offsets up to the last row of the stage) and 1 x 3 -> 1 x 16384 (64 tiles of 256 rows)"""
    for mode, items in ((PLAIN, tt.LIMIT_ITEMS), (ALPHA_WEIGHTED, tt.LIMIT_ITEMS[:1])):
        for f in ((F16, CHW, *IMAGENET), tensors.fmt(U8, HWC)):
            got = run(ctx, limits, FILTER_BICUBIC, 4, items, mode, f)
            assert ctx.tensor_stats()[:2] == (1, 1)
            assert_items(limits, got, items, 4, mode, f, ("limits", mode, f[0]))


def test_sub_batches(api, pack):
    c = api.Context(0)
    try:
        f = (BF16, CHW, *IMAGENET)
        images = len({it[0] for it in ITEMS})
        single = run(c, pack, FILTER_BICUBIC, 4, ITEMS, ALPHA_WEIGHTED, f)
        assert c.tensor_stats()[:2] == (1, 1) and c.tensor_stats()[3] == images
        _, _, the_plan, largest = bicubic.plan(pack.descs, ITEMS, 1)
        assert len(the_plan) == images > 1
        forced = run(c, pack, FILTER_BICUBIC, 4, ITEMS, ALPHA_WEIGHTED, f, staging=1)      # a staging so small that every image is a sub-batch
        assert c.tensor_stats() == (images, images, largest, images), c.tensor_stats()
        assert all(np.array_equal(x, y) for x, y in zip(forced, single))
        assert_items(pack, forced, ITEMS, 4, ALPHA_WEIGHTED, f, "sub-batches")
    finally:
        c.close()


def test_rejections_on_a_live_context(api, ctx, pack):
    p = pack
    lib = api.load_library()
    n = p.n
    buf = filled(1 << 17, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    two = [(SOFT, 0, 0, 60, 40, 10, 10, 0), (STRIP, 0, 0, 8, 3, 8, 8, 1)]
    ok = (F16, CHW, *IMAGENET)

    def fm(f, reserved=(0, 0)):
        t = api.tensor_format(f)
        return api.QoimiTensorFormat(t.dtype, t.layout, t.scale, t.bias, (ctypes.c_uint * 2)(*reserved))

    def call(items=two, offsets=(128, 128 + 800), channels=4, filter=FILTER_BICUBIC, mode=0, f=fm(ok), null_format=False):
        arr = (api.QoimiResize * len(items))(*[api.QoimiResize(*it) for it in items])
        return lib.qoimi_decode_tensors(ctx._h, *args, channels, arr, len(items), filter, mode, None if null_format else ctypes.byref(f),
                                        buf.data_ptr(), (ctypes.c_size_t * len(items))(*offsets), 0, None)

    assert call() == 0, api.last_error()                                              # side by side: accepted
    got = buf.cpu().numpy()
    for it, o, nb in ((two[0], 128, 800), (two[1], 928, 512)):
        assert np.array_equal(got[o:o + nb], tensors.convert(model(p, it, 4, PLAIN), ok).view(np.uint8).reshape(-1))
    assert np.all(got[:128] == GUARD) and np.all(got[928 + 512:] == GUARD)
    stats = ctx.tensor_stats()
    assert stats[:2] == (1, 1) and stats[3] == 2
    # both sides of each limit: 16 times is accepted ...
    assert call(items=[(STRIP, 0, 0, 128, 3, 8, 1, 0), (SOFT, 0, 0, 2, 32, 1, 2, 0)], offsets=(128, 512)) == 0, api.last_error()
    stats = ctx.tensor_stats()
    buf.fill_(GUARD)
    one, zero = (1.0,) * 4, (0.0,) * 4
    rejected = [
        (lambda: call(items=[(STRIP, 0, 0, 129, 3, 8, 1, 0)], offsets=(64,)), "more than 16"), (lambda: call(items=[(SOFT, 0, 0, 2, 33, 1, 2, 0)], offsets=(64,)), "more than 16"),
        (lambda: call(items=[(ONE, 0, 0, 1, 1, 16385, 1, 0)], offsets=(64,)), "16384"), (lambda: call(items=[(ONE, 0, 0, 1, 1, 1, 16385, 0)], offsets=(64,)), "16384"),
        (lambda: call(filter=2), "filter"), (lambda: call(filter=4), "filter"),
        (lambda: call(null_format=True), "format"), (lambda: call(f=fm((4, HWC, one, zero))), "dtype"), (lambda: call(f=fm((F16, 2, one, zero))), "layout"),
        (lambda: call(f=fm(ok, (1, 0))), "reserved"), (lambda: call(f=fm((F32, HWC, (1.0, float("inf"), 1.0, 1.0), zero))), "finite"),
        (lambda: call(f=fm((U8, HWC, (1.0, 1.0, 2.0, 1.0), zero))), "QOIMI_TENSOR_U8"),
        (lambda: call(offsets=(129, 1024)), "multiple of the element size"), (lambda: call(offsets=(128, 128 + 798)), "overlap"),
        (lambda: call(items=[(SOFT, 60, 0, 10, 10, 10, 10, 0)], offsets=(64,)), "leaves"), (lambda: call(items=[(SOFT, 0, 0, 10, 10, 10, 10, 4)], offsets=(64,)), "flag"),
        (lambda: call(items=[(SOFT, 0, 0, 10, 10, 0, 10, 0)], offsets=(64,)), "zero"),
        (lambda: call(mode=2), "mode"), (lambda: call(channels=5), "channels"),
        (lambda: call(items=[(RGB, 0, 0, 1, 1, 1, 1, 0), (SOFT, 0, 0, 1, 1, 1, 1, 0)], offsets=(64, 128), channels=0), "channel"),
        # the order: the filter in front of the format, the format in front of the items, the rectangle in front of the limits, the items in
        # front of the alignment
        (lambda: call(filter=2, null_format=True), "filter"), (lambda: call(items=[(STRIP, 0, 0, 129, 3, 8, 1, 0)], offsets=(63,), f=fm((4, HWC, one, zero))), "dtype"),
        (lambda: call(items=[(STRIP, 2, 0, 129, 3, 8, 1, 0)], offsets=(63,)), "leaves"), (lambda: call(items=[(STRIP, 0, 0, 129, 3, 8, 1, 0)], offsets=(63,)), "more than 16"),
        (lambda: call(items=[(ONE, 0, 0, 1, 1, 16385, 1, 4)], offsets=(64,)), "flag"),
    ]
    for f, word in rejected:
        assert f() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.tensor_stats() == stats, word
    with pytest.raises(api.QoiError):
        ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [(STRIP, 0, 0, 129, 3, 8, 1, 0)], FILTER_BICUBIC, PLAIN, ok, buf.data_ptr(), [128])
    assert bool((buf == GUARD).all()) and ctx.tensor_stats() == stats
    # the context works afterwards
    assert_items(p, run(ctx, p, FILTER_BICUBIC, 3, ITEMS[:3], PLAIN, ok), ITEMS[:3], 3, PLAIN, ok, "afterwards")


def test_the_tools_on_the_gpu(api, oracle, tmp_path):
    """--filter bicubic of both tools: two small files to a tensor and to PNGs whose values are the model's of the oracle's decode"""
    from qoi_amd import synth
    from tools import png_io
    from tools import qoiresize_mi355x as resize_tool
    from tools import qoitensor_mi355x as tensor_tool
    images = {"a": (synth.frame_rgba("sprite_alpha", 130, 70, 0), 130, 70, 4), "b": (synth.frame_rgb("photo", 64, 48, 1), 64, 48, 3)}
    src = tmp_path / "in"
    src.mkdir()
    for name, (px, w, h, ch) in images.items():
        assert api.qoi_write(str(src / (name + ".qoi")), px.reshape(-1), api.QoiDesc(w, h, ch, 0)) > 0
    lines = []
    assert tensor_tool.main([str(src), "--size", "37x23", "--filter", "bicubic", "--dtype", "f16", "-o", str(tmp_path / "t.npy")], out=lines.append) == 0
    assert resize_tool.main([str(src), "--size", "37x23", "--filter", "bicubic", "--mode", "weighted", "-o", str(tmp_path / "png")], out=lines.append) == 0
    got = np.load(tmp_path / "t.npy")
    unit = (F16, CHW, np.full(4, 1 / 255, np.float32), np.zeros(4, np.float32))
    for j, (name, (px, w, h, ch)) in enumerate(sorted(images.items())):
        d3, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 3)
        d4, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 4)
        want = tensors.tensors(d3.reshape(h, w, 3), (0, 0, w, h), (37, 23), 0, FILTER_BICUBIC, PLAIN, unit)
        assert np.array_equal(got[j].view(np.uint8), want.view(np.uint8)), name
        png, pw, ph = png_io.read_png((tmp_path / "png" / (name + ".png")).read_bytes(), 4)
        assert (pw, ph) == (37, 23) and np.array_equal(np.asarray(png).reshape(23, 37, 4), bicubic.bicubic(d4.reshape(h, w, 4), (0, 0, w, h), (37, 23), 0, ALPHA_WEIGHTED)), name
    # 130 to 8 is beyond this filter's 16 and inside the tent's 32
    assert tensor_tool.main([str(src), "--size", "8x8", "--filter", "bicubic", "-o", str(tmp_path / "u.npy")], out=lines.append) == 1 and "left out" in lines[-3]
