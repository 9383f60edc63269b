"""QOIMI_WARP_NEAREST on the GPU (-m gpu), through qoimi_decode_warped, qoimi_decode_warped_tensors (F16 CHW) and qoimi_decode_warped_indexed:
every output is compared bit for bit, over its whole length, with the definition - the oracle decodes the stream at the call's output
channel count, qoi_amd/warp.py selects from that, qoi_amd/tensors.py: convert makes the tensor (each u8 model is computed once and shared).
The pack is small: 130 x 70 photographs with 4 and with 3 channels, a 64 x 64 label map (four values in sharp regions), a 4096 x 1 strip
and a 1 x 1 image.  Outputs stand behind, between and in front of guard bytes (gpu_calls.py: run_warp, run_tensors); every
guard byte is checked after every call."""
import ctypes

import numpy as np
import pytest

from qoi_amd import tensors, warp
from qoi_amd.tensors import CHW, F16
from qoi_amd.warp import ALPHA_WEIGHTED, NEAREST, ONE, PLAIN, REPLICATE
from gpu_calls import WARP, run_tensors as run, run_warp
from gpu_pack import E_ARG, GUARD, IMAGENET, Pack, batch_of, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FILL = 0x40C08020
PHOTO4, PHOTO3, LABELS, STRIP, DOT = 0, 1, 2, 3, 4
SHAPES = [(130, 70, 4), (130, 70, 3), (64, 64, 4), (4096, 1, 4), (1, 1, 4)]
LABEL_VALUES = (3, 7, 20, 200)


def pixels():
    rng = np.random.default_rng(20250)
    photo4 = rng.integers(0, 256, size=(70, 130, 4), dtype=np.uint8)
    photo3 = rng.integers(0, 256, size=(70, 130, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:64, 0:64]
    region = (yy // 22 + xx // 32 + ((yy - 32) ** 2 + (xx - 32) ** 2 < 21 ** 2)) % 4
    labels = np.empty((64, 64, 4), dtype=np.uint8)
    for c in range(4):
        labels[:, :, c] = np.asarray(LABEL_VALUES, dtype=np.uint8)[(region + c) % 4]
    strip = rng.integers(0, 256, size=(1, 4096, 4), dtype=np.uint8)
    dot = np.array([[[200, 100, 50, 180]]], dtype=np.uint8)
    return [photo4, photo3, labels, strip, dot]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, SHAPES, pixels()))


_MODELS = {}


def model(p, it, och):
    """the u8 result P of one item: computed once, never changed"""
    key = (tuple(it), och)
    if key not in _MODELS:
        i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
        P = warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_items(p, got, items, och, f, what):
    for j, it in enumerate(items):
        w = tensors.convert(model(p, it, och), f).view(np.uint8).reshape(-1)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, it, int(np.argmax(got[j] != w)) // tensors.ELEM[f[0]])


# ---------------------------------------------------------------------------------- the warp with QOIMI_WARP_NEAREST
def warp_items(flag=NEAREST):
    """over the label map: the identity; a 30 degree turn with fill (61 x 47: its corners leave the rectangle) and with REPLICATE (41 x 29) - several tiles each; a shear; the
    identity moved past the top-left corner by 3 columns, 2 rows and a hair, with both borders; over the photographs a turn each"""
    rect = (6, 5, 50, 44)
    past = (ONE, 0, -6 * ONE - 1, 0, ONE, -4 * ONE - 1)
    return [warp.item(LABELS, rect, (50, 44), flags=flag, fill=FILL),
            warp.item(LABELS, rect, (61, 47), warp.rotation((50, 44), (61, 47), 30.0), flag, FILL),
            warp.item(LABELS, rect, (41, 29), warp.rotation((50, 44), (41, 29), 30.0, 0.8), flag | REPLICATE, FILL),
            warp.item(LABELS, rect, (17, 40), (ONE, 23001, -40000, -9001, ONE + 701, 12345), flag, 0x00FFFFFF),
            warp.item(LABELS, rect, (20, 12), past, flag, FILL), warp.item(LABELS, rect, (20, 12), past, flag | REPLICATE, FILL),
            warp.item(PHOTO4, (10, 8, 100, 50), (23, 40), warp.rotation((100, 50), (23, 40), 90.0, 0.4), flag, 0),
            warp.item(PHOTO3, (0, 0, 130, 70), (16, 16), warp.rotation((130, 70), (16, 16), -20.0, 0.2), flag | REPLICATE, FILL)]


def test_warp_nearest_against_the_model(ctx, pack):
    p = pack
    items = warp_items()
    for channels, mode in ((4, PLAIN), (4, ALPHA_WEIGHTED), (3, PLAIN)):
        got = run_warp(ctx, p, channels, items, mode, front=64 + 1)
        for j, it in enumerate(items):
            w = model(p, it, channels).reshape(-1)
            assert np.array_equal(got[j], w), ("warped", channels, mode, j, int(np.argmax(got[j] != w)))
    assert ctx.warp_stats()[:2] == (1, 1)
    # the values of the label map's outputs are source values or bytes of the fill: nothing is invented
    fill_bytes = {(FILL >> (8 * k)) & 255 for k in range(4)}
    for j in (0, 1, 2, 4, 5):
        allowed = set(LABEL_VALUES) | (set() if items[j][7] & REPLICATE else fill_bytes)
        assert set(np.unique(got[j]).tolist()) <= allowed, j
    assert set(np.unique(got[2]).tolist()) <= set(LABEL_VALUES) and not set(np.unique(got[1]).tolist()) <= set(LABEL_VALUES)
    # the identity is the rectangle
    assert np.array_equal(model(p, items[0], 4), p.decoded(LABELS, 4)[5:49, 6:56])
    # the same items as tensors (F16 CHW) and through a seek index
    f = (F16, CHW, *IMAGENET)
    got = run(ctx, p, WARP, 4, items, PLAIN, f)
    assert_items(p, got, items, 4, f, "warped tensors")
    intervals = [8, 8, 8, 1, 128]
    points, firsts = ctx.build_seek_index(p.packed.data_ptr(), p.so, p.sizes, p.descs, intervals)
    got = run_warp(ctx, p, 4, items, PLAIN, call=lambda out, offsets: ctx.decode_warped_indexed(
        p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, items, PLAIN, out, offsets, intervals, points, firsts))
    for j, it in enumerate(items):
        assert np.array_equal(got[j], model(p, it, 4).reshape(-1)), ("indexed", j)


@pytest.mark.parametrize("channels", [4, 3])
def test_warp_orientations_equal_the_bilinear_call(api, ctx, pack, channels):
    """every position is a pixel centre: with the flag and without it the device writes the same bytes"""
    p = pack
    plain_items, flagged = [], []
    for i, rect in ((LABELS, (3, 2, 40, 33)), (PHOTO4, (0, 0, 130, 70)), (PHOTO3, (17, 11, 31, 7)), (DOT, (0, 0, 1, 1))):
        for o in range(1, 9):
            w, h, ch = p.shapes[i]
            it = api.warp_orient(w, h, ch, rect, o)
            it.image = i
            plain_items.append(warp.fields(it))
            it.flags = NEAREST | (REPLICATE if o & 1 else 0)
            flagged.append(warp.fields(it))
    without = run_warp(ctx, p, channels, plain_items, PLAIN, front=64 + 3)
    with_flag = run_warp(ctx, p, channels, flagged, ALPHA_WEIGHTED, front=64 + 3)
    for j, (a, b) in enumerate(zip(without, with_flag)):
        assert np.array_equal(a, b), (channels, j)
        assert np.array_equal(b, model(p, flagged[j], channels).reshape(-1)), (channels, j)


def test_warp_bilinear_and_nearest_items_in_one_call(ctx, pack):
    """the flag is the item's: a bilinear item beside a nearest one keeps its bytes"""
    p = pack
    tent, near = warp_items(0)[1], warp_items()[1]
    alone = run_warp(ctx, p, 4, [tent], ALPHA_WEIGHTED)[0]
    for items in ([tent, near], [near, tent, near]):
        got = run_warp(ctx, p, 4, items, ALPHA_WEIGHTED)
        for g, it in zip(got, items):
            if it[7] & NEAREST:
                assert np.array_equal(g, model(p, it, 4).reshape(-1))
            else:
                assert np.array_equal(g, alone)
    i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = tent
    assert np.array_equal(alone, warp.warp(p.decoded(i, 4), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, ALPHA_WEIGHTED).reshape(-1))
    assert not np.array_equal(alone, model(p, near, 4).reshape(-1))


def test_rejections_on_a_live_context(api, ctx, pack):
    p = pack
    lib = api.load_library()
    n = p.n
    buf = filled(1 << 16, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    fmt = api.tensor_format((F16, CHW, *IMAGENET))
    good = warp_items()[1]

    def warped(flags, tensor=False, out=(10, 10)):
        arr = (api.QoimiWarp * 1)(api.QoimiWarp(*warp.item(LABELS, (0, 0, 10, 10), out, flags=flags)))
        head, tail = (ctx._h, *args, 4, arr, 1, 0), (buf.data_ptr(), (ctypes.c_size_t * 1)(64), 0, None)
        return lib.qoimi_decode_warped_tensors(*head, ctypes.byref(fmt), *tail) if tensor else lib.qoimi_decode_warped(*head, *tail)

    assert np.array_equal(run_warp(ctx, p, 4, [good])[0], model(p, good, 4).reshape(-1))
    stats = ctx.warp_stats()
    for tensor in (False, True):
        for flags in (2, 8, 6, 0x80000004):
            assert warped(flags, tensor) == E_ARG and "flag" in api.last_error(), (flags, api.last_error())
            assert bool((buf == GUARD).all()) and ctx.warp_stats() == stats, flags
        for out, word in (((1 << 20, 1), "2^20"), ((1, 1 << 20), "2^20"), ((20000, 20000), "400 000 000")):       # both size limits, with the flag
            assert warped(NEAREST, tensor, out) == E_ARG and word in api.last_error(), (out, api.last_error())
            assert bool((buf == GUARD).all()) and ctx.warp_stats() == stats, out
    # the context works afterwards, and so do the accepted flags
    assert np.array_equal(run_warp(ctx, p, 3, [good])[0], model(p, good, 3).reshape(-1))
    assert warped(NEAREST) == 0 and warped(NEAREST | REPLICATE) == 0 and warped(NEAREST, True) == 0, api.last_error()
