"""QOIMI_FILTER_MODE on the GPU (-m gpu): the kernel tensor_mode through qoimi_decode_tensors.  The expectation is always the definition -
the oracle decodes the stream to 4 channels, qoi_amd/mode.py votes over that and drops alpha for 3 output channels, qoi_amd/tensors.py:
convert makes the tensor; each u8 model is computed once and shared - and every comparison is of bits and covers the whole output.  Every
call lays its outputs at element-aligned but otherwise odd addresses with 1 to 3 guard bytes (0xA5) between neighbours, rounded up to whole
elements; every guard byte is checked after every call (the layout and the call: tests/test_gpu_labels.py)."""
import ctypes

import numpy as np
import pytest

import mode_cases as MC
import table_tiles as TT
from qoi_amd import mode, tensors
from qoi_amd.tensors import ALPHA_WEIGHTED, BF16, CHW, F16, F32, FILTER_AREA, FILTER_MODE, FILTER_NEAREST, HW, HWC, I32, I64, PLAIN, U8
from gpu_calls import fmt_of, run_label_tensors as run
from gpu_pack import E_ARG, GUARD, Pack, batch_of, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DTYPES = (U8, F16, BF16, F32, I32, I64)
LAYOUTS = (HWC, CHW, HW)
SMALL, WIDE, DISTINCT, BLOCKS, CONST, SIXTEEN, LONG, TALL = range(8)
SHAPES = [(37, 29, 3), (70, 45, 4), (70, 45, 4), (64, 48, 3), (37, 29, 4), (64, 48, 4), (16384, 3, 3), (3, 16384, 3)]

# every lg the split can choose: cells 1 x 1 (0), 1 x 5 (1), 5 x 2 (2), 5 x 5 (3), 8 x 8 (4), 11 x 8 (5), 16 x 12 and 16 x 16 (6); a 1 x 1
# output, 1-wide and 1-high rectangles, reduce-x with enlarge-y, rectangles at odd offsets; the flips take turns
LG_ITEMS = [(WIDE, 3, 5, 31, 23, 50, 41, 1), (SMALL, 0, 0, 37, 29, 50, 7, 2), (WIDE, 3, 5, 31, 23, 7, 20, 3), (WIDE, 0, 0, 70, 45, 16, 11, 0), (WIDE, 3, 5, 31, 23, 4, 3, 1),
            (WIDE, 3, 5, 31, 23, 3, 3, 2), (WIDE, 3, 5, 31, 23, 2, 2, 3), (SIXTEEN, 0, 0, 64, 48, 4, 3, 0), (SIXTEEN, 1, 1, 16, 16, 1, 1, 1), (WIDE, 7, 0, 1, 45, 1, 3, 2),
            (WIDE, 0, 9, 70, 1, 5, 1, 3), (SMALL, 1, 2, 33, 25, 3, 50, 0), (SMALL, 5, 3, 9, 9, 1, 1, 0)]
LG_OF = [0, 1, 2, 3, 4, 5, 6, 6, 6, 2, 2, 2, 5]


def pixels():
    rng = np.random.default_rng(77)
    n = np.arange(70 * 45, dtype=np.uint32).reshape(45, 70)
    distinct = np.stack([n & 255, n >> 8, 7 - (n & 7), 255 - (n & 1)], axis=2).astype(np.uint8)
    yy, xx = np.mgrid[0:48, 0:64]
    blocks = MC.PALETTE[((xx // 11) + 2 * (yy // 7)) % 3][:, :, :3]                      # piecewise constant: most groups are uniform
    const = np.empty((29, 37, 4), dtype=np.uint8)
    const[:] = (9, 200, 31, 77)
    return MC.images() + [distinct, blocks, const, MC.label_map(64, 48, 4, 5, 13), MC.PALETTE[rng.integers(0, 3, size=(3, 16384))][:, :, :3],
                          MC.PALETTE[rng.integers(0, 3, size=(16384, 3))][:, :, :3]]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    p = Pack(ctx, oracle, batch_of(api, oracle, SHAPES, pixels()))
    for i, px in enumerate(pixels()):                                                  # the streams hold what the tests think they hold
        assert np.array_equal(p.decoded(i, SHAPES[i][2]), px), i
    return p


_MODELS = {}


def model(p, filt, it, och):
    """the u8 result P of one item: the vote over the 4-channel decode, alpha dropped afterwards; computed once, never changed"""
    key = (filt, tuple(it), och)
    if key not in _MODELS:
        i, x, y, cw, rh, ow, oh, flags = it
        if filt == FILTER_MODE:
            P = mode.mode(p.decoded(i, 4), (x, y, cw, rh), (ow, oh), flags, och=och)
        else:
            P = tensors.tensors(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, filt)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


def assert_items(p, got, items, och, f, what, filt=FILTER_MODE):
    for j, it in enumerate(items):
        w = tensors.convert(model(p, filt, it, och), f).view(np.uint8).reshape(-1)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, it, int(np.argmax(got[j] != w)) // tensors.elem(f[0]))


def check(ctx, p, items, channels, f, what, mode_=PLAIN, staging=0):
    och = channels or p.shapes[items[0][0]][2]
    assert_items(p, run(ctx, p, FILTER_MODE, channels, items, mode_, f, staging), items, och, f, what)


# ------------------------------------------------------------------ 1: the label inputs and what they reach
def test_the_label_inputs_and_their_reach(ctx, pack):
    reach = MC.reach_of(lambda i: pack.decoded(i, 4), MC.LABEL_ITEMS)
    assert all(reach[c] >= 1 for c in "abcd"), reach
    for channels in (4, 3):
        for f in (tensors.fmt(U8, HWC), tensors.fmt(I64, HW)):
            check(ctx, pack, MC.LABEL_ITEMS, channels, f, ("labels", channels))
    for it in MC.LABEL_ITEMS:                                                          # and the model is the brute-force statement
        assert np.array_equal(model(pack, FILTER_MODE, it, 4), MC.brute(pack.decoded(it[0], 4), it[1:5], it[5:7], it[7]))
    assert ctx.tensor_stats()[:2] == (1, 1) and ctx.tensor_stats()[3] == 2
    # alpha votes and och 3 drops it afterwards: not the vote over the 3-channel decode
    it = MC.LABEL_ITEMS[1]
    assert not np.array_equal(model(pack, FILTER_MODE, it, 3), mode.mode(pack.decoded(MC.WIDE, 3), it[1:5], it[5:7]))


def test_distinct_constant_and_piecewise_constant_images(ctx, pack):
    f = tensors.fmt(U8, HWC)
    distinct = [(DISTINCT, 0, 0, 70, 45, 16, 11, 0), (DISTINCT, 5, 3, 63, 41, 4, 3, 3), (DISTINCT, 0, 0, 70, 45, 100, 3, 1), (DISTINCT, 1, 0, 64, 32, 4, 2, 2)]
    got = run(ctx, pack, FILTER_MODE, 4, distinct, PLAIN, f)
    near = run(ctx, pack, FILTER_NEAREST, 4, distinct, PLAIN, f)
    assert all(np.array_equal(a, b) for a, b in zip(got, near))                        # all pixels distinct: the nearest filter's output of the same call
    assert_items(pack, got, distinct, 4, f, "distinct")
    flat = [(CONST, 2, 1, 33, 25, 3, 2, 0), (CONST, 0, 0, 37, 29, 9, 7, 3), (CONST, 0, 0, 37, 29, 50, 3, 1), (BLOCKS, 0, 0, 64, 48, 4, 3, 0), (BLOCKS, 1, 1, 63, 47, 16, 11, 2),
            (BLOCKS, 0, 0, 64, 48, 32, 24, 0), (BLOCKS, 3, 0, 55, 48, 5, 6, 1)]
    for items in (flat[:3], flat[3:]):
        for channels in (3, 4):
            check(ctx, pack, items, channels, f, ("flat", channels))
    got = run(ctx, pack, FILTER_MODE, 4, flat[:3], PLAIN, f)
    assert all(np.array_equal(g.reshape(-1, 4), np.broadcast_to(np.array([9, 200, 31, 77], np.uint8), (g.size // 4, 4))) for g in got)


# ------------------------------------------------------------------ 2: every lane count, format and flip
def test_every_lane_count_in_one_call(ctx, pack):
    assert [mode.split(it[3], it[4], it[5], it[6])[0] for it in LG_ITEMS] == LG_OF and set(LG_OF) == set(range(7))
    assert mode.split(64, 48, 4, 3) == (6, 4) and mode.cell(0, 64, 4) == (0, 16) and mode.cell(2, 48, 3) == (32, 16)
    for channels, mode_ in ((4, PLAIN), (3, ALPHA_WEIGHTED)):
        check(ctx, pack, LG_ITEMS, channels, tensors.fmt(U8, HWC), ("lanes", channels), mode_)
    check(ctx, pack, LG_ITEMS, 4, tensors.fmt(I64, HW), "lanes I64 HW")
    assert ctx.tensor_stats()[:2] == (1, 1)


@pytest.mark.parametrize("flags", range(4))
def test_flips_and_channel_counts(ctx, pack, flags):
    items = [it[:7] + (flags,) for it in LG_ITEMS]
    for channels in (3, 4):
        check(ctx, pack, items, channels, tensors.fmt(U8, HWC), ("flip", flags, channels))
    # channels = 0: the output channel count is the images' - 3-channel streams (alpha 255 votes), then 4-channel ones
    for chosen in ([it for it in items if it[0] == SMALL] + [(BLOCKS, 1, 1, 63, 47, 16, 11, flags)], [it for it in items if it[0] in (WIDE, SIXTEEN)]):
        check(ctx, pack, chosen, 0, tensors.fmt(I32, CHW), ("channels 0", flags))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_mode_in_every_format(ctx, pack, dtype, layout):
    f = fmt_of(dtype, layout)
    items = [LG_ITEMS[k] for k in (0, 1, 3, 5, 7, 11)] + MC.LABEL_ITEMS[:1]
    for channels in (4, 3):
        check(ctx, pack, items, channels, f, (dtype, layout, channels))


def test_sub_batches(api, pack):
    """a staging of one byte: one image per sub-batch, three of them"""
    c = api.Context(0)
    try:
        f = tensors.fmt(I64, HW)
        single = run(c, pack, FILTER_MODE, 4, LG_ITEMS, PLAIN, f)
        assert c.tensor_stats()[:2] == (1, 1) and c.tensor_stats()[3] == 3
        _, _, subs, largest = mode.plan(pack.descs, LG_ITEMS, 1)
        assert len(subs) == 3
        forced = run(c, pack, FILTER_MODE, 4, LG_ITEMS, PLAIN, f, staging=1)
        assert c.tensor_stats() == (3, 3, largest, 3), c.tensor_stats()
        assert all(np.array_equal(x, y) for x, y in zip(forced, single))
        assert_items(pack, forced, LG_ITEMS, 4, f, "three sub-batches")
    finally:
        c.close()


def test_tile_walk(ctx, pack):
    """more tiles than twice the launch's workgroups (tests/table_tiles.py: needed): large enlarging items of one lane a pixel between
    items of every other lane count, so that a workgroup takes several tiles and steps from item to item, from one lg to the next"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    items, tiles, j = [], 0, 0
    while tiles < TT.needed(cus):
        items += [LG_ITEMS[j % len(LG_ITEMS)][:7] + (j & 3,), (SMALL, 3 + j % 5, 2, 5, 4, 700, 400 + j, (j + 1) & 3), (SMALL, 0, 0, 37, 29, 9, 300 + j, j & 3)]
        tiles += sum(mode.tiles(*it[3:7]) for it in items[-3:])
        j += 1
    assert tiles > 2 * TT.WG_PER_CU * cus and len(items) < 40
    check(ctx, pack, items, 4, tensors.fmt(I64, HW), "many tiles")
    assert ctx.tensor_stats()[:2] == (1, 1)


def test_the_far_ends(ctx, pack):
    items = [(LONG, 0, 0, 16384, 3, 1024, 3, 1), (TALL, 0, 0, 3, 16384, 3, 1024, 2), (LONG, 1, 1, 16383, 2, 16384, 1, 0)]
    assert [mode.split(*it[3:7])[0] for it in items] == [2, 2, 0]
    check(ctx, pack, items, 3, tensors.fmt(U8, HWC), "far ends")
    check(ctx, pack, items[:2], 4, tensors.fmt(I64, HW), "far ends I64 HW")


# ------------------------------------------------------------------ 3: rejections on a live context, and the context afterwards
def test_rejections_leave_the_output_untouched(api, ctx, pack):
    p = pack
    lib = api.load_library()
    n = p.n
    buf = filled(65536, GUARD)
    args = (p.packed.data_ptr(), (ctypes.c_size_t * n)(*p.so), (ctypes.c_int * n)(*p.sizes), (api.QoiDesc * n)(*p.descs), n)
    two = [(WIDE, 0, 0, 70, 45, 10, 10, 0), (SMALL, 0, 0, 8, 8, 8, 8, 1)]              # 800 and 512 bytes as I64 HW
    ok = tensors.fmt(I64, HW)

    def call(items=two, offsets=(128, 128 + 800), channels=4, filter=FILTER_MODE, f=ok):
        arr = (api.QoimiResize * len(items))(*[api.QoimiResize(*it) for it in items])
        t = api.tensor_format(f)
        return lib.qoimi_decode_tensors(ctx._h, *args, channels, arr, len(items), filter, 0, ctypes.byref(t), buf.data_ptr(), (ctypes.c_size_t * len(items))(*offsets), 0, None)

    assert call() == 0, api.last_error()
    got = buf.cpu().numpy()
    for it, o, nb in ((two[0], 128, 800), (two[1], 928, 512)):
        assert np.array_equal(got[o:o + nb], tensors.convert(model(p, FILTER_MODE, it, 4), ok).view(np.uint8).reshape(-1))
    assert np.all(got[:128] == GUARD) and np.all(got[928 + 512:] == GUARD)
    stats = ctx.tensor_stats()
    buf.fill_(GUARD)
    one = lambda it: dict(items=[it], offsets=(64,))                                    # noqa: E731
    rejected = [
        (lambda: call(filter=10), "filter"), (lambda: call(filter=12), "filter"),
        (lambda: call(**one((WIDE, 0, 0, 33, 2, 2, 2, 0))), "16 in an axis"), (lambda: call(**one((WIDE, 0, 0, 2, 33, 2, 2, 0))), "16 in an axis"),
        (lambda: call(**one((LONG, 0, 0, 16384, 1, 1023, 1, 0))), "16 in an axis"), (lambda: call(**one((WIDE, 0, 0, 1, 1, 16385, 1, 0))), "16384"),
        (lambda: call(**one((WIDE, 0, 0, 1, 1, 1, 16385, 0))), "16384"),
        # the order: the rectangle rules, the ratio, the size
        (lambda: call(**one((WIDE, 0, 0, 70, 0, 1, 1, 4))), "zero"), (lambda: call(**one((WIDE, 60, 0, 70, 1, 1, 1, 4))), "flag"), (lambda: call(**one((WIDE, 60, 0, 70, 1, 1, 1, 0))), "leaves"),
        (lambda: call(items=[two[0], (WIDE, 0, 0, 70, 45, 4, 16385, 0)], offsets=(64, 8192)), "16 in an axis"),
        (lambda: call(offsets=(128, 128 + 792)), "overlap"), (lambda: call(offsets=(132, 1024)), "multiple of the element size"),
    ]
    for c, word in rejected:
        assert c() == E_ARG and word in api.last_error(), (word, api.last_error())
        assert bool((buf == GUARD).all()) and ctx.tensor_stats() == stats, word
    # 70 to 4 is no fault under the area filter's limit of 64 either; 33 to 2 is the nearest filter's; the context works afterwards
    assert call(**one((WIDE, 0, 0, 33, 2, 2, 2, 0)), filter=FILTER_NEAREST) == 0 and call(**one((WIDE, 0, 0, 33, 2, 2, 2, 0)), filter=FILTER_AREA) == 0
    check(ctx, p, MC.LABEL_ITEMS, 3, ok, "afterwards")
