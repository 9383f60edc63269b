"""qoi_amd/nearest.py, the normative statement of QOIMI_FILTER_NEAREST, and the integer dtypes and the one-plane layout of qoi_amd/tensors.py,
on the CPU: ``nearest.nearest`` against a double loop; its three identities - with the output the size of the rectangle it is ``crops.crop``,
with cw = f * ow it takes column X * f + f // 2, and it equals ``warp.warp`` with NEAREST and a scale map wherever the quotients are whole;
the index against torch's interpolate(mode="nearest-exact"), which computes it in float: the two differ only where the output pixel's
centre lies exactly on the boundary of two source cells, and there torch is one lower; ``tensors.convert`` for I32, I64 and HW against
torch's own conversion; ``ELEM`` and the signatures the earlier dtypes came with."""
import inspect

import numpy as np
import pytest

from qoi_amd import crops, nearest, tensors, warp
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_NEAREST, HW, HWC, I32, I64, U8

RNG = np.random.default_rng(20261020)
D4 = RNG.integers(0, 256, size=(45, 70, 4), dtype=np.uint8)
D3 = RNG.integers(0, 256, size=(29, 37, 3), dtype=np.uint8)
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def test_constants():
    assert (I32, I64, HW, FILTER_NEAREST) == (5, 6, 3, 9)
    assert (tensors.U8, tensors.F16, tensors.BF16, tensors.F32, tensors.HWC, tensors.CHW) == (0, 1, 2, 3, 0, 1)
    assert (tensors.FILTER_AREA, tensors.FILTER_BILINEAR, tensors.FILTER_BICUBIC, tensors.FILTER_LANCZOS) == (0, 1, 3, 6)
    assert nearest.MAX_SIZE == 16384 and nearest.THREADS == 256


def loop(D, rect, out_size, flags):
    x, y, cw, rh = rect
    ow, oh = out_size
    out = np.zeros((oh, ow, D.shape[2]), np.uint8)
    for Y in range(oh):
        for X in range(ow):
            k, r = ((2 * X + 1) * cw) // (2 * ow), ((2 * Y + 1) * rh) // (2 * oh)
            assert 0 <= k < cw and 0 <= r < rh
            out[oh - 1 - Y if flags & 2 else Y, ow - 1 - X if flags & 1 else X] = D[y + r, x + k]
    return out


@pytest.mark.parametrize("D", [D4, D3], ids=["70x45x4", "37x29x3"])
def test_nearest_against_a_double_loop(D):
    h, w = D.shape[:2]
    for rect in [(0, 0, w, h), (3, 5, w - 7, h - 9), (1, 1, 2, 14), (w - 1, h - 1, 1, 1), (0, 2, 1, h - 2)]:
        for out_size in [(1, 1), (3, 2), (rect[2], rect[3]), (41, 23), (50, 41), (2 * rect[2], 3 * rect[3]), (7, 300)]:
            for flags in range(4):
                got = nearest.nearest(D, rect, out_size, flags)
                assert got.dtype == np.uint8 and got.flags.c_contiguous and np.array_equal(got, loop(D, rect, out_size, flags)), (rect, out_size, flags)
            assert np.array_equal(nearest.nearest(D, rect, out_size, 1, nearest.ALPHA_WEIGHTED), nearest.nearest(D, rect, out_size, 1, nearest.PLAIN))
            assert nearest.size(w, h, rect, out_size, 3, D.shape[2]) == out_size[0] * out_size[1] * D.shape[2]
    for n_src, n_out in [(1, 1), (1, 300), (300, 1), (16384, 16384), (16384, 1), (2, 41)]:
        k = nearest.index(n_src, n_out)
        assert k.min() >= 0 and k.max() < n_src and np.all(np.diff(k) >= 0)


def test_limits_and_errors():
    w, h = 20000, 17000
    assert nearest.size(w, h, (0, 0, 16384, 1), (1, 1), 0, 4) == 4                             # no ratio limit
    assert nearest.size(w, h, (0, 0, 16385, 1), (1, 1), 0, 4) == 0 and nearest.size(w, h, (0, 0, 1, 16385), (1, 1), 0, 4) == 0
    assert nearest.size(w, h, (0, 0, 1, 1), (16385, 1), 0, 4) == 0 and nearest.size(w, h, (0, 0, 1, 1), (1, 16385), 0, 3) == 0
    assert nearest.size(w, h, (0, 0, 1, 1), (16384, 16384), 3, 3) == 3 * 2 ** 28
    assert nearest.size(w, h, (w - 1, 0, 2, 1), (1, 1), 0, 4) == 0 and nearest.size(w, h, (0, 0, 1, 1), (1, 1), 4, 4) == 0
    assert nearest.size(w, h, (0, 0, 0, 1), (1, 1), 0, 4) == 0 and nearest.size(w, h, (0, 0, 1, 1), (1, 1), 0, 5) == 0
    # the order: the rectangle rules in front of the size limit
    for rect, out_size, flags, word in [((0, 0, 0, 1), (16385, 1), 4, "zero"), ((0, 0, 16385, 1), (1, 1), 4, "flag"), ((w - 1, 0, 16385, 1), (1, 1), 0, "leaves"),
                                        ((0, 0, 16385, 1), (1, 1), 0, "16384")]:
        assert word in nearest._wrong(w, h, rect, out_size, flags)
    for bad in [lambda: nearest.nearest(D4[:, :, 0], (0, 0, 1, 1), (1, 1)), lambda: nearest.nearest(D4, (0, 0, 1, 1), (1, 1), 0, 2), lambda: nearest.nearest(D4, (69, 0, 2, 1), (1, 1)),
                lambda: nearest.nearest(D4, (0, 0, 1, 1), (0, 1)), lambda: nearest.nearest(D4.astype(np.int32), (0, 0, 1, 1), (1, 1)), lambda: nearest.index(0, 1)]:
        with pytest.raises(ValueError):
            bad()
    descs = [(70, 45, 4), (37, 29, 3)]
    items = [(1, 1, 1, 2, 14, 41, 23, 0), (0, 5, 3, 63, 41, 3, 2, 3)]
    assert nearest.plan(descs, items, 0) == crops.plan(descs, [(1, 1, 1, 2, 14, 0), (0, 5, 3, 63, 41, 3)], 0)
    assert nearest.tiles(50, 41) == 9 and nearest.tiles(16, 16) == 1 and nearest.tiles(1, 257) == 2
    assert nearest.place(50 * 40 + 49, 37, 29, 50, 41) == (49, 40, (99 * 37) // 100, (81 * 29) // 82)


def test_identity_equal_size_is_the_crop():
    for D, rect in [(D4, (5, 3, 63, 41)), (D3, (0, 0, 37, 29)), (D4, (69, 44, 1, 1))]:
        for flags in range(4):
            assert np.array_equal(nearest.nearest(D, rect, rect[2:], flags), crops.crop(D, rect, flags)), (rect, flags)


def test_identity_whole_factor_takes_the_middle_column():
    for f in (1, 2, 3, 4, 5, 8, 17, 100):
        for ow in (1, 2, 7, 64):
            k = nearest.index(f * ow, ow)
            assert np.array_equal(k, np.arange(ow) * f + f // 2), (f, ow)
    got = nearest.nearest(D4, (7, 1, 60, 40), (20, 8))                                          # factors 3 and 5
    assert np.array_equal(got, D4[1 + 2:41:5, 7 + 1:67:3])


def test_identity_the_nearest_warp_with_a_scale_map():
    """a = 65536 * cw / ow, e = 65536 * rh / oh, everything else 0: wherever both quotients are whole the warp's Px >> 17 is this index"""
    seen = 0
    for D, rect in [(D4, (5, 3, 63, 41)), (D3, (1, 1, 2, 14)), (D4, (0, 0, 64, 32))]:
        cw, rh = rect[2:]
        for ow, oh in [(cw, rh), (3, 2), (41, 23), (128, 64), (16, 1), (256, 4), (63 * 4, 41 * 2), (2 * 65536, 7)]:
            if (65536 * cw) % ow or (65536 * rh) % oh:
                continue
            if ow > nearest.MAX_SIZE:
                continue
            m = (65536 * cw // ow, 0, 0, 0, 65536 * rh // oh, 0)
            for flags in (warp.NEAREST, warp.NEAREST | warp.REPLICATE):
                assert np.array_equal(nearest.nearest(D, rect, (ow, oh)), warp.warp(D, rect, (ow, oh), m, flags, 0x11223344)), (rect, ow, oh)
            seen += 1
    assert seen >= 8


N_SRC = list(range(1, 70)) + [97, 224, 255, 256, 257, 511, 1000, 1023, 4097]
N_OUT = list(range(1, 70)) + [97, 224, 256, 299, 1000, 3000]


def test_against_torch_nearest_exact():
    """torch computes floor((X + 0.5) * scale) in float.  Every position where it differs from the integer definition has (2X + 1) * n_src
    divisible by 2 * n_out - the output pixel's centre lies exactly on the boundary of two source cells - and torch's index is exactly one
    lower: on those boundaries the integer definition is the exact one.  (110 such positions in these 5850 geometries with the torch this
    was written against; the number is printed, what is asserted is where they lie.)"""
    import torch
    differing = 0
    for n_src in N_SRC:
        src = torch.arange(n_src, dtype=torch.float32).reshape(1, 1, 1, n_src)
        for n_out in N_OUT:
            t = torch.nn.functional.interpolate(src, size=(1, n_out), mode="nearest-exact").reshape(-1).numpy().astype(np.int64)
            k = nearest.index(n_src, n_out)
            for X in np.flatnonzero(t != k):
                assert ((2 * int(X) + 1) * n_src) % (2 * n_out) == 0 and t[X] == k[X] - 1, (n_src, n_out, int(X), int(t[X]), int(k[X]))
                differing += 1
    assert len(N_SRC) * len(N_OUT) == 5850
    print(f"nearest-exact: {differing} boundary positions differ in 5850 geometries")
    # a two-dimensional item, away from the boundaries: 63 x 41 to 50 x 37 has none ((2X + 1) * 63 is odd, (2Y + 1) * 41 too)
    P = nearest.nearest(D4, (5, 3, 63, 41), (50, 37))
    T = torch.nn.functional.interpolate(torch.from_numpy(D4[3:44, 5:68].astype(np.float32)).permute(2, 0, 1)[None], size=(37, 50), mode="nearest-exact")
    assert np.array_equal(P, T[0].permute(1, 2, 0).numpy().astype(np.uint8))


@pytest.mark.parametrize("och", [3, 4])
@pytest.mark.parametrize("layout", [HWC, CHW, HW])
@pytest.mark.parametrize("dtype", [U8, F16, BF16, F32, I32, I64])
def test_convert_against_torch(dtype, layout, och):
    import torch
    P = nearest.nearest(D4[:, :, :och], (5, 3, 63, 41), (19, 11), 1)
    integer = dtype in (U8, I32, I64)
    f = tensors.fmt(dtype, layout) if integer else (dtype, layout, *IMAGENET)
    got = tensors.convert(P, f)
    assert got.flags.c_contiguous and got.dtype == tensors.numpy_dtype(dtype) and got.nbytes == 19 * 11 * (1 if layout == HW else och) * tensors.elem(dtype)
    t = torch.from_numpy(P)
    if integer:
        t = t.to({U8: torch.uint8, I32: torch.int32, I64: torch.int64}[dtype])
    else:
        t = t.to(torch.float32) * torch.from_numpy(IMAGENET[0][:och])
        t = (t + torch.from_numpy(IMAGENET[1][:och])).to({F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}[dtype])
    t = {HWC: t, CHW: t.permute(2, 0, 1), HW: t[..., 0]}[layout].contiguous()
    assert got.shape == tuple(t.shape)
    want = t.view(torch.int16).numpy().view(np.uint16) if dtype == BF16 else t.numpy()
    assert np.array_equal(got.view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)), (dtype, layout, och)
    if dtype == I64 and layout == HW:
        assert np.array_equal(got, torch.from_numpy(P)[..., 0].to(torch.int64).numpy()) and got.dtype.itemsize == 8 and got.dtype.byteorder in "<="


def test_formats_the_model_accepts_and_rejects():
    one, zero = (1.0,) * 4, (0.0,) * 4
    for dtype in (U8, F16, BF16, F32, I32, I64):
        for layout in (HWC, CHW, HW):
            assert tensors.wrong(tensors.fmt(dtype, layout)) == ""
    for dtype in (4, 7, 9, -1, 2 ** 32 - 1):
        assert "dtype" in tensors.wrong((dtype, HWC, one, zero))
    for layout in (2, 4, 9, -1):
        assert "layout" in tensors.wrong((F16, layout, one, zero))
    for dtype, name in ((U8, "QOIMI_TENSOR_U8"), (I32, "QOIMI_TENSOR_I32"), (I64, "QOIMI_TENSOR_I64")):
        for f in [(dtype, HW, (1.0, 1.0, 1.0, 0.5), zero), (dtype, HWC, one, (0.0, -0.0, 0.0, 0.0)), (dtype, CHW, one, (0.0, 0.0, 1.0, 0.0))]:
            assert tensors.wrong(tensors.fmt(*f)) == name + " takes scale 1 and bias +0 only", f
        assert "finite" in tensors.wrong(tensors.fmt(dtype, HW, (float("nan"), 1.0, 1.0, 1.0)))
    assert "finite" in tensors.wrong(tensors.fmt(F32, HW, (1.0, 1.0, 1.0, float("inf"))))      # HW ignores scale[3], but it must be finite
    with pytest.raises(ValueError):
        tensors.convert(D4, (4, HWC, one, zero))
    with pytest.raises(ValueError):
        tensors.convert(D4, (I64, 2, one, zero))


def test_the_model_dispatches_and_hw_takes_scale_0():
    f = (F32, HW, np.array([2.0, 3.0, 5.0, 7.0], np.float32), np.array([-1.0, 9.0, 9.0, 9.0], np.float32))
    got = tensors.tensors(D4, (5, 3, 63, 41), (9, 7), 2, FILTER_NEAREST, tensors.PLAIN, f)
    assert np.array_equal(got, nearest.nearest(D4, (5, 3, 63, 41), (9, 7), 2)[:, :, 0].astype(np.float32) * np.float32(2.0) + np.float32(-1.0))
    lab = tensors.tensors(D3, (0, 0, 37, 29), (37, 29), 0, FILTER_NEAREST, tensors.PLAIN, tensors.fmt(I64, HW))
    assert lab.dtype == np.int64 and np.array_equal(lab, D3[:, :, 0])
    w = tensors.warped_tensors(D4, (0, 0, 8, 8), (8, 8), warp.IDENTITY, warp.NEAREST, 0, warp.PLAIN, tensors.fmt(I32, HW))
    assert w.dtype == np.int32 and np.array_equal(w, D4[:8, :8, 0])
    for filt in (2, 4, 5, 7, 8, 10, -1):
        with pytest.raises(ValueError):
            tensors.tensors(D4, (0, 0, 8, 8), (4, 4), 0, filt)


def test_elem_and_the_old_signatures_are_unchanged():
    assert tensors.ELEM == {0: 1, 1: 2, 2: 2, 3: 4}
    assert tensors.INT_ELEM == {5: 4, 6: 8} and not set(tensors.ELEM) & set(tensors.INT_ELEM)
    assert [tensors.elem(d) for d in (U8, F16, BF16, F32, I32, I64)] == [1, 2, 2, 4, 4, 8]
    assert list(inspect.signature(tensors.convert).parameters) == ["P", "f"]
    assert list(inspect.signature(tensors.wrong).parameters) == ["f"]
    assert list(inspect.signature(tensors.size).parameters) == ["u8_bytes", "dtype"]
    assert list(inspect.signature(tensors.fmt).parameters) == ["dtype", "layout", "scale", "bias"]
    assert list(inspect.signature(tensors.tensors).parameters) == ["D", "rect", "out_size", "flags", "filter", "mode", "f"]
    assert tensors.size(12, I32) == 48 and tensors.size(12, I64) == 96 and tensors.size(12, F16) == 24 and tensors.size(0, I64) == 0
    assert tensors.size_hw(12, 3, I64) == 32 and tensors.size_hw(12, 4, U8) == 3 and tensors.size_hw(0, 4, I32) == 0
    assert tensors.DTYPE_NAMES["i32"] == I32 and tensors.DTYPE_NAMES["i64"] == I64 and tensors.LAYOUT_NAMES == {"hwc": HWC, "chw": CHW, "hw": HW}
