"""qoi_amd/tensors.py: convert - the normative statement of the tensor outputs - against an independent evaluation by torch on the CPU
(uint8 -> float32, one mul, one add, one narrowing; permuted for CHW), bit for bit in all four dtypes: all 256 values in every channel under the
ImageNet normalisation, under 1 / 255, under a scale that takes binary16 to infinity, under one that lands in the subnormals of binary16 and of
bfloat16, under products that lie exactly halfway between two bfloat16 / binary16 values (ties go to even), and where a negative scale or bias
decides between -0 and +0.  U8 with HWC is the identity, U8 with CHW the transpose."""
import numpy as np
import pytest
import torch

from qoi_amd import bilinear, resize, tensors, warp
from qoi_amd.tensors import BF16, CHW, F16, F32, HWC, U8

TORCH = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}
T = 2.0 ** -7
FORMATS = {
    "imagenet": tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "unit": ([1 / 255] * 4, [0.0] * 4),
    "f16 overflows": ([300.0, 257.0, 256.0, 1e36], [0.0, -16.0, 240.0, 1e38]),             # 255 * 300 > 65504; 255 * 1e36 + 1e38 > float32
    "subnormals": ([2.0 ** -24, 3e-8, 1e-40, 5e-41], [0.0, 1e-7, 0.0, -1e-39]),             # binary16 below 2^-14, bfloat16 / binary32 below 2^-126
    "ties": ([1 + T / 2, 1 + T + T / 2, 1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11], [0.0] * 4),
    "signed zeros": ([-1.0, 1.0, -1e-30, 1.0], [-0.0, -5.0, -0.0, -0.0]),
}


def ramp(och):
    """uint8[256, och + 1, och]: all 256 values in every channel, beside every value of another channel once"""
    P = np.zeros((256, och + 1, och), np.uint8)
    for c in range(och):
        P[:, c, c] = np.arange(256)
        P[:, och, c] = (np.arange(256) * (2 * c + 3) + 11 * c) % 256
    return P


def by_torch(P, dtype, layout, scale, bias):
    och = P.shape[2]
    t = torch.from_numpy(P).to(torch.float32).mul(torch.tensor(np.asarray(scale, np.float32)[:och])).add(torch.tensor(np.asarray(bias, np.float32)[:och])).to(TORCH[dtype])
    if layout == CHW:
        t = t.permute(2, 0, 1)
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.itemsize])


@pytest.mark.parametrize("name", list(FORMATS))
@pytest.mark.parametrize("och", [3, 4])
def test_convert_against_torch(name, och):
    scale, bias = FORMATS[name]
    P = ramp(och)
    for dtype in (F16, BF16, F32):
        for layout in (HWC, CHW):
            f = tensors.fmt(dtype, layout, scale, bias)
            got = tensors.convert(P, f)
            assert got.dtype == tensors.numpy_dtype(dtype) and got.flags["C_CONTIGUOUS"]
            assert got.shape == ((och, 256, och + 1) if layout == CHW else (256, och + 1, och))
            want = by_torch(P, dtype, layout, f[2], f[3])
            assert np.array_equal(bits(got), bits(want)), (name, dtype, layout, int(np.argmax(bits(got).reshape(-1) != bits(want).reshape(-1))))


def test_the_inputs_are_what_they_are_called():
    """the overflow, the subnormals, the ties and the signed zeros really occur (and go the way the definition says)"""
    P = ramp(4)
    col = lambda name, dtype, c: bits(tensors.convert(P, tensors.fmt(dtype, HWC, *FORMATS[name])))[:, c, c]
    assert col("f16 overflows", F16, 0)[255] == 0x7C00 and col("f16 overflows", F16, 0)[200] != 0x7C00
    assert col("f16 overflows", F16, 2)[255] == 0x7C00 and col("f16 overflows", F16, 1)[255] == 0x7BFF          # 65520: the tie to infinity; 65519
    assert col("f16 overflows", F32, 3)[255] == 0x7F800000 and col("f16 overflows", BF16, 3)[255] == 0x7F80
    assert list(col("subnormals", F16, 0)[:4]) == [0, 1, 2, 3]                                                   # multiples of 2^-24
    assert 0 < col("subnormals", F32, 2)[7] < 0x00800000 and 0 < col("subnormals", BF16, 2)[100] < 0x0080
    assert col("subnormals", F32, 3)[1] >> 31 == 1                                                               # a negative subnormal
    # v * (1 + 2^-8) = v + v * 2^-8 is halfway between two bfloat16 at v = 1, 2, 4: down to the even one; with 1 + 2^-7 + 2^-8: up
    assert list(col("ties", BF16, 0)[[1, 2, 4]]) == [0x3F80, 0x4000, 0x4080] and list(col("ties", BF16, 1)[[1, 2, 4]]) == [0x3F82, 0x4002, 0x4082]
    assert list(col("ties", F16, 2)[[1, 2, 4]]) == [0x3C00, 0x4000, 0x4400] and list(col("ties", F16, 3)[[1, 2, 4]]) == [0x3C02, 0x4002, 0x4402]
    for dtype, top in ((F16, 15), (BF16, 15), (F32, 31)):
        assert col("signed zeros", dtype, 0)[0] == 1 << top                                                      # -0 * 1 + -0 = -0
        assert col("signed zeros", dtype, 1)[5] == 0                                                             # 5 - 5 = +0
        assert col("signed zeros", dtype, 3)[0] == 0                                                             # +0 + -0 = +0
    assert col("signed zeros", F16, 2)[9] == 0x8000 and col("signed zeros", F32, 2)[9] != 0x80000000            # underflows in binary16 only


def test_u8_is_the_identity_or_the_transpose():
    rng = np.random.default_rng(3)
    for och in (3, 4):
        P = rng.integers(0, 256, size=(7, 5, och), dtype=np.uint8)
        assert np.array_equal(tensors.convert(P, tensors.fmt(U8, HWC)), P)
        assert np.array_equal(tensors.convert(P, tensors.fmt(U8, CHW)), P.transpose(2, 0, 1))
    for bad in (tensors.fmt(U8, HWC, [2.0] * 4), tensors.fmt(U8, HWC, [1.0] * 4, [-0.0] * 4), tensors.fmt(F16, 2), tensors.fmt(4, HWC),
                tensors.fmt(F32, HWC, [np.inf] * 4), tensors.fmt(F32, HWC, [1.0] * 4, [np.nan] * 4)):
        assert tensors.wrong(bad)
        with pytest.raises(ValueError):
            tensors.convert(P, bad)
    assert not tensors.wrong(tensors.fmt(F16, CHW, [1e30] * 4, [-1e30] * 4))


def test_items_are_the_u8_models_converted():
    rng = np.random.default_rng(4)
    D = rng.integers(0, 256, size=(23, 31, 4), dtype=np.uint8)
    f = tensors.fmt(BF16, CHW, *FORMATS["imagenet"])
    rect, out = (3, 2, 20, 17), (9, 5)
    assert np.array_equal(tensors.tensors(D, rect, out, resize.FLIP_X, tensors.FILTER_AREA, tensors.ALPHA_WEIGHTED, f),
                          tensors.convert(resize.resize(D, rect, out, resize.FLIP_X, resize.ALPHA_WEIGHTED), f))
    assert np.array_equal(tensors.tensors(D, rect, out, 3, tensors.FILTER_BILINEAR, tensors.PLAIN, f), tensors.convert(bilinear.bilinear(D, rect, out, 3), f))
    m = warp.rotation((20, 17), out, 30.0)
    assert np.array_equal(tensors.warped_tensors(D, rect, out, m, warp.REPLICATE, 0, tensors.PLAIN, f), tensors.convert(warp.warp(D, rect, out, m, warp.REPLICATE), f))
    assert tensors.plan is __import__("qoi_amd.crops", fromlist=["plan"]).plan
    assert tensors.size(45, F16) == 90 and tensors.size(45, F32) == 180 and tensors.size(0, BF16) == 0
    s, b = tensors.normalise((0.5,), (0.25,))
    assert s.dtype == np.float32 and s[0] == np.float32(1 / (255 * 0.25)) and b[0] == np.float32(-2.0) and s[3] == np.float32(1 / 255) and b[3] == 0
