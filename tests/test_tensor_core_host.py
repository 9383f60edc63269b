"""The store end of the tensor kernels (qoi_amd/csrc/qoi_tensor_core.h: pixel word -> channel values -> scale, bias, two roundings -> narrowing
-> whole aligned stores at the HWC or CHW place, flipped or not) compiled with g++ (tests/host/tensor_host.cpp) and compared with the Python
model qoi_amd/tensors.py: convert on the CPU: every dtype x layout x och 3 and 4 x the four flip values x the filter tiles' and the warp tile's
sink, outputs of 1 x 1, 5 x 3 and 17 x 16, the output at every multiple of the element size within 16 bytes.  The counting memory functor
checks that each output byte is written exactly once, that no byte beside an output is written and that every store is naturally aligned.
The narrowing to binary16 is compared with NumPy's over every exponent and around every tie.  The same source is built as a stand-alone
program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing sanitized is loaded into this process)."""
import numpy as np
import pytest

import hostbuild
from hostbuild import cint, f32, f32p, i64, u32, u32p, u64, u8p
from qoi_amd import tensors
from qoi_amd.tensors import BF16, CHW, F16, F32, HWC, U8

SRC = "tensor_host.cpp"
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FORMATS = {"imagenet": IMAGENET, "unit": (np.full(4, 1 / 255, np.float32), np.zeros(4, np.float32)),
           "wild": (np.array([300.0, 1e-6, 2.4e-8, 1e-40], np.float32), np.array([-300.0, 6e-8, -1e-41, -0.0], np.float32)),
           "huge": (np.array([-257.0, 65504 / 255, 1e30, 3e38], np.float32), np.array([65535.0, 16.0, -1e30, 3e38], np.float32))}


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "tensor_host_run": (i64, [u32p, u32, u32, u32, u32, cint, u32, u32, f32p, f32p, u64, u64, u8p, u8p, u64]),
        "tensor_host_value": (u32, [u32, f32, f32, u32]),
        "tensor_host_f16": (u32, [u32]),
        "tensor_host_bf16": (u32, [u32]),
        "tensor_host_elem": (u32, [u32])})


def walk(lib, P, och, flags, warp, f, a):
    """P uint8[oh, ow, 4] handed over pixel by pixel, the tensor written at BASE + BAND + a; returns (stores, output bytes)"""
    oh, ow = P.shape[:2]
    dtype, layout, scale, bias = f
    words = np.ascontiguousarray(P).view(np.uint32).reshape(-1)
    band = hostbuild.Banded(ow * oh * och * tensors.ELEM[dtype], a)
    stores = lib.tensor_host_run(words.ctypes.data_as(u32p), ow, oh, och, flags, warp, dtype, layout, scale.ctypes.data_as(f32p), bias.ctypes.data_as(f32p), *band.args)
    what = (dtype, layout, och, flags, warp, a, (ow, oh))
    assert stores >= 0, (what, stores)      # (negative: a store out of bounds or misaligned)
    return stores, band.inside(what)


@pytest.mark.parametrize("layout", [HWC, CHW])
@pytest.mark.parametrize("dtype", [U8, F16, BF16, F32])
def test_store_against_the_model(host_lib, dtype, layout):
    rng = np.random.default_rng(dtype * 2 + layout)
    elem = tensors.ELEM[dtype]
    assert host_lib.tensor_host_elem(dtype) == elem
    for name, (scale, bias) in FORMATS.items():
        if dtype == U8 and name != "imagenet":
            continue
        f = tensors.fmt(dtype, layout) if dtype == U8 else (dtype, layout, scale, bias)
        for (ow, oh) in [(1, 1), (5, 3), (17, 16)]:
            P = rng.integers(0, 256, size=(oh, ow, 4), dtype=np.uint8)
            P.reshape(-1)[:min(P.size, 8)] = [0, 255, 1, 254, 128, 127, 2, 3][:min(P.size, 8)]
            for och in (3, 4):
                for flags in range(4):
                    Q = P[::-1] if flags & 2 else P
                    Q = Q[:, ::-1] if flags & 1 else Q
                    for warp, shown in ((0, Q), (1, P)):                   # (the warp tile's sink knows no flips)
                        want = tensors.convert(shown[:, :, :och], f).view(np.uint8).reshape(-1)
                        for a in range(0, 16, elem):
                            stores, got = walk(host_lib, P, och, flags, warp, f, a)
                            assert np.array_equal(got, want), (name, dtype, layout, och, flags, warp, a, (ow, oh), int(np.argmax(got != want)))
                            one_dword = dtype == U8 and layout == HWC and och == 4 and a % 4 == 0
                            assert stores == (ow * oh if one_dword else ow * oh * och)


def test_values_against_numpy(host_lib):
    """tensor_value for all 256 values under every format; the binary16 narrowing over every exponent, around every tie and at the edges"""
    for name, (scale, bias) in FORMATS.items():
        for c in range(4):
            P = np.zeros((256, 1, 4), np.uint8)
            P[:, 0, c] = np.arange(256)
            for dtype in (F16, BF16, F32):
                want = tensors.convert(P, (dtype, HWC, scale, bias))[:, 0, c]
                want = want.view({2: np.uint16, 4: np.uint32}[want.itemsize])
                got = [host_lib.tensor_host_value(v, float(scale[c]), float(bias[c]), dtype) for v in range(256)]
                assert got == [int(w) for w in want], (name, c, dtype)
    rng = np.random.default_rng(5)
    h = np.arange(0, 0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)             # every finite binary16 ...
    nxt = np.append(h[1:], 65536.0)
    mid = ((h + nxt) / 2).astype(np.float32)                                 # ... and the value halfway to the next one: exact in binary32
    cases = np.concatenate([h.astype(np.float32), mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)),
                            rng.integers(0, 0x7F800000, size=20000).astype(np.uint32).view(np.float32),
                            np.array([0.0, 65504.0, 65519.996, 65520.0, 65536.0, 1e38, np.inf, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, 1e-45], np.float32)])
    cases = np.concatenate([cases, -cases])
    with np.errstate(over="ignore"):
        want16 = cases.astype(np.float16).view(np.uint16)
    bits = cases.view(np.uint32)
    got16 = np.array([host_lib.tensor_host_f16(int(b)) for b in bits], np.uint16)
    assert np.array_equal(got16, want16), int(np.argmax(got16 != want16))
    gotbf = np.array([host_lib.tensor_host_bf16(int(b)) for b in bits], np.uint16)
    assert np.array_equal(gotbf, tensors.bf16_bits(cases))


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "TENSOR_HOST_MAIN", tmp_path) == "tensor_host: 9216 items ok\n"
