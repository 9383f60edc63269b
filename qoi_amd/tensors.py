"""What qoimi_decode_tensors and qoimi_decode_warped_tensors compute, stated in NumPy: the normative definition of the tensor outputs (the C
header repeats it; qoi_amd/csrc/qoi_tensor_core.h holds the arithmetic of the kernels).

Let P be the uint8[oh, ow, och] result of the underlying call - ``resize.resize`` for ``FILTER_AREA``, ``bilinear.bilinear`` for
``FILTER_BILINEAR``, ``bicubic.bicubic`` for ``FILTER_BICUBIC``, ``lanczos.lanczos`` for ``FILTER_LANCZOS``, ``nearest.nearest`` for ``FILTER_NEAREST`` and ``mode.mode`` for ``FILTER_MODE`` (which have no u8 call of their own), ``warp.warp`` for the warp call - with the same item, channels and mode, byte for byte, flips included.  A format is
(dtype, layout, scale, bias): scale and bias are four binary32 numbers, per channel r, g, b, a.  Element (Y, X, c) has the value v = P[Y][X][c]:

    U8      the element is v; scale must be all 1 and bias all +0
    F32     t = float32(v); m = t * scale[c], rounded to nearest even in binary32; s = m + bias[c], rounded to nearest even in binary32 -
            TWO roundings, never a fused multiply-add; the element is s
    F16     s converted to binary16, round to nearest even
    BF16    s converted to bfloat16, round to nearest even: on the bits of s, (bits + 0x7FFF + (bits >> 16 & 1)) >> 16
    I32     the element is v as a little-endian two's-complement integer of 4 bytes; scale must be all 1 and bias all +0, as for U8
    I64     ... of 8 bytes: the class indices a loss function takes

Subnormals are kept in every format; a result too large becomes infinity; scale and bias are finite, so no NaN arises.  The layout is
``HWC`` - [oh, ow, och], P's own -, ``CHW`` - [och, oh, ow] - or ``HW`` - [oh, ow]: only the FIRST channel (r) of each pixel, as one plane, with
scale[0] and bias[0] (the others are ignored but must still be finite); och still says how the image is decoded -, tightly packed.  Every
layout goes with every dtype.  U8 with HWC is P itself; everything else is a pure function
of P, so the exact-integer definitions of the filters stand as they are.

``HW_ID24`` is one plane [oh, ow] as ``HW`` is, but its element is ``r | g << 8 | b << 16`` of the pixel: the 24-bit id of the COCO panoptic
convention, what ``tiles.LABELS_ID24`` packs.  Alpha is ignored; och still says how the image is decoded.  It goes with I32 and I64 only
(the last of ``wrong``'s checks) and with every filter and the warp, but means something only under the selections - ``FILTER_NEAREST`` /
``FILTER_MODE``, the warp's NEAREST / VOTE2 / VOTE4 -, which invent no pixel.

NumPy has no bfloat16: ``convert`` returns BF16 as uint16 holding the bits (``numpy_dtype`` says what an output's array is).

Normalisation (p / 255 - mean) / std is scale = 1 / (255 * std), bias = -mean / std: ``normalise`` computes both in float64 and rounds once.

The plan is ``crops.plan`` over the items' rectangles, as for every gather call.
"""
from typing import Sequence, Tuple

import numpy as np

from . import bicubic, bilinear, crops, lanczos, mode, nearest, resize, warp

U8, F16, BF16, F32 = 0, 1, 2, 3
I32, I64 = 5, 6                 # (4 is not a dtype)
HWC, CHW = 0, 1
HW = 3                          # (2 is not a layout)
HW_ID24 = 5                     # (nor is 4)
FILTER_AREA, FILTER_BILINEAR = 0, 1
FILTER_BICUBIC = 3              # (2 is not a filter)
FILTER_LANCZOS = 6              # (nor are 4, 5 and 7)
FILTER_NEAREST = 9              # (nor is 8)
FILTER_MODE = 11                # (nor is 10)
_FILTERS = {FILTER_AREA: resize.resize, FILTER_BILINEAR: bilinear.bilinear, FILTER_BICUBIC: bicubic.bicubic, FILTER_LANCZOS: lanczos.lanczos,
            FILTER_NEAREST: nearest.nearest, FILTER_MODE: mode.mode}
ELEM = {U8: 1, F16: 2, BF16: 2, F32: 4}
INT_ELEM = {I32: 4, I64: 8}     # the integer class-index dtypes, beside ELEM
DTYPE_NAMES = {"u8": U8, "f16": F16, "bf16": BF16, "f32": F32, "i32": I32, "i64": I64}
LAYOUT_NAMES = {"hwc": HWC, "chw": CHW, "hw": HW}
ID_LAYOUT_NAMES = {"id24": HW_ID24}     # the id layouts, beside LAYOUT_NAMES
_INT_NAMES = {U8: "QOIMI_TENSOR_U8", I32: "QOIMI_TENSOR_I32", I64: "QOIMI_TENSOR_I64"}
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED

plan = crops.plan


def fmt(dtype: int = U8, layout: int = HWC, scale: Sequence[float] = (1.0, 1.0, 1.0, 1.0), bias: Sequence[float] = (0.0, 0.0, 0.0, 0.0)):
    """A format as (dtype, layout, float32[4] scale, float32[4] bias); a shorter scale or bias is padded with 1 / 0."""
    s = np.ones(4, np.float32)
    b = np.zeros(4, np.float32)
    s[:len(scale)] = np.asarray(scale, np.float32)
    b[:len(bias)] = np.asarray(bias, np.float32)
    return int(dtype), int(layout), s, b


def normalise(mean: Sequence[float], std: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """(scale, bias) as float32[4] for (p / 255 - mean) / std: 1 / (255 * std) and -mean / std in float64, rounded once; channels beyond
    those given get 1 / 255 and 0."""
    m = np.zeros(4, np.float64)
    s = np.ones(4, np.float64)
    m[:len(mean)] = np.asarray(mean, np.float64)
    s[:len(std)] = np.asarray(std, np.float64)
    return (1.0 / (255.0 * s)).astype(np.float32), (-m / s).astype(np.float32)


def elem(dtype: int) -> int:
    """Bytes of an element: ``ELEM`` or ``INT_ELEM``."""
    return ELEM[dtype] if dtype in ELEM else INT_ELEM[dtype]


def wrong(f) -> str:
    """"" if the calls accept the format, else what is wrong with it - in the order the calls look."""
    dtype, layout, scale, bias = f
    if dtype not in ELEM and dtype not in INT_ELEM:
        return "unknown dtype"
    if layout not in (HWC, CHW, HW, HW_ID24):
        return "unknown layout"
    scale, bias = np.asarray(scale, np.float32), np.asarray(bias, np.float32)
    if scale.shape != (4,) or bias.shape != (4,) or not (np.isfinite(scale).all() and np.isfinite(bias).all()):
        return "scale or bias is not finite"
    if dtype in _INT_NAMES and not ((scale == 1.0).all() and (bias.view(np.uint32) == 0).all()):
        return _INT_NAMES[dtype] + " takes scale 1 and bias +0 only"
    if layout == HW_ID24 and dtype not in INT_ELEM:
        return "QOIMI_TENSOR_HW_ID24 takes QOIMI_TENSOR_I32 or QOIMI_TENSOR_I64 only"
    return ""


def numpy_dtype(dtype: int):
    """The dtype of the array ``convert`` returns: BF16 as the uint16 of its bits."""
    return {U8: np.uint8, F16: np.float16, BF16: np.uint16, F32: np.float32, I32: np.dtype("<i4"), I64: np.dtype("<i8")}[dtype]


def bf16_bits(s: np.ndarray) -> np.ndarray:
    """float32 (finite or infinite) -> uint16: the bfloat16 nearest to it, ties to even, by integer arithmetic on its bits."""
    bits = np.ascontiguousarray(s, np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def convert(P: np.ndarray, f) -> np.ndarray:
    """P uint8[oh, ow, och] (och 3 or 4), f a format -> [oh, ow, och] (HWC), [och, oh, ow] (CHW) or [oh, ow] (HW: channel 0) of
    ``numpy_dtype(dtype)``, contiguous; [oh, ow] of ``r | g << 8 | b << 16`` under ``HW_ID24``."""
    P = np.asarray(P)
    if P.ndim != 3 or P.shape[2] not in (3, 4) or P.dtype != np.uint8:
        raise ValueError("convert: P is uint8[oh, ow, 3 or 4]")
    what = wrong(f)
    if what:
        raise ValueError("convert: " + what)
    dtype, layout, scale, bias = f
    och = P.shape[2]
    if layout == HW_ID24:
        ids = P[:, :, 0].astype(np.uint32) | (P[:, :, 1].astype(np.uint32) << 8) | (P[:, :, 2].astype(np.uint32) << 16)
        return np.ascontiguousarray(ids.astype(numpy_dtype(dtype)))
    if dtype == U8:
        out = P
    elif dtype in INT_ELEM:
        out = P.astype(numpy_dtype(dtype))
    else:
        with np.errstate(over="ignore", under="ignore"):
            m = P.astype(np.float32) * np.asarray(scale, np.float32)[:och]      # (one float32 operation per line: two roundings)
            s = m + np.asarray(bias, np.float32)[:och]
            out = s if dtype == F32 else (s.astype(np.float16) if dtype == F16 else bf16_bits(s))
    if layout == HW:
        return np.ascontiguousarray(out[:, :, 0])
    return np.ascontiguousarray(out.transpose(2, 0, 1) if layout == CHW else out)


def size(u8_bytes: int, dtype: int) -> int:
    """Bytes of an output whose u8 form takes u8_bytes (``resize.size``, ``bilinear.size``, ``bicubic.size``, ``lanczos.size``, ``warp.size``; 0 stays 0)."""
    return u8_bytes * elem(dtype)


def size_hw(u8_bytes: int, och: int, dtype: int) -> int:
    """... under ``HW`` and ``HW_ID24``: one element per pixel, u8_bytes / och of them."""
    return u8_bytes // och * elem(dtype)


def tensors(D: np.ndarray, rect, out_size, flags: int = 0, filter: int = FILTER_AREA, mode: int = PLAIN, f=None) -> np.ndarray:
    """One item of qoimi_decode_tensors: ``convert`` of ``resize.resize``, ``bilinear.bilinear``, ``bicubic.bicubic``, ``lanczos.lanczos``,
    ``nearest.nearest`` or ``mode.mode`` of the same arguments."""
    if filter not in _FILTERS:
        raise ValueError("tensors: unknown filter")
    P = _FILTERS[filter](D, rect, out_size, flags, mode)
    return convert(P, f if f is not None else fmt())


def warped_tensors(D: np.ndarray, rect, out_size, matrix=warp.IDENTITY, flags: int = 0, fill: int = 0, mode: int = PLAIN, f=None) -> np.ndarray:
    """One item of qoimi_decode_warped_tensors: ``convert`` of ``warp.warp`` of the same arguments."""
    return convert(warp.warp(D, rect, out_size, matrix, flags, fill, mode), f if f is not None else fmt())
