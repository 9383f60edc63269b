"""Tensors as the source of qoimi_encode_tiles, the model (qoi_amd/tiles.py: convert, source_flags, tile with QOIMI_TILE_SRC*): the conversion
against an independent statement in exact rational arithmetic, the nine round trips with qoimi_decode_tensors' elements over all 256 bytes,
ties, special values, and the identity of a tile with SRC alone.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from qoi_amd import tensors, tiles

DTYPES = (tiles.F16, tiles.BF16, tiles.F32)
RANGES = (tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES)


def bits_of(values, dtype):
    """float values -> the array of that dtype holding them rounded to it (BF16: uint16 bits)"""
    v = np.asarray(values, np.float32)
    if dtype == tiles.F32:
        return v
    if dtype == tiles.F16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16)
    return tensors.bf16_bits(v)


def f32_round(q: Fraction) -> float:
    """the binary32 nearest to the rational q, ties to even (via float64: exact for the products and sums of two binary32 numbers, which
    hold at most 48 and, for operands whose exponents lie within 29 of each other, 53 significant bits - asserted)"""
    d = float(q)
    assert Fraction(d) == q, "not exact in float64: the test's own arithmetic would round twice"
    return float(np.float32(d))


def byte_by_definition(x: float, rng: int) -> int:
    """one finite or infinite or NaN binary32 element by the header's words, in rational arithmetic"""
    if np.isnan(x):
        return 0
    if np.isinf(x):
        t = x
    elif rng == tiles.UNIT:
        t = f32_round(Fraction(x) * 255)
    elif rng == tiles.SYMMETRIC:
        m = f32_round(Fraction(x) * Fraction(255, 2))
        if np.isinf(m):
            t = m
        else:
            s = Fraction(m) + Fraction(255, 2)
            d = float(s)
            t = float(np.float32(d)) if Fraction(d) == s else float(np.float32(m) + np.float32(127.5))   # far apart: the sum is the larger operand
    else:
        t = x
    if t <= 0:
        return 0
    if t >= 255:
        return 255
    q = Fraction(t)
    lo = int(q)                                                  # t > 0
    rest = q - lo
    return lo + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1) else 0)


def widened(a, dtype):
    return tiles.widen(np.asarray(a), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rng", RANGES)
def test_convert_against_the_definition(dtype, rng):
    r = np.random.default_rng(dtype * 16 + (rng >> 8))
    scale = {tiles.UNIT: 1.0, tiles.SYMMETRIC: 2.0, tiles.BYTES: 255.0}[rng]
    x = r.uniform(-0.25, 1.25, size=3000) * scale - (1.0 if rng == tiles.SYMMETRIC else 0.0)
    # and the neighbourhood of every tie k + 1/2
    ties = (np.arange(0, 256) + 0.5)
    ties = {tiles.UNIT: ties / 255.0, tiles.SYMMETRIC: ties / 127.5 - 1.0, tiles.BYTES: ties}[rng]
    x = np.concatenate([x, ties, np.nextafter(ties.astype(np.float32), np.float32(9)), np.nextafter(ties.astype(np.float32), np.float32(-9))])
    a = bits_of(x, dtype)
    got = tiles.to_bytes(widened(a, dtype), rng)
    want = [byte_by_definition(float(v), rng) for v in widened(a, dtype)]
    assert got.tolist() == want
    assert 0 in want and 255 in want and len(set(want)) == 256


def test_convert_layouts_and_dtypes():
    r = np.random.default_rng(3)
    for sch in (3, 4):
        B = r.integers(0, 256, size=(5, 7, sch), dtype=np.uint8)
        assert np.array_equal(tiles.convert(B, tiles.SRC), B)
        assert np.array_equal(tiles.convert(np.ascontiguousarray(B.transpose(2, 0, 1)), tiles.source_flags(tiles.U8, tiles.CHW)), B)
        for dtype in DTYPES:
            A = bits_of(B.astype(np.float32), dtype)               # 0..255 are exact in all three
            for layout in (tiles.HWC, tiles.CHW):
                T = np.ascontiguousarray(A.transpose(2, 0, 1)) if layout == tiles.CHW else A
                assert np.array_equal(tiles.convert(T, tiles.source_flags(dtype, layout, tiles.BYTES)), B), (sch, dtype, layout)
    with pytest.raises(ValueError):
        tiles.convert(B.astype(np.float32), tiles.SRC)             # the array is not the flags' dtype
    with pytest.raises(ValueError):
        tiles.convert(B, tiles.SRC_CHW)                            # a bit without SRC
    with pytest.raises(ValueError):
        tiles.convert(B, tiles.SRC | tiles.SRC_BYTES)              # a range with u8
    with pytest.raises(ValueError):
        tiles.convert(B.astype(np.float32), tiles.SRC | tiles.SRC_F32 | 768)
    with pytest.raises(ValueError):
        tiles.source_flags(tiles.U8, tiles.HWC, tiles.SYMMETRIC)
    assert tiles.source_flags(tiles.BF16, tiles.CHW, tiles.SYMMETRIC) == 16 | 32 | 128 | 256
    assert tiles.source_format(16 | 32 | 192 | 512 | 3) == (tiles.F32, tiles.CHW, tiles.BYTES)
    assert tiles.source_bytes(7, 5, 3, tiles.source_flags(tiles.F16)) == 210 and tiles.source_bytes(7, 5, 4, 0) == 140


PAIRINGS = [(tiles.UNIT, 1.0 / 255.0, 0.0), (tiles.SYMMETRIC, 2.0 / 255.0, -1.0), (tiles.BYTES, 1.0, 0.0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", PAIRINGS, ids=["unit", "symmetric", "bytes"])
def test_round_trip_with_decode_tensors(dtype, pairing):
    """every byte v: the element qoimi_decode_tensors writes for v converts back to v - exhaustive, nine pairs"""
    rng, scale, bias = pairing
    P = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    fmt = tensors.fmt(dtype, tensors.HWC, (scale,) * 4, (bias,) * 4)
    E = tensors.convert(P, fmt)
    assert E.dtype == tiles.SOURCE_ARRAYS[dtype]
    back = tiles.convert(E, tiles.source_flags(dtype, tiles.HWC, rng))
    assert np.array_equal(back, P)


def test_ties_in_bytes():
    for dtype in DTYPES:
        got = tiles.to_bytes(widened(bits_of([0.5, 1.5, 2.5, 254.5, 3.5, 253.5], dtype), dtype), tiles.BYTES)
        assert got.tolist() == [0, 2, 2, 254, 4, 254], dtype      # (bfloat16 holds 254.5 and 253.5 as 254: the element is no tie there)


def specials(dtype):
    """(bits as the dtype's array, the values widened)"""
    sub = {tiles.F16: np.array([1], np.uint16).view(np.float16), tiles.BF16: np.array([1], np.uint16), tiles.F32: np.array([1], np.uint32).view(np.float32)}[dtype]
    with np.errstate(over="ignore"):
        a = bits_of([np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 65504.0], dtype)
    a = np.concatenate([a, sub])
    return a, widened(a, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype):
    a, x = specials(dtype)
    assert np.isnan(x[0]) and x[1] == np.inf and x[2] == -np.inf and np.signbit(x[3]) and x[3] == 0 and x[7] > 0
    if dtype == tiles.F16:
        assert x[4] == np.inf and x[5] == -np.inf and x[6] == 65504.0 and x[7] == 2.0 ** -24
    for rng in RANGES:
        got = tiles.to_bytes(x, rng).tolist()
        #       NaN  +inf -inf -0.0 1e30 -1e30 65504 smallest subnormal
        assert got == [0, 255, 0, 128 if rng == tiles.SYMMETRIC else 0, 255, 0, 255, 128 if rng == tiles.SYMMETRIC else 0], (dtype, rng)
        assert got == [byte_by_definition(float(v), rng) for v in x]


def test_src_alone_is_the_tile_without_it():
    r = np.random.default_rng(11)
    for (w, h, sch) in [(1, 1, 3), (5, 3, 4), (37, 23, 3), (70, 9, 4)]:
        S = r.integers(0, 256, size=(h, w, sch), dtype=np.uint8)
        rects = [(0, 0, w, h)] + ([(1, 0, w - 2, h), (w - 4, 1, 4, h - 1)] if w > 4 else [])
        for (x, y, cw, ch) in rects:
            for flips in range(4):
                for och in (0, 3, 4):
                    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED, tiles.NEAREST, tiles.MODE):
                        t = (0, x, y, cw, ch, 1, flips)
                        assert np.array_equal(tiles.tile(S, (0, x, y, cw, ch, 1, flips | tiles.SRC), och, mode), tiles.tile(S, t, och, mode))
                    assert tiles.size(w, h, sch, (0, x, y, cw, ch, 1, flips | tiles.SRC), och) == tiles.size(w, h, sch, t, och)


def test_tile_of_a_tensor_is_the_tile_of_its_bytes():
    r = np.random.default_rng(12)
    A = r.uniform(-1.5, 1.5, size=(4, 9, 13)).astype(np.float16)
    flags = tiles.source_flags(tiles.F16, tiles.CHW, tiles.SYMMETRIC)
    B = tiles.convert(A, flags)
    assert B.shape == (9, 13, 4) and B.min() == 0 and B.max() == 255
    t = (0, 2, 1, 10, 7, 1)
    for flips in range(4):
        for och in (0, 3, 4):
            assert np.array_equal(tiles.tile(A, t + (flags | flips,), och), tiles.tile(B, t + (flips,), och))
    with pytest.raises(ValueError):
        tiles.tile(A, (0, 2, 1, 10, 7, 2, flags))                 # factor 2 over a tensor source


def test_size_plan_and_items_with_the_bits():
    f16 = tiles.source_flags(tiles.F16, tiles.CHW)
    assert tiles.size(8, 8, 3, (0, 0, 0, 8, 8, 1, f16 | 3), 4) == (256, 8, 8)
    for bad in (tiles.SRC_CHW, tiles.SRC_F16, tiles.SRC_BYTES, tiles.SRC | tiles.SRC_F32 | 768, tiles.SRC | tiles.SRC_SYMMETRIC, 4, 8, 1 << 10, 1 << 31):
        assert tiles.size(8, 8, 3, (0, 0, 0, 8, 8, 1, bad), 4) == (0, 0, 0), bad
    assert tiles.size(8, 8, 3, (0, 0, 0, 8, 8, 2, f16), 4) == (0, 0, 0)
    descs = [(8, 8, 3), (5, 3, 4)]
    ts = [(0, 0, 0, 8, 8, 1, f16), (1, 0, 0, 5, 3, 1, tiles.SRC), (0, 1, 1, 2, 2, 1, f16 | 1)]
    plain = [(t[0], t[1], t[2], t[3], t[4], t[5], t[6] & 3) for t in ts]
    assert tiles.plan(descs, ts, 0, 0) == tiles.plan(descs, plain, 0, 0)       # no size changes
    with pytest.raises(ValueError):
        tiles.plan(descs, ts[:2] + plain[2:], 0, 0)                # a byte tile in a tensor call
    with pytest.raises(ValueError):
        tiles.plan(descs, ts[:2] + [(0, 1, 1, 2, 2, 1, tiles.SRC)], 0, 0)      # image 0 in two formats
    for cw, ch in [(1, 1), (4, 1), (5, 1), (37, 23), (1024, 1), (1025, 1), (2200, 2000)]:
        assert tiles.ingest_items(cw, ch) == (cw * ch + 3) // 4
        assert tiles.ingest_tiles(cw, ch) == (tiles.ingest_items(cw, ch) + 255) // 256
    assert tiles.INGEST_PIXELS == 4 and tiles.THREADS == 256


def test_the_tool_plans_its_call():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import qoifromtensor_mi355x as tool
    assert tool.plan_call((5, 3, 17, 30), np.float16, "symmetric") == (5, 30, 17, 3, tiles.source_flags(tiles.F16, tiles.CHW, tiles.SYMMETRIC), 30 * 17 * 3 * 2)
    assert tool.plan_call((2, 17, 30, 4), np.float32, "bytes") == (2, 30, 17, 4, tiles.source_flags(tiles.F32, tiles.HWC, tiles.BYTES), 30 * 17 * 4 * 4)
    assert tool.plan_call((2, 3, 9, 3), np.uint8, "bytes") == (2, 3, 9, 3, tiles.source_flags(tiles.U8, tiles.CHW), 81)       # both fit: CHW first; u8 has no range
    assert tool.plan_call((2, 3, 9, 3), np.uint8, "unit", "hwc") == (2, 9, 3, 3, tiles.SRC, 81)
    for shape, dtype in [((5, 2, 17, 30), np.float16), ((3, 17, 30), np.uint8), ((1, 3, 17, 30), np.float64), ((0, 3, 4, 4), np.uint8), ((1, 3, 20000, 20000), np.uint8)]:
        assert isinstance(tool.plan_call(shape, dtype), str)
    assert tool.main(["nothing.npy"], out=lambda s: None) == 2         # no -o
