"""qoi_amd/thumbs.py - the normative statement of qoimi_decode_thumbnails' box reduction - against an independent brute force: pixel by pixel,
Python ints and fractions, no numpy arithmetic.  Tiny images; every comparison is exact."""
from fractions import Fraction
from math import floor

import numpy as np
import pytest

from qoi_amd import thumbs
from qoi_amd.thumbs import ALPHA_WEIGHTED, PLAIN


def round_half_up(num: int, den: int) -> int:
    """floor(num / den + 1/2) in exact rational arithmetic - what (num + den // 2) // den must equal for every den >= 1 (an odd den never
    meets an exact half: 2 * num + den is odd)"""
    return floor(Fraction(num, den) + Fraction(1, 2))


def brute(px, f, mode):
    h, w, ch = px.shape
    tw, th = -(-w // f), -(-h // f)
    out = np.zeros((th, tw, ch), dtype=np.uint8)
    for Y in range(th):
        for X in range(tw):
            block = [[int(v) for v in px[y, x]] for y in range(Y * f, min(h, Y * f + f)) for x in range(X * f, min(w, X * f + f))]
            cnt = len(block)
            plain = [(sum(p[c] for p in block) + cnt // 2) // cnt for c in range(ch)]
            res = list(plain)
            if mode == ALPHA_WEIGHTED and ch == 4:
                A = sum(p[3] for p in block)
                if A > 0:
                    res[:3] = [(sum(p[c] * p[3] for p in block) + A // 2) // A for c in range(3)]
            out[Y, X] = res
    return out


def test_round_half_up_is_the_integer_formula():
    for den in list(range(1, 70)) + [4096, 4095, 255 * 4096]:
        for num in list(range(0, 3 * den + 2)) if den < 70 else [0, den // 2 - 1, den // 2, den // 2 + 1, den - 1, den, 255 * den]:
            assert (num + den // 2) // den == round_half_up(num, den), (num, den)


def grey(values, w, h, ch=4):
    return np.array([[v] * ch for v in values], dtype=np.uint8).reshape(h, w, ch)


def test_rounding_halves():
    for mode in (PLAIN, ALPHA_WEIGHTED):
        assert thumbs.thumbnail(grey([0, 0, 1, 1], 2, 2, 3), 2, mode).tolist() == [[[1, 1, 1]]]          # 2 / 4: the half rounds up
        assert thumbs.thumbnail(grey([0, 0, 0, 1], 2, 2, 3), 2, mode).tolist() == [[[0, 0, 0]]]          # 1 / 4
        assert thumbs.thumbnail(grey([0, 1, 1, 1], 2, 2, 3), 2, mode).tolist() == [[[1, 1, 1]]]          # 3 / 4
    assert thumbs.thumbnail(grey([0, 0, 1, 1], 2, 2, 4), 2, PLAIN).tolist() == [[[1, 1, 1, 1]]]
    assert thumbs.thumbnail(grey([0, 0, 0, 1], 2, 2, 4), 2, PLAIN).tolist() == [[[0, 0, 0, 0]]]
    assert thumbs.thumbnail(grey([0, 1, 2], 3, 1, 3), 3).tolist() == [[[1, 1, 1]]]
    assert thumbs.thumbnail(grey([0, 1], 1, 2, 3), 2).tolist() == [[[1, 1, 1]]]                            # cnt 2: 1 / 2 rounds up


SHAPES = [(5, 3, 2), (5, 3, 3), (5, 3, 4), (3, 7, 4), (7, 3, 4), (3, 9, 8), (9, 2, 8), (1, 1, 64), (1, 1, 1), (2, 2, 64), (13, 11, 5), (13, 11, 7), (16, 8, 4),
          (17, 9, 16), (70, 3, 64), (3, 70, 64), (6, 6, 3), (8, 8, 2)]


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_partial_edge_blocks_against_brute_force(ch, mode):
    rng = np.random.default_rng(20240 + ch + mode)
    for (w, h, f) in SHAPES:
        px = rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8)
        if ch == 4:
            px[:, :, 3] = rng.choice(np.array([0, 0, 1, 128, 255, 255], dtype=np.uint8), size=(h, w))
        got = thumbs.thumbnail(px, f, mode)
        assert got.dtype == np.uint8 and got.shape == (-(-h // f), -(-w // f), ch), (w, h, f)
        assert thumbs.size(w, h, f) == (got.shape[1], got.shape[0])
        assert np.array_equal(got, brute(px, f, mode)), (w, h, f, ch, mode)


def test_three_channels_weighted_is_plain():
    px = np.random.default_rng(5).integers(0, 256, size=(9, 10, 3), dtype=np.uint8)
    for f in (2, 3, 4, 64):
        assert np.array_equal(thumbs.thumbnail(px, f, ALPHA_WEIGHTED), thumbs.thumbnail(px, f, PLAIN))


def test_weighted_mode():
    # alphas (0, 255) with colours (200, 100): the transparent pixel's colour does not count
    px = np.array([[[200, 200, 200, 0], [100, 100, 100, 255]]], dtype=np.uint8)
    assert thumbs.thumbnail(px, 2, ALPHA_WEIGHTED).tolist() == [[[100, 100, 100, 128]]]
    assert thumbs.thumbnail(px, 2, PLAIN).tolist() == [[[150, 150, 150, 128]]]
    # an all-transparent block falls back to the plain value
    px = np.array([[[10, 20, 30, 0], [11, 21, 30, 0]], [[10, 20, 31, 0], [12, 20, 30, 0]]], dtype=np.uint8)
    assert thumbs.thumbnail(px, 2, ALPHA_WEIGHTED).tolist() == thumbs.thumbnail(px, 2, PLAIN).tolist() == [[[11, 20, 30, 0]]]
    # the largest sums: 64 x 64 of 0xFFFFFFFF at f = 64
    px = np.full((64, 64, 4), 255, dtype=np.uint8)
    for mode in (PLAIN, ALPHA_WEIGHTED):
        assert thumbs.thumbnail(px, 64, mode).tolist() == [[[255, 255, 255, 255]]]
    assert 64 * 64 * 255 * 255 + 64 * 64 * 255 // 2 < 2 ** 32
    # a single faint pixel decides the colour of its block
    px = np.zeros((4, 4, 4), dtype=np.uint8)
    px[:, :, :3] = 250
    px[2, 3] = (7, 8, 9, 1)
    assert thumbs.thumbnail(px, 4, ALPHA_WEIGHTED).tolist() == [[[7, 8, 9, 0]]]
    assert np.array_equal(thumbs.thumbnail(px, 4, ALPHA_WEIGHTED), brute(px, 4, ALPHA_WEIGHTED))


@pytest.mark.parametrize("ch", [3, 4])
def test_factor_one_is_the_identity(ch):
    px = np.random.default_rng(77).integers(0, 256, size=(6, 11, ch), dtype=np.uint8)
    if ch == 4:
        px[0, :4, 3] = 0
        px[1, :4, 3] = 1
    for mode in (PLAIN, ALPHA_WEIGHTED):
        assert np.array_equal(thumbs.thumbnail(px, 1, mode), px)


def test_factor_for_at_its_edges():
    assert thumbs.factor_for(256, 100, 256) == 1 and thumbs.factor_for(257, 100, 256) == 2 and thumbs.factor_for(100, 257, 256) == 2
    assert thumbs.factor_for(512, 512, 256) == 2 and thumbs.factor_for(513, 1, 256) == 3
    assert thumbs.factor_for(3840, 2160, 256) == 15 and thumbs.factor_for(3840, 2160, 60) == 64
    assert thumbs.factor_for(64 * 100, 5, 100) == 64 and thumbs.factor_for(64 * 100 + 1, 5, 100) == 64      # nothing fits: 64 all the same
    assert thumbs.factor_for(1, 1, 1) == 1 and thumbs.factor_for(64, 64, 1) == 64 and thumbs.factor_for(63, 2, 1) == 63
    assert thumbs.factor_for(10 ** 6, 10 ** 6, 1) == 64
    with pytest.raises(ValueError):
        thumbs.factor_for(10, 10, 0)


def test_arguments():
    px = np.zeros((2, 2, 4), dtype=np.uint8)
    for f in (0, 65, -1):
        with pytest.raises(ValueError):
            thumbs.thumbnail(px, f, PLAIN)
    with pytest.raises(ValueError):
        thumbs.thumbnail(px, 2, 2)
    with pytest.raises(ValueError):
        thumbs.thumbnail(np.zeros((2, 2, 2), dtype=np.uint8), 2, PLAIN)
    assert thumbs.size(1, 1, 64) == (1, 1) and thumbs.size(65, 64, 64) == (2, 1)
