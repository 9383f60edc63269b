"""qoi_amd/warp.py with REFLECT, REFLECT_101 and WRAP - the normative statement of the three folding borders of qoimi_decode_warped.  fold
against numpy.pad of an index ramp (an implementation that shares nothing with it) for every small n and k, and at the largest accepted
index against the periodic extension of that table; the identity plus a whole-pixel translation into a larger output is numpy.pad of the
rectangle byte for byte in all three samplings, both channel counts and both modes, for pads larger than the rectangle and for a rectangle
of one pixel; a constant stays the constant; every pixel whose taps all lie inside the rectangle equals the call without the flag; the
bilinear and the bicubic sampling stay within 1 of a float64 evaluation with the same border rule (made by padding the rectangle with
numpy.pad far enough and sampling the padded array: each tap folded on its own IS a padded array); the rejections and their order.  No GPU,
no library."""
import numpy as np
import pytest

from qoi_amd import warp
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, WRAP

PAD_MODE = {REFLECT: "symmetric", REFLECT_101: "reflect", WRAP: "wrap"}
BORDERS = sorted(PAD_MODE)
SAMPLINGS = (0, NEAREST, BICUBIC)
FILL = 0x40C08020


def image(w, h, och, seed):
    """random pixels, at 4 channels a third of them transparent"""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4:
        D[:, :, 3][rng.integers(0, 3, size=(h, w)) == 0] = 0
    return D


def test_the_values():
    assert (REFLECT, REFLECT_101, WRAP) == (64, 128, 256) and warp.BORDERS == 1 | 64 | 128 | 256


# ---------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_fold_is_numpy_pad_of_the_indices(n, border):
    ramp = np.pad(np.arange(n), (40, 41 - n), mode=PAD_MODE[border])      # ramp[40 + k] for k in -40 .. 40
    k = np.arange(-40, 41)
    got = warp.fold(k, n, border)
    assert got.dtype == np.int64 and np.array_equal(got, ramp), (n, border, got, ramp)
    # the periodic extension of that table at the largest accepted index, with Python's integers
    P = {REFLECT: 2 * n, REFLECT_101: max(2 * n - 2, 1), WRAP: n}[border]
    table = ramp[40:40 + P]
    assert np.array_equal(ramp[40 + P:40 + 2 * P], table)                                     # (it is the period)
    for big in (2 ** 40 - 1, -(2 ** 40 - 1), 2 ** 40 - 2, -(2 ** 40 - 2), 2 ** 33 + 5, -(2 ** 33) - 5):
        assert int(warp.fold(big, n, border)) == int(table[big % P]), (n, border, big)


def test_fold_rejects_what_is_no_border():
    for border in (0, REPLICATE, REFLECT | WRAP, 32):
        with pytest.raises(ValueError):
            warp.fold(0, 3, border)
    with pytest.raises(ValueError):
        warp.fold(0, 0, WRAP)


# ---------------------------------------------------------------------------------- numpy.pad identities
def translation(left, top):
    """the identity moved so that output pixel (left, top) is pixel (0, 0) of the rectangle"""
    return (ONE, 0, -2 * ONE * left, 0, ONE, -2 * ONE * top)


@pytest.mark.parametrize("och", [3, 4])
@pytest.mark.parametrize("border", BORDERS)
def test_translation_into_a_larger_output_is_numpy_pad(border, och):
    D = image(23, 17, och, 3)
    for rect, (left, right, top, bottom) in [((3, 5, 7, 9), (4, 3, 2, 5)), ((3, 5, 7, 9), (20, 31, 25, 19)), ((22, 16, 1, 1), (3, 4, 2, 5)),
                                              ((0, 4, 23, 1), (5, 6, 4, 3)), ((5, 0, 1, 17), (3, 2, 40, 1)), ((0, 0, 2, 2), (7, 8, 9, 6)),
                                              ((1, 1, 5, 3), (0, 11, 0, 7)), ((1, 1, 17, 9), (18, 0, 10, 0))]:
        x, y, cw, rh = rect
        want = np.pad(D[y:y + rh, x:x + cw], ((top, bottom), (left, right), (0, 0)), mode=PAD_MODE[border])
        for sampling in SAMPLINGS:
            for mode in (PLAIN, ALPHA_WEIGHTED):
                got = warp.warp(D, rect, (cw + left + right, rh + top + bottom), translation(left, top), border | sampling, FILL, mode)
                assert np.array_equal(got, want), (rect, left, top, sampling, mode)


@pytest.mark.parametrize("border", BORDERS)
def test_a_constant_stays_the_constant(border):
    for och in (3, 4):
        D = np.empty((9, 11, och), dtype=np.uint8)
        D[:] = (7, 130, 255, 90)[:och]
        for rect in ((2, 1, 7, 5), (4, 4, 1, 1)):
            m = warp.rotation(rect[2:], (19, 21), 30.0, 0.4)
            for sampling in SAMPLINGS:
                for mode in (PLAIN, ALPHA_WEIGHTED):
                    got = warp.warp(D, rect, (19, 21), m, border | sampling, FILL, mode)
                    assert (got == D[0, 0]).all(), (och, rect, sampling, mode)


@pytest.mark.parametrize("border", BORDERS)
def test_the_interior_is_the_unflagged_call(border):
    D = image(40, 24, 4, 5)
    rect = (3, 2, 17, 9)
    out = (31, 27)
    m = warp.rotation(rect[2:], out, 30.0, 0.7)
    a, b, c, d, e, f = m
    U = (2 * np.arange(out[0], dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(out[1], dtype=np.int64) + 1)[:, None]
    Px, Py = a * U + b * V + c, d * U + e * V + f
    for sampling in SAMPLINGS:
        if sampling == NEAREST:
            k, r = Px >> 17, Py >> 17
            inner = (k >= 0) & (k < rect[2]) & (r >= 0) & (r < rect[3])
        else:
            axis = warp._cubic_axis if sampling == BICUBIC else warp._axis
            inner = axis(Px, rect[2], 0)[2].all(axis=-1) & axis(Py, rect[3], 0)[2].all(axis=-1)
        assert inner.any() and not inner.all()
        for mode in (PLAIN, ALPHA_WEIGHTED):
            got = warp.warp(D, rect, out, m, border | sampling, FILL, mode)
            for plain in (warp.warp(D, rect, out, m, sampling, FILL, mode), warp.warp(D, rect, out, m, sampling | REPLICATE, FILL, mode)):
                assert np.array_equal(got[inner], plain[inner]), (sampling, mode)
            assert not np.array_equal(got, warp.warp(D, rect, out, m, sampling, FILL, mode))          # ... and the border is not the fill


# ---------------------------------------------------------------------------------- float64
def padded(D, rect, border, margin):
    """(the rectangle padded by margin on every side with numpy.pad, its own rectangle): what the border extends R to"""
    x, y, cw, rh = rect
    big = np.pad(D[y:y + rh, x:x + cw], ((margin, margin), (margin, margin), (0, 0)), mode=PAD_MODE[border])
    return big, (0, 0, cw + 2 * margin, rh + 2 * margin)


def bilinear_reference(R, out_size, m):
    """float64[oh, ow, och]: the 2 x 2 blend of R at the positions of m, neither rounded nor weighted; every tap must lie inside R"""
    ow, oh = out_size
    a, b, c, d, e, f = (float(v) for v in m)
    U = (2.0 * np.arange(ow) + 1.0)[None, :]
    V = (2.0 * np.arange(oh) + 1.0)[:, None]

    def axis(P, n):
        p = (P - 65536.0) / 131072.0
        k0 = np.floor(p)
        assert k0.min() >= 0 and k0.max() + 1 < n
        return k0.astype(np.int64), p - k0

    kx, fx = axis(a * U + b * V + c, R.shape[1])
    ky, fy = axis(d * U + e * V + f, R.shape[0])
    R = R.astype(np.float64)
    top = R[ky, kx] * (1.0 - fx)[..., None] + R[ky, kx + 1] * fx[..., None]
    bottom = R[ky + 1, kx] * (1.0 - fx)[..., None] + R[ky + 1, kx + 1] * fx[..., None]
    return top * (1.0 - fy)[..., None] + bottom * fy[..., None]


@pytest.mark.parametrize("och", [3, 4])
@pytest.mark.parametrize("border", BORDERS)
def test_within_1_of_float64_with_the_same_border(border, och):
    """PLAIN.  The bound is the unflagged sampling's: 1 for both (warp.cubic_bound for the bicubic), the arithmetic being unchanged."""
    D = image(40, 24, och, 7)
    margin = 64
    for rect in ((3, 2, 17, 9), (30, 20, 5, 3), (8, 8, 1, 7)):
        out = (29, 23)
        for m in (warp.rotation(rect[2:], out, 30.0, 0.5), warp.rotation(rect[2:], out, -77.0, 0.8), (65537, -3, -9 * ONE + 12345, 7, 65535, -54321)):
            big, whole = padded(D, rect, border, margin)
            shifted = m[:2] + (m[2] + 2 * ONE * margin,) + m[3:5] + (m[5] + 2 * ONE * margin,)
            # bilinear: the float blend of the padded array
            got = warp.warp(D, rect, out, m, border, FILL).astype(np.float64)
            ref = bilinear_reference(big, out, shifted)
            assert np.abs(got - np.rint(ref)).max() <= 1 and np.abs(got - ref).max() < 0.5 + 2.0 ** -20, (rect, m)
            # bicubic: cubic_reference with the border, which is cubic_reference of the padded array
            got = warp.warp(D, rect, out, m, border | BICUBIC, FILL).astype(np.float64)
            ref = warp.cubic_reference(D, rect, out, m, border | BICUBIC, FILL)
            assert np.allclose(ref, warp.cubic_reference(big, whole, out, shifted, BICUBIC, FILL), rtol=0, atol=1e-9)
            exact = np.clip(ref, 0.0, 255.0)
            assert np.abs(got - np.rint(exact)).max() <= warp.cubic_bound() == 1 and np.abs(got - exact).max() < 0.5 + 0.036, (rect, m)
            # nearest: the padded array's sample
            got = warp.warp(D, rect, out, m, border | NEAREST, FILL)
            assert np.array_equal(got, warp.warp(big, whole, out, shifted, NEAREST, FILL))


@pytest.mark.parametrize("border", BORDERS)
def test_taps_many_periods_away(border):
    """offsets near the limits: the model's integers are exact there; the result is the one a congruent small offset gives"""
    D = image(12, 9, 4, 9)
    rect = (2, 1, 5, 3)
    for n_axis, axis in ((rect[2], 0), (rect[3], 1)):
        P = {REFLECT: 2 * n_axis, REFLECT_101: 2 * n_axis - 2, WRAP: n_axis}[border]
        for big in (2 ** 56 - 1, 1 - 2 ** 56):
            periods = (big >> 17) // P * P                                          # a whole number of periods, in pixels
            small = big - (periods << 17)
            m_big = (ONE, 0, big, 0, ONE, 12345) if axis == 0 else (ONE, 0, 12345, 0, ONE, big)
            m_small = (ONE, 0, small, 0, ONE, 12345) if axis == 0 else (ONE, 0, 12345, 0, ONE, small)
            for sampling in SAMPLINGS:
                assert np.array_equal(warp.warp(D, rect, (9, 7), m_big, border | sampling), warp.warp(D, rect, (9, 7), m_small, border | sampling))


# ---------------------------------------------------------------------------------- the flag rule
def test_rejections_and_their_order():
    def wrong(flags, reserved=0, rect=(1, 2, 10, 8)):
        return warp._wrong(20, 15, rect, (30, 20), warp.IDENTITY, flags, reserved)

    for border in (0, REPLICATE, REFLECT, REFLECT_101, WRAP):
        for sampling in SAMPLINGS:
            assert wrong(border | sampling) == "", (border, sampling)
            assert warp.size(20, 15, warp.item(0, (1, 2, 10, 8), (30, 20), flags=border | sampling), 3) == 1800
    for flags in (2, 8, 32, 512, 1 << 31, 64 | 2, 128 | 8, 256 | 32, 64 | 128 | 32, 4 | 16 | 2):           # 1. an unknown bit, whatever else is set
        assert wrong(flags) == "unknown flag bit", flags
        assert wrong(flags, reserved=1) == "unknown flag bit"
    for flags in (4 | 16, 4 | 16 | 64, 4 | 16 | 64 | 128, 4 | 16 | 1 | 256):                               # 2. the two samplings, two borders or not
        assert wrong(flags) == wrong(flags, reserved=1) == "NEAREST and BICUBIC together", flags
    for flags in (1 | 64, 1 | 128, 1 | 256, 64 | 128, 64 | 256, 128 | 256, 1 | 64 | 128 | 256, 4 | 64 | 128, 16 | 1 | 256):   # 3. two borders
        assert wrong(flags) == wrong(flags, reserved=1) == "more than one border of REPLICATE, REFLECT, REFLECT_101 and WRAP", flags
        assert warp.size(20, 15, warp.item(0, (1, 2, 10, 8), (30, 20), flags=flags), 4) == 0
    for flags in (64, 128 | 4, 256 | 16):                                                                  # 4. reserved
        assert wrong(flags, reserved=1) == "reserved is not 0"
    assert wrong(64 | 128, rect=(1, 2, 0, 8)) == "zero width or height" and wrong(32, rect=(15, 2, 10, 8)) == "the rectangle leaves its image"
    with pytest.raises(ValueError, match="more than one border"):
        warp.warp(image(20, 15, 3, 1), (1, 2, 10, 8), (30, 20), warp.IDENTITY, REFLECT | WRAP)
