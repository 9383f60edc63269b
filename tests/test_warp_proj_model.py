"""QOIMI_WARP_PROJECTIVE in the Python model (qoi_amd/warp.py): with g = h = 0 the item is the unflagged item in every sampling, border and
mode; ``positions`` is floor(N * 2**F / W) by Python's big integers at the extremes of N, W and F, with numbers of 88 bits and negative N
that floor; a bilinear item agrees within 1 with a float64 evaluation of the same quantised homography on a smooth image; the three new
rejections, their order and their place behind the older ones; ``homography`` and ``perspective`` round-trip and report an upper bound at
the four corners."""
import numpy as np
import pytest

from qoi_amd import warp
from qoi_amd.warp import (ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, PROJECTIVE, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4,
                          WRAP)

BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
SAMPLINGS = (0, NEAREST, BICUBIC)
FILL = 0x80FF4007
BOTH = "the projective map is defined for the bilinear, nearest and bicubic samplings: PROJECTIVE with a SUPER or VOTE flag"
OFFSETS = "|c| or |f| from 2**53 with PROJECTIVE"
HORIZON = "the denominator of PROJECTIVE falls below 1/8 inside the output"


def image(w, h, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, ch), dtype=np.uint8)


def test_the_constants():
    assert PROJECTIVE == 131072 == 1 << 17 and warp.PROJ_BASE == 14 and warp.PROJ_MAX_OFFSET == 1 << 53
    assert [warp.proj_bits(*s) for s in ((1, 1), (2, 1), (3, 2), (4, 4), (5, 1), (17, 9), (70000, 3), (2 ** 20 - 1, 3))] == [14, 15, 16, 16, 17, 19, 31, 34]
    for g, h in ((0, 0), (1, -1), (-32768, 32767), (32767, -32768), (-1, 12345)):
        assert warp.proj_of(warp.proj_reserved(g, h)) == (g, h)
    assert warp.proj_reserved(-1, 0) == 0xFFFF and warp.proj_reserved(0, -2) == 0xFFFE0000
    with pytest.raises(ValueError):
        warp.proj_reserved(32768, 0)
    it = warp.item(2, (1, 2, 3, 4), (5, 6), warp.IDENTITY, REPLICATE, 7, proj=(-3, 9))
    assert it[7] == REPLICATE | PROJECTIVE and warp.proj_of(it[13]) == (-3, 9) and warp.item(2, (1, 2, 3, 4), (5, 6))[13] == 0


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_zero_coefficients_are_the_unflagged_item(sampling, border):
    D4 = image(23, 17, 4, 3)
    rect = (2, 1, 19, 14)
    for out_size, matrix in (((17, 9), warp.rotation((19, 14), (17, 9), 30.0, 0.8)), ((1, 1), (ONE, 0, 12345, 0, ONE, -777)),
                             ((33, 40), (ONE, 23000, -40000, -9000, ONE + 700, 12345)), ((5, 3), (3 * ONE, 0, 2 * ONE * 19 * 300 + 777, 0, 3 * ONE, -999))):
        for D in (D4, D4[:, :, :3]):
            for mode in (PLAIN, ALPHA_WEIGHTED):
                plain = warp.warp(D, rect, out_size, matrix, sampling | border, FILL, mode)
                flagged = warp.warp(D, rect, out_size, matrix, sampling | border | PROJECTIVE, FILL, mode, reserved=0)
                assert np.array_equal(plain, flagged), (out_size, matrix, mode)
        Px, Py = warp.positions(out_size, matrix, PROJECTIVE, 0)
        Nx, Ny = warp.positions(out_size, matrix, 0, 0)
        assert np.array_equal(np.broadcast_to(Nx, Px.shape), Px) and np.array_equal(np.broadcast_to(Ny, Py.shape), Py)


def big(out_size, matrix, reserved):
    """positions by Python's integers, pixel by pixel: {(X, Y): (Px, Py, W)}"""
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    g, h = warp.proj_of(reserved)
    F = warp.proj_bits(ow, oh)
    out = {}
    for Y in sorted({0, 1, oh // 2, oh - 1} & set(range(oh))):
        for X in sorted({0, 1, 2, ow // 3, ow // 2, ow - 2, ow - 1} & set(range(ow))):
            U, V = 2 * X + 1, 2 * Y + 1
            W = 2 ** F + g * (U - ow) + h * (V - oh)
            out[X, Y] = ((a * U + b * V + c) * 2 ** F // W, (d * U + e * V + f) * 2 ** F // W, W)
    return out


EXTREMES = [
    # (an item reaches |Nx| of about 1.5 * 2**53, not 2**54 - ow * oh < 400 000 000 keeps one of a * U and b * V small -, and a W between
    # 2**(F-3) and 1.875 * 2**F; the quotient itself is walked to +-(2**54 - 1) and to 5 * 2**F - 1 in test_the_extremes_are_extreme)
    ((2 ** 20 - 1, 3), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 53 - 1, -2 ** 31, -2 ** 31, 1 - 2 ** 53), (0, 0)),            # F = 34, W = 2**F
    ((2 ** 20 - 1, 3), (2 ** 31 - 1, -2 ** 31, 2 ** 53 - 1, -2 ** 31, 2 ** 31 - 1, 1 - 2 ** 53), (-14336, 0)),       # F = 34: W falls to about 2**(F-3) on the right
    ((2 ** 20 - 1, 3), (-2 ** 31, 5, 1 - 2 ** 53, 7, -2 ** 31, 2 ** 53 - 1), (14336, -32768)),                      # F = 34: W rises and falls
    ((1, 1), (2 ** 31 - 1, -2 ** 31, 2 ** 53 - 1, -2 ** 31, 2 ** 31 - 1, 1 - 2 ** 53), (32767, -32768)),            # F = 14: Uc = Vc = 0, W = 2**14
    ((16, 16), (ONE, 31, 2 ** 53 - 1, -17, ONE, 1 - 2 ** 53), (-15291, 0)),                                        # F = 18: 15291 * 15 is 11 short of 7/8 * 2**18
    ((16, 16), (-3 * ONE - 1, 1, -5, -1, -2 * ONE - 3, -131073), (477, -478)),                                      # negative N that floor
    ((70000, 3), (ONE, 0, 0, 0, ONE, 0), (-26843, 0)),                                                             # F = 31
    ((2047, 9), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 53 - 1, -2 ** 31, -2 ** 31, 1 - 2 ** 53), (-14000, 90)),           # F = 25: both coefficients at work
]


@pytest.mark.parametrize("out_size,matrix,proj", EXTREMES)
def test_positions_against_big_integers(out_size, matrix, proj):
    reserved = warp.proj_reserved(*proj)
    Px, Py = warp.positions(out_size, matrix, PROJECTIVE, reserved)
    assert Px.dtype == np.int64 and Px.shape == (out_size[1], out_size[0]) == Py.shape
    for (X, Y), (px, py, W) in big(out_size, matrix, reserved).items():
        assert W > 0 and (int(Px[Y, X]), int(Py[Y, X])) == (px, py), (X, Y, W)


def test_the_extremes_are_extreme():
    ow, oh = 2 ** 20 - 1, 3
    a, b, c = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 53 - 1
    assert a * (2 * ow - 1) + b * (2 * oh - 1) + c > 2 ** 53 + 2 ** 52 - 2 ** 34 and (a * (2 * ow - 1) + b * 5 + c) << 34 > 2 ** 87        # 88 bits
    F = warp.proj_bits(ow, oh)
    assert F == 34 and 2 ** F - 14336 * (ow - 1) < 2 ** (F - 3) + 2 ** 25          # next to the limit of 1/8 (the limit itself is tested below)
    assert warp._wrong(ow, 3, (0, 0, 1, 1), (ow, oh), EXTREMES[1][1], PROJECTIVE, warp.proj_reserved(-14336, 0)) == ""
    # the most 16 bits can make of W is below 5 * 2**F at every size
    for ow, oh in ((1, 1), (2, 2), (16, 16), (17, 17), (2 ** 20 - 1, 2 ** 20 - 1)):
        F = warp.proj_bits(ow, oh)
        assert 2 ** F + 32768 * (ow - 1) + 32768 * (oh - 1) < 5 * 2 ** F < 2 ** 37
    # the scaled quotient itself, next to 5 * 2**F and at 2**(F - 3), against Python's integers
    rng = np.random.default_rng(7)
    for F in (14, 17, 18, 31, 34):
        for W in (2 ** (F - 3), 2 ** (F - 3) + 1, 2 ** F - 1, 2 ** F, 5 * 2 ** F - 1):
            N = np.concatenate([np.array([2 ** 54 - 1, 1 - 2 ** 54, 0, -1, 1, -W, W - 1, -W - 1], dtype=np.int64), rng.integers(-2 ** 54 + 1, 2 ** 54, 200)])
            got = warp._scaled_quotient(N, np.full(N.shape, W, dtype=np.int64), F)
            assert [int(v) for v in got] == [int(n) * 2 ** F // W for n in N], (F, W)


def float_homography(D, rect, out_size, matrix, proj, flags):
    """float64[oh, ow, ch]: the bilinear sample of the SAME quantised homography, positions and weights in float64, REPLICATE or the fill"""
    x, y, cw, rh = rect
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    g, h = proj
    F = warp.proj_bits(ow, oh)
    U = (2.0 * np.arange(ow) + 1)[None, :]
    V = (2.0 * np.arange(oh) + 1)[:, None]
    W = 2.0 ** F + g * (U - ow) + h * (V - oh)
    kx = ((a * U + b * V + c) * 2.0 ** F / W / ONE - 1) / 2
    ky = ((d * U + e * V + f) * 2.0 ** F / W / ONE - 1) / 2
    R = D[y:y + rh, x:x + cw].astype(np.float64)
    x0, y0 = np.floor(kx), np.floor(ky)
    out = np.zeros((oh, ow, D.shape[2]))
    for dy in (0, 1):
        for dx in (0, 1):
            wgt = (1 - np.abs(kx - (x0 + dx))) * (1 - np.abs(ky - (y0 + dy)))
            out += wgt[..., None] * R[np.clip(y0 + dy, 0, rh - 1).astype(int), np.clip(x0 + dx, 0, cw - 1).astype(int)]
    return out


def test_within_one_of_a_float_homography_on_a_smooth_image():
    """a smooth image: the value moves by less than 2**-11 per 2**-17 of a pixel, so the floored position costs nothing that shows"""
    w, h = 64, 48
    yy, xx = np.mgrid[0:h, 0:w]
    D = np.stack([xx * 3 + yy, 200 - xx - yy * 2, (xx * 2 + yy * 3) % 256 * 0 + 100 + xx - yy, 255 - xx * 2], axis=-1).clip(0, 255).astype(np.uint8)
    rect = (0, 0, w, h)
    for out_size, corners in (((33, 40), [(5.0, 3.0), (60.0, 8.0), (55.5, 44.0), (2.0, 40.0)]), ((17, 9), [(10.0, 10.0), (50.0, 4.0), (62.0, 47.0), (0.0, 30.0)])):
        matrix, proj, _ = warp.perspective((w, h), out_size, corners)
        assert proj != (0, 0)
        got = warp.warp(D, rect, out_size, matrix, REPLICATE | PROJECTIVE, 0, PLAIN, reserved=warp.proj_reserved(*proj)).astype(np.float64)
        ref = float_homography(D, rect, out_size, matrix, proj, REPLICATE)
        err = np.abs(got - ref)
        assert err.max() <= 0.5 + 2.0 ** -10, err.max()                  # the rounded value: within 1 of the float's rounding, at a boundary only
        assert (np.abs(got - np.rint(ref)) <= 1).all() and (got != np.rint(ref)).mean() < 0.01


def test_a_constant_stays_the_constant_and_lines_stay_lines():
    D = np.full((9, 11, 4), (7, 200, 31, 99), dtype=np.uint8)
    for sampling in SAMPLINGS:
        got = warp.warp(D, (1, 1, 9, 7), (17, 9), warp.rotation((9, 7), (17, 9), 40.0, 0.3), sampling | REPLICATE | PROJECTIVE, 0, ALPHA_WEIGHTED,
                        reserved=warp.proj_reserved(9000, -12000))
        assert (got == D[0, 0]).all(), sampling
    # the positions of a row of output pixels are collinear in the source to the flooring
    matrix, proj, _ = warp.perspective((64, 48), (33, 40), [(5.0, 3.0), (60.0, 8.0), (55.5, 44.0), (2.0, 40.0)])
    Px, Py = warp.positions((33, 40), matrix, PROJECTIVE, warp.proj_reserved(*proj))
    for Y in (0, 17, 39):
        x0, y0, x1, y1 = int(Px[Y, 0]), int(Py[Y, 0]), int(Px[Y, 32]), int(Py[Y, 32])
        cross = (Px[Y].astype(object) - x0) * (y1 - y0) - (Py[Y].astype(object) - y0) * (x1 - x0)
        assert max(abs(int(v)) for v in cross) <= 2 * (abs(x1 - x0) + abs(y1 - y0)), Y       # within two units of 2**-17 pixel of the line


def wrong(flags, reserved=0, out_size=(4, 4), matrix=warp.IDENTITY):
    return warp._wrong(8, 8, (0, 0, 4, 4), out_size, matrix, flags, reserved)


def test_the_rejections_and_their_order():
    far = (ONE, 0, 2 ** 53, 0, ONE, 0)
    horizon = warp.proj_reserved(32767, 0)                               # 2**16 - 32767 * 3 < 2**13
    for flags in (PROJECTIVE | 32768, PROJECTIVE | 65536, 32768, 65536, PROJECTIVE | 2, PROJECTIVE | SUPER2 | 512, PROJECTIVE | (1 << 18)):         # an unknown bit first
        assert wrong(flags, horizon, matrix=far) == "unknown flag bit", flags
    assert wrong(PROJECTIVE | NEAREST | BICUBIC | SUPER2, horizon, matrix=far) == "NEAREST and BICUBIC together"
    assert wrong(PROJECTIVE | REPLICATE | WRAP | VOTE2, horizon, matrix=far).startswith("more than one border")
    assert wrong(PROJECTIVE | SUPER2 | SUPER4, horizon, matrix=far) == "SUPER2 and SUPER4 together"
    assert wrong(PROJECTIVE | SUPER2 | NEAREST, horizon, matrix=far).startswith("supersampling is defined")
    assert wrong(PROJECTIVE | VOTE2 | VOTE4, horizon, matrix=far) == "VOTE2 and VOTE4 together"
    assert wrong(PROJECTIVE | VOTE2 | NEAREST, horizon, matrix=far).startswith("the vote is a sampling of its own")
    for flags in (SUPER2, SUPER4 | WRAP, VOTE2, VOTE4 | REPLICATE):                                               # 1. with a SUPER or VOTE flag
        assert wrong(PROJECTIVE | flags, horizon, matrix=far) == BOTH == wrong(PROJECTIVE | flags), flags
    for m in (far, (ONE, 0, -2 ** 53, 0, ONE, 0), (ONE, 0, 0, 0, ONE, 2 ** 53), (ONE, 0, 0, 0, ONE, -2 ** 55)):     # 2. the offsets
        assert wrong(PROJECTIVE | BICUBIC, horizon, matrix=m) == OFFSETS == wrong(PROJECTIVE, 0, matrix=m), m
        assert wrong(0, 0, matrix=m) == ""                                                                     # (without the flag 2**56 is the limit)
    assert wrong(PROJECTIVE, 0, matrix=(ONE, 0, 2 ** 53 - 1, 0, ONE, 1 - 2 ** 53)) == ""
    # 3. the least denominator: out 4 x 4 has F = 16, the limit is 2**16 - 3 |g| - 3 |h| >= 2**13, so |g| + |h| <= 19114
    for g, h in ((19115, 0), (0, -19115), (-9557, 9558), (32767, 32767), (-32768, -32768)):
        assert wrong(PROJECTIVE | NEAREST | WRAP, warp.proj_reserved(g, h)) == HORIZON, (g, h)
    for g, h in ((19114, 0), (0, -19114), (-9557, 9557), (0, 0), (-1, 1)):
        assert wrong(PROJECTIVE | NEAREST | WRAP, warp.proj_reserved(g, h)) == "", (g, h)
    assert wrong(PROJECTIVE, warp.proj_reserved(32767, -32768), out_size=(1, 1)) == ""                              # Uc = Vc = 0: any g and h
    assert wrong(PROJECTIVE, warp.proj_reserved(-32768, 0), out_size=(2, 1)) == HORIZON and wrong(PROJECTIVE, warp.proj_reserved(-28672, 0), out_size=(2, 1)) == ""
    # without the flag reserved is rejected as before, with it reserved is g and h
    assert wrong(0, 1) == "reserved is not 0" == wrong(BICUBIC | WRAP, 0x00010000) and wrong(PROJECTIVE, 1) == ""
    assert warp.size(8, 8, warp.item(0, (0, 0, 4, 4), (4, 4), proj=(19114, 0)), 3) == 48 and warp.size(8, 8, warp.item(0, (0, 0, 4, 4), (4, 4), proj=(19115, 0)), 3) == 0
    with pytest.raises(ValueError, match="falls below 1/8"):
        warp.warp(image(8, 8, 4, 1), (0, 0, 4, 4), (4, 4), warp.IDENTITY, PROJECTIVE, 0, PLAIN, reserved=horizon)


def test_homography_and_perspective():
    # an affine H is the affine item: g = h = 0 and rotation's matrix
    t = np.deg2rad(30.0)
    co, si = np.cos(t) / 0.8, np.sin(t) / 0.8
    cw, rh, ow, oh = 40, 30, 33, 21
    # output pixel (X, Y) -> source (k, r): the centres coincide
    H = np.array([[co, -si, (cw - 1) / 2 - co * (ow - 1) / 2 + si * (oh - 1) / 2], [si, co, (rh - 1) / 2 - si * (ow - 1) / 2 - co * (oh - 1) / 2], [0, 0, 1]])
    matrix, proj, moved = warp.homography((cw, rh), (ow, oh), H)
    assert proj == (0, 0) and moved < 1e-3
    assert np.abs(np.array(matrix) - np.array(warp.rotation((cw, rh), (ow, oh), 30.0, 0.8))).max() <= 1
    assert warp.homography((cw, rh), (ow, oh), 5 * H)[:2] == (matrix, proj)                       # the scale of H does not matter
    # four corners round-trip through the integer positions
    for out_size, corners in (((33, 40), [(5.0, 3.0), (60.0, 8.0), (55.5, 44.0), (2.0, 40.0)]), ((224, 224), [(30.0, 10.0), (480.0, 60.0), (500.0, 500.0), (10.0, 430.0)]),
                              ((17, 9), [(0.0, 0.0), (16.0, 0.0), (16.0, 8.0), (0.0, 8.0)])):
        matrix, proj, moved = warp.perspective((512, 512), out_size, corners)
        Px, Py = warp.positions(out_size, matrix, PROJECTIVE, warp.proj_reserved(*proj))
        ow, oh = out_size
        worst = 0.0
        for (X, Y), (k, r) in zip([(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)], corners):
            got = ((Px[Y, X] / ONE - 1) / 2, (Py[Y, X] / ONE - 1) / 2)
            worst = max(worst, float(np.hypot(got[0] - k, got[1] - r)))
        assert worst <= moved + 2.0 ** -16 and moved < 0.05, (out_size, worst, moved)             # the report bounds the corners (to the flooring and the solve)
        assert warp._wrong(512, 512, (0, 0, 512, 512), out_size, matrix, PROJECTIVE, warp.proj_reserved(*proj)) == ""
    assert warp.perspective((17, 9), (17, 9), [(0.0, 0.0), (16.0, 0.0), (16.0, 8.0), (0.0, 8.0)])[1] == (0, 0)           # the identity
    for bad in (lambda: warp.perspective((8, 8), (1, 5), [(0, 0), (1, 0), (1, 1), (0, 1)]), lambda: warp.perspective((8, 8), (4, 4), [(0, 0), (0, 0), (0, 0), (0, 0)]),
                lambda: warp.homography((8, 8), (4, 4), np.array([[1.0, 0, 0], [0, 1, 0], [1, 0, -1.5]])), lambda: warp.homography((8, 8), (4, 4), np.eye(2))):
        with pytest.raises(ValueError):
            bad()
