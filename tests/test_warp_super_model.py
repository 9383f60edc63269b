"""qoi_amd/warp.py with SUPER2 and SUPER4 - the normative statement of the supersampled bilinear warp of qoimi_decode_warped.  The box identity
(a = e = s * ONE into an output of 1 / s the rectangle is thumbs.thumbnail at factor s and resize.resize byte for byte, both modes); a
constant stays the constant under a reducing turn with each border; the result is within 1 of a float64 evaluation of the same s**2 positions
and differs from it only at a rounding boundary; a period-2 checkerboard reduced 4 : 1 is 128 everywhere with SUPER4 and only 0 or 255
without - the one statement about what the flags are for; the flag rule in its order; 512, 1 << 16 and 1 << 31 still no flags; an item without
a SUPER flag gives the bytes the model gave before the flags existed (tests/golden/warp_unflagged.npz: recorded from that model).  No GPU, no
library."""
import os

import numpy as np
import pytest

from qoi_amd import resize, thumbs, warp
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, WRAP

BORDERS = (REPLICATE, REFLECT, REFLECT_101, WRAP)
SUPERS = ((SUPER2, 2), (SUPER4, 4))
FILL = 0x40C08020
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_unflagged.npz")


def image(w, h, och, seed, soft=False):
    """random pixels; at 4 channels a third of them transparent, or - soft - every alpha random"""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4 and not soft:
        D[:, :, 3][rng.integers(0, 3, size=(h, w)) == 0] = 0
    return D


def test_the_values():
    assert (SUPER2, SUPER4) == (1024, 2048) and warp.SUPERS == 1024 | 2048
    assert [warp.super_log2(f) for f in (0, REPLICATE, SUPER2, SUPER4 | WRAP)] == [0, 0, 1, 2]


# ---------------------------------------------------------------------------------- the box identity
@pytest.mark.parametrize("flag,s", SUPERS)
@pytest.mark.parametrize("shape,soft", [((8, 8), False), ((12, 20), False), ((12, 20), True)])
def test_the_box_identity(shape, soft, flag, s):
    w, h = shape
    for och in (3, 4):
        D = image(w, h, och, 7 + w, soft)
        for mode in (PLAIN, ALPHA_WEIGHTED):
            want = thumbs.thumbnail(D, s, mode)
            assert want.shape == (h // s, w // s, och)
            assert np.array_equal(resize.resize(D, (0, 0, w, h), (w // s, h // s), 0, mode), want)
            for border in (0,) + BORDERS:
                got = warp.warp(D, (0, 0, w, h), (w // s, h // s), (s * ONE, 0, 0, 0, s * ONE, 0), flag | border, FILL, mode)
                assert np.array_equal(got, want), (shape, soft, och, mode, border)
    if soft:
        assert not np.array_equal(thumbs.thumbnail(D, s, PLAIN), thumbs.thumbnail(D, s, ALPHA_WEIGHTED))        # the modes differ here
    # ... and of a rectangle inside the image
    D = image(w + 3, h + 2, 4, 11, soft)
    want = resize.resize(D, (2, 1, w, h), (w // s, h // s), 0, ALPHA_WEIGHTED)
    assert np.array_equal(warp.warp(D, (2, 1, w, h), (w // s, h // s), (s * ONE, 0, 0, 0, s * ONE, 0), flag, FILL, ALPHA_WEIGHTED), want)


# ---------------------------------------------------------------------------------- a constant stays the constant
@pytest.mark.parametrize("flag,s", SUPERS)
@pytest.mark.parametrize("border", BORDERS)
def test_a_constant_stays_the_constant(border, flag, s):
    D = np.empty((21, 33, 4), dtype=np.uint8)
    D[:] = (200, 3, 97, 131)
    m = warp.rotation((33, 21), (19, 17), 30.0, 1 / 3)                   # reduces by 3; the output's corners leave the rectangle
    for mode in (PLAIN, ALPHA_WEIGHTED):
        got = warp.warp(D, (0, 0, 33, 21), (19, 17), m, flag | border, FILL, mode)
        assert np.all(got == np.array([200, 3, 97, 131], dtype=np.uint8)), (border, mode)
    assert not np.all(warp.warp(D, (0, 0, 33, 21), (19, 17), m, flag, FILL) == np.array([200, 3, 97, 131], dtype=np.uint8))   # the fill shows


# ---------------------------------------------------------------------------------- the bound against float64
@pytest.mark.parametrize("flag,s", SUPERS)
@pytest.mark.parametrize("shape,out", [((33, 21), (13, 9)), ((5, 1), (7, 3))])
def test_within_one_of_float64_and_only_at_a_rounding_boundary(shape, out, flag, s):
    """every scale both as a reduction (what the flags are for) and as an enlargement"""
    w, h = shape
    D = image(w, h, 4, 3)
    differing = cases = 0
    for degrees in (0.0, 17.0, 45.0, 90.0):
        for scale in (1.0, 1 / 2.5, 1 / 4, 2.5, 4.0):
            m = warp.rotation(shape, out, degrees, scale)
            for border in (0,) + BORDERS:
                got = warp.warp(D, (0, 0, w, h), out, m, flag | border, FILL).astype(np.int64)
                ref = warp.super_reference(D, (0, 0, w, h), out, m, flag | border, FILL)
                near = np.floor(ref + 0.5).astype(np.int64)
                diff = np.abs(got - near)
                assert diff.max() <= 1, (degrees, scale, border, int(diff.max()))
                at_boundary = np.abs(ref - np.floor(ref) - 0.5) < 1e-6
                assert np.all(at_boundary[diff != 0]), (degrees, scale, border)
                differing += int((diff != 0).sum())
                cases += 1
    assert cases == 4 * 5 * 5
    print("bytes that differ from the rounded float64 value:", differing)


# ---------------------------------------------------------------------------------- what the flags are for
def test_a_checkerboard_reduced_four_to_one():
    """a = e = 4 * ONE; c = f = ONE moves the map by half a source pixel, so that the one sample of the unflagged warp is a pixel centre - the
    aliasing case: it picks one colour of the board (with c = f = 0 it would fall on the corner between four pixels and give 128 by
    accident).  The 16 sub-samples of SUPER4 then each lie between four pixels of the board: 127.5 sixteen times, rounded once.  The output
    of 11 x 7 ends one output pixel before the rectangle does, so no tap leaves the rectangle and the border does not matter."""
    yy, xx = np.mgrid[0:32, 0:48]
    D = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    m = (4 * ONE, 0, ONE, 0, 4 * ONE, ONE)
    for border in (0,) + BORDERS:
        assert np.all(warp.warp(D, (0, 0, 48, 32), (11, 7), m, SUPER4 | border) == 128)
        plain = warp.warp(D, (0, 0, 48, 32), (11, 7), m, border)
        assert set(np.unique(plain).tolist()) <= {0, 255} and plain.size == 11 * 7 * 3
    # with the borders that continue the board (48 and 32 are even) the whole rectangle's output is 128 as well
    for border in (REFLECT_101, WRAP):
        assert np.all(warp.warp(D, (0, 0, 48, 32), (12, 8), m, SUPER4 | border) == 128)


# ---------------------------------------------------------------------------------- the flag rule
BOTH = "SUPER2 and SUPER4 together"
BILINEAR_ONLY = "supersampling is defined for the bilinear sampling only"


def wrong(flags, reserved=0):
    return warp._wrong(8, 8, (0, 0, 4, 4), (4, 4), warp.IDENTITY, flags, reserved)


def test_the_flag_rule_in_its_order():
    for flags in (512, 1 << 16, 1 << 31, 2, 8, 32, 4096, 512 | SUPER2, SUPER2 | SUPER4 | 512, SUPER4 | NEAREST | BICUBIC | 2, SUPER2 | 1 | 64 | 32):   # 1. an unknown bit
        assert wrong(flags) == "unknown flag bit" == wrong(flags, reserved=1), flags
    for flags in (SUPER2 | NEAREST | BICUBIC, SUPER2 | SUPER4 | NEAREST | BICUBIC | 1 | 64):                                                       # 2. the two samplings
        assert wrong(flags) == "NEAREST and BICUBIC together" == wrong(flags, reserved=1), flags
    for flags in (SUPER2 | 1 | 64, SUPER2 | SUPER4 | 128 | 256, SUPER4 | NEAREST | 1 | 256):                                                       # 3. two borders
        assert wrong(flags).startswith("more than one border") and wrong(flags, reserved=1) == wrong(flags), flags
    for flags in (SUPER2 | SUPER4, SUPER2 | SUPER4 | REFLECT, SUPER2 | SUPER4 | NEAREST, SUPER2 | SUPER4 | BICUBIC | REPLICATE):                     # 4. both SUPER flags
        assert wrong(flags) == BOTH == wrong(flags, reserved=1), flags
    for flags in (SUPER2 | NEAREST, SUPER4 | BICUBIC, SUPER4 | NEAREST | WRAP, SUPER2 | BICUBIC | REPLICATE):                                     # 5. not the bilinear sampling
        assert wrong(flags).startswith(BILINEAR_ONLY) and wrong(flags, reserved=1) == wrong(flags), flags
    for flags in (SUPER2, SUPER4, SUPER2 | REPLICATE, SUPER4 | REFLECT, SUPER2 | REFLECT_101, SUPER4 | WRAP):                                     # 6. reserved
        assert wrong(flags) == "" and wrong(flags, reserved=1) == "reserved is not 0", flags
    it = warp.item(0, (0, 0, 4, 4), (3, 2), flags=SUPER4 | WRAP)
    assert warp.size(8, 8, it, 3) == 18 and warp.size(8, 8, it, 4) == 24
    for flags in (SUPER2 | SUPER4, SUPER2 | NEAREST, SUPER4 | BICUBIC, 512):
        assert warp.size(8, 8, warp.item(0, (0, 0, 4, 4), (3, 2), flags=flags), 4) == 0
    with pytest.raises(ValueError, match=BOTH):
        warp.warp(image(8, 8, 3, 1), (0, 0, 4, 4), (4, 4), flags=SUPER2 | SUPER4)
    with pytest.raises(ValueError, match="bilinear sampling only"):
        warp.warp(image(8, 8, 3, 1), (0, 0, 4, 4), (4, 4), flags=SUPER2 | NEAREST)
    # the plan and the tiles do not look at the flags
    assert warp.tiles(40, 24) == 6 and warp.as_crop(it) == (0, 0, 0, 4, 4, 0)


# ---------------------------------------------------------------------------------- older items keep their bytes
def unflagged_cases():
    """(key, arguments of warp.warp) of the recorded calls: every sampling, border and mode at 3 and 4 channels under a reducing turn"""
    for och in (3, 4):
        D = image(33, 21, och, 20 + och)
        for sampling in (0, NEAREST, BICUBIC):
            for border in (0,) + BORDERS:
                for mode in (PLAIN, ALPHA_WEIGHTED):
                    m = warp.rotation((29, 17), (9, 7), 17.0, 1 / 2.5)
                    yield "%d_%d_%d_%d" % (och, sampling, border, mode), (D, (3, 2, 29, 17), (9, 7), m, sampling | border, FILL, mode)


def test_an_item_without_the_flag_gives_what_it_gave_before():
    recorded = np.load(GOLDEN)
    keys = []
    for key, args in unflagged_cases():
        assert np.array_equal(warp.warp(*args), recorded[key]), key
        keys.append(key)
    assert sorted(keys) == sorted(recorded.files) and len(keys) == 2 * 3 * 5 * 2
