"""qoi_amd/warp.py with VOTE2 and VOTE4 - the normative statement of the majority vote in the affine warp of qoimi_decode_warped.  ``warp``
against the deliberately naive ``vote_reference`` over random maps (scale 0.3 to 5, any turn, a little shear), both flags, the fill and all
four borders, 3 and 4 channels, on label images with stripes one pixel wide, so that ties occur and both the centre rule and the lowest
key decide some; the consequences the definition states: no invented value; the identity and every orientation are crops.crop and the
NEAREST warp; the whole-factor reduction is mode.mode and the MODE tile of tiles.py's definition loop (tests/labelimg.py: loop); a constant
stays the constant under every border; beyond 4 : 1 source pixels are still skipped; the flag rule in its order, 4096 still no flag.  No
GPU, no library."""
import numpy as np
import pytest

import labelimg
from qoi_amd import crops, mode, warp
from qoi_amd.warp import ALPHA_WEIGHTED, BICUBIC, NEAREST, ONE, PLAIN, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4, WRAP

BORDERS = (REPLICATE, REFLECT, REFLECT_101, WRAP)
VOTES = ((VOTE2, 2), (VOTE4, 4))
FILL = 0xFF000007                                                     # r 7, g 0, b 0, a 255: a class of the palette


def labels(w, h, ch, seed):
    """a label image with stripes one pixel wide in both directions"""
    D = labelimg.label_image(w, h, ch, seed)
    D[:, 2::7] = labelimg.PALETTE[2][:ch]
    D[3::6, :] = labelimg.PALETTE[5][:ch]
    return D


def test_the_values():
    assert (VOTE2, VOTE4) == (8192, 16384) and warp.VOTES == 8192 | 16384
    assert [warp.vote_log2(f) for f in (0, REPLICATE, SUPER4, VOTE2, VOTE4 | WRAP)] == [0, 0, 0, 1, 2]


# ---------------------------------------------------------------------------------- the model against the naive reference
def random_map(rng, rect_size, out_size):
    """a turn by any angle at a scale whose reciprocal lies in 0.3 .. 5, with a little shear and an offset of up to two pixels"""
    a, b, c, d, e, f = warp.rotation(rect_size, out_size, float(rng.uniform(0, 360)), 1 / float(rng.uniform(0.3, 5.0)))
    return (a, b + int(rng.integers(-3000, 3000)), c + int(rng.integers(-4 * ONE, 4 * ONE)), d, e, f + int(rng.integers(-4 * ONE, 4 * ONE)))


CENSUS = {}


@pytest.mark.parametrize("flag,s", VOTES)
@pytest.mark.parametrize("border", (0,) + BORDERS)
def test_against_the_naive_reference(border, flag, s):
    rng = np.random.default_rng(100 * s + border)
    census = CENSUS.setdefault(flag, {})
    for ch in (3, 4):
        D = labels(33, 21, ch, 3 + ch)
        for rect, out in (((0, 0, 33, 21), (17, 9)), ((4, 3, 25, 16), (9, 12)), ((30, 20, 1, 1), (3, 2)), ((0, 5, 33, 1), (7, 3))):
            for _ in range(3):
                m = random_map(rng, rect[2:], out)
                got = warp.warp(D, rect, out, m, flag | border, FILL)
                want = warp.vote_reference(D, rect, out, m, flag | border, FILL, census)
                assert got.shape == (out[1], out[0], ch) and np.array_equal(got, want), (ch, rect, out, m)
                assert np.array_equal(warp.warp(D, rect, out, m, flag | border, FILL, ALPHA_WEIGHTED), got)        # both modes give the same bytes
    # a 4-channel decode at och 3: alpha votes, the output lacks it
    D = labels(33, 21, 4, 9)
    m = random_map(rng, (33, 21), (17, 9))
    got = warp.warp(D, (0, 0, 33, 21), (17, 9), m, flag | border, FILL, och=3)
    assert np.array_equal(got, warp.warp(D, (0, 0, 33, 21), (17, 9), m, flag | border, FILL)[:, :, :3])
    assert np.array_equal(got, warp.vote_reference(D, (0, 0, 33, 21), (17, 9), m, flag | border, FILL, och=3))


def test_the_centre_and_the_lowest_key_decided_some():
    """every way a vote is decided occurs under both flags (counted over the cases above where they ran, and over two of them here)"""
    for flag, s in VOTES:
        for border in (0, REFLECT_101):
            test_against_the_naive_reference(border, flag, s)
        census = CENSUS.get(flag, {})
        assert census.get("unique", 0) > 0 and census.get("centre", 0) > 0 and census.get("lowest", 0) > 0, (flag, census)


# ---------------------------------------------------------------------------------- the consequences
def sub_sample_values(D4, rect, out, m, flags, fill):
    """the set of sub-sample values of every output pixel, by NEAREST items: sub-sample (i, j) of the VOTE item is the NEAREST sample of the
    map moved to it - where a * (2i + 1 - s) is a multiple of s, which the maps of this test see to"""
    a, b, c, d, e, f = m
    s = 1 << warp.vote_log2(flags)
    border = flags & warp.BORDERS
    out_sets = []
    for j in range(s):
        for i in range(s):
            di, dj = 2 * i + 1 - s, 2 * j + 1 - s
            assert (a * di + b * dj) % s == 0 and (d * di + e * dj) % s == 0
            out_sets.append(warp.warp(D4, rect, out, (a, b, c + (a * di + b * dj) // s, d, e, f + (d * di + e * dj) // s), NEAREST | border, fill))
    return np.stack(out_sets, axis=2)                                  # [oh, ow, s * s, 4]


@pytest.mark.parametrize("flag,s", VOTES)
def test_no_invented_value(flag, s):
    D = labels(33, 21, 4, 21)
    rect, out = (0, 0, 33, 21), (13, 8)
    a, b, c, d, e, f = warp.rotation((33, 21), out, 30.0, 0.4)
    m = (a & ~3, b & ~3, c, d & ~3, e & ~3, f)                          # multiples of 4: every sub-sample is a NEAREST sample of a moved map
    for border in (0,) + BORDERS:
        got = warp.warp(D, rect, out, m, flag | border, FILL)
        subs = sub_sample_values(D, rect, out, m, flag | border, FILL)
        assert np.all((subs == got[:, :, None, :]).all(axis=3).any(axis=2)), border


@pytest.mark.parametrize("flag,s", VOTES)
def test_the_identity_and_the_orientations(flag, s):
    for ch in (3, 4):
        D = labels(33, 21, ch, 30 + ch)
        rect = (2, 1, 29, 17)
        for border in (0,) + BORDERS:
            assert np.array_equal(warp.warp(D, rect, (29, 17), warp.IDENTITY, flag | border, FILL), crops.crop(D, rect, 0))
        for orientation in range(1, 9):
            it = warp.orient(33, 21, rect, orientation)
            out, m = it[5:7], (it[8], it[9], it[14], it[10], it[11], it[15])
            want = warp.warp(D, rect, out, m, NEAREST, FILL)
            for border in (0, REFLECT):
                assert np.array_equal(warp.warp(D, rect, out, m, flag | border, FILL), want), (orientation, border)


@pytest.mark.parametrize("flag,s", VOTES)
def test_the_whole_factor_reduction(flag, s):
    for ch in (3, 4):
        D = labels(40, 24, ch, 40 + ch)
        for rect in ((0, 0, 40, 24), (4, 4, 32, 16), (3, 1, 4, 4)):
            x, y, cw, rh = rect
            out = (cw // s, rh // s)
            m = (s * ONE, 0, 0, 0, s * ONE, 0)
            want = mode.mode(D, rect, out)
            tile = labelimg.loop(D, (0, x, y, cw, rh, s), 0, labelimg.MODE)                 # QOIMI_TILE_MODE at factor s, by its definition loop
            assert np.array_equal(want, tile)
            for border in (0,) + BORDERS:
                for alpha_mode in (PLAIN, ALPHA_WEIGHTED):
                    assert np.array_equal(warp.warp(D, rect, out, m, flag | border, FILL, alpha_mode), want), (ch, rect, border)
    # a 4-channel decode at 3 output channels: mode.mode's och
    D = labels(40, 24, 4, 44)
    assert np.array_equal(warp.warp(D, (0, 0, 40, 24), (40 // s, 24 // s), (s * ONE, 0, 0, 0, s * ONE, 0), flag, FILL, och=3),
                          mode.mode(D, (0, 0, 40, 24), (40 // s, 24 // s), och=3))


@pytest.mark.parametrize("flag,s", VOTES)
@pytest.mark.parametrize("border", BORDERS)
def test_a_constant_stays_the_constant(border, flag, s):
    D = np.empty((21, 33, 4), dtype=np.uint8)
    D[:] = (200, 3, 97, 131)
    m = warp.rotation((33, 21), (19, 17), 30.0, 1 / 3)                   # reduces by 3; the output's corners leave the rectangle
    got = warp.warp(D, (0, 0, 33, 21), (19, 17), m, flag | border, FILL)
    assert np.all(got == np.array([200, 3, 97, 131], dtype=np.uint8)), border
    assert not np.all(warp.warp(D, (0, 0, 33, 21), (19, 17), m, flag, FILL) == np.array([200, 3, 97, 131], dtype=np.uint8))   # the fill shows


def test_beyond_four_to_one_pixels_are_still_skipped():
    """no adaptivity: at 8 : 1 the 16 sub-samples of VOTE4 look at every second source pixel of a row and column.  Columns of period 2 - class
    A on the even, class B on the odd columns - reduced 8 : 1 with the sub-samples on the even columns give A everywhere, although B holds
    half of every cell; at 4 : 1 the same image is a tie that the centre decides."""
    D = np.empty((16, 64, 4), dtype=np.uint8)
    D[:, 0::2] = labelimg.PALETTE[3]
    D[:, 1::2] = labelimg.PALETTE[1]
    got = warp.warp(D, (0, 0, 64, 16), (8, 2), (8 * ONE, 0, 0, 0, 8 * ONE, 0), VOTE4)          # sub-sample columns 8X + 1, 3, 5, 7
    assert np.all(got == labelimg.PALETTE[1])
    got = warp.warp(D, (0, 0, 64, 16), (16, 4), (4 * ONE, 0, 0, 0, 4 * ONE, 0), VOTE4)         # columns 4X .. 4X + 3: 8 : 8, the centre (4X + 2) decides
    assert np.all(got == labelimg.PALETTE[3])


def test_what_the_flags_are_for():
    """a class one pixel wide in every fourth column, reduced 4 : 1: NEAREST shows it everywhere or nowhere with the phase, the vote never
    lets it win"""
    D = np.empty((16, 64, 3), dtype=np.uint8)
    D[:] = labelimg.PALETTE[0][:3]
    D[:, 2::4] = labelimg.PALETTE[3][:3]
    m = (4 * ONE, 0, 0, 0, 4 * ONE, 0)
    assert np.all(warp.warp(D, (0, 0, 64, 16), (16, 4), m, NEAREST) == labelimg.PALETTE[3][:3])           # the centre column 4X + 2: the thin class alone
    assert np.all(warp.warp(D, (0, 0, 64, 16), (16, 4), m, VOTE4) == labelimg.PALETTE[0][:3])
    assert np.all(warp.warp(D, (0, 0, 64, 16), (16, 4), m, VOTE2) == labelimg.PALETTE[0][:3])             # (2 x 2 at 4 : 1 looks at columns 4X + 1 and 4X + 3)


# ---------------------------------------------------------------------------------- the flag rule
BOTH = "VOTE2 and VOTE4 together"
OWN = "the vote is a sampling of its own"


def wrong(flags, reserved=0):
    return warp._wrong(8, 8, (0, 0, 4, 4), (4, 4), warp.IDENTITY, flags, reserved)


def test_the_flag_rule_in_its_order():
    for flags in (4096, 512, 2, 8, 32, 1 << 15, 1 << 16, 1 << 31, 4096 | VOTE2, VOTE2 | VOTE4 | 4096, VOTE4 | NEAREST | BICUBIC | 2, VOTE2 | 1 | 64 | 32, VOTE2 | SUPER2 | 512):   # 1. an unknown bit
        assert wrong(flags) == "unknown flag bit" == wrong(flags, reserved=1), flags
    for flags in (VOTE2 | NEAREST | BICUBIC, VOTE2 | VOTE4 | SUPER2 | SUPER4 | NEAREST | BICUBIC | 1 | 64):                                       # 2. the two samplings
        assert wrong(flags) == "NEAREST and BICUBIC together" == wrong(flags, reserved=1), flags
    for flags in (VOTE2 | 1 | 64, VOTE2 | VOTE4 | 128 | 256, VOTE4 | NEAREST | 1 | 256, VOTE2 | SUPER2 | SUPER4 | 64 | 128):                         # 3. two borders
        assert wrong(flags).startswith("more than one border") and wrong(flags, reserved=1) == wrong(flags), flags
    for flags in (VOTE2 | SUPER2 | SUPER4, VOTE2 | VOTE4 | SUPER2 | SUPER4 | WRAP):                                                               # 4. both SUPER flags
        assert wrong(flags) == "SUPER2 and SUPER4 together" == wrong(flags, reserved=1), flags
    for flags in (VOTE2 | SUPER2 | NEAREST, VOTE2 | VOTE4 | SUPER4 | BICUBIC | REPLICATE):                                                       # 5. a SUPER flag, not bilinear
        assert wrong(flags).startswith("supersampling is defined for the bilinear sampling only") and wrong(flags, reserved=1) == wrong(flags), flags
    for flags in (VOTE2 | VOTE4, VOTE2 | VOTE4 | REFLECT, VOTE2 | VOTE4 | NEAREST, VOTE2 | VOTE4 | SUPER2, VOTE2 | VOTE4 | BICUBIC | REPLICATE):     # 6. both VOTE flags
        assert wrong(flags) == BOTH == wrong(flags, reserved=1), flags
    for flags in (VOTE2 | NEAREST, VOTE4 | BICUBIC, VOTE4 | NEAREST | WRAP, VOTE2 | SUPER2, VOTE4 | SUPER4 | REPLICATE, VOTE2 | SUPER4 | REFLECT_101):   # 7. not a sampling of its own
        assert wrong(flags).startswith(OWN) and wrong(flags, reserved=1) == wrong(flags), flags
    for flags in (VOTE2, VOTE4, VOTE2 | REPLICATE, VOTE4 | REFLECT, VOTE2 | REFLECT_101, VOTE4 | WRAP):                                           # 8. reserved
        assert wrong(flags) == "" and wrong(flags, reserved=1) == "reserved is not 0", flags
    it = warp.item(0, (0, 0, 4, 4), (3, 2), flags=VOTE4 | WRAP)
    assert warp.size(8, 8, it, 3) == 18 and warp.size(8, 8, it, 4) == 24
    for flags in (VOTE2 | VOTE4, VOTE2 | NEAREST, VOTE4 | BICUBIC, VOTE2 | SUPER2, 4096):
        assert warp.size(8, 8, warp.item(0, (0, 0, 4, 4), (3, 2), flags=flags), 4) == 0
    with pytest.raises(ValueError, match=BOTH):
        warp.warp(labels(8, 8, 3, 1), (0, 0, 4, 4), (4, 4), flags=VOTE2 | VOTE4)
    with pytest.raises(ValueError, match=OWN):
        warp.warp(labels(8, 8, 3, 1), (0, 0, 4, 4), (4, 4), flags=VOTE2 | NEAREST)
    # the plan and the tiles do not look at the flags
    assert warp.tiles(40, 24) == 6 and warp.as_crop(it) == (0, 0, 0, 4, 4, 0)
