"""qoi_amd/warp.py - the normative statement of qoimi_decode_warped.  (a) Its identities, byte for byte: the identity map is crops.crop, the
mirrored maps are the flipped crops, the eight maps of warp.orient are numpy's flips and transposes, enlarging by a power of two with REPLICATE
is bilinear.bilinear, a constant stays the constant.  (b) Two independent references: the same rational definition stated pixel by pixel in
float64 (every intermediate below 2**53: it must agree exactly) and torch's float64 affine_grid + grid_sample fed the same quantised matrix
(every value within 1), both modes and both channel counts.  Then the size, plan and tile arithmetic.  No GPU, no library."""
import math

import numpy as np
import pytest

from qoi_amd import bilinear, crops, warp
from qoi_amd.packplan import slot
from qoi_amd.warp import ALPHA_WEIGHTED, ONE, PLAIN, REPLICATE


def image(w, h, och, seed):
    """random pixels, a quarter of them with alpha 0 and - at 4 channels - one all-transparent block in the lower left"""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4:
        D[:, :, 3][rng.integers(0, 4, size=(h, w)) == 0] = 0
        D[h // 2:, :w // 2, 3] = 0
    return D


RECTS = [(0, 0, 23, 17), (3, 5, 7, 9), (22, 16, 1, 1), (0, 4, 23, 1), (5, 0, 1, 17)]

# (matrix as floats a, b, d, e of the inverse map; the centre goes to the centre), all quantised by warp.rotation or by hand below
MAPS = {"rot30": (30.0, 1.0), "rot-77": (-77.0, 1.0), "rot90": (90.0, 1.0), "down": (0.0, 0.37), "up": (0.0, 3.1), "rot200-up": (200.0, 1.7)}


def matrices(cw, rh, ow, oh):
    out = {name: warp.rotation((cw, rh), (ow, oh), deg, scale) for name, (deg, scale) in MAPS.items()}
    out["shear"] = (ONE, 23000, cw * ONE - ONE * ow - 23000 * oh, -9000, ONE + 700, rh * ONE + 9000 * ow - (ONE + 700) * oh)
    out["far"] = (ONE, 0, 40 * cw * ONE, 0, ONE, -37 * rh * ONE)        # the whole output outside the rectangle
    out["odd"] = (65537, -3, 12345, 7, 65535, -54321)                   # fractions that use all 17 bits
    return out


# ---------------------------------------------------------------------------------- (a) identities
@pytest.mark.parametrize("och", [3, 4])
def test_identity_and_mirrors_are_the_crops(och):
    D = image(23, 17, och, 3)
    for rect in RECTS:
        cw, rh = rect[2:]
        for flags in (0, REPLICATE):
            for mode in (PLAIN, ALPHA_WEIGHTED):
                assert np.array_equal(warp.warp(D, rect, (cw, rh), warp.IDENTITY, flags, 0x12345678, mode), crops.crop(D, rect)), rect
                mx = (-ONE, 0, 2 * cw * ONE, 0, ONE, 0)
                my = (ONE, 0, 0, 0, -ONE, 2 * rh * ONE)
                assert np.array_equal(warp.warp(D, rect, (cw, rh), mx, flags, 0x12345678, mode), crops.crop(D, rect, crops.FLIP_X)), rect
                assert np.array_equal(warp.warp(D, rect, (cw, rh), my, flags, 0x12345678, mode), crops.crop(D, rect, crops.FLIP_Y)), rect


def oriented(R, orientation):
    """the rectangle as an image viewer shows it for the EXIF orientation, in numpy"""
    return {1: R, 2: R[:, ::-1], 3: R[::-1, ::-1], 4: R[::-1], 5: R.transpose(1, 0, 2), 6: np.rot90(R, -1), 7: R[::-1, ::-1].transpose(1, 0, 2),
            8: np.rot90(R, 1)}[orientation]


@pytest.mark.parametrize("och", [3, 4])
def test_the_eight_orientations(och):
    D = image(23, 17, och, 5)
    for rect in RECTS:
        x, y, cw, rh = rect
        for o in range(1, 9):
            it = warp.orient(23, 17, rect, o)
            f = warp.fields(it)
            assert f[:5] == (0, x, y, cw, rh) and f[5:8] == ((rh, cw, 0) if o >= 5 else (cw, rh, 0)) and f[12:14] == (0, 0)
            got = warp.warp(D, rect, f[5:7], (f[8], f[9], f[14], f[10], f[11], f[15]), 0, 0xDEADBEEF, PLAIN)
            assert np.array_equal(got, oriented(D[y:y + rh, x:x + cw], o)), (rect, o)
    assert warp.orient(23, 17, (0, 0, 24, 17), 1) is None and warp.orient(23, 17, (0, 0, 23, 17), 0) is None and warp.orient(23, 17, (0, 0, 23, 17), 9) is None
    assert warp.orient(23, 17, (0, 0, 0, 17), 1) is None


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_power_of_two_enlargement_is_bilinear(och, mode):
    D = image(23, 17, och, 7)
    for rect in RECTS:
        x, y, cw, rh = rect
        for sx, sy in [(2, 2), (4, 4), (8, 8), (2, 4), (4, 2), (1, 8)]:
            m = (ONE // sx, 0, 0, 0, ONE // sy, 0)
            got = warp.warp(D, rect, (cw * sx, rh * sy), m, REPLICATE, 0, mode)
            assert np.array_equal(got, bilinear.bilinear(D, rect, (cw * sx, rh * sy), 0, mode)), (rect, sx, sy)


@pytest.mark.parametrize("och", [3, 4])
def test_a_constant_stays_the_constant(och):
    D = np.empty((9, 11, och), dtype=np.uint8)
    D[:] = [200, 3, 255, 77][:och]
    for name, m in matrices(7, 5, 13, 10).items():
        for mode in (PLAIN, ALPHA_WEIGHTED):
            got = warp.warp(D, (2, 3, 7, 5), (13, 10), m, REPLICATE, 0, mode)
            assert np.all(got == D[0, 0]), name
    # ... and a transparent constant in the alpha-weighted mode keeps its colour (A == 0: the plain value)
    if och == 4:
        D[:, :, 3] = 0
        assert np.all(warp.warp(D, (2, 3, 7, 5), (13, 10), matrices(7, 5, 13, 10)["rot30"], REPLICATE, 0, ALPHA_WEIGHTED) == D[0, 0])


def test_the_fill_is_never_the_image():
    """samples outside the rectangle take the fill (or the rectangle's edge), never the image's pixels beside the rectangle"""
    D = image(23, 17, 4, 9)
    rect = (5, 4, 6, 5)
    E = D.copy()
    E[:4] = 1; E[9:] = 2; E[:, :5] = 3; E[:, 11:] = 4
    for name, m in matrices(6, 5, 12, 9).items():
        for flags in (0, REPLICATE):
            assert np.array_equal(warp.warp(D, rect, (12, 9), m, flags, 0x80FF0040), warp.warp(E, rect, (12, 9), m, flags, 0x80FF0040)), name
    far = warp.warp(D, rect, (12, 9), matrices(6, 5, 12, 9)["far"], 0, 0x80FF0040)
    assert np.all(far == [0x40, 0x00, 0xFF, 0x80])
    assert np.all(warp.warp(D[:, :, :3].copy(), rect, (12, 9), matrices(6, 5, 12, 9)["far"], 0, 0x80FF0040) == [0x40, 0x00, 0xFF])
    # the far map with REPLICATE: the rectangle's top right corner (the map leaves to the right and above)
    assert np.all(warp.warp(D, rect, (12, 9), matrices(6, 5, 12, 9)["far"], REPLICATE, 0) == D[4, 10])


# ---------------------------------------------------------------------------------- (b) independent references
def float_pixel(R, cw, rh, m, X, Y, replicate, fill, weighted):
    """the definition for one output pixel in Python floats (float64): every intermediate is an integer below 2**53, so exact"""
    a, b, c, d, e, f = (float(v) for v in m)
    U, V = 2.0 * X + 1.0, 2.0 * Y + 1.0

    def axis(P, n):
        p = P - 65536.0
        k0 = math.floor(p / 131072.0)
        fr = p - k0 * 131072.0
        taps = []
        for k, wgt in ((k0, 131072.0 - fr), (k0 + 1, fr)):
            if wgt == 0.0:
                continue
            if replicate:
                k = min(max(k, 0), n - 1)
            taps.append((int(k) if 0 <= k < n else None, wgt))
        return taps

    N, M = [0.0] * 4, [0.0] * 3
    for r, wy in axis(d * U + e * V + f, rh):
        for k, wx in axis(a * U + b * V + c, cw):
            v = [float(t) for t in R[r, k]] if r is not None and k is not None else [float((fill >> (8 * t)) & 255) for t in range(4)]
            if len(v) == 3:
                v.append(255.0)
            for t in range(4):
                N[t] += wy * wx * v[t]
            for t in range(3):
                M[t] += wy * wx * v[t] * v[3]
    assert all(n < 2.0 ** 53 for n in N + M)
    px = [math.floor((n + 2.0 ** 33) / 2.0 ** 34) for n in N]
    if weighted and N[3] > 0.0:
        for t in range(3):
            num = M[t] + math.floor(N[3] / 2.0)
            px[t] = (num - math.fmod(num, N[3])) / N[3]
    return px


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_against_the_float64_statement(och, mode):
    D = image(16, 12, och, 11)
    x, y, cw, rh, ow, oh = 3, 2, 9, 7, 14, 11
    for name, m in matrices(cw, rh, ow, oh).items():
        for flags in (0, REPLICATE):
            got = warp.warp(D, (x, y, cw, rh), (ow, oh), m, flags, 0x40C08020, mode)
            R = D[y:y + rh, x:x + cw]
            want = [[float_pixel(R, cw, rh, m, X, Y, bool(flags), 0x40C08020, mode == ALPHA_WEIGHTED and och == 4)[:och] for X in range(ow)] for Y in range(oh)]
            assert np.array_equal(got, np.array(want, dtype=np.uint8)), (name, flags)


def torch_warp(R, out_size, m, replicate, weighted):
    """float64[oh, ow, och]: torch's affine_grid + grid_sample (bilinear, align_corners=False; zeros or border padding) over the rectangle,
    fed the quantised matrix: a normalised output coordinate is U / ow - 1, a normalised source coordinate Px / (65536 * cw) - 1."""
    import torch
    rh, cw, och = R.shape
    ow, oh = out_size
    a, b, c, d, e, f = (float(v) for v in m)
    S = 65536.0
    theta = torch.tensor([[[a * ow / (S * cw), b * oh / (S * cw), (a * ow + b * oh + c) / (S * cw) - 1.0],
                           [d * ow / (S * rh), e * oh / (S * rh), (d * ow + e * oh + f) / (S * rh) - 1.0]]], dtype=torch.float64)
    grid = torch.nn.functional.affine_grid(theta, (1, och, oh, ow), align_corners=False)
    t = torch.from_numpy(R.astype(np.float64)).permute(2, 0, 1)[None]
    if weighted:
        t = torch.cat([t[:, :3] * t[:, 3:4], t[:, 3:4]], dim=1)

    def sample(v):
        return torch.nn.functional.grid_sample(v, grid, mode="bilinear", padding_mode="border" if replicate else "zeros", align_corners=False)[0].permute(1, 2, 0).numpy()

    s = sample(t)
    if weighted:
        plain = sample(torch.from_numpy(R.astype(np.float64)).permute(2, 0, 1)[None])
        # A == 0 is a discontinuity of the definition.  The exact A is 0 or at least 2**-34 (one unit of alpha under the smallest weight); where
        # a position is a sample's centre, float64 leaves a neighbour a weight of about 1e-14, A of up to 255 times that: "positive" is
        # above 2**-35
        A = s[..., 3:4]
        has = A > 2.0 ** -35
        s = np.concatenate([np.where(has, s[..., :3] / np.where(has, A, 1.0), plain[..., :3]), A], axis=2)
    return s


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_against_torch_float64(och, mode):
    """Within 1 everywhere; a difference can arise only where the float result lies at a rounding boundary.  The share of values that differ
    is printed (DESIGN.md section 4i quotes it).  The fill is 0: torch pads with zeros."""
    D = image(70, 50, och, 13)
    x, y, cw, rh, ow, oh = 4, 3, 60, 41, 57, 64
    differ = total = 0
    for name, m in matrices(cw, rh, ow, oh).items():
        for flags in (0, REPLICATE):
            got = warp.warp(D, (x, y, cw, rh), (ow, oh), m, flags, 0, mode).astype(np.float64)
            ref = torch_warp(D[y:y + rh, x:x + cw], (ow, oh), m, bool(flags), mode == ALPHA_WEIGHTED and och == 4)
            err = np.abs(got - np.floor(ref + 0.5))
            assert err.max() <= 1.0, (name, flags, float(err.max()))
            differ += int(np.count_nonzero(err)); total += err.size
    print("torch float64 grid_sample: %d of %d values differ, each by 1" % (differ, total))


# ---------------------------------------------------------------------------------- size, plan, tiles
def test_size_and_limits():
    ok = warp.item(0, (1, 2, 10, 8), (30, 20))
    assert warp.size(20, 15, ok, 3) == 1800 and warp.size(20, 15, ok, 4) == 2400 and warp.size(20, 15, ok, 5) == 0
    for bad in [warp.item(0, (1, 2, 0, 8), (30, 20)), warp.item(0, (1, 2, 10, 8), (0, 20)), warp.item(0, (11, 2, 10, 8), (30, 20)), warp.item(0, (1, 8, 10, 8), (30, 20)),
                warp.item(0, (1, 2, 10, 8), (1 << 20, 1)), warp.item(0, (1, 2, 10, 8), (1, 1 << 20)), warp.item(0, (1, 2, 10, 8), (20000, 20000)),
                warp.item(0, (1, 2, 10, 8), (30, 20), (ONE, 0, 1 << 56, 0, ONE, 0)), warp.item(0, (1, 2, 10, 8), (30, 20), (ONE, 0, 0, 0, ONE, -(1 << 56))),
                warp.item(0, (1, 2, 10, 8), (30, 20), flags=2), ok[:13] + (1,) + ok[14:]]:
        assert warp.size(20, 15, bad, 4) == 0, bad
    edge = warp.item(0, (1, 2, 10, 8), ((1 << 20) - 1, 381), (-2 ** 31, 2 ** 31 - 1, (1 << 56) - 1, 0, 0, 1 - (1 << 56)), REPLICATE)
    assert warp.size(20, 15, edge, 4) == ((1 << 20) - 1) * 381 * 4


def test_plan_is_the_crop_plan():
    descs = [(100, 80), (64, 64), (33, 7)]
    items = [warp.item(2, (0, 0, 33, 7), (5, 5)), warp.item(0, (10, 20, 30, 40), (300, 2), warp.rotation((30, 40), (300, 2), 45.0)), warp.item(0, (0, 0, 5, 5), (1, 1))]
    images, slots, subs, largest = warp.plan(descs, items, 0)
    assert images == [0, 2] and slots == [slot(100 * 60 * 4), slot(33 * 7 * 4)] and subs == [(0, 2)] and largest == sum(slots)
    assert warp.plan(descs, items, 1) == (images, slots, [(0, 1), (1, 1)], max(slots))
    assert warp.plan(descs, items, 0) == crops.plan(descs, [warp.as_crop(it) for it in items], 0)


def test_tiles_cover_the_output_once():
    for ow, oh in [(1, 1), (16, 16), (17, 1), (1, 17), (33, 18), (48, 32)]:
        seen = np.zeros((oh, ow), dtype=np.int32)
        n = warp.tiles(ow, oh)
        assert n == math.ceil(ow / 16) * math.ceil(oh / 16)
        for tile in range(n):
            for wave in range(4):
                got = [warp.place(tile, wave * 64 + lane, ow, oh) for lane in range(64)]
                inside = [p for p in got if p is not None]
                for X, Y in inside:
                    seen[Y, X] += 1
                if inside:                                                  # a wavefront: 16 columns x 4 rows at most
                    xs, ys = [p[0] for p in inside], [p[1] for p in inside]
                    assert max(xs) - min(xs) < 16 and max(ys) - min(ys) < 4
        assert np.all(seen == 1), (ow, oh)
    assert warp.place(warp.tiles(33, 18) - 1, 255, 33, 18) is None
