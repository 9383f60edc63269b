"""The NEAREST flag of qoi_amd/warp.py, the normative statement of QOIMI_WARP_NEAREST, on the CPU: the flag values; the identity map against
crops.crop; all eight warp.orient items against the bilinear model (every position is a pixel centre); a float64 evaluation of floor under a
rotation and a shear with no position on a boundary; label preservation - which the bilinear warp breaks on the same input -; positions
left of and above the rectangle, where Px is negative; and the fill - with and without REPLICATE, for 3 and 4 channels."""
import numpy as np
import pytest

from qoi_amd import crops, tensors, warp


def label_map(h, w, och, seed=0, labels=(3, 7, 20, 200)):
    """uint8[h, w, och]: a few distinct values in sharp regions (every channel holds a label; alpha too)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((yy * 3 // max(h, 1)) + (xx * 2 // max(w, 1)) + ((yy - h // 2) ** 2 + (xx - w // 2) ** 2 < (min(h, w) // 3) ** 2)) % len(labels)
    D = np.empty((h, w, och), dtype=np.uint8)
    for c in range(och):
        D[:, :, c] = np.asarray(labels, dtype=np.uint8)[(region + c) % len(labels)]
    D[rng.integers(0, h), rng.integers(0, w)] = labels[0]
    return D


# ---------------------------------------------------------------------------------- the warp with the NEAREST flag
NEAREST, REPLICATE, ONE = warp.NEAREST, warp.REPLICATE, warp.ONE
FILL = 0x80C04020


def test_the_flag_values():
    assert (REPLICATE, NEAREST) == (1, 4)
    D = np.zeros((4, 4, 4), dtype=np.uint8)
    for flags in (2, 6, 8, 0x80000004):                                  # 2 is still no flag
        with pytest.raises(ValueError, match="unknown flag bit"):
            warp.warp(D, (0, 0, 4, 4), (4, 4), warp.IDENTITY, flags)
        assert warp.size(4, 4, warp.item(0, (0, 0, 4, 4), (4, 4), flags=flags), 4) == 0
    for flags in (0, 1, 4, 5):
        assert warp.size(4, 4, warp.item(0, (0, 0, 4, 4), (4, 4), flags=flags), 4) == 64


@pytest.mark.parametrize("och", [3, 4])
def test_warp_identity_is_the_crop(och):
    D = np.random.default_rng(och + 20).integers(0, 256, size=(20, 24, och), dtype=np.uint8)
    rect = (3, 2, 13, 11)
    for flags in (NEAREST, NEAREST | REPLICATE):
        for mode in (warp.PLAIN, warp.ALPHA_WEIGHTED):
            assert np.array_equal(warp.warp(D, rect, (13, 11), warp.IDENTITY, flags, FILL, mode), crops.crop(D, rect))


@pytest.mark.parametrize("och", [3, 4])
def test_warp_orientations_equal_the_bilinear_model(och):
    D = np.random.default_rng(och + 30).integers(0, 256, size=(20, 24, och), dtype=np.uint8)
    rect = (3, 2, 13, 11)
    for orientation in range(1, 9):
        it = warp.orient(24, 20, rect, orientation)
        out_size, matrix = (it[5], it[6]), (it[8], it[9], it[14], it[10], it[11], it[15])
        want = warp.warp(D, rect, out_size, matrix, 0, FILL)
        for flags in (NEAREST, NEAREST | REPLICATE):
            assert np.array_equal(warp.warp(D, rect, out_size, matrix, flags, FILL), want), orientation
    assert len({warp.orient(24, 20, rect, o)[8:12] for o in range(1, 9)}) == 8


def float_floor_warp(D, rect, out_size, matrix, flags, fill):
    """the same map evaluated in float64 over real pixel coordinates: source pixel k is [k, k + 1), output pixel X has its centre at X + 1/2;
    returns (result, positions that lie exactly on a boundary)"""
    x, y, cw, rh = rect
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    och = D.shape[2]
    Xc = np.arange(ow, dtype=np.float64)[None, :] + 0.5
    Yc = np.arange(oh, dtype=np.float64)[:, None] + 0.5
    xs = (a / 65536.0) * Xc + (b / 65536.0) * Yc + c / 131072.0
    ys = (d / 65536.0) * Xc + (e / 65536.0) * Yc + f / 131072.0
    on_boundary = int(np.count_nonzero((xs == np.floor(xs)) | (ys == np.floor(ys))))
    k, r = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    inside = (k >= 0) & (k < cw) & (r >= 0) & (r < rh)
    if flags & REPLICATE:
        inside[:] = True
    R = D[y:y + rh, x:x + cw]
    F = np.array([(fill >> (8 * i)) & 255 for i in range(och)], dtype=np.uint8)
    return np.where(inside[..., None], R[np.clip(r, 0, rh - 1), np.clip(k, 0, cw - 1)], F[None, None, :]), on_boundary


def off_boundary(matrix):
    """the map with c and f moved by 2**-17 of a pixel where needed so that a + b + c and d + e + f are odd: U and V are odd, so every Px and Py
    is odd and none is a multiple of 2**17 - no position lies on a boundary between two source pixels"""
    a, b, c, d, e, f = matrix
    return (a, b, c + (a + b + c + 1) % 2, d, e, f + (d + e + f + 1) % 2)


@pytest.mark.parametrize("och", [3, 4])
def test_warp_rotation_and_shear_against_float64(och):
    D = label_map(64, 64, och, seed=4)
    rect, out_size = (4, 6, 50, 44), (57, 39)
    shear = (ONE, 23001, -40001, -9001, ONE + 701, 12345)
    excluded = filled = 0
    for matrix in (off_boundary(m) for m in (warp.rotation((50, 44), out_size, 30.0), warp.rotation((50, 44), out_size, 30.0, 1.7), shear)):
        for flags in (NEAREST, NEAREST | REPLICATE):
            want, on_boundary = float_floor_warp(D, rect, out_size, matrix, flags, FILL)
            excluded += on_boundary
            got = warp.warp(D, rect, out_size, matrix, flags, FILL)
            assert np.array_equal(got, want), (matrix, flags)
            allowed = set(np.unique(D[6:50, 4:54]).tolist()) | ({(FILL >> (8 * i)) & 255 for i in range(och)} if not flags & REPLICATE else set())
            assert set(np.unique(got).tolist()) <= allowed
            filled += int(np.count_nonzero((got[:, :, :3] == [0x20, 0x40, 0xC0]).all(axis=2))) if not flags & REPLICATE else 0
    assert filled > 0                                                    # the maps leave the rectangle somewhere
    # what the flag is for: under REPLICATE every value is a label of the rectangle; the bilinear warp of the same item invents values
    turn = off_boundary(warp.rotation((50, 44), out_size, 30.0))
    present = set(np.unique(D[6:50, 4:54]).tolist())
    assert set(np.unique(warp.warp(D, rect, out_size, turn, NEAREST | REPLICATE, FILL)).tolist()) <= present
    assert not set(np.unique(warp.warp(D, rect, out_size, turn, REPLICATE, FILL)).tolist()) <= present
    assert excluded == 0                                                 # no position on a boundary: nothing is left out of the comparison


@pytest.mark.parametrize("och", [3, 4])
def test_warp_left_of_and_above_the_rectangle(och):
    """Px, Py negative: the shift floors, so column -1 is [-131072, 0) and not a mirror of column 0"""
    D = np.random.default_rng(och + 40).integers(0, 256, size=(12, 14, och), dtype=np.uint8)
    rect = (2, 3, 9, 7)
    R = D[3:10, 2:11]
    fill_px = np.array([(FILL >> (8 * i)) & 255 for i in range(och)], dtype=np.uint8)
    # the identity moved by 3 columns and 2 rows and a hair: output pixel (X, Y) looks at column X - 3, row Y - 2 (the hair stays inside the pixel)
    for hair in (0, -1, -ONE + 1, ONE - 1):
        matrix = (ONE, 0, -6 * ONE + hair, 0, ONE, -4 * ONE + hair)
        got = warp.warp(D, rect, (9, 7), matrix, NEAREST, FILL)
        want = np.broadcast_to(fill_px, (7, 9, och)).copy()
        want[2:, 3:] = R[:5, :6]
        assert np.array_equal(got, want), hair
        got = warp.warp(D, rect, (9, 7), matrix, NEAREST | REPLICATE, FILL)
        assert np.array_equal(got, R[np.clip(np.arange(7) - 2, 0, 6)][:, np.clip(np.arange(9) - 3, 0, 8)]), hair
    # one unit further and the position -65536 - 1 + ... crosses into the next column: floor, not truncation
    got = warp.warp(D, rect, (1, 1), (ONE, 0, -ONE - 1, 0, ONE, -ONE), NEAREST, FILL)       # Px = -1 -> column -1, Py = 0 -> row 0
    assert np.array_equal(got[0, 0], fill_px)
    got = warp.warp(D, rect, (1, 1), (ONE, 0, -ONE, 0, ONE, -ONE), NEAREST, FILL)           # Px = 0 -> column 0
    assert np.array_equal(got[0, 0], R[0, 0])


@pytest.mark.parametrize("och", [3, 4])
def test_warp_fill(och):
    D = np.random.default_rng(och + 50).integers(0, 256, size=(8, 8, och), dtype=np.uint8)
    far = (ONE, 0, 40 * ONE * 8, 0, ONE, 0)                              # every position right of the rectangle
    for fill in (0, FILL, 0xFFFFFFFF, 0x01020304):
        fill_px = np.array([(fill >> (8 * i)) & 255 for i in range(och)], dtype=np.uint8)
        got = warp.warp(D, (0, 0, 8, 8), (5, 4), far, NEAREST, fill)
        assert np.array_equal(got, np.broadcast_to(fill_px, (4, 5, och)))                   # a 3-channel output ignores the fill's alpha
        got = warp.warp(D, (0, 0, 8, 8), (5, 4), far, NEAREST | REPLICATE, fill)
        assert np.array_equal(got, np.broadcast_to(D[:4, 7:8], (4, 5, och)))                # the last column, whatever the fill
        for mode in (warp.PLAIN, warp.ALPHA_WEIGHTED):
            assert np.array_equal(warp.warp(D, (0, 0, 8, 8), (5, 4), far, NEAREST, fill, mode), np.broadcast_to(fill_px, (4, 5, och)))
    f = tensors.fmt(tensors.F16, tensors.CHW)
    assert np.array_equal(tensors.warped_tensors(D, (0, 0, 8, 8), (8, 8), warp.IDENTITY, NEAREST, 0, warp.PLAIN, f), D.transpose(2, 0, 1).astype(np.float16))
