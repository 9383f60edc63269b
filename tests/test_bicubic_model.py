"""qoi_amd/bicubic.py, the normative statement of QOIMI_FILTER_BICUBIC, on the CPU: the weights sum to 2**15 with W > 0 and stay inside the
bounds the kernel's 16-bit tables rely on, for every pair of sizes up to 64 within the ratio limit; identity, constants, the 4 x 4 support
when enlarging, flip symmetry; the deviation from a float64 evaluation of the same filter against the bound the docstring derives; `size` on
both sides of each limit; single pixels at the limits in Python `int` arithmetic against the 64-bit bounds the docstring claims."""
import numpy as np
import pytest

from qoi_amd import bicubic, crops
from qoi_amd.bicubic import ALPHA_WEIGHTED, FLIP_X, FLIP_Y, PLAIN


def image(w, h, och, seed=0):
    rng = np.random.default_rng(seed + w * 131 + h)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4:
        D[:, :, 3][rng.integers(0, 4, size=(h, w)) == 0] = 0
        D[h // 2:, : w // 2, 3] = 0
    return D


def test_weights_sum_exactly_and_stay_in_their_bounds():
    lo, hi, l1 = 0, 0, 0
    for n_src in range(1, 65):
        for n_out in range(1, 65):
            if n_src > bicubic.MAX_RATIO * n_out:
                with pytest.raises(ValueError):
                    bicubic.bicubic(np.zeros((1, n_src, 3), np.uint8), (0, 0, n_src, 1), (n_out, 1))
                continue
            c = bicubic.kernel(n_src, n_out)
            assert (c.sum(axis=1) > 0).all(), (n_src, n_out)                       # W(X) > 0
            q = bicubic.weights(n_src, n_out)                                      # (asserts W > 0 and the bounds itself)
            assert (q.sum(axis=1) == bicubic.ONE).all(), (n_src, n_out)
            assert not q[c == 0].any() and int(np.count_nonzero(c, axis=1).max()) <= bicubic.taps(n_src, n_out) <= 64, (n_src, n_out)
            lo, hi, l1 = min(lo, int(q.min())), max(hi, int(q.max())), max(l1, int(np.abs(q).sum(axis=1).max()))
            for X in {0, n_out // 2, n_out - 1}:
                nz = np.nonzero(c[X])[0]
                k0 = bicubic.first(X, n_src, n_out)
                assert k0 <= nz[0] and nz[-1] < k0 + bicubic.taps(n_src, n_out) and (k0 == 0 or c[X, k0 - 1] == 0), (n_src, n_out, X)
    print("q in [%d, %d], sum |q| <= %d" % (lo, hi, l1))
    assert bicubic.Q_MIN <= lo < 0 and bicubic.ONE < hi <= bicubic.Q_MAX and bicubic.ONE < l1 <= bicubic.L1_MAX
    # the deficit goes to the largest c, the lowest k on a tie: 2 -> 1 has c = (9, 9) * u^3 / 8, 2**14 each and nothing to add
    assert bicubic.weights(2, 1).tolist() == [[1 << 14, 1 << 14]]
    q = bicubic.weights(3, 1)[0]                                                    # symmetric: q[0] == q[2] before the deficit, which the middle takes
    assert q[0] == q[2] and q.sum() == bicubic.ONE and q[1] > q[0]
    for n_src, n_out in ((16384, 1024), (16383, 1024), (3, 16384), (16384, 16384), (1, 16384), (16384, 1025)):
        rows = sorted({0, 1, n_out // 3, n_out // 2, n_out - 2, n_out - 1})
        assert (bicubic.weights(n_src, n_out, rows).sum(axis=1) == bicubic.ONE).all()


def test_the_polynomials_are_keys_kernel():
    for n_src, n_out in ((7, 7), (5, 13), (31, 4)):
        u = 2 * max(n_src, n_out)
        c = bicubic.kernel(n_src, n_out)
        for X in range(n_out):
            for k in range(n_src):
                t = abs((2 * X + 1) * n_src - (2 * k + 1) * n_out) / u
                keys = 1.5 * t ** 3 - 2.5 * t ** 2 + 1 if t <= 1 else (-0.5 * t ** 3 + 2.5 * t ** 2 - 4 * t + 2 if t < 2 else 0.0)
                assert abs(int(c[X, k]) - 2 * u ** 3 * keys) < 1e-6 * u ** 3, (n_src, n_out, X, k)
    assert (bicubic.kernel(9, 9) == np.eye(9, dtype=np.int64) * 2 * 18 ** 3).all()


@pytest.mark.parametrize("och", [3, 4])
def test_identity_constant_and_support(och):
    D = image(23, 17, och)
    for mode in (PLAIN, ALPHA_WEIGHTED):
        for flags in range(4):
            for rect in ((0, 0, 23, 17), (3, 2, 11, 9), (22, 16, 1, 1)):
                assert np.array_equal(bicubic.bicubic(D, rect, rect[2:], flags, mode), crops.crop(D, rect, flags)), (rect, flags, mode)
        C = np.empty((9, 11, och), np.uint8)
        C[:] = (7, 250, 0, 131)[:och]
        for out in ((1, 1), (11, 9), (3, 2), (40, 31), (2, 17)):
            got = bicubic.bicubic(C, (1, 1, 9, 7), out, 0, mode)
            assert (got == C[0, 0]).all(), (out, mode)
    for n_src, n_out in ((5, 17), (3, 64), (1, 9), (63, 64), (2, 3)):
        assert int(np.count_nonzero(bicubic.weights(n_src, n_out), axis=1).max()) <= 4 == bicubic.taps(n_src, n_out)


def test_flip_symmetry():
    D = image(41, 33, 4, 5)
    for rect, out in (((2, 1, 37, 29), (5, 7)), ((5, 3, 5, 3), (17, 11)), ((0, 0, 41, 33), (41, 12))):
        for mode in (PLAIN, ALPHA_WEIGHTED):
            base = bicubic.bicubic(D, rect, out, 0, mode)
            x, y, cw, rh = rect
            R = np.zeros_like(D)
            for flags, view in ((FLIP_X, base[:, ::-1]), (FLIP_Y, base[::-1]), (FLIP_X | FLIP_Y, base[::-1, ::-1])):
                assert np.array_equal(bicubic.bicubic(D, rect, out, flags, mode), view)
                # ... and it is the resampled mirrored rectangle: the kernel is symmetric, the deficit tap's tie goes to the mirrored k
                R[y:y + rh, x:x + cw] = crops.crop(D, rect, flags)
                mirrored = bicubic.bicubic(R, rect, out, 0, mode)
                assert np.abs(mirrored.astype(int) - view.astype(int)).max() <= 1


GEOMETRIES = [((64, 64), (4, 4)), ((64, 3), (4, 9)), ((37, 29), (5, 7)), ((5, 3), (17, 11)), ((31, 23), (30, 24)), ((1, 1), (9, 9)), ((67, 45), (20, 13)),
              ((130, 3), (9, 5)), ((48, 48), (3, 3)), ((40, 30), (40, 30))]


def test_deviation_from_float64():
    """|byte - round(clamp(reference))| against the derived bound, measured over noise, a checkerboard of 0 / 255 and an edge"""
    worst, worst_real = 0, 0.0
    for (cw, rh), (ow, oh) in GEOMETRIES:
        yy, xx = np.mgrid[0:rh, 0:cw]
        sources = [image(cw, rh, 3, 9), np.repeat((((xx + yy) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2),
                   np.repeat(((xx * 2 > cw) * 255).astype(np.uint8)[:, :, None], 3, axis=2)]
        b = bicubic.bound(cw, rh, ow, oh)
        assert b == 1, ((cw, rh), (ow, oh), b)                                  # E < 1 for every accepted geometry: at most 64 taps per axis
        for D in sources:
            got = bicubic.bicubic(D, (0, 0, cw, rh), (ow, oh)).astype(np.int64)
            ref = bicubic.reference(D, (0, 0, cw, rh), (ow, oh))
            clamped = np.clip(ref, 0.0, 255.0)
            d = int(np.abs(got - np.floor(clamped + 0.5).astype(np.int64)).max())
            worst, worst_real = max(worst, d), max(worst_real, float(np.abs(got - clamped).max()))
            assert d <= b, ((cw, rh), (ow, oh), d)
    print("largest difference to the rounded reference %d, to the real value %.4f" % (worst, worst_real))
    assert worst_real < 0.5 + 0.74
    # the bound of the largest geometry: 64 taps in both axes
    assert bicubic.bound(16384, 16384, 1024, 1024) == 1 and bicubic.taps(16384, 1024) == 64


def test_size_on_both_sides_of_each_limit():
    w = h = 1 << 20
    for (rect, out, want) in [((0, 0, 16, 1), (1, 1), 1), ((0, 0, 17, 1), (1, 1), 0), ((0, 0, 1, 32), (1, 2), 2), ((0, 0, 1, 33), (1, 2), 0),
                              ((0, 0, 16384, 1), (1024, 1), 1024), ((0, 0, 16385, 1), (1025, 1), 0), ((0, 0, 1, 16384), (1, 16384), 16384),
                              ((0, 0, 1, 16385), (1, 16385), 0), ((0, 0, 1, 1), (16384, 16384), 16384 ** 2), ((0, 0, 1, 1), (16385, 1), 0), ((0, 0, 1, 1), (1, 16385), 0),
                              ((0, 0, 0, 1), (1, 1), 0), ((0, 0, 1, 1), (1, 0), 0), ((w - 1, h - 1, 2, 1), (1, 1), 0)]:
        for och in (3, 4):
            assert bicubic.size(w, h, rect, out, 0, och) == want * och, (rect, out)
            assert bicubic.size(w, h, rect, out, 4, och) == 0
    assert bicubic.size(w, h, (0, 0, 1, 1), (1, 1), 0, 2) == 0
    assert bicubic.plan is not None and bicubic.MAX_RATIO == 16 and bicubic.MAX_SIZE == 16384


def int_axis(Z, n_src, n_out):
    """[(k, c, q)] of the samples with c != 0 and W, in Python integers, straight from the definition"""
    u, o = 2 * max(n_src, n_out), (2 * Z + 1) * n_src
    mid = o // (2 * n_out)
    cs = []
    for k in range(max(0, mid - 70), min(n_src, mid + 70)):
        d = abs(o - (2 * k + 1) * n_out)
        terms = (3 * d ** 3, 5 * u * d ** 2, 2 * u ** 3) if d <= u else ((d ** 3, 5 * u * d ** 2, 8 * u * u * d, 4 * u ** 3) if d < 2 * u else (0,))
        assert all(t < 2 ** 50 for t in terms)
        c = (3 * d ** 3 - 5 * u * d ** 2 + 2 * u ** 3) if d <= u else ((-d ** 3 + 5 * u * d ** 2 - 8 * u * u * d + 4 * u ** 3) if d < 2 * u else 0)
        if c:
            cs.append((k, c))
    W = sum(c for _, c in cs)
    assert 0 < W < 2 ** 53 and all(abs(c) * 2 ** 15 < 2 ** 62 for _, c in cs) and u <= 2 ** 15
    q = [(c * 2 ** 15 + W // 2) // W for _, c in cs]
    best = max(range(len(cs)), key=lambda i: (cs[i][1], -i))
    q[best] += 2 ** 15 - sum(q)
    return [(k, c, qq) for (k, c), qq in zip(cs, q)], W


LIMIT = [(16384, 16384, 1024, 1024), (1, 1, 16384, 16384), (16383, 2, 1024, 16384), (3, 16384, 16384, 1024), (16384, 1, 16384, 1)]


def test_single_pixels_at_the_limits():
    """the largest W, |c|, sum |q| and - for pixels of 255 under every positive weight, 0 under every negative one - the largest N and M"""
    largest = [0, 0, 0, 0, 0]
    for (cw, rh, ow, oh) in LIMIT:
        assert cw <= 16 * ow and rh <= 16 * oh and max(cw, ow, rh, oh) == 16384
        for X in sorted({0, ow // 2, ow - 1}):
            for Y in sorted({0, oh // 3, oh - 1}):
                (cols, Wx), (rows, Wy) = int_axis(X, cw, ow), int_axis(Y, rh, oh)
                assert [q for _, _, q in cols] == bicubic.weights(cw, ow, [X])[0][[k for k, _, _ in cols]].tolist()
                assert [q for _, _, q in rows] == bicubic.weights(rh, oh, [Y])[0][[k for k, _, _ in rows]].tolist()
                l1x, l1y = sum(abs(q) for _, _, q in cols), sum(abs(q) for _, _, q in rows)
                assert all(bicubic.Q_MIN <= q <= bicubic.Q_MAX for _, _, q in cols + rows) and max(l1x, l1y) <= bicubic.L1_MAX
                N = 255 * sum(qy * qx for _, _, qy in rows for _, _, qx in cols if qy * qx > 0)
                largest = [max(a, b) for a, b in zip(largest, (max(Wx, Wy), max(abs(c) for _, c, _ in cols + rows), max(l1x, l1y), N, 255 * N))]
    print("largest W %d, |c| %d, sum |q| %d, N %d, M %d" % tuple(largest))
    assert 2 ** 49 < largest[0] < 2 ** 52 and 2 ** 45 < largest[1] <= 2 ** 46 and largest[3] < 2 ** 40 and largest[4] < 2 ** 48
    assert 255 * bicubic.L1_MAX ** 2 < 2 ** 40 and 255 * 255 * bicubic.L1_MAX ** 2 < 2 ** 48 and bicubic.Q_MAX ** 2 < 2 ** 31
