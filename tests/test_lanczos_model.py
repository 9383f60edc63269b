"""qoi_amd/lanczos.py, the normative statement of QOIMI_FILTER_LANCZOS, on the CPU: the kernel table against mpmath (a second, independent
evaluation) and against the committed header; the weights sum to 2**15 with W > 0 and stay inside the bounds the kernel's 16-bit tables rely
on, for every pair of sizes up to 64 within the ratio limit and at the extremes; identity, constants, the 6 x 6 support when enlarging, flip
symmetry; the deviation from a float64 evaluation of the same filter against the bound the docstring derives; PIL's LANCZOS beside it; `size`
on both sides of each limit."""
import os
import re

import numpy as np
import pytest

from qoi_amd import crops, lanczos
from qoi_amd.lanczos import ALPHA_WEIGHTED, FLIP_X, FLIP_Y, PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def image(w, h, och, seed=0):
    rng = np.random.default_rng(seed + w * 131 + h)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4:
        D[:, :, 3][rng.integers(0, 4, size=(h, w)) == 0] = 0
        D[h // 2:, : w // 2, 3] = 0
    return D


def test_the_table_against_mpmath_and_the_header():
    mpmath = pytest.importorskip("mpmath")
    T = lanczos.table()
    assert T.shape == (3073,) and T[0] == 1 << 30 and T[3072] == 0 and T[1024] == 0 and T[2048] == 0
    assert T[512] == 652756755 and T[1536] == -145057057 and T.min() == -158126265 and T.max() == 1 << 30
    with mpmath.workdps(50):
        for i in range(1, 3072):
            v = (1 << 30) * mpmath.sincpi(mpmath.mpf(i) / 1024) * mpmath.sincpi(mpmath.mpf(i) / 3072)
            assert int(mpmath.nint(v)) == int(T[i]) and abs(abs(v - int(T[i])) - mpmath.mpf(1) / 2) > mpmath.mpf(10) ** -12, i    # correctly rounded, no tie
    text = open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_lanczos_table.h")).read()
    assert text == lanczos.header_text()                                           # the header is what the generator prints
    body = text[text.index("{", text.index("kLanczosTable")) + 1:text.rindex("};")]
    assert [int(v) for v in re.findall(r"-?\d+", body)] == T.tolist()


def scan(n_src, n_out, rows=None):
    c = lanczos.kernel(n_src, n_out, rows)
    W = c.sum(axis=1)
    assert (W > 0).all() and (W < lanczos.W_MAX).all(), (n_src, n_out)
    q = lanczos.weights(n_src, n_out, rows)                                        # (asserts W and the bounds itself)
    assert (q.sum(axis=1) == lanczos.ONE).all(), (n_src, n_out)
    assert not q[c == 0].any() and int(np.count_nonzero(c, axis=1).max()) <= lanczos.taps(n_src, n_out) <= 96, (n_src, n_out)
    Xs = range(n_out) if rows is None else rows
    for j, X in enumerate(Xs):
        if rows is None and X not in (0, n_out // 2, n_out - 1):
            continue
        nz = np.nonzero(c[j])[0]
        k0 = lanczos.first(X, n_src, n_out)
        assert k0 <= nz[0] and nz[-1] < k0 + lanczos.taps(n_src, n_out) and (k0 == 0 or c[j, k0 - 1] == 0), (n_src, n_out, X)
    u = 2 * max(n_src, n_out)
    return int(q.min()), int(q.max()), int(np.abs(q).sum(axis=1).max()), int(W.max()), float(W.min()) * 2 * n_out / (u * u * 2.0 ** 30)


def test_weights_sum_exactly_and_stay_in_their_bounds():
    seen = []
    for n_src in range(1, 65):
        for n_out in range(1, 65):
            if n_src > lanczos.MAX_RATIO * n_out:
                with pytest.raises(ValueError):
                    lanczos.lanczos(np.zeros((1, n_src, 3), np.uint8), (0, 0, n_src, 1), (n_out, 1))
                continue
            seen.append(scan(n_src, n_out))
    lo, hi, l1 = min(s[0] for s in seen), max(s[1] for s in seen), max(s[2] for s in seen)
    print("up to 64: q in [%d, %d], sum |q| <= %d, W < 2**%d, W / full window >= %.4f" % (lo, hi, l1, max(s[3] for s in seen).bit_length(), min(s[4] for s in seen)))
    assert (lo, hi) == (-9198, 41966)                                               # at 2 -> 64: the figures the docstring quotes
    for b in range(1, 40):
        seen.append(scan(16 * b, b))
        seen.append(scan(16 * b - 1, b))
    for n_src, n_out in ((16384, 1024), (16383, 1024), (1000, 16384), (1, 16384), (2, 16384), (3, 16384), (16384, 16384), (16384, 1025)):
        seen.append(scan(n_src, n_out, sorted({0, 1, 2, n_out // 3, n_out // 2, n_out - 3, n_out - 2, n_out - 1})))
    lo, hi, l1 = min(s[0] for s in seen), max(s[1] for s in seen), max(s[2] for s in seen)
    print("in all: q in [%d, %d], sum |q| <= %d, W < 2**%d, W / full window >= %.4f" % (lo, hi, l1, max(s[3] for s in seen).bit_length(), min(s[4] for s in seen)))
    assert lanczos.Q_MIN <= lo == -9362 and lanczos.ONE < hi == 42130 <= lanczos.Q_MAX and lanczos.ONE < l1 <= lanczos.L1_MAX
    assert lanczos.Q_MIN + lanczos.BIAS >= 0 and lanczos.Q_MAX + lanczos.BIAS < 1 << 16 and min(s[4] for s in seen) >= 0.25
    assert 255 * lanczos.L1_MAX ** 2 < 2 ** 40 and 255 * 255 * lanczos.L1_MAX ** 2 < 2 ** 48 and lanczos.Q_MAX ** 2 >= 2 ** 31
    # the deficit goes to the largest c, the lowest k on a tie: 2 -> 1 is symmetric, 2**14 each and nothing to add
    assert lanczos.weights(2, 1).tolist() == [[1 << 14, 1 << 14]]
    q = lanczos.weights(3, 1)[0]
    assert q[0] == q[2] and q.sum() == lanczos.ONE and q[1] > q[0]


def test_the_kernel_is_the_interpolated_table():
    T = lanczos.table()
    for n_src, n_out in ((7, 7), (5, 13), (31, 4)):
        u = 2 * max(n_src, n_out)
        c = lanczos.kernel(n_src, n_out)
        for X in range(n_out):
            for k in range(n_src):
                d = abs((2 * X + 1) * n_src - (2 * k + 1) * n_out)
                want = 0
                if d < 3 * u:
                    i, r = divmod(1024 * d, u)
                    want = int(T[i]) * (u - r) + int(T[i + 1]) * r
                assert int(c[X, k]) == want, (n_src, n_out, X, k)
                assert abs(want / (u * 2.0 ** 30) - (np.sinc(d / u) * np.sinc(d / u / 3) if d < 3 * u else 0.0)) < 4.5e-7
    assert (lanczos.kernel(9, 9) == np.eye(9, dtype=np.int64) * 18 * (1 << 30)).all()


@pytest.mark.parametrize("och", [3, 4])
def test_identity_constant_and_support(och):
    D = image(23, 17, och)
    for mode in (PLAIN, ALPHA_WEIGHTED):
        for flags in range(4):
            for rect in ((0, 0, 23, 17), (3, 2, 11, 9), (22, 16, 1, 1)):
                assert np.array_equal(lanczos.lanczos(D, rect, rect[2:], flags, mode), crops.crop(D, rect, flags)), (rect, flags, mode)
        C = np.empty((9, 11, och), np.uint8)
        C[:] = (7, 250, 0, 131)[:och]
        for out in ((1, 1), (11, 9), (3, 2), (40, 31), (2, 17)):
            got = lanczos.lanczos(C, (1, 1, 9, 7), out, 0, mode)
            assert (got == C[0, 0]).all(), (out, mode)
    for n_src, n_out in ((5, 17), (3, 64), (1, 9), (63, 64), (2, 3)):
        assert int(np.count_nonzero(lanczos.weights(n_src, n_out), axis=1).max()) <= 6 == lanczos.taps(n_src, n_out)


def test_flip_symmetry():
    D = image(41, 33, 4, 5)
    for rect, out in (((2, 1, 37, 29), (5, 7)), ((5, 3, 5, 3), (17, 11)), ((0, 0, 41, 33), (41, 12))):
        for mode in (PLAIN, ALPHA_WEIGHTED):
            base = lanczos.lanczos(D, rect, out, 0, mode)
            x, y, cw, rh = rect
            R = np.zeros_like(D)
            for flags, view in ((FLIP_X, base[:, ::-1]), (FLIP_Y, base[::-1]), (FLIP_X | FLIP_Y, base[::-1, ::-1])):
                assert np.array_equal(lanczos.lanczos(D, rect, out, flags, mode), view)
                # ... and it is the resampled mirrored rectangle: the kernel is symmetric, the deficit tap's tie goes to the mirrored k
                R[y:y + rh, x:x + cw] = crops.crop(D, rect, flags)
                mirrored = lanczos.lanczos(R, rect, out, 0, mode)
                assert np.abs(mirrored.astype(int) - view.astype(int)).max() <= 1


GEOMETRIES = [((64, 64), (4, 4)), ((64, 3), (4, 9)), ((37, 29), (5, 7)), ((5, 3), (17, 11)), ((31, 23), (30, 24)), ((1, 1), (9, 9)), ((67, 45), (20, 13)),
              ((130, 3), (9, 5)), ((48, 48), (3, 3)), ((40, 30), (40, 30)), ((128, 33), (8, 3)), ((2, 2), (64, 64))]


def sources(cw, rh):
    yy, xx = np.mgrid[0:rh, 0:cw]
    return [image(cw, rh, 3, 9), np.repeat((((xx + yy) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2),
            np.repeat(((xx * 2 > cw) * 255).astype(np.uint8)[:, :, None], 3, axis=2)]


def test_deviation_from_float64():
    """|byte - round(clamp(reference))| against the derived bound, measured over noise, a checkerboard of 0 / 255 and an edge.  Observed: the
    largest difference to the rounded reference is 1, to the real value 0.5073."""
    worst, worst_real = 0, 0.0
    for (cw, rh), (ow, oh) in GEOMETRIES:
        b = lanczos.bound(cw, rh, ow, oh)
        tx, ty = lanczos.taps(cw, ow), lanczos.taps(rh, oh)
        assert b == (1 if (tx - 1) + (ty - 1) <= 125 else 2), ((cw, rh), (ow, oh), b)
        for D in sources(cw, rh):
            got = lanczos.lanczos(D, (0, 0, cw, rh), (ow, oh)).astype(np.int64)
            ref = lanczos.reference(D, (0, 0, cw, rh), (ow, oh))
            clamped = np.clip(ref, 0.0, 255.0)
            d = int(np.abs(got - np.floor(clamped + 0.5).astype(np.int64)).max())
            worst, worst_real = max(worst, d), max(worst_real, float(np.abs(got - clamped).max()))
            assert d <= b, ((cw, rh), (ow, oh), d)
    print("largest difference to the rounded reference %d, to the real value %.4f" % (worst, worst_real))
    assert worst_real < 0.5 + 1.5
    # the bound of the largest geometry: 96 taps in both axes; of an enlargement: 6
    assert lanczos.bound(16384, 16384, 1024, 1024) == 2 and lanczos.taps(16384, 1024) == 96 and lanczos.bound(3, 3, 16384, 16384) == 1


def test_against_pil_lanczos():
    """PIL's Image.LANCZOS is the same kernel on the same centres, renormalised at the borders alike, but it runs two passes - x, then y - and
    rounds AND clamps to 0..255 between them.  Where its first pass stays inside 0..255 only the extra rounding separates it from the one
    rounding here: the largest difference observed over these geometries and sources is 1, the test allows 2 more.  Where the first pass
    overshoots PIL cuts the overshoot off before the second pass and the results part by what was cut - up to 45 on the 2 x 2 checkerboard
    enlarged to 64 x 64, 38 on 5 x 3 -> 17 x 11; that this is all of it shows the model's own weights run PIL's way (two passes, rounded and
    clamped between): within 1 of PIL over every geometry and source, allowed 2 more."""
    Image = pytest.importorskip("PIL.Image")
    worst, worst_two, worst_cut, compared = 0, 0, 0, 0
    for (cw, rh), (ow, oh) in GEOMETRIES:
        qx, qy = lanczos.weights(cw, ow), lanczos.weights(rh, oh)
        for D in sources(cw, rh):
            got = lanczos.lanczos(D, (0, 0, cw, rh), (ow, oh)).astype(np.int64)
            pil = np.asarray(Image.fromarray(D, "RGB").resize((ow, oh), Image.LANCZOS)).astype(np.int64)
            H = (np.einsum("Xk,rkc->rXc", qx, D.astype(np.int64)) + (1 << 14)) >> 15           # PIL's first pass with the model's weights
            two = np.clip((np.einsum("Yr,rXc->YXc", qy, np.clip(H, 0, 255)) + (1 << 14)) >> 15, 0, 255)
            worst_two = max(worst_two, int(np.abs(two - pil).max()))
            if H.min() >= 0 and H.max() <= 255:
                worst, compared = max(worst, int(np.abs(got - pil).max())), compared + 1
            else:
                worst_cut = max(worst_cut, int(np.abs(got - pil).max()))
    print("largest difference to PIL %d over %d comparisons; %d where its first pass is cut; PIL's way %d" % (worst, compared, worst_cut, worst_two))
    assert compared >= len(GEOMETRIES) and worst <= 1 + 2 and worst_two <= 1 + 2


def test_size_on_both_sides_of_each_limit():
    w = h = 1 << 20
    for (rect, out, want) in [((0, 0, 16, 1), (1, 1), 1), ((0, 0, 17, 1), (1, 1), 0), ((0, 0, 1, 32), (1, 2), 2), ((0, 0, 1, 33), (1, 2), 0),
                              ((0, 0, 16384, 1), (1024, 1), 1024), ((0, 0, 16385, 1), (1025, 1), 0), ((0, 0, 1, 16384), (1, 16384), 16384),
                              ((0, 0, 1, 16385), (1, 16385), 0), ((0, 0, 1, 1), (16384, 16384), 16384 ** 2), ((0, 0, 1, 1), (16385, 1), 0), ((0, 0, 1, 1), (1, 16385), 0),
                              ((0, 0, 0, 1), (1, 1), 0), ((0, 0, 1, 1), (1, 0), 0), ((w - 1, h - 1, 2, 1), (1, 1), 0)]:
        for och in (3, 4):
            assert lanczos.size(w, h, rect, out, 0, och) == want * och, (rect, out)
            assert lanczos.size(w, h, rect, out, 4, och) == 0
    assert lanczos.size(w, h, (0, 0, 1, 1), (1, 1), 0, 2) == 0
    assert lanczos.plan is not None and lanczos.MAX_RATIO == 16 and lanczos.MAX_SIZE == 16384
