"""qoi_amd/bilinear.py - the normative statement of qoimi_decode_bilinear - against an independent statement of the definition in Python integers
(written here), its identity with crops.crop, constants, the mirror symmetry, the bounds of the weights over a sweep of sizes, a float64
evaluation of the same filter by torch on the CPU, the alpha-weighted mode, the plan, the size arithmetic and the kernel's work items.  No GPU,
no library."""
import numpy as np
import pytest

from qoi_amd import bilinear, crops
from qoi_amd.bilinear import ALPHA_WEIGHTED, FLIP_X, FLIP_Y, PLAIN
from qoi_amd.packplan import slot


def tent(Z, k, n_src, n_out):
    return max(0, 2 * max(n_src, n_out) - abs((2 * Z + 1) * n_src - (2 * k + 1) * n_out))


def pixel(D, rect, out_size, X, Y, mode):
    """output pixel (X, Y) of the unflipped result, tap by tap in Python integers"""
    x, y, cw, rh = rect
    ow, oh = out_size
    och = D.shape[2]
    N, M, Wx, Wy = [0] * och, [0] * 3, sum(tent(X, k, cw, ow) for k in range(cw)), sum(tent(Y, r, rh, oh) for r in range(rh))
    for r in range(rh):
        ty = tent(Y, r, rh, oh)
        if ty == 0:
            continue
        for k in range(cw):
            tx = tent(X, k, cw, ow)
            p = [int(v) for v in D[y + r, x + k]]
            for c in range(och):
                N[c] += ty * tx * p[c]
            if och == 4:
                for c in range(3):
                    M[c] += ty * tx * p[c] * p[3]
    Dv = Wx * Wy
    px = [(n + Dv // 2) // Dv for n in N]
    if mode == ALPHA_WEIGHTED and och == 4 and N[3] > 0:
        px[:3] = [(m + N[3] // 2) // N[3] for m in M]
    return px


def brute(D, rect, out_size, flags, mode):
    ow, oh = out_size
    out = [[pixel(D, rect, out_size, X, Y, mode) for X in range(ow)] for Y in range(oh)]
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = [row[::-1] for row in out]
    return np.array(out, dtype=np.uint8)


def image(w, h, och, seed):
    """random pixels, a quarter of them with alpha 0 and - at 4 channels - one all-transparent block in the lower left"""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4:
        D[:, :, 3][rng.integers(0, 4, size=(h, w)) == 0] = 0
        D[h // 2:, :w // 2, 3] = 0
    return D


SIZES = [((11, 9), (3, 2)), ((11, 9), (5, 4)), ((11, 9), (13, 11)), ((11, 9), (1, 1)), ((11, 9), (4, 9)), ((5, 3), (13, 7)), ((1, 1), (4, 3)),
         ((11, 3), (4, 8)), ((3, 11), (7, 2)), ((32, 32), (1, 1)), ((64, 3), (2, 3))]


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
@pytest.mark.parametrize("och", [3, 4])
def test_against_python_integers(och, mode):
    for n, ((cw, rh), (ow, oh)) in enumerate(SIZES):
        D = image(cw + 3, rh + 2, och, n)
        rect = (2, 1, cw, rh)
        got = bilinear.bilinear(D, rect, (ow, oh), n & 3, mode)
        assert got.shape == (oh, ow, och) and got.dtype == np.uint8
        assert np.array_equal(got, brute(D, rect, (ow, oh), n & 3, mode)), (cw, rh, ow, oh)


@pytest.mark.parametrize("och", [3, 4])
def test_identity_is_the_crop(och):
    D = image(23, 17, och, 3)
    for rect in [(0, 0, 23, 17), (3, 5, 7, 9), (22, 16, 1, 1), (0, 4, 23, 1)]:
        for flags in range(4):
            for mode in (PLAIN, ALPHA_WEIGHTED):
                assert np.array_equal(bilinear.bilinear(D, rect, rect[2:], flags, mode), crops.crop(D, rect, flags)), (rect, flags, mode)
    for n in (1, 2, 7, 100):                                              # a single tap of weight rad
        w = bilinear.weights(n, n)
        assert np.array_equal(w, 2 * n * np.eye(n, dtype=np.int64))


def test_a_constant_stays_the_constant():
    for och in (3, 4):
        D = np.empty((40, 70, och), dtype=np.uint8)
        D[:] = [201, 3, 255, 77][:och]
        for rect, out in [((0, 0, 70, 40), (3, 2)), ((5, 5, 1, 1), (9, 4)), ((1, 2, 64, 33), (2, 77)), ((0, 0, 7, 5), (224, 224)), ((3, 0, 37, 40), (36, 41))]:
            for mode in (PLAIN, ALPHA_WEIGHTED):
                got = bilinear.bilinear(D, rect, out, 0, mode)
                assert np.all(got == D[0, 0]), (rect, out, mode)


@pytest.mark.parametrize("mode", [PLAIN, ALPHA_WEIGHTED])
def test_flipping_is_resampling_the_mirrored_source(mode):
    D = image(29, 19, 4, 4)
    for rect, out in [((2, 1, 25, 17), (7, 5)), ((0, 0, 5, 3), (13, 7)), ((3, 3, 11, 4), (4, 9))]:
        R = crops.crop(D, rect)
        whole = (0, 0, rect[2], rect[3])
        for flags in range(4):
            assert np.array_equal(bilinear.bilinear(D, rect, out, flags, mode), bilinear.bilinear(crops.crop(R, whole, flags), whole, out, 0, mode)), (rect, out, flags)


def test_weights_over_a_sweep():
    """W(X) >= 1, at most 64 (2 when enlarging) samples with a weight, contiguous from `first`, symmetric under mirroring; the sweep holds
    n_src = 1, n_out = 1, the ratio of exactly 32 and one just below it"""
    pairs = [(s, o) for s in list(range(1, 40)) + [63, 64, 65, 127, 128, 130] for o in range(1, 45) if s <= 32 * o]
    pairs += [(32 * o, o) for o in range(1, 9)] + [(32 * o - 1, o) for o in range(1, 9)] + [(1, 1000), (1000, 32), (999, 32), (1, 1), (31, 1), (32, 1)]
    assert (1, 1) in pairs and (64, 2) in pairs and (63, 2) in pairs
    most = 0
    for n_src, n_out in pairs:
        w = bilinear.weights(n_src, n_out)
        rad = 2 * max(n_src, n_out)
        assert w.shape == (n_out, n_src) and w.min() >= 0 and w.max() <= rad
        assert np.array_equal(w, w[::-1, ::-1]), (n_src, n_out)
        W = w.sum(axis=1)
        assert W.min() >= 1 and W.max() <= bilinear.taps(n_src, n_out) * rad <= 128 * max(n_src, n_out), (n_src, n_out)
        count = np.count_nonzero(w, axis=1)
        assert count.max() <= bilinear.taps(n_src, n_out) <= 64, (n_src, n_out)
        if n_src <= n_out:
            assert count.max() <= 2
        most = max(most, int(count.max()))
        for X in (0, n_out // 2, n_out - 1):
            nz = np.nonzero(w[X])[0]
            assert nz[0] == bilinear.first(X, n_src, n_out) and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)), (n_src, n_out, X)
    assert most == 64                                                     # the bound is reached: 64 -> 2, an even ratio of 32
    # enlarging: the usual half-pixel-centre bilinear interpolation with replicated borders
    w = bilinear.weights(2, 4)                                            # centres of the outputs at 0.25, 0.75, 1.25, 1.75 source pitches
    assert (w / w.sum(axis=1, keepdims=True)).tolist() == [[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1]]


TORCH_SHAPES = [((1, 1), (5, 3)), ((7, 1), (3, 1)), ((2, 9), (2, 40)), ((37, 23), (80, 50)), ((130, 70), (37, 23)), ((64, 64), (2, 2)), ((96, 96), (224, 224)),
                ((101, 13), (30, 40)), ((13, 101), (40, 30)), ((63, 5), (2, 5)), ((256, 192), (56, 56)), ((33, 31), (32, 33))]


def test_against_torch_float64():
    """torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) in float64 is the same filter evaluated in
    floating point.  Every value is within 1 of the rounded float result: the float error is far below one half, so one rounding can flip
    and nothing more - 1 is no measurement.  The share of values that differ is printed.  (No shape here is a single column resampled in y
    alone: torch 2.10 returns its first row everywhere for a tensor of width 1 with antialias=True, so it is no reference there.)"""
    torch = pytest.importorskip("torch")
    differ = total = 0
    for n, ((cw, rh), (ow, oh)) in enumerate(TORCH_SHAPES):
        D = np.random.default_rng(100 + n).integers(0, 256, size=(rh, cw, 4), dtype=np.uint8)
        got = bilinear.bilinear(D, (0, 0, cw, rh), (ow, oh)).astype(np.int64)
        t = torch.from_numpy(D.astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
        want = np.floor(ref + 0.5).astype(np.int64)
        assert np.abs(got - want).max() <= 1, ((cw, rh), (ow, oh), int(np.abs(got - want).max()))
        assert np.abs(got - ref).max() <= 0.5 + 1e-6, ((cw, rh), (ow, oh))  # (what "one rounding can flip" means: the exact value is at a boundary)
        differ += int(np.count_nonzero(got != want))
        total += got.size
    print("values that differ from the rounded float64 result: %d of %d (%.6f %%)" % (differ, total, 100.0 * differ / total))
    assert any(cw > ow and rh < oh for (cw, rh), (ow, oh) in TORCH_SHAPES) and any(cw < ow and rh > oh for (cw, rh), (ow, oh) in TORCH_SHAPES)


def test_alpha_weighted():
    D = image(40, 30, 4, 6)
    D[:12, 20:, 3] = 0                                                    # a fully transparent neighbourhood in the upper right
    for rect, out in [((0, 0, 40, 30), (10, 10)), ((0, 0, 40, 30), (90, 70)), ((3, 1, 35, 28), (5, 9))]:
        plain, wgt = bilinear.bilinear(D, rect, out, 0, PLAIN), bilinear.bilinear(D, rect, out, 0, ALPHA_WEIGHTED)
        assert np.array_equal(plain[:, :, 3], wgt[:, :, 3])
        ow, oh = out
        clear = 0
        for (X, Y) in [(0, 0), (ow - 1, 0), (ow - 1, 1), (ow // 2, oh // 2), (0, oh - 1), (ow - 1, oh - 1), (ow - 2, 0)]:
            want = pixel(D, rect, out, X, Y, ALPHA_WEIGHTED)
            assert wgt[Y, X].tolist() == want, (rect, out, X, Y)
            if wgt[Y, X, 3] == 0 and want == pixel(D, rect, out, X, Y, PLAIN):
                clear += 1
        assert clear >= 1                                                 # A == 0 there: the PLAIN colours
        assert not np.array_equal(plain, wgt)
    assert np.array_equal(bilinear.bilinear(D[:, :, :3].copy(), (0, 0, 40, 30), (7, 7), 0, ALPHA_WEIGHTED), bilinear.bilinear(D[:, :, :3].copy(), (0, 0, 40, 30), (7, 7), 0, PLAIN))
    Z = D.copy()
    Z[:, :, 3] = 0
    assert np.array_equal(bilinear.bilinear(Z, (0, 0, 40, 30), (9, 4), 0, ALPHA_WEIGHTED), bilinear.bilinear(Z, (0, 0, 40, 30), (9, 4), 0, PLAIN))


def test_limits_and_size():
    D = image(130, 66, 4, 1)
    assert bilinear.bilinear(D, (0, 0, 32, 32), (1, 1)).shape == (1, 1, 4) and bilinear.bilinear(D, (0, 0, 64, 3), (2, 3)).shape == (3, 2, 4)
    for rect, out in [((0, 0, 33, 1), (1, 1)), ((0, 0, 1, 33), (1, 1)), ((0, 0, 65, 3), (2, 3)), ((1, 0, 130, 1), (2, 1)), ((0, 0, 4, 4), (0, 1)), ((0, 0, 4, 4), (1, 0)),
                      ((0, 0, 0, 4), (1, 1)), ((127, 0, 4, 4), (1, 1)), ((0, 63, 4, 4), (1, 1)), ((0, 0, 1, 1), (1 << 15, 1 << 15)), ((0, 0, 130, 1), (1 << 30, 1))]:
        with pytest.raises(ValueError):
            bilinear.bilinear(D, rect, out)
        assert bilinear.size(130, 66, rect, out, 0, 4) == 0
    with pytest.raises(ValueError):
        bilinear.bilinear(D, (0, 0, 4, 4), (2, 2), 4)
    with pytest.raises(ValueError):
        bilinear.bilinear(D, (0, 0, 4, 4), (2, 2), 0, 2)
    assert bilinear.size(130, 66, (0, 0, 130, 66), (224, 224), 3, 3) == 224 * 224 * 3
    assert bilinear.size(130, 66, (0, 0, 1, 1), ((1 << 15) - 1, 1 << 15), 0, 4) == ((1 << 15) - 1) * (1 << 15) * 4
    assert bilinear.size(130, 66, (0, 0, 1, 1), (1, 1), 0, 5) == 0 and bilinear.size(130, 66, (0, 0, 1, 1), (1, 1), 4, 4) == 0
    assert bilinear.MAX_RATIO == 32 and bilinear.MAX_AREA == 1 << 30


def test_plan_is_the_crop_plan():
    descs = [(130, 70), (64, 48), (37, 23), (333, 7)]
    items = [(3, 0, 0, 333, 7, 50, 1, 0), (0, 5, 1, 121, 2, 224, 224, 1), (0, 0, 0, 130, 40, 37, 23, 2), (2, 1, 3, 35, 19, 7, 7, 3)]
    projected = [(3, 0, 0, 333, 7, 0), (0, 5, 1, 121, 2, 1), (0, 0, 0, 130, 40, 2), (2, 1, 3, 35, 19, 3)]
    for staging in (0, 1, 10000, 22000, 1 << 20):
        assert bilinear.plan(descs, items, staging) == crops.plan(descs, projected, staging)
    images, slots, subs, largest = bilinear.plan(descs, items, 1)
    assert images == [0, 2, 3] and slots == [slot(130 * 40 * 4), slot(37 * 22 * 4), slot(333 * 7 * 4)] and len(subs) == 3 and largest == max(slots)


def test_work_items_cover_every_tap_once():
    """the kernel's split: the lanes of an output pixel hold each of its columns with a weight exactly once, and all of its rows"""
    regimes = set()
    for (cw, rh, ow, oh) in [(11, 9, 3, 2), (5, 3, 13, 7), (1, 1, 4, 4), (3, 1, 2, 1), (63, 35, 2, 3), (128, 64, 4, 2), (130, 70, 37, 23), (7, 7, 7, 7), (45, 9, 3, 2), (29, 5, 2, 5), (21, 5, 3, 2)]:
        lg, c = bilinear.split(cw, ow)
        regimes.add(lg)
        tx, ty = bilinear.weights(cw, ow), bilinear.weights(rh, oh)
        assert c <= 4 and c << lg >= bilinear.taps(cw, ow) and bilinear.tiles(cw, ow, oh) == -(-(ow * oh << lg) // 256)
        for o in range(ow * oh):
            cols = []
            for l in range(1 << lg):
                X, Y, lane_cols, rows = bilinear.share((o << lg) | l, cw, rh, ow, oh)
                assert (Y, X) == divmod(o, ow) and len(lane_cols) <= c
                cols += lane_cols
                assert rows == [(r, int(ty[Y, r])) for r in np.nonzero(ty[Y])[0]]
            assert cols == [(k, int(tx[X, k])) for k in np.nonzero(tx[X])[0]], (cw, ow, o)
    assert regimes == {0, 1, 2, 3, 4}
    assert bilinear.split(128, 4) == (4, 4) and bilinear.split(5, 13) == (0, 2)
