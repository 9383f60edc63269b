"""qoi_amd/mode.py - the normative statement of QOIMI_FILTER_MODE - against an independent brute-force statement (tests/mode_cases.py:
collections.Counter over the pixels the centre inequality selects), the properties of the cells of an axis, the consequences the header
states, the flips, both channel counts and both modes, tensors.tensors with FILTER_MODE in every dtype and layout, the limits, the split
of a cell over lanes - and REACH: over the label inputs the brute-force statement must meet a lone winner that is not the nearest pixel, a
tie the centre decides, a tie the lowest key decides and an item with an empty cell on one axis and a vote on the other."""
import numpy as np
import pytest

import mode_cases as MC
from qoi_amd import mode, nearest, tensors
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_MODE, FILTER_NEAREST, HW, HWC, I32, I64, U8

IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def pairs():
    rng = np.random.default_rng(5)
    return [(s, o) for s in range(1, 70) for o in range(1, 70)] + [tuple(int(v) for v in rng.integers(1, 16385, size=2)) for _ in range(3000)]


def test_the_cells_of_an_axis():
    for n_src, n_out in pairs():
        Z = np.arange(n_out + 1, dtype=np.int64)
        first = (2 * Z * n_src + n_out - 1) // (2 * n_out)
        assert first[0] == 0 and first[-1] == n_src and np.all(np.diff(first) >= 0)          # the non-empty cells partition [0, n_src) in order
        assert int((2 * Z * n_src + n_out).max()) < 2 ** 30                                  # one 32-bit division
        n = np.diff(first)
        near = nearest.index(n_src, n_out)
        full = n > 0
        if n_src >= n_out:
            assert full.all()                                                                 # reducing: no cell is empty
        assert np.all((first[:-1] <= near)[full] & (near < first[1:])[full])                  # the nearest sample lies in every non-empty cell
        if n_src <= 16 * n_out:
            assert n.max() <= -(-n_src // n_out) <= 16
        for z in {0, n_out // 2, n_out - 1}:
            lo, c = mode.cell(z, n_src, n_out)
            assert mode.first(z, n_src, n_out) == first[z]
            assert (lo, c) == ((int(first[z]), int(n[z])) if n[z] else (int(near[z]), 1))
            if c == 1:
                assert lo == near[z]                                                          # a one-sample cell is the nearest sample
    for n_src, n_out in [(1, 1), (2, 41), (41, 2), (37, 9), (29, 7), (7, 29), (64, 4), (70, 16), (16, 1), (33, 3)]:
        for z in range(n_out):
            lo, c = mode.cell(z, n_src, n_out)
            assert list(range(lo, lo + c)) == MC.axis_cell(z, n_src, n_out), (n_src, n_out, z)    # first() selects what the centre inequality selects


@pytest.fixture(scope="module")
def label_images():
    return MC.images()


def test_labels_against_the_brute_force_statement_and_reach(label_images):
    reach = MC.reach_of(lambda i: label_images[i], MC.LABEL_ITEMS)
    assert all(reach[c] >= 1 for c in "abcd"), reach
    assert reach["d"] == 1
    two_to_one = MC.reach_of(lambda i: label_images[i], [(MC.WIDE, 0, 0, 70, 44, 35, 22, 0)])
    assert two_to_one["b"] >= 1                                                               # (2 x 2 cells: ties, the centre decides some)
    extra = [(MC.WIDE, 5, 3, 63, 41, 7, 20, 0), (MC.WIDE, 3, 1, 64, 44, 4, 3, 0), (MC.SMALL, 1, 2, 33, 25, 33, 2, 0), (MC.SMALL, 0, 0, 37, 29, 3, 50, 0), (MC.WIDE, 0, 0, 70, 44, 35, 22, 0)]
    for it in MC.LABEL_ITEMS + extra:
        for och in (3, 4):
            D = label_images[it[0]]
            D = D[:, :, :och] if D.shape[2] >= och else np.concatenate([D, np.full(D.shape[:2] + (1,), 255, np.uint8)], axis=2)
            for flags in range(4):
                want = MC.brute(D, it[1:5], it[5:7], flags)
                for m in (mode.PLAIN, mode.ALPHA_WEIGHTED):
                    got = mode.mode(D, it[1:5], it[5:7], flags, m)
                    assert got.dtype == np.uint8 and got.shape == (it[6], it[5], och) and np.array_equal(got, want), (it, och, flags, m)
    # the two colours that differ in alpha alone vote apart; och 3 drops alpha after the vote, which is not the vote over the 3-channel decode
    D = label_images[MC.WIDE]
    it = MC.LABEL_ITEMS[1]
    full = mode.mode(D, it[1:5], it[5:7])
    after = mode.mode(D, it[1:5], it[5:7], och=3)
    assert (D[:, :, 3] == 128).any() and np.array_equal(after, full[:, :, :3]) and np.array_equal(after, MC.brute(D, it[1:5], it[5:7], och=3))
    assert not np.array_equal(after, mode.mode(D[:, :, :3], it[1:5], it[5:7]))
    assert np.array_equal(mode.mode(label_images[MC.SMALL], (0, 0, 37, 29), (9, 7), och=4)[:, :, 3], np.full((7, 9), 255, np.uint8))


def test_the_consequences(label_images):
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, size=(45, 70, 4), dtype=np.uint8)
    distinct = np.arange(45 * 70, dtype=np.uint32).reshape(45, 70)
    distinct = np.ascontiguousarray(np.stack([distinct & 255, distinct >> 8, 7 - (distinct & 7), 255 - (distinct & 1)], axis=2).astype(np.uint8))
    assert len({MC.key(p) for p in distinct.reshape(-1, 4)}) == 45 * 70
    L = label_images[MC.WIDE]
    # the output the size of the rectangle or larger on both axes: the nearest filter byte for byte
    for D in (noise, L):
        for rect, out in [((0, 0, 70, 45), (70, 45)), ((3, 5, 31, 23), (50, 41)), ((3, 5, 31, 23), (31, 90)), ((0, 0, 1, 1), (7, 5)), ((69, 44, 1, 1), (1, 1))]:
            for flags in (0, 3):
                assert np.array_equal(mode.mode(D, rect, out, flags), nearest.nearest(D, rect, out, flags)), (rect, out)
    # all pixels distinct: the nearest filter at any size
    for rect, out in [((0, 0, 70, 45), (16, 11)), ((5, 3, 63, 41), (4, 3)), ((0, 0, 70, 45), (100, 3)), ((1, 0, 64, 32), (4, 2))]:
        assert np.array_equal(mode.mode(distinct, rect, out, 1), nearest.nearest(distinct, rect, out, 1)), (rect, out)
    # a constant rectangle gives the constant
    const = np.empty((29, 37, 4), dtype=np.uint8)
    const[:] = (9, 200, 31, 77)
    for out in [(3, 2), (9, 7), (50, 3), (37, 29)]:
        assert np.all(mode.mode(const, (2, 1, 33, 25), out) == np.array([9, 200, 31, 77], dtype=np.uint8))
        assert np.all(mode.mode(const[:, :, :3], (2, 1, 33, 25), out) == np.array([9, 200, 31], dtype=np.uint8))
    # cw = f * ow, rh = g * oh: the cells are the f x g blocks
    f, g = 4, 5
    got = mode.mode(L, (2, 0, 16 * f, 9 * g), (16, 9))
    for Y in range(9):
        for X in range(16):
            assert mode.cell(X, 16 * f, 16) == (X * f, f) and mode.cell(Y, 9 * g, 9) == (Y * g, g)
            block = L[Y * g:(Y + 1) * g, 2 + X * f:2 + (X + 1) * f].reshape(-1, 4)
            counts = {}
            for p in block:
                counts[MC.key(p)] = counts.get(MC.key(p), 0) + 1
            assert counts[MC.key(got[Y, X])] == max(counts.values())


@pytest.mark.parametrize("dtype", (U8, F16, BF16, F32, I32, I64))
@pytest.mark.parametrize("layout", (HWC, CHW, HW))
def test_tensors_with_the_mode_filter(label_images, dtype, layout):
    f = tensors.fmt(dtype, layout) if dtype in (U8, I32, I64) else (dtype, layout, *IMAGENET)
    it = MC.LABEL_ITEMS[1]
    for och in (3, 4):
        D = label_images[MC.WIDE][:, :, :och]
        P = mode.mode(D, it[1:5], it[5:7], 2)
        got = tensors.tensors(D, it[1:5], it[5:7], 2, FILTER_MODE, tensors.ALPHA_WEIGHTED, f)
        assert got.dtype == tensors.numpy_dtype(dtype) and np.array_equal(got.view(np.uint8), tensors.convert(P, f).view(np.uint8))
        assert got.shape == {HWC: (11, 16, och), CHW: (och, 11, 16), HW: (11, 16)}[layout]
        assert not np.array_equal(P, tensors.tensors(D, it[1:5], it[5:7], 2, FILTER_NEAREST))
    assert FILTER_MODE == 11
    with pytest.raises(ValueError):
        tensors.tensors(label_images[0], (0, 0, 4, 4), (2, 2), 0, 10)
    with pytest.raises(ValueError):
        tensors.tensors(label_images[0], (0, 0, 4, 4), (2, 2), 0, 12)


def test_the_limits_and_their_order():
    D = np.zeros((40, 40, 4), dtype=np.uint8)
    w = h = 20000
    for rect, out, flags, word in [((0, 0, 0, 33), (1, 1), 4, "zero"), ((0, 0, 33, 33), (1, 0), 4, "zero"), ((39, 0, 33, 1), (1, 1), 4, "flag"), ((39, 0, 33, 1), (1, 1), 0, "leaves"),
                                   ((0, 0, 33, 1), (2, 1), 0, "16 in an axis"), ((0, 0, 1, 17), (1, 1), 0, "16 in an axis"), ((0, 0, 1, 1), (16385, 1), 0, "16384"),
                                   ((0, 0, 1, 1), (1, 16385), 0, "16384")]:
        with pytest.raises(ValueError, match=word):
            mode.mode(D, rect, out, flags)
    # the ratio before the size
    assert "16 in an axis" in mode._wrong(w, h, (0, 0, 16385, 1), (1, 1), 0) and "16384" in mode._wrong(w, h, (0, 0, 16385, 1), (1025, 1), 0)
    assert mode._wrong(w, h, (0, 0, 16384, 16384), (1024, 1024), 3) == "" and "16 in" in mode._wrong(w, h, (0, 0, 16384, 16384), (1023, 1024), 0)
    assert mode.size(w, h, (0, 0, 32, 16), (2, 1), 0, 4) == 8 and mode.size(w, h, (0, 0, 33, 16), (2, 1), 0, 4) == 0 and mode.size(w, h, (0, 0, 32, 17), (2, 1), 0, 3) == 0
    assert mode.size(w, h, (0, 0, 16384, 3), (1024, 3), 0, 3) == 9216 and mode.size(w, h, (0, 0, 16385, 3), (1025, 3), 0, 3) == 0
    assert mode.size(w, h, (0, 0, 32, 16), (2, 1), 0, 5) == 0
    assert np.array_equal(mode.mode(D, (0, 0, 32, 16), (2, 1)), np.zeros((1, 2, 4), np.uint8))


def test_the_split_of_a_cell_over_lanes():
    seen = set()
    for cw, rh, ow, oh in [(1, 1, 1, 1), (7, 5, 50, 41), (37, 29, 9, 7), (70, 45, 16, 11), (64, 48, 4, 3), (16384, 3, 1024, 3), (3, 16384, 3, 1024), (8, 2, 4, 2), (10, 2, 2, 1),
                           (9, 9, 3, 3), (17, 17, 3, 3), (33, 33, 3, 3), (63, 48, 4, 3), (37, 29, 50, 7)]:
        lg, c = mode.split(cw, rh, ow, oh)
        cells = -(-cw // ow) * -(-rh // oh)
        seen.add(lg)
        assert 0 <= lg <= 6 and 1 <= c <= 4 and (c << lg) >= cells and (lg == 0 or (4 << (lg - 1)) < cells), (cw, rh, ow, oh)
        assert mode.tiles(cw, rh, ow, oh) == -(-(ow * oh << lg) // 256)
        for X in {0, ow // 2, ow - 1}:
            for Y in {0, oh - 1}:
                nx, ny = mode.cell(X, cw, ow)[1], mode.cell(Y, rh, oh)[1]
                held = [mode.held(l, lg, nx, ny) for l in range(1 << lg)]
                assert all(len(hh) <= c for hh in held)
                assert sorted(p for hh in held for p in hh) == sorted((k, r) for r in range(ny) for k in range(nx))      # every pixel of the cell, once
    assert seen == set(range(7))
    assert mode.split(64, 48, 4, 3) == (6, 4) and mode.split(1024, 768, 224, 224) == (3, 3)
