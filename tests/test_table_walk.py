"""The geometry of the device tests of the two table filters, from the models alone (no GPU, no library): that the call of
tests/table_tiles.py: items makes a workgroup of tensor_cubic / tensor_lanczos run three tiles whose LDS tables differ from one to the next -
for devices of 256, 304 and 8 compute units - and that the items tests/test_gpu_bicubic.py adds take the paths they are named for."""
from math import gcd

import numpy as np
import pytest

import table_tiles as tt
from qoi_amd import bicubic
from qoi_amd.tensors import FILTER_BICUBIC, FILTER_LANCZOS

FILTERS = [FILTER_BICUBIC, FILTER_LANCZOS]


@pytest.mark.parametrize("cus", [256, 304, 8])
@pytest.mark.parametrize("filt", FILTERS)
def test_a_workgroup_runs_three_tiles_with_different_tables(filt, cus):
    m = tt.MODELS[filt]
    call = tt.items(filt, cus)
    tiles, grid, per_wg, ranges = tt.walk(filt, call, cus)
    # more tiles than twice the clamp: three per workgroup, two at least in every workgroup with work but the last
    assert tiles == sum(m.tiles(it[3], it[5], it[6]) for it in call) >= 2 * 8 * cus + 37 and 8 * cus < tiles
    assert grid == 8 * cus and per_wg == -(-tiles // grid) == 3
    assert [t for r in ranges for t in r] == [(j, t) for j, it in enumerate(call) for t in range(m.tiles(it[3], it[5], it[6]))]
    busy = [r for r in ranges if r]
    assert len(busy) > 2 * grid // 3 and all(len(r) == 3 for r in busy[:-1]) and len(busy[-1]) >= 1
    # the table's order is the call's
    assert [it[0] for it in call] == sorted(it[0] for it in call) and {it[0] for it in call} == {0, 1}
    # the cycle: its items and its tiles are both coprime to the tiles of a workgroup, so a workgroup begins at every tile of the cycle
    per_cycle = sum(m.tiles(g[2], g[4], g[5]) for g in tt.CYCLE)
    assert [m.tiles(g[2], g[4], g[5]) for g in tt.CYCLE] == [1, 1, 1, 1, 3, 1, 1, 1]
    assert gcd(len(tt.CYCLE), per_wg) == 1 and gcd(per_cycle, per_wg) == 1 and len(set(tt.CYCLE)) == len(tt.CYCLE)
    begins = {(call[r[0][0]][1:7], r[0][1]) for r in busy}
    assert begins == {(g, t) for g in tt.CYCLE for t in range(m.tiles(g[2], g[4], g[5]))}
    # a workgroup lands in the middle of an item, and workgroups step from item to item
    assert any(r[0][1] > 0 for r in busy) and any(a[0] != b[0] for r in busy for a, b in zip(r, r[1:]))
    assert any(a[0] == b[0] for r in busy for a, b in zip(r, r[1:]))
    # two tiles a workgroup runs back to back differ in (lg, sx, sy), in their columns or in their rows - and in what the tables then hold
    seen = {}
    pairs = set()
    for r in busy:
        for (ja, ta), (jb, tb) in zip(r, r[1:]):
            key = (call[ja][1:7], ta, call[jb][1:7], tb)
            pairs.add(key)
            if key not in seen:
                a, b = tt.tables(filt, call[ja], ta), tt.tables(filt, call[jb], tb)
                seen[key] = a[:3] != b[:3] and a[3] != b[3]
            assert seen[key], key
    assert len(pairs) == per_cycle                                        # every neighbouring pair of the cycle's tiles
    # the flips take turns: neighbours differ, every geometry meets all four
    assert all(a[7] != b[7] for a, b in zip(call, call[1:]))
    assert all({it[7] for it in call if it[1:7] == g} == {0, 1, 2, 3} for g in tt.CYCLE)
    # small: few distinct items for the models, every item inside its image, the outputs of a call within a few MB at 2 bytes an element
    assert len(set(call)) <= 2 * 4 * len(tt.CYCLE)
    assert all(bicubic._wrong(*tt.SHAPES[it[0]][:2], it[1:5], it[5:7], it[7]) == "" for it in set(call))
    assert sum(it[5] * it[6] for it in call) * 4 * 2 < 4 << 20


@pytest.mark.parametrize("filt", FILTERS)
def test_the_cycle_holds_the_geometries_it_is_there_for(filt):
    m = tt.MODELS[filt]
    most = 64 if filt == FILTER_BICUBIC else 96
    _, _, cw, rh, ow, oh = tt.SIXTEEN
    assert m.taps(cw, ow) == most and m.split(cw, ow)[0] == 4 and m.tiles(cw, ow, oh) == 1
    _, _, cw, rh, ow, oh = tt.MANY_ROWS
    assert cw < ow and m.split(cw, ow)[0] == 0 and m.tiles(cw, ow, oh) == 1 and len(m.tile(0, cw, ow, oh)[1]) == 11
    assert m.first(0, cw, ow) == 0 and m.taps(cw, ow) > cw              # fewer samples than taps: the kernel of every column and row is cut
    _, _, cw, rh, ow, oh = tt.TWO_LANES
    assert m.split(cw, ow)[0] == 1
    _, _, cw, rh, ow, oh = tt.COLUMN
    assert ow == 1 and oh >= 30 and m.taps(rh, oh) >= 16 and m.tile(0, cw, ow, oh) == ([0], list(range(oh)))
    _, _, cw, rh, ow, oh = tt.WRAP
    assert m.split(cw, ow)[0] == 0 and m.tiles(cw, ow, oh) == 3 and ow > 256
    assert m.tile(1, cw, ow, oh) == (list(range(256, 300)) + list(range(212)), [0, 1]) and m.tile(2, cw, ow, oh) == (list(range(212, 300)), [1])
    _, _, cw, rh, ow, oh = tt.FOUR_LANES
    assert m.split(cw, ow)[0] == 2
    for g in (tt.DOT, tt.SAME):
        assert int(m.weights(g[2], g[4]).max()) == 1 << 15 == int(m.weights(g[3], g[5]).max())
    assert all(w <= 70 and h <= 165 for w, h, _ in tt.SHAPES)
    a, b = tt.pixels()
    assert a.shape == b.shape == (165, 70, 4) and not np.array_equal(a, b) and (a[:, :, 3] == 0).any() and (a[:, :, 3] == 255).any()


def test_the_limit_items():
    for m, most in ((tt.MODELS[FILTER_BICUBIC], 64), (tt.MODELS[FILTER_LANCZOS], 96)):
        across, down, up = tt.LIMIT_ITEMS
        assert m.taps(16384, 1024) == most and m.split(across[3], across[5])[0] == 4 and across[7] == m.FLIP_X
        assert m.split(down[3], down[5])[0] == 0 and m.tiles(down[3], down[5], down[6]) == 4 and down[7] == m.FLIP_Y
        assert m.tile(3, 1, 1, 1024) == ([0], list(range(768, 1024))) and m.weights(16384, 1024, [1023])[0, 16383] != 0
        assert m.tiles(up[3], up[5], up[6]) == 64 and len(m.tile(63, 1, 1, 16384)[1]) == 256 and m.taps(3, 16384) in (4, 6)
        for it in tt.LIMIT_ITEMS:
            assert m._wrong(*tt.LIMIT_SHAPES[it[0]][:2], it[1:5], it[5:7], it[7]) == ""


def test_the_bicubic_items_take_the_paths_they_are_named_for():
    from model_cases import assert_bicubic_paths
    assert_bicubic_paths()
