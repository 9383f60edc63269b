"""What the device tests of the two filters that keep their weights in LDS tables share (QOIMI_FILTER_BICUBIC and QOIMI_FILTER_LANCZOS;
tests/test_gpu_table_walk.py, test_gpu_bicubic.py, test_gpu_lanczos.py) and what tests/test_table_walk.py asserts of it without a GPU:

* ``items(filter, compute units)``: one call whose tiles outnumber the launch's workgroups (qoi_ctx.h: grid_bound, eight per compute unit) by
  more than two to one, so that a workgroup of tensor_cubic / tensor_lanczos runs three tiles, one behind the other, over the same two LDS
  tables (qoi_table_tiles.h: table_tile_run) - tiles of different items, of different lane counts and table strides;
* ``walk``: qoi_dev.h: walk_tiles stated again - which tiles of which table entries a workgroup takes;
* the pack and the items at the far end of the size limits (``LIMIT_SHAPES``, ``limit_pixels``, ``LIMIT_ITEMS``).

Numpy and the models only: no GPU, no library."""
from bisect import bisect_right

import numpy as np

from qoi_amd import bicubic, lanczos
from qoi_amd.tensors import FILTER_BICUBIC, FILTER_LANCZOS

MODELS = {FILTER_BICUBIC: bicubic, FILTER_LANCZOS: lanczos}
WG_PER_CU = 8                           # qoi_ctx.h: grid_bound

# ---------------------------------------------------------------------------------- the tile walk
# Two images of the same size and different pixels: the first half of the items names the first, the rest the second, so the table's entries
# (sorted by image, otherwise as given: qoi_stage_plan.h: plan_items) stand in the order of the items.  165 rows, not the 66 of the other
# packs: an output of 30 rows or more whose rows have 16 entries or more takes more than 3.75 * 30 source rows under the bicubic filter.
SHAPES = [(70, 165, 4), (70, 165, 4)]
# (x, y, width, height, out_width, out_height); the tiles of a cycle: 1, 1, 1, 1, 3, 1, 1, 1
SIXTEEN = (3, 2, 32, 9, 2, 1)           # 64 / 96 taps: sixteen lanes, one tile of 32 work items
MANY_ROWS = (30, 20, 3, 3, 19, 11)      # one lane, a tile of 11 rows, the kernel cut at every border
TWO_LANES = (5, 40, 20, 4, 12, 3)       # 7 / 10 taps
COLUMN = (69, 0, 1, 160, 1, 32)         # one column of 32 rows with 20 / 30 entries each
WRAP = (9, 7, 5, 3, 300, 2)             # three tiles of one lane, each narrower than a row
FOUR_LANES = (11, 50, 30, 7, 9, 3)      # 14 / 20 taps
DOT = (0, 164, 1, 1, 5, 5)              # q = 2^15 in both axes
SAME = (40, 100, 6, 4, 6, 4)            # the identity: one tap of 2^15
CYCLE = [SIXTEEN, MANY_ROWS, TWO_LANES, COLUMN, WRAP, FOUR_LANES, DOT, SAME]


def pixels():
    """noise with ramps of alpha and runs of alpha 0 between them"""
    rng = np.random.default_rng(20250)
    out = []
    for (w, h, _), (a, b) in zip(SHAPES, ((5, 3), (3, 7))):
        px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        px[:, :, 3] = np.clip(((xx * a + yy * b) % 300) - 40, 0, 255)
        out.append(px)
    return out


def needed(cus):
    """the fewest tiles of the call: with them ceil(tiles / (8 * cus)) is 3"""
    return 2 * WG_PER_CU * cus + 37


def items(filt, cus):
    """The items of the call for a device of `cus` compute units: the cycle again and again until the tiles suffice; item j of cycle number
    j // 8 has the flips (j + j // 8) & 3, so neighbours differ and every geometry meets every flip."""
    m, out, tiles = MODELS[filt], [], 0
    while tiles < needed(cus):
        j = len(out)
        x, y, cw, rh, ow, oh = CYCLE[j % len(CYCLE)]
        out.append((x, y, cw, rh, ow, oh, (j + j // len(CYCLE)) & 3))
        tiles += m.tiles(cw, ow, oh)
    return [(int(2 * j >= len(out)),) + it for j, it in enumerate(out)]


def walk(filt, call, cus):
    """(tiles, workgroups, tiles per workgroup, ranges): walk_tiles over the table of `call` on a device of `cus` compute units.  ranges[g] is
    what workgroup g runs, in its order: (index into `call`, tile within that item); a workgroup without a tile has the empty list."""
    m = MODELS[filt]
    order = sorted(range(len(call)), key=lambda j: call[j][0])            # (stable: the entries of an image as the caller gave them)
    first = [0]
    for j in order:
        first.append(first[-1] + m.tiles(call[j][3], call[j][5], call[j][6]))
    tiles = first.pop()
    grid = min(tiles, WG_PER_CU * cus)
    per_wg = -(-tiles // grid)
    ranges = []
    for g in range(grid):
        lo, hi = g * per_wg, min(g * per_wg + per_wg, tiles)
        ranges.append([(order[e], t - first[e]) for t in range(lo, hi) for e in (bisect_right(first, t) - 1,)])
    return tiles, grid, per_wg, ranges


def tables(filt, it, t):
    """What tile t of item `it` keeps in LDS: ((lg, sx, sy), columns, rows, the weights of those columns and rows as bytes)"""
    m = MODELS[filt]
    _, _, _, cw, rh, ow, oh, _ = it
    lg, c = m.split(cw, ow)
    cols, rows = m.tile(t, cw, ow, oh)
    q = m.weights(cw, ow, cols).tobytes() + m.weights(rh, oh, rows).tobytes()
    return (lg, c << lg, m.taps(rh, oh)), tuple(cols), tuple(rows), q


# ---------------------------------------------------------------------------------- the far end of the limits
LIMIT_SHAPES = [(16384, 1, 4), (1, 16384, 4)]
LIMIT_ITEMS = [(0, 0, 0, 16384, 1, 1024, 1, 1),      # a reduction by exactly 16 at the largest size: 64 / 96 taps, sixteen lanes, flipped in x
               (1, 0, 0, 1, 16384, 1, 1024, 2),      # its vertical twin: four tiles of 256 rows at full sy, row offsets up to the last row
               (1, 0, 5, 1, 3, 1, 16384, 0)]         # 64 tiles of 256 rows of 4 / 6 entries


def limit_pixels():
    rng = np.random.default_rng(20251)
    out = []
    for w, h, _ in LIMIT_SHAPES:
        px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        px[:, :, 3] = np.clip((np.arange(w * h).reshape(h, w) * 7 % 400) - 100, 0, 255)
        out.append(px)
    return out
