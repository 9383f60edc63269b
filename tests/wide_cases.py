"""What the wide-regime GPU tests share: the 17.7 Mpx image of tests/resize_window.py with a block of noise and a label map planted in
its last rows (every pixel index there is at least 2**24), the tables of the many-tiles-per-workgroup walks over it, and the offsets of
tensor sources around byte 2**32.  The pack itself is a fixture of each module (gpu_pack.OraclePack over these pixels)."""
import numpy as np

import ingest_cases
import resize_window as rw
from mode_cases import label_map
from qoi_amd import tiles, warp
from qoi_amd.warp import BICUBIC, NEAREST, ONE, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, WRAP

DOT, ODD, HUGE, SPRITE = range(4)
HW_, HH = rw.HUGE
FIRST_ROW = -(-(1 << 24) // HW_)       # 3641: from this row on every pixel of `huge` has an index of at least 2**24
NOISE_AT = (96, 3650, 420, 186)        # (x, y, width, height) of the planted noise ...
LABELS_AT = (1000, 3644, 1200, 192)    # ... and of the planted label map
FILL = 0x40C08020
NOISE_RECT = (100, 3652, 400, 180)


def huge_with_plantings():
    D = rw.huge_image()
    x, y, w, h = NOISE_AT
    D[y:y + h, x:x + w] = np.random.default_rng(24).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    x, y, w, h = LABELS_AT
    D[y:y + h, x:x + w] = label_map(w, h, 4, 5, 24)
    return D


def first_index(it):
    """the staged pixel index of the first - the lowest - pixel of an item's rectangle"""
    return it[2] * HW_ + it[1]


def past_2_24(items):
    """the items over `huge`: at least two, and not one pixel of their rectangles has an index below 2**24"""
    big = [it for it in items if it[0] == HUGE]
    return len(big) >= 2 and all(first_index(it) >= 1 << 24 for it in big)


def walk_shape(cus):
    """(ow, oh, across, down) of an output of more than 3 * 8 * cus tiles of 16 x 16 whose last tile column and row are partial"""
    across = 80
    down = (3 * 8 * cus) // across + 1
    return 16 * across - 3, 16 * down - 5, across, down


def window_of(it, X0, Y0, ow, oh):
    """the item whose output is the ow x oh window at (X0, Y0) of `it`'s: U = U' + 2 * X0 and V = V' + 2 * Y0 move every sub-sample's sum by
    2 * s * (a * X0 + b * Y0), a multiple of s, so the shift passes it on exactly: c' = c + 2 * (a * X0 + b * Y0), f' likewise"""
    i, x, y, cw, rh, _, _, flags, a, b, d, e, fill, _, c, f = it
    return warp.item(i, (x, y, cw, rh), (ow, oh), (a, b, c + 2 * (a * X0 + b * Y0), d, e, f + 2 * (d * X0 + e * Y0)), flags, fill)


def super_walk_table(cus):
    """(items, big's index) of tests/test_gpu_warp_super.py: test_many_tiles_per_workgroup_beyond_2_24 - [small, big, small x 5, small]: big shears
    the planted noise under SUPER2 | REFLECT into more than 3 * 8 * cus tiles, the five behind it are one-tile items of `huge` of both flags and
    the older samplings"""
    ow, oh, _, _ = walk_shape(cus)
    rect = NOISE_RECT
    a, b, d, e = round(ONE * 1.1 * rect[2] / ow), round(ONE * 0.12 * rect[2] / oh), round(-ONE * 0.1 * rect[3] / ow), round(ONE * 1.1 * rect[3] / oh)
    big = warp.item(HUGE, rect, (ow, oh), (a, b, rect[2] * ONE - a * ow - b * oh, d, e, rect[3] * ONE - d * ow - e * oh), SUPER2 | REFLECT, FILL)     # a shear about the centre
    kinds = (SUPER4 | REPLICATE, NEAREST, SUPER2, BICUBIC | WRAP, SUPER4 | REFLECT_101)
    inner = [warp.item(HUGE, (HW_ - 19 - j, HH - 17 - j, 19, 17), (11 + j, 5), warp.rotation((19, 17), (11 + j, 5), 25.0 * j, 0.4), s, FILL) for j, s in enumerate(kinds)]
    return [warp.item(DOT, (0, 0, 1, 1), (5, 4), (ONE // 3, 0, 0, 0, ONE // 3, 0), SUPER4, FILL), big] + inner + [warp.item(SPRITE, (100, 40, 30, 30), (7, 7), (4 * ONE, 0, 0, 0, 4 * ONE, 0), SUPER4)]


def super_windows(ow, oh):
    """the four 45 x 27 windows of the big entry of super_walk_table that are compared with the model: the corners of the walk"""
    return ((0, 0), (ow - 45, 3), (5, oh - 27), (ow - 45, oh - 27))


B32 = 1 << 32
MIB = 1 << 20
ARENA = B32 + 96 * MIB
LANE = 4 * MIB                  # the room of one layout's control items, and of its items beyond B32
CONTROL = 16 * MIB              # control items: [16 MiB + lane * 4 MiB, + 4 MiB), lanes 0..7; [0, 16 MiB) is the alias of a straddling item's tail
BEYOND = B32 + 48 * MIB         # items beyond: [B32 + 48 MiB + lane * 4 MiB, + 4 MiB); their aliases lie from 48 MiB on, behind the control items


def layout(sizes, elem=1, lane=0, straddle=True, spans=None):
    """Byte offsets for items of `sizes` bytes in an arena: the item with the longest span (the bytes really read or written, default: its
    size) straddles B32 - unless straddle is False -, the others are control and beyond in turn, at odd element-aligned addresses with 1 to 3
    guard bytes (in whole elements) between neighbours.  Asserts what makes a dropped high half a wrong answer and never a fault."""
    sizes = [int(s) for s in sizes]
    spans = sizes if spans is None else [int(s) for s in spans]
    n = len(sizes)
    assert 0 <= lane < 8 and sum(sizes) + 4 * elem * n + 256 <= LANE and all(0 < sp <= sz and sz % elem == 0 for sp, sz in zip(spans, sizes)), (lane, sum(sizes) + 4 * elem * n + 256)
    s = max(range(n), key=lambda j: spans[j]) if straddle else -1
    offsets = [0] * n
    pos = {False: CONTROL + lane * LANE + 64 + elem, True: BEYOND + lane * LANE + 64 + elem}
    far = False
    for j in range(n):
        if j == s:
            k = (spans[j] // elem // 2 | 1) * elem
            assert 0 < k < spans[j] and k // elem % 2 == 1, (k, k // elem % 2)
            offsets[j] = B32 - k
        else:
            offsets[j] = pos[far]
            pos[far] += sizes[j] + -(-(1 + j % 3) // elem) * elem
            far = not far
    ranges = sorted(zip(offsets, sizes))
    assert all(o % elem == 0 and 0 <= o and o + sz <= ARENA for o, sz in ranges), "all(o % elem == 0 and 0 <= o and o + sz <= ARENA for o, sz in ranges)"
    assert all(a + sz <= b for (a, sz), (b, _) in zip(ranges, ranges[1:])), "all(a + sz <= b for (a, sz), (b, _) in zip(ranges, ranges[1:]))"
    kinds = {"control" if o + sz <= B32 else "straddling" if o < B32 else "beyond" for o, sz in ranges}
    assert kinds == ({"control", "straddling", "beyond"} if straddle else {"control", "beyond"}), kinds
    for o, sz in ranges:                                           # the alias of whatever lies beyond B32: inside the arena, on no item
        if o + sz > B32:
            lo, hi = max(o, B32) - B32, o + sz - B32
            assert 0 <= lo < hi <= ARENA and all(hi <= a or a + n2 <= lo for a, n2 in ranges), (o, sz)
    return offsets


def tensor_offsets():
    """pixel_offsets of the tensor call: ingest_cases.WIDE_SPECS control, across byte B32 (the longest: f32 CHW) and beyond in turn; every
    offset is a multiple of 4, the largest element"""
    return layout([tiles.source_bytes(w, h, sch, tiles.source_flags(*fmt)) for w, h, sch, fmt in ingest_cases.WIDE_SPECS], elem=ingest_cases.WIDE_ELEM, lane=2)
