"""``qoimi_decode_tensors`` with ``FILTER_MODE`` as pure functions - the normative statement of the result (what tensor_mode of qoi_mode.hip
makes of the decoded pixels of an image), of the staging plan and of the kernel's work items (plain numpy / integer arithmetic, no GPU).
A majority vote, not an average and not a selection: for REDUCING label maps - segmentation masks, instance ids, palette indices -, where
``nearest.nearest`` looks at one pixel of each cell and thin classes come and go with the sampling phase.  The filter has no u8 call of its
own: ``tensors.U8`` with ``tensors.HWC`` gives these bytes.

An item is ``(image, x, y, width, height, out_width, out_height, flags)`` - the fields of ``qoimi_resize`` in their order, as for
``qoi_amd/nearest.py``.  With D the decode of stream ``image`` as ``uint8[h, w, 4]`` (a 3-channel decode has alpha 255),
``R = D[y:y+height, x:x+width]``, ``cw = width``, ``rh = height``, ``ow = out_width``, ``oh = out_height``; all arithmetic is integer, every
division floors.

The cell of output sample Z on an axis of ``n_src`` source and ``n_out`` output samples is ``[first(Z), first(Z + 1))`` with

    first(Z) = (2 * Z * n_src + n_out - 1) // (2 * n_out)

- on the line of length ``2 * n_src * n_out`` of ``qoi_amd/nearest.py``, where source sample k has its centre at ``(2k + 1) * n_out`` and
output sample Z covers ``[2Z * n_src, (2Z + 2) * n_src)``: the source samples whose centre lies in the output sample's extent, a centre on
the boundary of two extents belonging to the upper one.  An empty cell - only when enlarging on that axis - is replaced by the single
sample ``nearest.index``: ``((2Z + 1) * n_src) // (2 * n_out)``.  The non-empty cells of an axis partition ``[0, n_src)`` in order; with
``n_src >= n_out`` none is empty; the nearest sample lies in every non-empty cell, and a cell of one sample is the nearest sample; with
``n_src <= 16 * n_out`` a cell has at most ``ceil(n_src / n_out) <= 16`` samples.

The vote.  Output pixel (X, Y) looks at the pixels of R in columns cell(X) x rows cell(Y), at most 16 x 16 = 256 of them.  A pixel votes as
a whole - all four bytes as decoded: colour-coded masks and 24-bit instance ids survive, no colour is invented.  The count of a value is the
number of pixels equal to it; the winners are the values with the largest count.  One winner is the output.  Of several winners the output
is the pixel at (nearest.index(X), nearest.index(Y)) - what ``FILTER_NEAREST`` takes - if that pixel is a winner, else the winner with the
lowest ``key = r << 24 | g << 16 | b << 8 | a``.  (At 2 : 1 every straight class boundary makes 2-2 ties; the lowest key alone would grow
class 0 along each of them.)  och 3 then drops alpha - AFTER the vote: two colours of a 4-channel stream that differ in alpha alone vote
apart and look alike in a 3-channel output; there are no modes: ``PLAIN`` and ``ALPHA_WEIGHTED`` give the same bytes.  The
``oh x ow`` result has its rows reversed for ``FLIP_Y`` and its columns for ``FLIP_X``, and is written tightly packed row-major.

* With ``ow >= cw`` and ``oh >= rh`` every range is one sample: the result is ``nearest.nearest`` byte for byte.
* An image whose pixels are all distinct gives ``nearest.nearest`` at any size (every count is 1, the centre is a winner).
* A constant rectangle gives the constant.
* With ``cw = f * ow`` and ``rh = g * oh`` the cells are the f x g blocks.

Limits, in this order.  The rectangle rules of the other filters; then ``cw <= 16 * ow`` and ``rh <= 16 * oh`` (a cell is at most 16 x 16);
then ``max(cw, ow) <= 16384`` and ``max(rh, oh) <= 16384``: ``2 * Z * n_src + n_out < 2**30``, ``first`` is one 32-bit division.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height, flags)``.

The work items of the kernel: ``L = 2**lg`` neighbouring lanes share an output pixel, work item ``(Y * ow + X) * L + l`` is lane l of pixel
(X, Y) of the unflipped result; a tile is 256 work items of one item of the call.  ``split`` chooses lg from the largest cell the item can
have, so that a lane holds at most 4 pixels; lane l holds the pixels ``p = l, l + L, l + 2L, l + 3L`` below ``nx * ny`` of its cell, pixel p
being column ``p % nx`` and row ``p // nx`` of the cell.
"""
from typing import Tuple

import numpy as np

from . import crops, nearest, resize

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED
MAX_RATIO = 16                  # a rectangle is reduced by at most this in an axis: a cell is at most 16 x 16
MAX_SIZE = 16384                # no width or height of a rectangle or an output above it
THREADS = 256                   # work items of a tile
HOLD = 4                        # pixels a lane holds at most
MAX_LG = 6                      # 64 lanes per output pixel at most

fields = resize.fields
as_crop = resize.as_crop


def first(Z: int, n_src: int, n_out: int) -> int:
    """The first source sample whose centre is not below the lower end of output sample Z's extent; ``first(n_out) == n_src``."""
    return (2 * Z * n_src + n_out - 1) // (2 * n_out)


def cell(Z: int, n_src: int, n_out: int) -> Tuple[int, int]:
    """(lo, n): the range [lo, lo + n) of source samples that output sample Z looks at - its cell, or the nearest sample if the cell is
    empty."""
    lo, hi = first(Z, n_src, n_out), first(Z + 1, n_src, n_out)
    if hi > lo:
        return lo, hi - lo
    return ((2 * Z + 1) * n_src) // (2 * n_out), 1


def _wrong(w: int, h: int, rect, out_size, flags: int) -> str:
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    if cw < 1 or rh < 1 or ow < 1 or oh < 1:
        return "zero width or height"
    if flags & ~(FLIP_X | FLIP_Y):
        return "unknown flag bit"
    if x < 0 or y < 0 or x + cw > w or y + rh > h:
        return "the rectangle leaves its image"
    if cw > MAX_RATIO * ow or rh > MAX_RATIO * oh:
        return "reduced by more than 16 in an axis"
    if max(cw, ow, rh, oh) > MAX_SIZE:
        return "a width or height above 16384"
    return ""


def key(px) -> int:
    """r << 24 | g << 16 | b << 8 | a of a pixel of 4 bytes"""
    return int(px[0]) << 24 | int(px[1]) << 16 | int(px[2]) << 8 | int(px[3])


def vote(R4: np.ndarray, cols: Tuple[int, int], rows: Tuple[int, int], centre: Tuple[int, int]) -> np.ndarray:
    """The winner among the pixels of R4 (uint8[rh, cw, 4]) in columns [cols[0], cols[0] + cols[1]) x rows likewise; centre = (k, r) of
    the pixel that decides a tie if it is a winner."""
    block = R4[rows[0]:rows[0] + rows[1], cols[0]:cols[0] + cols[1]].reshape(-1, 4)
    values, counts = np.unique(block, axis=0, return_counts=True)      # (rows sorted lexicographically: by key)
    winners = values[counts == counts.max()]
    c = R4[centre[1], centre[0]]
    if len(winners) > 1 and (winners == c).all(axis=1).any():
        return c
    return winners[0]


def mode(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int = 0, mode: int = PLAIN, och: int = 0) -> np.ndarray:
    """D uint8[h, w, 3 or 4], rect (x, y, width, height) inside it, out_size (out_width, out_height) -> uint8[out_height, out_width, och];
    och 0 is D's own channel count.  D with 3 channels is a decode whose alpha is 255 (a 3-channel stream, or what a caller has left of one);
    a 4-channel stream decoded with och 3 is stated by its 4-channel decode as D and och = 3: its alpha votes, the output lacks it."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("mode: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("mode: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, flags)
    if wrong:
        raise ValueError("mode: " + wrong)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    if och not in (0, 3, 4):
        raise ValueError("mode: och must be 3 or 4")
    sch, och = D.shape[2], och or D.shape[2]
    R4 = np.full((rh, cw, 4), 255, dtype=np.uint8)                      # the image is decoded to 4 channels: alpha 255 takes part in the vote
    R4[:, :, :sch] = D[y:y + rh, x:x + cw]
    cols = [cell(X, cw, ow) for X in range(ow)]
    rows = [cell(Y, rh, oh) for Y in range(oh)]
    ix, iy = nearest.index(cw, ow), nearest.index(rh, oh)
    out = R4[iy[:, None], ix[None, :]].copy()                          # cells of one pixel: the nearest sample
    for Y in range(oh):
        for X in range(ow):
            if cols[X][1] * rows[Y][1] > 1:
                out[Y, X] = vote(R4, cols[X], rows[Y], (int(ix[X]), int(iy[Y])))
    out = out[:, :, :och]
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def size(w: int, h: int, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int, och: int) -> int:
    """Bytes of the item's u8 HWC output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_tensor_size`` returns 0 for an
    accepted descriptor (an empty rectangle or output, an unknown flag bit, a rectangle that leaves the image, reduced by more than 16 in an
    axis, a side above 16384, och not 3 / 4)."""
    if och not in (3, 4) or _wrong(w, h, rect, out_size, flags):
        return 0
    return int(out_size[0]) * int(out_size[1]) * och


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height, flags): (images, slots, subs, largest); ``len(subs)`` is what
    ``qoimi_tensor_stats`` reports as [0] and [1], ``largest`` as [2], ``len(images)`` as [3]."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


# ---------------------------------------------------------------------------------- the kernel's work items
def split(cw: int, rh: int, ow: int, oh: int) -> Tuple[int, int]:
    """(lg, c): L = 2**lg lanes share an output pixel and hold at most c <= 4 pixels each - the smallest lg for the largest cell of the
    item, ceil(cw / ow) x ceil(rh / oh) pixels (1 x 1 when enlarging)."""
    cells = -(-cw // ow) * -(-rh // oh)
    lg = 0
    while lg < MAX_LG and -(-cells // (1 << lg)) > HOLD:
        lg += 1
    return lg, -(-cells // (1 << lg))


def tiles(cw: int, rh: int, ow: int, oh: int) -> int:
    """Tiles of 256 work items of an item: ceil(ow * oh * L / 256)."""
    return -(-((ow * oh) << split(cw, rh, ow, oh)[0]) // THREADS)


def held(l: int, lg: int, nx: int, ny: int):
    """[(column, row) within the cell] of the pixels lane l of 2**lg holds of a cell of nx x ny pixels: p = l, l + L, ... below nx * ny"""
    return [(p % nx, p // nx) for p in range(l, nx * ny, 1 << lg)][:HOLD]
