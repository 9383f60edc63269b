"""``qoimi_decode_tensors`` with ``FILTER_NEAREST`` as pure functions - the normative statement of the result (what tensor_nearest of
qoi_nearest.hip takes from the decoded pixels of an image), of the staging plan and of the kernel's work items (plain numpy / integer
arithmetic, no GPU).  Selection, not averaging: for label maps - segmentation masks, instance ids, palette indices - whose values must not
be mixed.  The filter has no u8 call of its own: ``tensors.U8`` with ``tensors.HWC`` gives these bytes.

An item is ``(image, x, y, width, height, out_width, out_height, flags)`` - the fields of ``qoimi_resize`` in their order, as for
``qoi_amd/resize.py``.  With D the decode of stream ``image`` as ``uint8[h, w, och]`` (a 3-channel decode has alpha 255; och 3 drops alpha),
``R = D[y:y+height, x:x+width]``, ``cw = width``, ``rh = height``, ``ow = out_width``, ``oh = out_height``; all arithmetic is integer, every
division floors.

Output pixel (X, Y) is ``R[r][k]`` byte for byte, with

    k = ((2X + 1) * cw) // (2 * ow),    r = ((2Y + 1) * rh) // (2 * oh)

- on the line of length ``2 * n_src * n_out`` the tent filter uses (``qoi_amd/bilinear.py``), where output sample X has its centre at
``(2X + 1) * n_src`` and source sample k covers ``[2k * n_out, (2k + 2) * n_out)``: the source pixel whose cell holds the output pixel's
centre; a centre on the boundary of two cells belongs to the upper one.  ``(2X + 1) * cw <= (2 * ow - 1) * cw < 2 * ow * cw``, so
``k < cw`` always holds: nothing outside R is read.  There are no modes: ``PLAIN`` and ``ALPHA_WEIGHTED`` give the same bytes.  The
``oh x ow`` result has its rows reversed for ``FLIP_Y`` and its columns for ``FLIP_X``, and is written tightly packed row-major.

* With ``out == rect`` k = X and r = Y: the result is ``crops.crop``.
* With ``cw = f * ow`` it takes column ``X * f + f // 2``.
* It equals ``warp.warp`` with ``warp.NEAREST`` and the map ``a = 65536 * cw / ow``, ``e = 65536 * rh / oh``, everything else 0, wherever both
  quotients are whole: there ``Px >> 17 = (a * (2X + 1)) >> 17 = ((2X + 1) * cw) // (2 * ow)``.
* ``torch.nn.functional.interpolate(mode="nearest-exact")`` computes ``floor((X + 0.5) * (n_src / n_out))`` in float: it agrees wherever
  ``(2X + 1) * n_src`` is no multiple of ``2 * n_out`` and is one lower at some of those boundaries, where the integer definition is the
  exact one.

Limits.  The rectangle rules of the other filters; then ``max(cw, ow) <= 16384`` and ``max(rh, oh) <= 16384`` (the bicubic filter's size
limit): ``(2X + 1) * cw < 2**29``, the kernel needs no 64-bit division.  There is no ratio limit: every output pixel is one load.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height, flags)``.

The work items of the kernel: work item ``Y * ow + X`` is output pixel (X, Y) of the unflipped result - one lane per pixel, no lane split; a
tile is 256 work items of one item of the call.
"""
from typing import Tuple

import numpy as np

from . import crops, resize

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED
MAX_SIZE = 16384                # no width or height of a rectangle or an output above it
THREADS = 256                   # work items of a tile

fields = resize.fields
as_crop = resize.as_crop


def index(n_src: int, n_out: int) -> np.ndarray:
    """int64[n_out]: entry X is the source sample of output sample X, ((2X + 1) * n_src) // (2 * n_out); every entry is below n_src."""
    if n_src < 1 or n_out < 1:
        raise ValueError("index: both sizes >= 1")
    X = np.arange(n_out, dtype=np.int64)
    return ((2 * X + 1) * n_src) // (2 * n_out)


def _wrong(w: int, h: int, rect, out_size, flags: int) -> str:
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    if cw < 1 or rh < 1 or ow < 1 or oh < 1:
        return "zero width or height"
    if flags & ~(FLIP_X | FLIP_Y):
        return "unknown flag bit"
    if x < 0 or y < 0 or x + cw > w or y + rh > h:
        return "the rectangle leaves its image"
    if max(cw, ow, rh, oh) > MAX_SIZE:
        return "a width or height above 16384"
    return ""


def nearest(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int = 0, mode: int = PLAIN) -> np.ndarray:
    """D uint8[h, w, och] (och 3 or 4), rect (x, y, width, height) inside it, out_size (out_width, out_height) -> uint8[out_height, out_width, och]."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("nearest: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("nearest: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, flags)
    if wrong:
        raise ValueError("nearest: " + wrong)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    out = D[y:y + rh, x:x + cw][index(rh, oh)[:, None], index(cw, ow)[None, :]]
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def size(w: int, h: int, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int, och: int) -> int:
    """Bytes of the item's u8 HWC output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_tensor_size`` returns 0 for an
    accepted descriptor (an empty rectangle or output, an unknown flag bit, a rectangle that leaves the image, a side above 16384, och not
    3 / 4)."""
    if och not in (3, 4) or _wrong(w, h, rect, out_size, flags):
        return 0
    return int(out_size[0]) * int(out_size[1]) * och


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height, flags): (images, slots, subs, largest); ``len(subs)`` is what
    ``qoimi_tensor_stats`` reports as [0] and [1], ``largest`` as [2], ``len(images)`` as [3]."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


# ---------------------------------------------------------------------------------- the kernel's work items
def tiles(ow: int, oh: int) -> int:
    """Tiles of 256 work items of an item: ceil(ow * oh / 256)."""
    return -(-(ow * oh) // THREADS)


def place(work_item: int, cw: int, rh: int, ow: int, oh: int) -> Tuple[int, int, int, int]:
    """(X, Y, k, r) of a work item below ow * oh: the output pixel of the unflipped result and the pixel of R it takes."""
    Y, X = divmod(work_item, ow)
    return X, Y, ((2 * X + 1) * cw) // (2 * ow), ((2 * Y + 1) * rh) // (2 * oh)
