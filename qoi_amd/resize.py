"""``qoimi_decode_resized`` as pure functions - the normative statement of the result (what qoi_resize.hip computes from the decoded pixels of an
image), of the staging plan and of the kernel's work items (plain numpy / integer arithmetic, no GPU).

An item is ``(image, x, y, width, height, out_width, out_height, flags)`` - the fields of ``qoimi_resize`` in their order; an
``api.QoimiResize`` is taken as well.  With D the decode of stream ``image`` as ``uint8[h, w, och]``, ``R = D[y:y+height, x:x+width]``,
``cw = width``, ``rh = height``, ``ow = out_width``, ``oh = out_height``; all arithmetic is integer, every division floors.

* Output column X weighs source column k of R with ``wx(X, k) = max(0, min((X+1)*cw, (k+1)*ow) - max(X*cw, k*ow))`` - the overlap of
  ``[X*cw, (X+1)*cw)`` with ``[k*ow, (k+1)*ow)``; ``sum_k wx(X, k) = cw``.  ``wy(Y, r)`` is the same with rh, oh; it sums to rh.  ``T = cw * rh``.
* ``PLAIN``: channel c of output pixel (X, Y) is ``(N_c + T // 2) // T``, ``N_c = sum_{r,k} wy(Y,r) * wx(X,k) * R[r][k].c`` - ONE rounding.
* ``ALPHA_WEIGHTED``, 4 channels only: ``A = N_a``; alpha is ``(A + T // 2) // T``; where ``A > 0`` r, g and b are
  ``(sum wy*wx*c*a + A // 2) // A``, where ``A == 0`` they are the PLAIN value.  With 3 channels this mode is PLAIN.
* The ``oh x ow`` result has its rows reversed for ``FLIP_Y`` and its columns for ``FLIP_X`` (the weights are symmetric: this is the resampled
  mirrored rectangle), and is written tightly packed row-major.

Upscaling is allowed in either axis; downscaling stops at 64 per axis: ``cw <= 64 * ow`` and ``rh <= 64 * oh``.  Then an output column
overlaps at most 65 source columns (``taps``).  ``T < 400 000 000``, ``N_c <= 255 * T < 2**37``, the alpha-weighted sums are below 2**45.

With ``out == rect`` the result is ``crops.crop``; where ``rect = f * out`` it is ``thumbs.thumbnail`` of the rectangle at f, in both modes.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height, flags)``.

The work items of the kernel: the source columns of an output pixel are shared by ``L = 1 << lg`` neighbouring lanes, ``c`` columns each
(``split``); work item ``(Y * ow + X) * L + l`` is lane l's share of the output pixel (X, Y) of the unflipped result (``share``); a tile
is 256 work items of one item of the call.
"""
from typing import List, Tuple

import numpy as np

from . import crops

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = 0
ALPHA_WEIGHTED = 1
MAX_RATIO = 64
THREADS = 256                   # work items of a tile
MAX_LANES_LOG2 = 4


def fields(it) -> Tuple[int, int, int, int, int, int, int, int]:
    """(image, x, y, width, height, out_width, out_height, flags) of an item given as such a tuple or as a ``qoimi_resize`` structure."""
    if hasattr(it, "image"):
        return (int(it.image), int(it.x), int(it.y), int(it.width), int(it.height), int(it.out_width), int(it.out_height), int(it.flags))
    image, x, y, w, h, ow, oh, flags = it
    return int(image), int(x), int(y), int(w), int(h), int(ow), int(oh), int(flags)


def as_crop(it) -> Tuple[int, int, int, int, int, int]:
    """The item's (image, x, y, width, height, flags): what the plan looks at."""
    image, x, y, w, h, _, _, flags = fields(it)
    return image, x, y, w, h, flags


def weights(n_src: int, n_out: int) -> np.ndarray:
    """int64[n_out, n_src]: entry (X, k) is the overlap of [X * n_src, (X+1) * n_src) with [k * n_out, (k+1) * n_out); rows sum to n_src."""
    if n_src < 1 or n_out < 1:
        raise ValueError("weights: both sizes >= 1")
    X = np.arange(n_out, dtype=np.int64)[:, None]
    k = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((X + 1) * n_src, (k + 1) * n_out) - np.maximum(X * n_src, k * n_out))


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
        return "reduced by more than 64"
    return ""


def resize(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int = 0, mode: int = PLAIN) -> np.ndarray:
    """D uint8[h, w, och] (och 3 or 4), rect (x, y, width, height) inside it, out_size (out_width, out_height) -> uint8[out_height, out_width, och]."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("resize: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("resize: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, flags)
    if wrong:
        raise ValueError("resize: " + wrong)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    R = D[y:y + rh, x:x + cw].astype(np.int64)
    wx, wy = weights(cw, ow), weights(rh, oh)
    T = cw * rh

    def filt(a):                                                        # sum_{r,k} wy[Y,r] * wx[X,k] * a[r,k,c]; below 2**45: exact in int64
        return np.einsum("Yr,rXc->YXc", wy, np.einsum("Xk,rkc->rXc", wx, a))

    N = filt(R)
    out = (N + T // 2) // T
    if mode == ALPHA_WEIGHTED and D.shape[2] == 4:
        A = N[:, :, 3:4]
        W = filt(R[:, :, :3] * R[:, :, 3:4])
        out[:, :, :3] = np.where(A > 0, (W + A // 2) // np.maximum(A, 1), out[:, :, :3])
    out = out.astype(np.uint8)
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def size(w: int, h: int, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int, och: int) -> int:
    """Bytes of the item's output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_resize_size`` returns 0 for an
    accepted descriptor (an empty rectangle or output, a rectangle that leaves the image, a reduction by more than 64, an unknown flag bit,
    och not 3 / 4, a size that does not fit 64 bits)."""
    if och not in (3, 4) or _wrong(w, h, rect, out_size, flags):
        return 0
    n = int(out_size[0]) * int(out_size[1]) * och
    return n if n < 2 ** 64 else 0


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height, flags): (images, slots, subs, largest); ``len(subs)`` is what
    ``qoimi_resize_stats`` reports as [0] and [1], ``largest`` as [2], ``len(images)`` as [3]."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


# ---------------------------------------------------------------------------------- the kernel's work items
def taps(n_src: int, n_out: int) -> int:
    """An upper bound of the source columns (rows) one output column (row) overlaps: n_src / n_out where that is whole, else two more than
    the floor; at most 65 under the cap."""
    return n_src // n_out + (2 if n_src % n_out else 0)


def split(cw: int, ow: int) -> Tuple[int, int]:
    """(lg, c): an output pixel's columns are shared by 1 << lg lanes (at most 16), c = ceil(taps / lanes) columns each - at most 4, 5 for 65
    taps."""
    t, lg = taps(cw, ow), 0
    while lg < MAX_LANES_LOG2 and (t + (1 << lg) - 1) >> lg > 4:
        lg += 1
    return lg, (t + (1 << lg) - 1) >> lg


def tiles(cw: int, ow: int, oh: int) -> int:
    """Tiles of 256 work items of an item: ceil(ow * oh * lanes / 256)."""
    return -(-((ow * oh) << split(cw, ow)[0]) // THREADS)


def share(work_item: int, cw: int, rh: int, ow: int, oh: int) -> Tuple[int, int, List[Tuple[int, int]], List[Tuple[int, int]]]:
    """(X, Y, columns, rows) of a work item below ow * oh * lanes: the output pixel of the unflipped result, the (k, wx) of this lane's
    columns of R with wx > 0 and the (r, wy) of the pixel's rows; the lanes of a pixel together hold each of its columns once."""
    lg, c = split(cw, ow)
    o, l = work_item >> lg, work_item & ((1 << lg) - 1)
    Y, X = divmod(o, ow)
    k0 = X * cw // ow + l * c
    cols = [(k, min((X + 1) * cw, (k + 1) * ow) - max(X * cw, k * ow)) for k in range(k0, k0 + c)]
    r0, r1 = Y * rh // oh, -(-(Y + 1) * rh // oh)
    rows = [(r, min((Y + 1) * rh, (r + 1) * oh) - max(Y * rh, r * oh)) for r in range(r0, r1)]
    return X, Y, [(k, v) for k, v in cols if v > 0], rows
