"""``qoimi_decode_bilinear`` as pure functions - the normative statement of the result (what bilinear_filter of qoi_resize.hip computes from the decoded pixels of
an image), of the staging plan and of the kernel's work items (plain numpy / integer arithmetic, no GPU).

An item is ``(image, x, y, width, height, out_width, out_height, flags)`` - the fields of ``qoimi_resize`` in their order, as for
``qoi_amd/resize.py``; an ``api.QoimiResize`` is taken as well.  With D the decode of stream ``image`` as ``uint8[h, w, och]``,
``R = D[y:y+height, x:x+width]``, ``cw = width``, ``rh = height``, ``ow = out_width``, ``oh = out_height``; all arithmetic is integer, every
division floors.

One axis, n_src source samples to n_out output samples, on a line of length ``2 * n_src * n_out``:

* source sample k has its centre at ``(2k + 1) * n_out``, output sample X at ``(2X + 1) * n_src``;
* ``rad = 2 * max(n_src, n_out)`` - one source pitch when enlarging, one output pitch when reducing;
* ``t(X, k) = max(0, rad - |(2X + 1) * n_src - (2k + 1) * n_out|)`` for ``0 <= k < n_src`` - a triangle (tent) of half-width rad;
* ``W(X) = sum_k t(X, k) >= 1``.  Samples outside the rectangle do not exist: the weights are renormalised by W(X), not clamped.

``tx``, ``Wx`` come from (cw, ow), ``ty``, ``Wy`` from (rh, oh).  Two axes, ONE rounding: ``D(X, Y) = Wx(X) * Wy(Y)``,
``N_c = sum_{r,k} ty(Y, r) * tx(X, k) * R[r][k].c``.

* ``PLAIN``: every channel is ``(N_c + D // 2) // D``.
* ``ALPHA_WEIGHTED``, 4 channels only: ``A = N_a``; alpha is ``(A + D // 2) // D``; where ``A > 0`` r, g and b are
  ``(sum ty*tx*c*a + A // 2) // A``, where ``A == 0`` they are the PLAIN value.  With 3 channels this mode is PLAIN.
* The ``oh x ow`` result has its rows reversed for ``FLIP_Y`` and its columns for ``FLIP_X`` (the tent is symmetric: this is the resampled
  mirrored rectangle), and is written tightly packed row-major.

Limits and bounds.  ``cw <= 32 * ow`` and ``rh <= 32 * oh``; ``max(cw, ow) * max(rh, oh) < 2**30``.  The samples with a weight have their
centres in the open interval of length ``2 * rad`` around the output centre and are ``2 * n_out`` apart: at most ``ceil(rad / n_out)`` of
them - 2 when enlarging, ``ceil(2 * n_src / n_out) <= 64`` when reducing (``taps``).  One ``t`` is at most rad, so
``ty * tx <= 4 * max(cw, ow) * max(rh, oh) < 2**32``; ``W <= taps * rad <= 128 * max(n_src, n_out)``, so
``D <= 2**14 * max(cw, ow) * max(rh, oh) < 2**44``; ``N_c <= 255 * D < 2**52`` and the alpha-weighted sums are at most ``255 * 255 * D < 2**60``:
everything fits 64 bits, each tap and channel is one 32 x 32 -> 64 multiply-add.

With ``out == rect`` the only sample with a weight is k = X (weight rad): the result is ``crops.crop``.  A constant rectangle gives the
constant at any size.  When enlarging, at most 2 x 2 samples have a weight: the usual half-pixel-centre bilinear interpolation with
replicated borders.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height, flags)``.

The work items of the kernel: the source columns of an output pixel are shared by ``L = 1 << lg`` neighbouring lanes, ``c`` columns each
(``split``; at most 4: 64 taps over 16 lanes); work item ``(Y * ow + X) * L + l`` is lane l's share of the output pixel (X, Y) of the
unflipped result (``share``); a tile is 256 work items of one item of the call.
"""
from typing import List, Tuple

import numpy as np

from . import crops, resize

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED
MAX_RATIO = 32
MAX_AREA = 2 ** 30              # max(cw, ow) * max(rh, oh) stays below it
THREADS = 256                   # work items of a tile
MAX_LANES_LOG2 = 4
_CHUNK = 1 << 22                # output values the model holds as 64-bit sums at a time

fields = resize.fields
as_crop = resize.as_crop


def weights(n_src: int, n_out: int) -> np.ndarray:
    """int64[n_out, n_src]: entry (X, k) is t(X, k) = max(0, rad - |(2X + 1) * n_src - (2k + 1) * n_out|), rad = 2 * max(n_src, n_out)."""
    if n_src < 1 or n_out < 1:
        raise ValueError("weights: both sizes >= 1")
    X = np.arange(n_out, dtype=np.int64)[:, None]
    k = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, 2 * max(n_src, n_out) - np.abs((2 * X + 1) * n_src - (2 * k + 1) * n_out))


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
        return "reduced by more than 32"
    if max(cw, ow) * max(rh, oh) >= MAX_AREA:
        return "max(width, out_width) * max(height, out_height) from 2**30"
    return ""


def bilinear(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int = 0, mode: int = PLAIN) -> np.ndarray:
    """D uint8[h, w, och] (och 3 or 4), rect (x, y, width, height) inside it, out_size (out_width, out_height) -> uint8[out_height, out_width, och]."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("bilinear: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("bilinear: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, flags)
    if wrong:
        raise ValueError("bilinear: " + wrong)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    och = D.shape[2]
    weighted = mode == ALPHA_WEIGHTED and och == 4
    R = D[y:y + rh, x:x + cw].astype(np.int64)
    if weighted:
        R = np.concatenate([R, R[:, :, :3] * R[:, :, 3:4]], axis=2)      # r, g, b, a, r*a, g*a, b*a
    tx, ty = weights(cw, ow), weights(rh, oh)
    Wx, Wy = tx.sum(axis=1), ty.sum(axis=1)
    H = np.einsum("Xk,rkc->rXc", tx, R)                                  # the rows resampled in x: below 2**45 (2**53 with alpha): exact in int64
    out = np.empty((oh, ow, och), dtype=np.uint8)
    step = max(1, _CHUNK // (ow * R.shape[2]))
    for Y0 in range(0, oh, step):                                        # (bands of output rows: the sums of a large output are not held at once)
        N = np.einsum("Yr,rXc->YXc", ty[Y0:Y0 + step], H)                # below 2**52 (2**60)
        Dn = (Wy[Y0:Y0 + step, None] * Wx[None, :])[:, :, None]
        px = (N[:, :, :och] + Dn // 2) // Dn
        if weighted:
            A = N[:, :, 3:4]
            px[:, :, :3] = np.where(A > 0, (N[:, :, 4:7] + A // 2) // np.maximum(A, 1), px[:, :, :3])
        out[Y0:Y0 + step] = px
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def size(w: int, h: int, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int, och: int) -> int:
    """Bytes of the item's output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_bilinear_size`` returns 0 for an
    accepted descriptor (an empty rectangle or output, a rectangle that leaves the image, a reduction by more than 32, the product limit, an
    unknown flag bit, och not 3 / 4)."""
    if och not in (3, 4) or _wrong(w, h, rect, out_size, flags):
        return 0
    return int(out_size[0]) * int(out_size[1]) * och


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height, flags): (images, slots, subs, largest); ``len(subs)`` is what
    ``qoimi_bilinear_stats`` reports as [0] and [1], ``largest`` as [2], ``len(images)`` as [3]."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


# ---------------------------------------------------------------------------------- the kernel's work items
def first(X: int, n_src: int, n_out: int) -> int:
    """The first source sample with a weight: the smallest k >= 0 with (2k + 1) * n_out > (2X + 1) * n_src - rad."""
    rad = 2 * max(n_src, n_out)
    return max(0, ((2 * X + 1) * n_src - rad - n_out) // (2 * n_out) + 1)


def taps(n_src: int, n_out: int) -> int:
    """An upper bound of the source columns (rows) with a weight for one output column (row): ceil(rad / n_out) - 2 when enlarging,
    ceil(2 * n_src / n_out) <= 64 when reducing."""
    return -(-2 * max(n_src, n_out) // n_out)


def split(cw: int, ow: int) -> Tuple[int, int]:
    """(lg, c): an output pixel's columns are shared by 1 << lg lanes (at most 16), c = ceil(taps / lanes) columns each - at most 4."""
    t, lg = taps(cw, ow), 0
    while lg < MAX_LANES_LOG2 and (t + (1 << lg) - 1) >> lg > 4:
        lg += 1
    return lg, (t + (1 << lg) - 1) >> lg


def tiles(cw: int, ow: int, oh: int) -> int:
    """Tiles of 256 work items of an item: ceil(ow * oh * lanes / 256)."""
    return -(-((ow * oh) << split(cw, ow)[0]) // THREADS)


def share(work_item: int, cw: int, rh: int, ow: int, oh: int) -> Tuple[int, int, List[Tuple[int, int]], List[Tuple[int, int]]]:
    """(X, Y, columns, rows) of a work item below ow * oh * lanes: the output pixel of the unflipped result, the (k, tx) of this lane's
    columns of R with tx > 0 and the (r, ty) of the pixel's rows; the lanes of a pixel together hold each of its columns once."""
    lg, c = split(cw, ow)
    o, l = work_item >> lg, work_item & ((1 << lg) - 1)
    Y, X = divmod(o, ow)

    def t(Z, k, n_src, n_out):
        return max(0, 2 * max(n_src, n_out) - abs((2 * Z + 1) * n_src - (2 * k + 1) * n_out)) if k < n_src else 0

    k0 = first(X, cw, ow) + l * c
    cols = [(k, t(X, k, cw, ow)) for k in range(k0, k0 + c)]
    r0 = first(Y, rh, oh)
    rows = []
    while t(Y, r0 + len(rows), rh, oh) > 0:
        rows.append((r0 + len(rows), t(Y, r0 + len(rows), rh, oh)))
    return X, Y, [(k, v) for k, v in cols if v > 0], rows
