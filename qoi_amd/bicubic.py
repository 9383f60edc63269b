"""``qoimi_decode_tensors`` with ``QOIMI_FILTER_BICUBIC`` as pure functions - the normative statement of the bytes P that ``tensors.convert``
then turns into elements (what tensor_cubic of qoi_cubic.hip computes from the decoded pixels of an image), of the staging plan and of the
kernel's work items (plain numpy / integer arithmetic, no GPU).  The filter is the antialiased bicubic filter - Keys' cubic with a = -1/2,
stretched by the reduction factor when reducing -, the one PIL ``BICUBIC`` and torchvision ``Resize(BICUBIC, antialias=True)`` use.

An item is ``(image, x, y, width, height, out_width, out_height, flags)`` - the fields of ``qoimi_resize`` in their order, as for
``qoi_amd/bilinear.py``; an ``api.QoimiResize`` is taken as well.  With D the decode of stream ``image`` as ``uint8[h, w, och]``,
``R = D[y:y+height, x:x+width]``, ``cw = width``, ``rh = height``, ``ow = out_width``, ``oh = out_height``; all arithmetic is integer, every
division and every shift floors, for negative numbers too.

One axis, n_src source samples to n_out output samples, on the line of the tent filter (length ``2 * n_src * n_out``):

* source sample k has its centre at ``(2k + 1) * n_out``, output sample X at ``(2X + 1) * n_src``;
* ``u = 2 * max(n_src, n_out)`` - one source pitch when enlarging, one output pitch when reducing;
* for ``0 <= k < n_src``, ``d = |(2X + 1) * n_src - (2k + 1) * n_out|`` and

      c(X, k) = 3d^3 - 5u*d^2 + 2u^3              for d <= u        [= (d - u) * (3d^2 - 2u*d - 2u^2), positive below u]
      c(X, k) = -d^3 + 5u*d^2 - 8u^2*d + 4u^3     for u < d < 2u    [= -(d - u) * (d - 2u)^2, negative]
      c(X, k) = 0                                 from 2u on

  which is ``2u^3`` times Keys' kernel with a = -1/2 at ``d / u``; it is 0 at d = u as well;
* ``W(X) = sum_k c(X, k)``.  Samples outside the rectangle do not exist: the weights are renormalised by W(X), not clamped.  ``W(X) > 0``
  (asserted here): when enlarging, the two samples next to the output centre have c(t) + c(1 - t) >= 2u^3 and the outer two at least
  -4/27 u^3 each; at a border the nearest sample is less than u / 2 away (c >= 9/8 u^3) with one negative neighbour; when reducing, W is
  ``u / (2 * n_out)`` times a Riemann sum of the kernel over a window that holds its middle.
  tests/test_bicubic_model.py walks every pair of sizes up to 64.

Weights in 15 fractional bits that sum exactly:

* ``q(X, k) = (c(X, k) * 2**15 + W // 2) // W``;
* the deficit ``2**15 - sum_k q(X, k)`` is added to the tap with the largest c (the lowest such k on a tie): ``sum_k q(X, k) == 2**15``;
* ``-2**13 <= q <= 5 * 2**13`` and ``sum_k |q| <= 3 * 2**14`` (asserted here; the kernel keeps ``q + 2**13`` in 16 bits and a product
  ``qy * qx`` in 32): the largest q belongs to an output sample at a border when enlarging, whose nearest source sample has
  c(t) / (c(t) + c(1 + t)) <= 1.15 of the weight; the negative lobes of the whole kernel weigh 1/12, so sum |q| is about 7/6 * 2**15.

Two axes, ONE rounding: ``qx`` from (cw, ow), ``qy`` from (rh, oh), ``N_c = sum_{r,k} qy(Y, r) * qx(X, k) * R[r][k].c``.

* ``PLAIN``: every channel is ``clamp((N_c + 2**29) >> 30, 0, 255)``.
* ``ALPHA_WEIGHTED``, 4 channels only: ``A = N_a``; alpha is the PLAIN value; where ``A > 0`` r, g and b are
  ``clamp((sum qy*qx*c*a + A // 2) // A, 0, 255)``, where ``A <= 0`` they are the PLAIN value.  With 3 channels this mode is PLAIN.
* The clamp is part of the definition: the negative lobes overshoot at edges.
* The ``oh x ow`` result has its rows reversed for ``FLIP_Y`` and its columns for ``FLIP_X`` (the kernel is symmetric: this is the resampled
  mirrored rectangle), and is written tightly packed row-major.

Limits and bounds.  ``cw <= 16 * ow`` and ``rh <= 16 * oh``; ``max(cw, ow) <= 16384`` and ``max(rh, oh) <= 16384``.  The samples with a
weight have their centres in the open interval of length ``4u`` around the output centre and are ``2 * n_out`` apart: at most
``ceil(2u / n_out)`` of them - 4 when enlarging, ``ceil(4 * n_src / n_out) <= 64`` when reducing (``taps``): the tap bound of the tent
filter, and its lane split.  ``u <= 2**15`` and ``d < 2u`` where c is evaluated, so every term of c is below ``2**50``
(``5u*d^2 < 5 * 2**47``, ``8u^2*d < 2**49``, ``d^3 < 2**48``) and ``|c| <= 2u^3 <= 2**46``: ``c * 2**15 < 2**62``.  At most
``2 * ceil(u / (2 * n_out)) + 1 <= 33`` samples have a positive c, so ``W < 33 * 2**46 < 2**52``.  ``|N_c| <= 255 * (3 * 2**14)**2 < 2**40``
and the alpha-weighted sums are below ``2**48``: everything fits signed 64 bits, a position on the line (below ``2**29``) 32.

With ``out == rect`` the only sample with ``c != 0`` is k = X, so q = 2**15: the result is ``crops.crop``.  A constant rectangle gives the
constant at any size (sum q == 2**15, one rounding).  When enlarging, at most 4 x 4 samples have a weight.

Against a float64 evaluation of the same renormalised filter (``reference``), PLAIN.  Let w = c / W and q = 2**15 * w + e.  |e| <= 1/2 for
every tap but the deficit tap, e = 0 where c = 0, and the e of an output sample sum to 0: so the deficit tap has |e| <= (T - 1) / 2 with T
the taps with c != 0, and ``sum_k e_k * v_k = sum_k e_k * (v_k - v_deficit)`` is at most ``255 * (T - 1) / 2`` for values v in 0..255.  With
L = sum |w| <= 3/2 per axis, ``N_c / 2**30`` differs from the exact sum by at most

    E = 255 / 2**16 * ((Tx - 1) * Ly + (Ty - 1) * Lx) + 255 * (Tx - 1) * (Ty - 1) / 2**31     (< 0.74 with 64 taps in both axes)

and the one rounding adds 1/2; the clamp does not widen a difference.  So a byte differs from the exact real value by less than 1/2 + E,
and from the rounded reference by at most ``floor(1 + E)``: 1 for every geometry the call accepts (``bound``; the 2 that 64 taps might
suggest does not arise).  The alpha-weighted colours are a quotient of two such sums and have no such bound where A is small.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height, flags)``.

The work items of the kernel: the source columns of an output pixel are shared by ``L = 1 << lg`` neighbouring lanes, ``c`` columns each
(``split``: ``bilinear.split`` with this filter's taps; at most 4: 64 taps over 16 lanes); work item ``(Y * ow + X) * L + l`` is lane l's
share of the output pixel (X, Y) of the unflipped result (``share``); a tile is 256 work items of one item of the call.  A tile first
normalises the weights of the output columns and rows it holds, once each (``tile``), then every lane reads its weights from there.
"""
from typing import List, Tuple

import numpy as np

from . import crops, resize

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED
MAX_RATIO = 16
MAX_SIZE = 16384                # max(cw, ow) and max(rh, oh) stay at or below it
ONE = 1 << 15                   # the weights of an output sample add up to it
Q_MIN, Q_MAX = -(1 << 13), 5 << 13
L1_MAX = 3 << 14                # sum |q| of an output sample stays at or below it
THREADS = 256                   # work items of a tile
MAX_LANES_LOG2 = 4
_CHUNK = 1 << 22                # output values the model holds as 64-bit sums at a time

fields = resize.fields
as_crop = resize.as_crop


def kernel(n_src: int, n_out: int, rows=None) -> np.ndarray:
    """int64[n_out, n_src]: entry (X, k) is c(X, k); with `rows` - output samples - int64[len(rows), n_src] of those X only."""
    if n_src < 1 or n_out < 1:
        raise ValueError("kernel: both sizes >= 1")
    if max(n_src, n_out) > MAX_SIZE:
        raise ValueError("kernel: a size above 16384")
    u = 2 * max(n_src, n_out)
    X = (np.arange(n_out, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64))[:, None]
    k = np.arange(n_src, dtype=np.int64)[None, :]
    d = np.minimum(np.abs((2 * X + 1) * n_src - (2 * k + 1) * n_out), 2 * u)          # (c(2u) = 0: d^3 stays below 2**48)
    return np.where(d <= u, 3 * d ** 3 - 5 * u * d ** 2 + 2 * u ** 3, -d ** 3 + 5 * u * d ** 2 - 8 * u * u * d + 4 * u ** 3)


def weights(n_src: int, n_out: int, rows=None) -> np.ndarray:
    """int64[n_out, n_src]: entry (X, k) is q(X, k), the deficit added; every row sums to 2**15.  `rows` as for ``kernel``."""
    c = kernel(n_src, n_out, rows)
    W = c.sum(axis=1)
    if not (W > 0).all():
        raise AssertionError("weights: W(X) <= 0 for %d -> %d" % (n_src, n_out))
    q = (c * ONE + (W // 2)[:, None]) // W[:, None]
    q[np.arange(len(q)), np.argmax(c, axis=1)] += ONE - q.sum(axis=1)                  # (argmax: the lowest k of the largest c)
    if q.min() < Q_MIN or q.max() > Q_MAX or np.abs(q).sum(axis=1).max() > L1_MAX:
        raise AssertionError("weights: a weight outside its bounds for %d -> %d" % (n_src, n_out))
    return q


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
        return "reduced by more than 16"
    if max(cw, ow) > MAX_SIZE or max(rh, oh) > MAX_SIZE:
        return "a width or height above 16384"
    return ""


def _clamp(v: np.ndarray) -> np.ndarray:
    return np.minimum(np.maximum(v, 0), 255)


def bicubic(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int = 0, mode: int = PLAIN) -> np.ndarray:
    """D uint8[h, w, och] (och 3 or 4), rect (x, y, width, height) inside it, out_size (out_width, out_height) -> uint8[out_height, out_width, och]."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("bicubic: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("bicubic: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, flags)
    if wrong:
        raise ValueError("bicubic: " + wrong)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    och = D.shape[2]
    weighted = mode == ALPHA_WEIGHTED and och == 4
    R = D[y:y + rh, x:x + cw].astype(np.int64)
    if weighted:
        R = np.concatenate([R, R[:, :, :3] * R[:, :, 3:4]], axis=2)      # r, g, b, a, r*a, g*a, b*a
    qx, qy = weights(cw, ow), weights(rh, oh)
    H = np.einsum("Xk,rkc->rXc", qx, R)                                  # the rows resampled in x: below 2**24 (2**32 with alpha): exact in int64
    out = np.empty((oh, ow, och), dtype=np.uint8)
    step = max(1, _CHUNK // (ow * R.shape[2]))
    for Y0 in range(0, oh, step):                                        # (bands of output rows: the sums of a large output are not held at once)
        N = np.einsum("Yr,rXc->YXc", qy[Y0:Y0 + step], H)                # below 2**40 (2**48)
        px = _clamp((N[:, :, :och] + (1 << 29)) >> 30)
        if weighted:
            A = N[:, :, 3:4]
            px[:, :, :3] = np.where(A > 0, _clamp((N[:, :, 4:7] + A // 2) // np.maximum(A, 1)), px[:, :, :3])
        out[Y0:Y0 + step] = px
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def reference(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int]) -> np.ndarray:
    """float64[out_height, out_width, och]: the same renormalised filter evaluated in float64, PLAIN, unflipped, neither rounded nor clamped."""
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)

    def w(n_src, n_out):
        u = 2.0 * max(n_src, n_out)
        X = np.arange(n_out, dtype=np.float64)[:, None]
        k = np.arange(n_src, dtype=np.float64)[None, :]
        t = np.abs((2 * X + 1) * n_src - (2 * k + 1) * n_out) / u
        c = np.where(t <= 1, 1.5 * t ** 3 - 2.5 * t ** 2 + 1, np.where(t < 2, -0.5 * t ** 3 + 2.5 * t ** 2 - 4 * t + 2, 0.0))
        return c / c.sum(axis=1, keepdims=True)

    R = np.asarray(D)[y:y + rh, x:x + cw].astype(np.float64)
    return np.einsum("Yr,rXc->YXc", w(rh, oh), np.einsum("Xk,rkc->rXc", w(cw, ow), R))


def bound(cw: int, rh: int, ow: int, oh: int) -> int:
    """The most a PLAIN byte differs from ``round(clamp(reference))``: floor(1 + E) of the docstring with Lx = Ly = 3/2."""
    tx, ty = taps(cw, ow), taps(rh, oh)
    e_num = 255 * 3 * ((tx - 1) + (ty - 1)) * (1 << 14) + 255 * (tx - 1) * (ty - 1)   # E * 2**31
    return 1 + e_num // (1 << 31)


def size(w: int, h: int, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int, och: int) -> int:
    """Bytes of the item's u8 output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_tensor_size`` with
    ``QOIMI_FILTER_BICUBIC`` returns 0 for an accepted descriptor (an empty rectangle or output, a rectangle that leaves the image, a
    reduction by more than 16, a size above 16384, an unknown flag bit, och not 3 / 4)."""
    if och not in (3, 4) or _wrong(w, h, rect, out_size, flags):
        return 0
    return int(out_size[0]) * int(out_size[1]) * och


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height, flags): (images, slots, subs, largest); ``len(subs)`` is what
    ``qoimi_tensor_stats`` reports as [0] and [1], ``largest`` as [2], ``len(images)`` as [3]."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


# ---------------------------------------------------------------------------------- the kernel's work items
def first(X: int, n_src: int, n_out: int) -> int:
    """The first source sample that may have a weight: the smallest k >= 0 with (2k + 1) * n_out > (2X + 1) * n_src - 2u."""
    u = 2 * max(n_src, n_out)
    return max(0, ((2 * X + 1) * n_src - 2 * u - n_out) // (2 * n_out) + 1)


def taps(n_src: int, n_out: int) -> int:
    """An upper bound of the source columns (rows) with a weight for one output column (row): ceil(2u / n_out) - 4 when enlarging,
    ceil(4 * n_src / n_out) <= 64 when reducing."""
    return -(-4 * max(n_src, n_out) // n_out)


def split(cw: int, ow: int) -> Tuple[int, int]:
    """(lg, c): an output pixel's columns are shared by 1 << lg lanes (at most 16), c = ceil(taps / lanes) columns each - at most 4."""
    t, lg = taps(cw, ow), 0
    while lg < MAX_LANES_LOG2 and (t + (1 << lg) - 1) >> lg > 4:
        lg += 1
    return lg, (t + (1 << lg) - 1) >> lg


def tiles(cw: int, ow: int, oh: int) -> int:
    """Tiles of 256 work items of an item: ceil(ow * oh * lanes / 256)."""
    return -(-((ow * oh) << split(cw, ow)[0]) // THREADS)


def tile(t: int, cw: int, ow: int, oh: int) -> Tuple[List[int], List[int]]:
    """(columns, rows): the output columns and rows whose weights tile t of an item normalises, in the order of its table: every column of
    the output where a tile holds at least a row of pixels, else the column of each of its pixels; the rows its pixels lie in."""
    per = THREADS >> split(cw, ow)[0]
    o0 = t * per
    n = min(per, ow * oh - o0)
    cols = list(range(ow)) if ow <= per else [(o0 + i) % ow for i in range(n)]
    return cols, list(range(o0 // ow, (o0 + n - 1) // ow + 1))


def share(work_item: int, cw: int, rh: int, ow: int, oh: int) -> Tuple[int, int, List[Tuple[int, int]], List[Tuple[int, int]]]:
    """(X, Y, columns, rows) of a work item below ow * oh * lanes: the output pixel of the unflipped result, the (k, qx) of this lane's
    columns of R with qx != 0 and the (r, qy) of the pixel's rows with qy != 0; the lanes of a pixel together hold each of its columns once."""
    lg, c = split(cw, ow)
    o, l = work_item >> lg, work_item & ((1 << lg) - 1)
    Y, X = divmod(o, ow)
    qx, qy = weights(cw, ow, [X])[0], weights(rh, oh, [Y])[0]
    k0 = first(X, cw, ow) + l * c
    return X, Y, [(k, int(qx[k])) for k in range(k0, min(cw, k0 + c)) if qx[k] != 0], [(r, int(qy[r])) for r in range(rh) if qy[r] != 0]
