"""``qoimi_decode_tensors`` with ``QOIMI_FILTER_LANCZOS`` as pure functions - the normative statement of the bytes P that ``tensors.convert``
then turns into elements (what tensor_lanczos of qoi_lanczos.hip computes from the decoded pixels of an image), of the kernel table, of the
staging plan and of the kernel's work items (plain numpy / integer arithmetic, no GPU).  The filter is the antialiased Lanczos filter with
three lobes - ``sinc(t) * sinc(t / 3)`` for ``|t| < 3``, stretched by the reduction factor when reducing -, PIL's ``Image.LANCZOS``.

Items, R, cw, rh, ow, oh, flips, modes, channels and the plan are those of ``qoi_amd/bicubic.py``; all arithmetic is integer, every division
and every shift floors, for negative numbers too.

The kernel table (``table``): ``T[i] = round(2**30 * sinc(i / 1024) * sinc(i / 3072))`` for i = 0 .. 3072 with ``sinc(t) = sin(pi t) / (pi t)``;
``T[0] = 2**30``, ``T[3072] = 0`` (and T[1024] = T[2048] = 0).  The table is data: ``qoi_amd/csrc/qoi_lanczos_table.h`` holds the same 3073
numbers (``python -m qoi_amd.lanczos`` prints that file) and tests/test_lanczos_model.py compares the two, and both with mpmath.  ``table``
computes the numbers without libm, in ``decimal`` with 60 digits: pi by Machin's formula, the sines by their Taylor series after a reduction
of the argument to [0, pi / 2], every series cut below 1e-70.  A value is below 2**30 < 1.1e9 and comes from fewer than 400 operations of
relative error 1e-59 each on terms of at most 1.6, so it is off by less than 1e-45; ``table`` asserts that no value lies within 1e-30 of a
half: every entry is the correctly rounded one, and there is no tie to break.

One axis, n_src source samples to n_out output samples, on the line of the bicubic filter:

* source sample k has its centre at ``(2k + 1) * n_out``, output sample X at ``(2X + 1) * n_src``; ``u = 2 * max(n_src, n_out)``;
* for ``0 <= k < n_src``, ``d = |(2X + 1) * n_src - (2k + 1) * n_out|``; ``c(X, k) = 0`` for ``d >= 3u``, else with ``z = 1024 * d``,
  ``i = z // u``, ``r = z - i * u``:  ``c(X, k) = T[i] * (u - r) + T[i + 1] * r`` - u times the table interpolated linearly at ``1024 d / u``;
* ``W(X) = sum_k c(X, k)`` over the samples that exist: renormalised, not clamped;
* ``q(X, k) = (c(X, k) * 2**15 + W // 2) // W``; the deficit ``2**15 - sum_k q(X, k)`` is added to the tap with the largest c (the lowest
  such k on a tie): ``sum_k q(X, k) == 2**15``.

Two axes, ONE rounding: ``qx`` from (cw, ow), ``qy`` from (rh, oh), ``N_c = sum_{r,k} qy(Y, r) * qx(X, k) * R[r][k].c``; PLAIN, ALPHA_WEIGHTED,
the clamp and the flips are exactly those of ``bicubic.bicubic`` (the pixel is ``cubic_pixel`` of qoi_cubic_core.h).

Limits.  ``cw <= 16 * ow`` and ``rh <= 16 * oh``; ``max(cw, ow) <= 16384`` and ``max(rh, oh) <= 16384``.

What is DERIVED.  The samples with a weight have their centres in the open interval of length ``6u`` around the output centre and are
``2 * n_out`` apart: at most ``ceil(3u / n_out)`` of them - 6 when enlarging, ``ceil(6 * n_src / n_out) <= 96`` when reducing (``taps``).
``u <= 2**15``, ``d < 3u`` where c is evaluated, so ``z < 2**27`` and ``i <= 3071``; ``|T| <= 2**30`` and ``(u - r) + r = u``, so
``|c| <= 2**45`` and ``c * 2**15 <= 2**60``; ``|W| <= 96 * 2**45 < 2**52``.  With ``out == rect`` d is a multiple of u: i is a multiple of
1024 and r = 0, so c = u * T[0] for k = X and u * T[1024 or 2048] = 0 next to it - one tap, q = 2**15, the result is ``crops.crop``.  A
constant rectangle gives the constant at any size (sum q == 2**15, one rounding).  The kernel is symmetric, so a flip is the resampled
mirrored rectangle up to the deficit tap's tie.

What is only ASSERTED (``weights`` raises where one fails; tests/test_lanczos_model.py walks every pair of sizes up to 64 within the ratio and
the extremes 16:1, 16b - 1 : b, 16384 : 1024, 1000 : 16384, 1 : 16384): ``W > 0``, ``W < 2**50`` and ``W * 8 * n_out >= u * u * 2**30`` -
the sum of the kernel's samples is at least a quarter of the ``u / (2 n_out)`` a full window would give (a window cut at a border keeps about
a half); ``Q_MIN = -2**14 <= q <= 3 * 2**14 - 1 = Q_MAX`` - what the kernel's 16-bit table entries ``q + 2**14`` hold (the bias 2**13 of the
bicubic filter's table does not).  The extremes belong to a rectangle of TWO samples enlarged, at its border: the output sample half a pitch
outside sample 0 has ``q -> f(1/2) / (f(1/2) + f(3/2)) = 1.2857 * 2**15`` and ``-0.2857 * 2**15`` as the enlargement grows - measured
-9198 and 41966 for sizes up to 64 (at 2 -> 64), -9362 and 42130 at 2 -> 16384; a third sample brings them back to 1.2229 and -0.2718.
``sum_k |q| <= L1_MAX = 2**16`` (measured 51492).  ``qy * qx`` is NOT kept in 32 bits - ``Q_MAX**2 > 2**31``, and the measured 42130**2 is
below it only just and only by measurement: the kernel forms the product in 64 bits.  With these, ``|N_c| <= 255 * 2**32 < 2**40`` and the
alpha-weighted sums are below ``2**48``: signed 64 bits hold everything, a position on the line (below ``2**29``) 32.

Against a float64 evaluation of the same renormalised filter from ``np.sinc`` (``reference``), PLAIN.  Per axis let w' be the reference's
weights, w = c / W the model's before quantisation, q = 2**15 * w + e.  As for the bicubic filter ``|e| <= 1/2`` but for the deficit tap,
the e of an output sample sum to 0, and ``|sum_k e_k v_k| <= 255 * (T - 1) / 2`` over values 0..255 with T the taps.  The table adds
g = w - w': linear interpolation over steps of 1/1024 is off by at most ``(1/1024)**2 / 8 * max |f''| < 4.4e-7`` (f = sinc(t) sinc(t / 3),
|f''| <= f''(0) = pi**2 / 3 * (1 + 1/9) < 3.66) and an entry's rounding by 2**-31, delta < 4.5e-7 per tap in units of the kernel; with the
asserted ``W >= (u / 2 n_out) / 4`` in those units, ``T <= 3u / n_out + 1`` and L = sum |w| <= 2 this gives
``G = sum_k |g_k| <= T * delta * (1 + L) / W < 28 * 3 * 4.5e-7 < 3.8e-5``, and since the g of an output sample sum to 0 as well,
``|sum_k g_k v_k| <= 127.5 * G``.  With L = 2 per axis, ``N_c / 2**30`` differs from the reference's sum by at most

    E = 2 * 255 / 2**16 * ((Tx - 1) + (Ty - 1)) + 255 * (Tx - 1) * (Ty - 1) / 2**31 + 4 * 127.5 * 3.9e-5 + 127.5 * 3.9e-5 * (Tx + Ty) / 2**15

(the last term: the cross terms of g with e, with room) - below 1.50 with 96 taps in both axes, below 0.10 when enlarging in both - and the
one rounding adds 1/2; the clamp does not widen a difference.  A byte differs from the exact real value by less than 1/2 + E and from the
rounded reference by at most ``floor(1 + E)`` (``bound``): 1 while ``(Tx - 1) + (Ty - 1) <= 125``, 2 from there to the cap.  The
alpha-weighted colours are a quotient of two such sums and have no such bound where A is small.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height, flags)``.

The work items of the kernel: the source columns of an output pixel are shared by ``L = 1 << lg`` neighbouring lanes, ``c`` columns each
(``split``: at most 6 - 96 taps over 16 lanes); work item ``(Y * ow + X) * L + l`` is lane l's share of the output pixel (X, Y) of the
unflipped result (``share``); a tile is 256 work items of one item of the call and first normalises the weights of the output columns and
rows it holds, once each (``tile``: ``bicubic.tile`` with this filter's split).
"""
from decimal import Decimal, localcontext
from fractions import Fraction
from typing import List, Tuple

import numpy as np

from . import bicubic, crops, resize

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED
MAX_RATIO = 16
MAX_SIZE = 16384                # max(cw, ow) and max(rh, oh) stay at or below it
LOBES = 3
STEPS = 1024                    # table entries per unit of the kernel's argument
ENTRIES = LOBES * STEPS + 1
ONE = 1 << 15                   # the weights of an output sample add up to it
Q_MIN, Q_MAX = -(1 << 14), (3 << 14) - 1
L1_MAX = 1 << 16                # sum |q| of an output sample stays at or below it
W_MAX = 1 << 50
BIAS = 1 << 14                  # the kernel's table entries are q + BIAS in 16 bits
THREADS = 256                   # work items of a tile
MAX_LANES_LOG2 = 4
MAX_COLS = 6                    # columns per lane: 96 taps over 16 lanes
_CHUNK = 1 << 22                # output values the model holds as 64-bit sums at a time

fields = resize.fields
as_crop = resize.as_crop
_TABLE = None


def _sin_pi(t: Decimal, pi: Decimal) -> Decimal:
    """sin(pi * t) for 0 <= t <= 3: the argument reduced to [0, pi / 2], then the Taylor series"""
    t = t % 2
    sign = 1
    if t > 1:
        t, sign = t - 1, -1
    if 2 * t > 1:
        t = 1 - t
    x = pi * t
    term, total, n, x2 = x, x, 1, x * x
    while abs(term) > Decimal(10) ** -70:
        term = -term * x2 / ((n + 1) * (n + 2))
        total += term
        n += 2
    return sign * total


def _arctan_inv(n: int) -> Decimal:
    """atan(1 / n) by its series"""
    x = Decimal(1) / n
    term, total, k, x2 = x, x, 1, x * x
    while abs(term) > Decimal(10) ** -70:
        term = -term * x2
        k += 2
        total += term / k
    return total


def table() -> np.ndarray:
    """int64[3073], read-only: T[i] = round(2**30 * sinc(i / 1024) * sinc(i / 3072)), computed once (the module docstring: how, and why every
    entry is the correctly rounded one)."""
    global _TABLE
    if _TABLE is None:
        with localcontext() as ctx:
            ctx.prec = 60
            pi = 4 * (4 * _arctan_inv(5) - _arctan_inv(239))
            T = [1 << 30]
            half, room = Decimal(1) / 2, Decimal(10) ** -30
            for i in range(1, ENTRIES):
                a, b = Decimal(i) / STEPS, Decimal(i) / (LOBES * STEPS)
                v = (1 << 30) * _sin_pi(a, pi) * _sin_pi(b, pi) / (pi * pi * a * b)
                n = int((v + half).to_integral_value(rounding="ROUND_FLOOR"))
                if i % STEPS == 0:
                    n = 0                                                # sin(pi * whole) is 0 exactly; the series leaves 1e-59
                elif abs(abs(v - n) - half) < room:
                    raise AssertionError("table: entry %d within 1e-30 of a tie" % i)
                T.append(n)
        _TABLE = np.array(T, dtype=np.int64)
        _TABLE.setflags(write=False)
    return _TABLE


def header_text() -> str:
    """The text of qoi_amd/csrc/qoi_lanczos_table.h: the table as a C array (``python -m qoi_amd.lanczos`` prints it)."""
    T = table()
    rows = ["    " + ", ".join("%d" % v for v in T[i:i + 12]) + "," for i in range(0, ENTRIES, 12)]
    return ("// qoi_lanczos_table.h — GENERATED by `python -m qoi_amd.lanczos`, do not edit: T[i] = round(2^30 * sinc(i / 1024) * sinc(i / 3072)),\n"
            "// i = 0 .. 3072, the kernel of QOIMI_FILTER_LANCZOS (qoi_lanczos_core.h interpolates it; qoi_amd/lanczos.py: table computes it and says\n"
            "// why every entry is correctly rounded; tests/test_lanczos_model.py compares this file with it).  QOIMI_LANCZOS_TABLE_SPACE: where the\n"
            "// including file wants the array - qoi_lanczos.hip puts it into device memory.\n"
            "#pragma once\n#include <stdint.h>\n\n#ifndef QOIMI_LANCZOS_TABLE_SPACE\n#define QOIMI_LANCZOS_TABLE_SPACE static\n#endif\n\nnamespace qoimi {\n\n"
            "QOIMI_LANCZOS_TABLE_SPACE const int32_t kLanczosTable[%d] = {\n" % ENTRIES + "\n".join(rows) + "\n};\n\n}  // namespace qoimi\n")


def kernel(n_src: int, n_out: int, rows=None) -> np.ndarray:
    """int64[n_out, n_src]: entry (X, k) is c(X, k); with `rows` - output samples - int64[len(rows), n_src] of those X only."""
    if n_src < 1 or n_out < 1:
        raise ValueError("kernel: both sizes >= 1")
    if max(n_src, n_out) > MAX_SIZE:
        raise ValueError("kernel: a size above 16384")
    T = table()
    u = 2 * max(n_src, n_out)
    X = (np.arange(n_out, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64))[:, None]
    k = np.arange(n_src, dtype=np.int64)[None, :]
    d = np.abs((2 * X + 1) * n_src - (2 * k + 1) * n_out)
    z = STEPS * np.minimum(d, LOBES * u - 1)
    i = z // u
    r = z - i * u
    return np.where(d >= LOBES * u, 0, T[i] * (u - r) + T[i + 1] * r)


def weights(n_src: int, n_out: int, rows=None) -> np.ndarray:
    """int64[n_out, n_src]: entry (X, k) is q(X, k), the deficit added; every row sums to 2**15.  `rows` as for ``kernel``.  Raises
    AssertionError where one of the asserted bounds of the module docstring does not hold."""
    c = kernel(n_src, n_out, rows)
    W = c.sum(axis=1)
    u = 2 * max(n_src, n_out)
    if not (W > 0).all() or not (W < W_MAX).all() or not (W * (8 * n_out) >= u * u * (1 << 30)).all():
        raise AssertionError("weights: W(X) outside its bounds for %d -> %d" % (n_src, n_out))
    q = (c * ONE + (W // 2)[:, None]) // W[:, None]
    q[np.arange(len(q)), np.argmax(c, axis=1)] += ONE - q.sum(axis=1)                  # (argmax: the lowest k of the largest c)
    if q.min() < Q_MIN or q.max() > Q_MAX or np.abs(q).sum(axis=1).max() > L1_MAX:
        raise AssertionError("weights: a weight outside its bounds for %d -> %d" % (n_src, n_out))
    return q


def _wrong(w: int, h: int, rect, out_size, flags: int) -> str:
    return bicubic._wrong(w, h, rect, out_size, flags)                                 # (the same limits)


def lanczos(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int = 0, mode: int = PLAIN) -> np.ndarray:
    """D uint8[h, w, och] (och 3 or 4), rect (x, y, width, height) inside it, out_size (out_width, out_height) -> uint8[out_height, out_width, och]."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("lanczos: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("lanczos: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, flags)
    if wrong:
        raise ValueError("lanczos: " + wrong)
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
        px = bicubic._clamp((N[:, :, :och] + (1 << 29)) >> 30)
        if weighted:
            A = N[:, :, 3:4]
            px[:, :, :3] = np.where(A > 0, bicubic._clamp((N[:, :, 4:7] + A // 2) // np.maximum(A, 1)), px[:, :, :3])
        out[Y0:Y0 + step] = px
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def reference(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int]) -> np.ndarray:
    """float64[out_height, out_width, och]: the same renormalised filter evaluated in float64 from ``np.sinc``, PLAIN, unflipped, neither
    rounded nor clamped."""
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)

    def w(n_src, n_out):
        u = 2.0 * max(n_src, n_out)
        X = np.arange(n_out, dtype=np.float64)[:, None]
        k = np.arange(n_src, dtype=np.float64)[None, :]
        t = np.abs((2 * X + 1) * n_src - (2 * k + 1) * n_out) / u
        c = np.where(t < LOBES, np.sinc(t) * np.sinc(t / LOBES), 0.0)
        return c / c.sum(axis=1, keepdims=True)

    R = np.asarray(D)[y:y + rh, x:x + cw].astype(np.float64)
    return np.einsum("Yr,rXc->YXc", w(rh, oh), np.einsum("Xk,rkc->rXc", w(cw, ow), R))


def bound(cw: int, rh: int, ow: int, oh: int) -> int:
    """The most a PLAIN byte differs from ``round(clamp(reference))``: floor(1 + E) of the docstring."""
    tx, ty = taps(cw, ow), taps(rh, oh)
    G = Fraction(39, 10 ** 6)
    E = (Fraction(2 * 255, 1 << 16) * ((tx - 1) + (ty - 1)) + Fraction(255 * (tx - 1) * (ty - 1), 1 << 31) + 4 * Fraction(255, 2) * G
         + Fraction(255, 2) * G * Fraction(tx + ty, 1 << 15))
    return int(1 + E)


def size(w: int, h: int, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], flags: int, och: int) -> int:
    """Bytes of the item's u8 output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_tensor_size`` with
    ``QOIMI_FILTER_LANCZOS`` returns 0 for an accepted descriptor (an empty rectangle or output, a rectangle that leaves the image, a
    reduction by more than 16, a size above 16384, an unknown flag bit, och not 3 / 4)."""
    return bicubic.size(w, h, rect, out_size, flags, och)


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height, flags), as ``bicubic.plan``."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


# ---------------------------------------------------------------------------------- the kernel's work items
def first(X: int, n_src: int, n_out: int) -> int:
    """The first source sample that may have a weight: the smallest k >= 0 with (2k + 1) * n_out > (2X + 1) * n_src - 3u."""
    u = 2 * max(n_src, n_out)
    return max(0, ((2 * X + 1) * n_src - LOBES * u - n_out) // (2 * n_out) + 1)


def taps(n_src: int, n_out: int) -> int:
    """An upper bound of the source columns (rows) with a weight for one output column (row): ceil(3u / n_out) - 6 when enlarging,
    ceil(6 * n_src / n_out) <= 96 when reducing."""
    return -(-2 * LOBES * max(n_src, n_out) // n_out)


def split(cw: int, ow: int) -> Tuple[int, int]:
    """(lg, c): an output pixel's columns are shared by 1 << lg lanes (at most 16), c = ceil(taps / lanes) columns each - at most 6."""
    t, lg = taps(cw, ow), 0
    while lg < MAX_LANES_LOG2 and (t + (1 << lg) - 1) >> lg > MAX_COLS:
        lg += 1
    return lg, (t + (1 << lg) - 1) >> lg


def tiles(cw: int, ow: int, oh: int) -> int:
    """Tiles of 256 work items of an item: ceil(ow * oh * lanes / 256)."""
    return -(-((ow * oh) << split(cw, ow)[0]) // THREADS)


def tile(t: int, cw: int, ow: int, oh: int) -> Tuple[List[int], List[int]]:
    """(columns, rows): the output columns and rows whose weights tile t of an item normalises, in the order of its table (as ``bicubic.tile``,
    with this filter's lanes per pixel)."""
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


if __name__ == "__main__":
    print(header_text(), end="")
