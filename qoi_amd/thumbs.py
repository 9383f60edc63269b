"""The box reduction of ``qoimi_decode_thumbnails`` as a pure function - the normative statement of what qoi_thumb.hip computes from the
decoded pixels of an image (plain numpy integer arithmetic, no GPU).

Output pixel (X, Y) of the ``tw x th`` thumbnail, ``tw = ceil(w / f)``, ``th = ceil(h / f)``, covers the source block
``x in [X*f, min(w, X*f+f))``, ``y in [Y*f, min(h, Y*f+f))`` of ``cnt`` pixels; ``S_c`` is the sum of channel c over the block.  All
divisions are integer divisions (floor), so a half rounds up.

* ``PLAIN``: every channel is ``(S_c + cnt // 2) // cnt``.
* ``ALPHA_WEIGHTED``, 4 channels only: ``A = S_a``; alpha is ``(A + cnt // 2) // cnt``; where ``A > 0`` r, g and b are
  ``(sum(c_k * a_k) + A // 2) // A``, where ``A == 0`` they are the PLAIN value.  With 3 channels this mode is PLAIN.

``f == 1`` is the identity in both modes.  Every sum fits in 32 bits: ``64 * 64 * 255 * 255 < 2**32``.
"""
from typing import Tuple

import numpy as np

PLAIN = 0
ALPHA_WEIGHTED = 1
MAX_FACTOR = 64


def size(w: int, h: int, f: int) -> Tuple[int, int]:
    """(tw, th) = (ceil(w / f), ceil(h / f))."""
    if not 1 <= f <= MAX_FACTOR:
        raise ValueError("factor outside 1..64")
    return (w + f - 1) // f, (h + f - 1) // f


def _block_sums(a: np.ndarray, f: int) -> np.ndarray:
    """Sums of a[h, w, ch] (int64) over f x f blocks; blocks at the right / lower edge hold what the image has."""
    h, w, _ = a.shape
    return np.add.reduceat(np.add.reduceat(a, np.arange(0, h, f), axis=0), np.arange(0, w, f), axis=1)


def thumbnail(px: np.ndarray, f: int, mode: int = PLAIN) -> np.ndarray:
    """px uint8[h, w, ch] (ch 3 or 4) -> uint8[th, tw, ch]."""
    px = np.asarray(px)
    if px.ndim != 3 or px.shape[2] not in (3, 4) or px.dtype != np.uint8:
        raise ValueError("thumbnail: px must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("thumbnail: mode must be PLAIN or ALPHA_WEIGHTED")
    h, w, ch = px.shape
    tw, th = size(w, h, f)
    a = px.astype(np.int64)
    xs = np.minimum(w, (np.arange(tw) + 1) * f) - np.arange(tw) * f
    ys = np.minimum(h, (np.arange(th) + 1) * f) - np.arange(th) * f
    cnt = (ys[:, None] * xs[None, :])[:, :, None]                       # pixels per block
    S = _block_sums(a, f)
    out = (S + cnt // 2) // cnt
    if mode == ALPHA_WEIGHTED and ch == 4:
        A = S[:, :, 3:4]
        W = _block_sums(a[:, :, :3] * a[:, :, 3:4], f)
        safe = np.maximum(A, 1)
        out[:, :, :3] = np.where(A > 0, (W + A // 2) // safe, out[:, :, :3])
    return out.astype(np.uint8)


def factor_for(w: int, h: int, max_side: int) -> int:
    """The smallest f in 1..64 with ceil(max(w, h) / f) <= max_side, else 64."""
    if max_side < 1:
        raise ValueError("max_side must be at least 1")
    side = max(w, h)
    for f in range(1, MAX_FACTOR + 1):
        if (side + f - 1) // f <= max_side:
            return f
    return MAX_FACTOR
