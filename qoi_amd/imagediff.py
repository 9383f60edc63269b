"""The pixel comparison of ``qoimi_compare_images`` / ``qoimi_verify_images`` as a pure function - the normative statement of what
qoi_compare.hip: cmp_pixels and cmp_first compute, so a caller (and the tests) can tell what a result must be."""
from typing import Tuple

import numpy as np

DIFF_PIXELS = 1          # QOIMI_DIFF_PIXELS: mismatched != 0
DIFF_HEADER = 2          # QOIMI_DIFF_HEADER: qoimi_verify_images did not decode the stream
NONE = 0xFFFFFFFFFFFFFFFF

# qoimi_image_diff: 32 bytes, offsets 0/8/16/20/24/28
DIFF_DTYPE = np.dtype([("mismatched", "<u8"), ("first", "<u8"), ("want", "<u4"), ("got", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])


def pixel_word(buf, index: int, channels: int) -> int:
    """Pixel `index` of a tightly packed buffer as r | g << 8 | b << 16 | a << 24; a channel the buffer does not hold reads 0xFF."""
    p = np.asarray(buf, dtype=np.uint8).reshape(-1)[index * channels:(index + 1) * channels]
    a = int(p[3]) if channels == 4 else 0xFF
    return int(p[0]) | int(p[1]) << 8 | int(p[2]) << 16 | a << 24


def diff(a, b, n_pixels: int, ca: int, cb: int) -> Tuple[int, int, int, int]:
    """(mismatched, first, want, got) of two tightly packed images of n_pixels pixels, ca bytes per pixel in `a` and cb in `b`
    (3 or 4 each).  Two pixels are equal when their first min(ca, cb) bytes are.  first is the lowest differing index (NONE if the
    images are equal), want / got are pixel `first` of a / b as ``pixel_word`` gives them (0 if the images are equal)."""
    assert ca in (3, 4) and cb in (3, 4) and n_pixels >= 0
    pa = np.asarray(a, dtype=np.uint8).reshape(-1)[:n_pixels * ca].reshape(n_pixels, ca)
    pb = np.asarray(b, dtype=np.uint8).reshape(-1)[:n_pixels * cb].reshape(n_pixels, cb)
    k = min(ca, cb)
    differ = np.flatnonzero((pa[:, :k] != pb[:, :k]).any(axis=1))
    if differ.size == 0:
        return 0, NONE, 0, 0
    first = int(differ[0])
    return int(differ.size), first, pixel_word(pa, first, ca), pixel_word(pb, first, cb)
