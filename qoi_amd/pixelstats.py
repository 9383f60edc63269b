"""``qoimi_pixel_stats`` as pure functions - the normative statement of the result (what qoi_stats.hip reduces from the decoded pixels of an
image), of the staging plan and of the kernel's tiles (plain numpy / integer arithmetic, no GPU).

A region is ``(image, x, y, width, height, flags)`` - the fields of ``qoimi_crop`` in their order; a ``api.QoimiCrop`` is taken as well.  With D
the decode of stream ``image`` at 4 channels as ``uint8[h, w, 4]`` (a 3-channel stream has alpha 255 everywhere), R is
``D[y:y+height, x:x+width]`` and the result holds, over the pixels of R: their number, per channel r, g, b, a the sum, the sum of squares, the
minimum and the maximum, how many pixels have a == 255, a == 0 and r == g == b, ``first`` and the flags.  The two flip bits of ``crops`` change
nothing but ``first``: pixel (0, 0) of the flipped rectangle - the first pixel ``qoimi_decode_crops`` would write - as r | g << 8 | b << 16 |
a << 24.  The flags are a function of the other fields (``flags_of``).  All arithmetic is integer.

The plan is that of ``qoimi_decode_crops`` over the regions (``crops.plan``).  A tile of the kernel is ``TILE_PX`` consecutive pixels of one
region in the rectangle's row-major order.
"""
from typing import Dict, Tuple

import numpy as np

from . import crops

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
CONSTANT = 1          # QOIMI_PS_CONSTANT: every pixel equals `first`: min[c] == max[c] for c = 0..3
OPAQUE = 2            # QOIMI_PS_OPAQUE: opaque_pixels == pixels
TRANSPARENT = 4       # QOIMI_PS_TRANSPARENT: transparent_pixels == pixels
GREY = 8              # QOIMI_PS_GREY: grey_pixels == pixels
FLAG_NAMES = ((CONSTANT, "constant"), (OPAQUE, "opaque"), (TRANSPARENT, "transparent"), (GREY, "grey"))
TILE_PX = 1024        # qoi_stats_core.h: kStatsTilePx
FIELDS = ("pixels", "sum", "sum_sq", "min", "max", "first", "flags", "opaque_pixels", "transparent_pixels", "grey_pixels")


def _region(D: np.ndarray, rect: Tuple[int, int, int, int]) -> np.ndarray:
    D = np.asarray(D)
    x, y, w, h = (int(v) for v in rect)
    if D.ndim != 3 or D.shape[2] != 4 or D.dtype != np.uint8:
        raise ValueError("pixelstats: D is uint8[h, w, 4]")
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > D.shape[1] or y + h > D.shape[0]:
        raise ValueError("pixelstats: the rectangle is empty or leaves the image")
    return D[y:y + h, x:x + w]


def flags_of(f: Dict) -> int:
    """The ``QOIMI_PS_*`` bits of a result, from its other fields."""
    n = int(f["pixels"])
    return ((CONSTANT if all(int(a) == int(b) for a, b in zip(f["min"], f["max"])) else 0) | (OPAQUE if int(f["opaque_pixels"]) == n else 0) |
            (TRANSPARENT if int(f["transparent_pixels"]) == n else 0) | (GREY if int(f["grey_pixels"]) == n else 0))


def flag_names(flags: int) -> str:
    return "|".join(name for bit, name in FLAG_NAMES if flags & bit) or "-"


def stats(D: np.ndarray, region) -> Dict:
    """D uint8[h, w, 4] and a region (x, y, width, height[, flags]) inside it (or a 6-tuple / ``QoimiCrop`` with the image in front, which is
    not looked at) -> the fields of ``qoimi_pixel_stat`` as a dict: ints, and 4-tuples of ints for sum, sum_sq, min and max."""
    if hasattr(region, "image") or len(region) == 6:
        _, x, y, w, h, flags = crops.fields(region)
    else:
        x, y, w, h = (int(v) for v in region[:4])
        flags = int(region[4]) if len(region) > 4 else 0
    if flags & ~(FLIP_X | FLIP_Y):
        raise ValueError("pixelstats: unknown flag bit")
    R = _region(D, (x, y, w, h)).reshape(-1, 4).astype(np.int64)
    head = np.asarray(D)[y + h - 1 if flags & FLIP_Y else y, x + w - 1 if flags & FLIP_X else x]
    f = {
        "pixels": w * h,
        "sum": tuple(int(v) for v in R.sum(axis=0)),
        "sum_sq": tuple(int(v) for v in (R * R).sum(axis=0)),
        "min": tuple(int(v) for v in R.min(axis=0)),
        "max": tuple(int(v) for v in R.max(axis=0)),
        "first": int(head[0]) | int(head[1]) << 8 | int(head[2]) << 16 | int(head[3]) << 24,
        "opaque_pixels": int((R[:, 3] == 255).sum()),
        "transparent_pixels": int((R[:, 3] == 0).sum()),
        "grey_pixels": int(((R[:, 0] == R[:, 1]) & (R[:, 1] == R[:, 2])).sum()),
    }
    f["flags"] = flags_of(f)
    return f


def hist(D: np.ndarray, region) -> np.ndarray:
    """uint32[4, 256]: how many pixels of the region have channel c equal to v (what ``d_hist[j]`` holds)."""
    if hasattr(region, "image") or len(region) == 6:
        _, x, y, w, h, _ = crops.fields(region)
    else:
        x, y, w, h = (int(v) for v in region[:4])
    R = _region(D, (x, y, w, h)).reshape(-1, 4)
    return np.stack([np.bincount(R[:, c], minlength=256) for c in range(4)]).astype(np.uint32)


def of_struct(s) -> Dict:
    """The fields of a ``api.QoimiPixelStat`` in the form ``stats`` returns."""
    return {"pixels": int(s.pixels), "sum": tuple(int(v) for v in s.sum), "sum_sq": tuple(int(v) for v in s.sum_sq), "min": tuple(int(v) for v in s.min),
            "max": tuple(int(v) for v in s.max), "first": int(s.first), "flags": int(s.flags), "opaque_pixels": int(s.opaque_pixels),
            "transparent_pixels": int(s.transparent_pixels), "grey_pixels": int(s.grey_pixels)}


def mean_std(f: Dict) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """Per-channel mean and (population) standard deviation from pixels, sum and sum_sq."""
    n = int(f["pixels"])
    mean = tuple(s / n for s in f["sum"])
    std = tuple(max(q / n - m * m, 0.0) ** 0.5 for q, m in zip(f["sum_sq"], mean))
    return mean, std


def tiles(width: int, height: int) -> int:
    """Tiles of a region of width x height pixels."""
    return -(-(int(width) * int(height)) // TILE_PX)


def plan(descs, regions, staging_bytes: int):
    """``crops.plan`` over the regions: what ``qoimi_pixel_stats_counters`` reports - ``len(subs)`` is [0] and [1], ``largest`` [2], ``len(images)``
    [3]."""
    return crops.plan(descs, regions, staging_bytes)
