"""``qoimi_decode_crops`` as pure functions - the normative statement of the result (what qoi_crop.hip gathers from the decoded pixels of an
image), of the staging plan and of the kernel's work items (plain numpy / integer arithmetic, no GPU).

A crop is ``(image, x, y, width, height, flags)`` - the fields of ``qoimi_crop`` in their order; a ``api.QoimiCrop`` is taken as well.  With D the
decode of stream ``image`` as ``uint8[h, w, och]``, output j is ``D[y:y+height, x:x+width]``, its rows reversed for ``FLIP_Y`` and its columns
for ``FLIP_X``, written tightly packed row-major.

The plan: the referenced images in ascending index order; ``rows_i`` is the maximum of ``y + height`` over the crops of image i - the decoder
stops behind that row; a slot is ``w_i * rows_i * 4`` rounded up to 256; sub-batches are cut by ``packplan.plan`` over those slots.

The items: the output of a crop is ``B = width * height * och`` bytes at the absolute address q.  An item is one aligned 16-byte word that
``[q, q + B)`` touches; item k covers the output bytes ``[16 * ((q >> 4) + k) - q, + 16)`` cut to ``[0, B)``.
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import packplan

FLIP_X = 1
FLIP_Y = 2
STAGING_DEFAULT = 1 << 30


def fields(c) -> Tuple[int, int, int, int, int, int]:
    """(image, x, y, width, height, flags) of a crop given as such a tuple or as a ``qoimi_crop`` structure."""
    if hasattr(c, "image"):
        return int(c.image), int(c.x), int(c.y), int(c.width), int(c.height), int(c.flags)
    image, x, y, w, h, flags = c
    return int(image), int(x), int(y), int(w), int(h), int(flags)


def _wh(d) -> Tuple[int, int]:
    return (int(d.width), int(d.height)) if hasattr(d, "width") else (int(d[0]), int(d[1]))


def crop(D: np.ndarray, rect: Tuple[int, int, int, int], flags: int = 0) -> np.ndarray:
    """D uint8[h, w, och], rect (x, y, width, height) inside it -> uint8[height, width, och]."""
    D = np.asarray(D)
    x, y, w, h = (int(v) for v in rect)
    if D.ndim != 3 or w < 1 or h < 1 or x < 0 or y < 0 or x + w > D.shape[1] or y + h > D.shape[0]:
        raise ValueError("crop: the rectangle is empty or leaves the image")
    if flags & ~(FLIP_X | FLIP_Y):
        raise ValueError("crop: unknown flag bit")
    out = D[y:y + h, x:x + w]
    if flags & FLIP_Y:
        out = out[::-1]
    if flags & FLIP_X:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def size(w: int, h: int, rect: Tuple[int, int, int, int], flags: int, och: int) -> int:
    """Bytes of the crop's output for an image of w x h: width * height * och, or 0 where ``qoimi_crop_size`` returns 0 for an accepted
    descriptor (an empty rectangle, one that leaves the image, an unknown flag bit, och not 3 / 4)."""
    x, y, cw, ch = (int(v) for v in rect)
    if cw < 1 or ch < 1 or x < 0 or y < 0 or x + cw > w or y + ch > h or (flags & ~(FLIP_X | FLIP_Y)) or och not in (3, 4):
        return 0
    return cw * ch * och


def rows_needed(descs: Sequence, crops: Sequence) -> Dict[int, int]:
    """{image: rows} for every image a crop names, ascending: the rows of the image that are decoded - the largest y + height of its crops."""
    rows: Dict[int, int] = {}
    for c in crops:
        image, _, y, _, h, _ = fields(c)
        if not 0 <= image < len(descs):
            raise ValueError("rows_needed: a crop names no image of the call")
        if h < 1 or y + h > _wh(descs[image])[1]:
            raise ValueError("rows_needed: a rectangle is empty or leaves its image")
        rows[image] = max(rows.get(image, 0), y + h)
    return dict(sorted(rows.items()))


def plan(descs: Sequence, crops: Sequence, staging_bytes: int):
    """(images, slots, subs, largest): the referenced images in ascending order, their staging slots, (first, count) of every sub-batch as
    indices into ``images`` (``packplan.plan`` over the slots; staging_bytes 0: 1 GiB) and the bytes of the largest sub-batch - what
    ``qoimi_crop_stats`` reports as [2]; ``len(subs)`` is [0] and [1], ``len(images)`` is [3]."""
    rows = rows_needed(descs, crops)
    images = list(rows)
    raw = [_wh(descs[i])[0] * rows[i] * 4 for i in images]
    slots = [packplan.slot(b) for b in raw]
    subs = packplan.plan(raw, staging_bytes if staging_bytes else STAGING_DEFAULT)
    largest = max((sum(slots[first:first + count]) for first, count in subs), default=0)
    return images, slots, subs, largest


def items(q: int, B: int) -> List[Tuple[int, int]]:
    """The byte ranges [b0, b1) of the output that the items of a crop of B >= 1 bytes at the address q cover, in item order."""
    if B < 1 or q < 0:
        raise ValueError("items: B >= 1, q >= 0")
    n = ((q + B + 15) >> 4) - (q >> 4)
    out = []
    for k in range(n):
        lo = 16 * ((q >> 4) + k) - q
        out.append((max(lo, 0), min(lo + 16, B)))
    return out
