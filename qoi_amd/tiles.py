"""``qoimi_encode_tiles`` as pure functions - the normative statement of a tile's pixels (what qoi_tile.hip gathers from the caller's images
before the encoder runs), of ``qoimi_tile_size``, of ``qoimi_tile_pyramid`` and of the staging plan (plain numpy / integer arithmetic, no GPU),
composed from the models of the serving side: ``thumbs.thumbnail`` and ``crops.crop``.

A tile is ``(image, x, y, width, height, factor, flags, reserved)`` - the fields of ``qoimi_tile`` in their order; an ``api.QoimiTile`` is taken
as well.  With S the image as ``uint8[h, w, sch]``: ``R = S[y:y+height, x:x+width]``, ``T = thumbs.thumbnail(R, factor, mode)`` at sch channels
(with 3 channels ALPHA_WEIGHTED is PLAIN), T is flipped as ``crops.crop`` flips, then converted to ``och = channels`` (or sch when channels is
0): 4 to 3 drops alpha - after the reduction -, 3 to 4 sets alpha to 255.  Stream j of the call is the reference encoder's stream of T with
the descriptor ``(tw, th, och, colorspace of the image)``.

The plan: tile j's slot is ``tw * th * och`` rounded up to 256 plus the encode bound of its descriptor rounded up to 256; sub-batches are cut
by ``packplan.plan`` over those slots, in tile order.
"""
from typing import List, Sequence, Tuple

import numpy as np

from . import crops, packplan, thumbs

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = thumbs.PLAIN
ALPHA_WEIGHTED = thumbs.ALPHA_WEIGHTED
MAX_FACTOR = thumbs.MAX_FACTOR
MAX_LEVELS = 7
MAX_TILE_SIDE = 1 << 24
STAGING_DEFAULT = 1 << 30
PIXEL_CAP = 400000000


def fields(t) -> Tuple[int, int, int, int, int, int, int, int]:
    """(image, x, y, width, height, factor, flags, reserved) of a tile given as such a tuple (flags and reserved may be left out: 0) or as a
    ``qoimi_tile`` structure."""
    if hasattr(t, "image"):
        return int(t.image), int(t.x), int(t.y), int(t.width), int(t.height), int(t.factor), int(t.flags), int(t.reserved)
    t = tuple(int(v) for v in t)
    if not 6 <= len(t) <= 8:
        raise ValueError("a tile is (image, x, y, width, height, factor[, flags[, reserved]])")
    return t + (0,) * (8 - len(t))


def _wh(d) -> Tuple[int, int]:
    return (int(d.width), int(d.height)) if hasattr(d, "width") else (int(d[0]), int(d[1]))


def _desc_ok(w: int, h: int, ch: int) -> bool:
    return w > 0 and h > 0 and ch in (3, 4) and h < PIXEL_CAP // w


def size(w: int, h: int, sch: int, t, channels: int = 0) -> Tuple[int, int, int]:
    """(bytes, tw, th) of a tile of an image of w x h x sch: ``tw * th * och`` with och = channels or sch - or (0, 0, 0) where
    ``qoimi_tile_size`` returns 0: a rejected image shape, an empty rectangle, one that leaves the image, a factor outside 1..64, an unknown
    flag bit, reserved != 0, channels not 0 / 3 / 4 (``image`` is not looked at)."""
    _, x, y, cw, ch, f, flags, reserved = fields(t)
    if not _desc_ok(w, h, sch) or channels not in (0, 3, 4):
        return 0, 0, 0
    if cw < 1 or ch < 1 or x < 0 or y < 0 or x + cw > w or y + ch > h or not 1 <= f <= MAX_FACTOR or (flags & ~(FLIP_X | FLIP_Y)) or reserved:
        return 0, 0, 0
    tw, th = thumbs.size(cw, ch, f)
    return tw * th * (channels or sch), tw, th


def tile(S: np.ndarray, t, channels: int = 0, mode: int = PLAIN) -> np.ndarray:
    """S uint8[h, w, sch] (sch 3 or 4), t a tile of it -> uint8[th, tw, och]: the pixels stream j encodes."""
    S = np.asarray(S)
    if S.ndim != 3 or S.shape[2] not in (3, 4) or S.dtype != np.uint8:
        raise ValueError("tile: S must be uint8[h, w, 3 or 4]")
    _, x, y, cw, ch, f, flags, _ = fields(t)
    if size(S.shape[1], S.shape[0], S.shape[2], t, channels)[0] == 0:
        raise ValueError("tile: the tile or the channel count is one qoimi_encode_tiles rejects")
    T = thumbs.thumbnail(S[y:y + ch, x:x + cw], f, mode)
    T = crops.crop(T, (0, 0, T.shape[1], T.shape[0]), flags)
    och = channels or S.shape[2]
    if och == 3:
        T = T[:, :, :3]
    elif T.shape[2] == 3:
        T = np.concatenate([T, np.full(T.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(T)


def pyramid(w: int, h: int, tile_w: int, tile_h: int, levels: int) -> List[Tuple[int, int, int, int, int, int, int, int]]:
    """The tiles of ``qoimi_tile_pyramid`` in its order (level, row, column): level l has f = 2^l, its image of ceil(w / f) x ceil(h / f) is cut
    into tiles of tile_w x tile_h; a tile's source rectangle begins at (col * tile_w * f, row * tile_h * f) and is cut to the image."""
    if w < 1 or h < 1 or h >= PIXEL_CAP // w:
        raise ValueError("pyramid: image shape rejected")
    if not (1 <= tile_w <= MAX_TILE_SIDE and 1 <= tile_h <= MAX_TILE_SIDE):
        raise ValueError("pyramid: tile_w and tile_h must be 1..2^24")
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("pyramid: levels must be 1..7")
    out = []
    for l in range(levels):
        f = 1 << l
        lw, lh = -(-w // f), -(-h // f)
        for row in range(-(-lh // tile_h)):
            for col in range(-(-lw // tile_w)):
                x, y = col * tile_w * f, row * tile_h * f
                out.append((0, x, y, min(tile_w * f, w - x), min(tile_h * f, h - y), f, 0, 0))
    if len(out) > 2 ** 31 - 1:
        raise ValueError("pyramid: more than 2^31 - 1 tiles")
    return out


def pyramid_index(w: int, h: int, tile_w: int, tile_h: int, levels: int) -> List[Tuple[int, int, int]]:
    """(level, row, col) of every tile of ``pyramid``, in its order."""
    return [(f.bit_length() - 1, y // (tile_h * f), x // (tile_w * f)) for (_, x, y, _, _, f, _, _) in pyramid(w, h, tile_w, tile_h, levels)]


def encode_bound(tw: int, th: int, och: int) -> int:
    """``qoimi_encode_bound`` of an accepted descriptor."""
    return tw * th * (och + 1) + 22


def plan(descs: Sequence, tiles: Sequence, channels: int, staging_bytes: int):
    """(slots, subs, largest, referenced): every tile's staging slot, (first, count) of every sub-batch as indices into ``tiles``
    (``packplan.plan`` over the slots; staging_bytes 0: 1 GiB), the bytes of the largest sub-batch - what ``qoimi_tile_stats`` reports as [2];
    ``len(subs)`` is [0] and [1] - and the number of images the tiles name: [3].  descs: ``QoiDesc`` or (w, h, channels) per image."""
    slots, named = [], set()
    for t in tiles:
        image = fields(t)[0]
        d = descs[image]
        w, h = _wh(d)
        sch = int(d.channels) if hasattr(d, "channels") else int(d[2])
        nbytes, tw, th = size(w, h, sch, t, channels)
        if nbytes == 0:
            raise ValueError("plan: a tile is one qoimi_encode_tiles rejects")
        slots.append(packplan.slot(nbytes) + packplan.slot(encode_bound(tw, th, channels or sch)))
        named.add(image)
    subs = packplan.plan(slots, staging_bytes if staging_bytes else STAGING_DEFAULT)      # (a slot is a multiple of 256 already)
    largest = max((sum(slots[first:first + count]) for first, count in subs), default=0)
    return slots, subs, largest, len(named)
