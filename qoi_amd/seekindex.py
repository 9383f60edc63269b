"""The row seek index as pure functions - the normative statement of ``qoimi_build_seek_index``, ``qoimi_seek_index_from_pixels``,
``qoimi_band_plan``, ``qoimi_make_band_streams`` and of the bands ``qoimi_decode_crops_indexed``, ``qoimi_decode_resized_indexed`` and
``qoimi_pixel_stats_indexed`` decode (plain numpy / integer arithmetic, no GPU).

A QOI decoder's whole state at a row boundary is small: the previous pixel, the 64-entry colour table, a byte position and what is left of
a run.  A SEEK POINT writes it down; a BAND STREAM spells it as QOI chunks in front of the original stream's bytes from there on, so that
any decoder, as it is, decodes the rows of a band without the rows above it.

Seek points.  For an image of w x h, a stream of ``size`` bytes, its 4-channel decode D and an interval of K rows with ``K * w >= 128`` the
points are at the rows K, 2K, ... < h: ``ceil(h / K) - 1`` of them.  Point k (0-based) sits at pixel ``P = (k + 1) * K * w`` and holds

* ``byte_off``, ``skip``: the byte-bounded chunk walk of ``streaminfo.inspect_stream`` - p = 14, end = size - 8, px = 0; while p < end: n =
  pixels of the chunk at p; if px + n > P stop, else px += n, p += the chunk's length.  Stopped inside the body: byte_off = p, skip = P - px
  (0..61, non-zero only inside a QOI_OP_RUN).  The walk ran out: byte_off = size - 8, skip = 0.
* ``prev``: pixel P - 1 of D as ``r | g << 8 | b << 16 | a << 24``.
* ``table[s]``: the last pixel of D before P whose hash ``(3r + 5g + 7b + 11a) % 64`` is s, else 0.

Why the pixel-defined table is the decoder's wherever a later chunk can read it: the reference decoder stores the current pixel into its
slot behind EVERY chunk, QOI_OP_RUN included (qoi.h:577), and nowhere else.  A pixel of D that no chunk of its own produced - the further
pixels of a run, the pixels behind the last chunk of a short stream - repeats the pixel of the chunk in front of it, which that chunk
stored: walking the pixels stores the same values into the same slots in the same order of last writes.  The single difference is a
stream without any chunk: D is the start pixel (0, 0, 0, 255) throughout and the model's table holds it in slot 53 where the decoder's
holds 0 - harmless, since without a chunk nothing reads the table (and a band stream loads ``prev`` in any case).

Band stream.  A band ``(first_row, rows)`` has ``first_row`` 0 or a seek row and ``first_row + rows <= h``; e is the point at first_row, e2
the first point at a row >= first_row + rows, if there is one.  The band stream is, concatenated:

* the header: ``qoif``, w, ``pad_rows + rows``, the original channels and colorspace;
* the loads: for s ascending every ``table[s]`` that is neither 0 nor ``prev`` as a chunk ``FF r g b a``, then ``prev`` the same way: n
  chunks, n <= 64, each of which also stores its pixel into its slot;
* ``pad_rows = max(1, ceil((n + skip) / w))``, and the pad run: with ``R = pad_rows * w - skip - n``, ``R // 62`` bytes ``0xFD`` and, if
  ``R % 62 != 0``, one byte ``0xC0 | (R % 62 - 1)`` - repetitions of ``prev``;
* the tail: the original bytes ``[byte_off, min(byte_off(e2) + 13, size))``, up to ``size`` without e2 (a chunk of at most 5 bytes at
  e2's position and 8 bytes that stand where a decoder expects the end marker).  With ``byte_off == size - 8`` this is exactly the stream's
  last 8 bytes.

With ``first_row == 0`` there are no loads, ``pad_rows = 0`` and the tail starts at byte 14.  Decoded by any decoder at 3 or 4 channels, the
rows ``pad_rows`` onward of a band stream are the rows ``first_row`` onward of the full decode.

An index handed to a call is the caller's data.  ``n <= 64`` holds for every point of a stream (``table[hash(prev)] == prev``, P >= 1); 64 table
words that are all non-zero and differ from ``prev`` are no such point, and ``band_info`` / ``band_stream`` raise as ``qoimi_band_plan`` rejects.

``pad_rows <= K``: n + skip <= 64 + 61 < 128 <= K * w, so ``ceil((n + skip) / w) <= K <= first_row``; the band's descriptor has no more rows
than the image and always passes the pixel cap.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import crops as _crops

POINT_BYTES = 272
MIN_INTERVAL_PIXELS = 128
# qoimi_seek_point: 272 bytes
POINT_DTYPE = np.dtype([("byte_off", "<u4"), ("skip", "<u4"), ("prev", "<u4"), ("reserved", "<u4"), ("table", "<u4", (64,))])
assert POINT_DTYPE.itemsize == POINT_BYTES


def chunk_at(s: bytes, p: int) -> Tuple[int, int]:
    """(pixels, bytes) of the chunk whose tag byte is s[p] (qoi.h:547-575)."""
    b = s[p]
    if b == 0xFE:
        return 1, 4
    if b == 0xFF:
        return 1, 5
    if b >> 6 == 2:
        return 1, 2
    if b >> 6 == 3:
        return (b & 63) + 1, 1
    return 1, 1


def n_points(w: int, h: int, K: int) -> int:
    """``qoimi_seek_points`` for an accepted descriptor: ceil(h / K) - 1, or -1 if K == 0 or K * w < 128."""
    if K <= 0 or K * w < MIN_INTERVAL_PIXELS:
        return -1
    return -(-h // K) - 1


def hash_slot(px: np.ndarray) -> np.ndarray:
    px = px.astype(np.uint32)
    return (px[..., 0] * 3 + px[..., 1] * 5 + px[..., 2] * 7 + px[..., 3] * 11) % 64


def points(data: bytes, w: int, h: int, K: int, D, size: Optional[int] = None) -> np.ndarray:
    """The seek points of the first `size` bytes of `data` (default: all) as a POINT_DTYPE array.  D: the 4-channel decode of exactly those
    bytes, uint8 of h * w * 4 values in any shape."""
    size = len(data) if size is None else int(size)
    n = n_points(w, h, K)
    if n < 0 or size < 22:
        raise ValueError("points: K * w >= 128 and size >= 22")
    s = bytes(data[:size])
    D = np.asarray(D, dtype=np.uint8).reshape(h * w, 4)
    words = D.view("<u4").reshape(-1)
    slots = hash_slot(D)
    out = np.zeros(n, dtype=POINT_DTYPE)
    p, end, px = 14, size - 8, 0
    table = np.zeros(64, dtype=np.uint32)
    done = 0                                        # pixels whose slots are in `table`
    for k in range(n):
        P = (k + 1) * K * w
        while p < end:
            cnt, length = chunk_at(s, p)
            if px + cnt > P:
                break
            px += cnt
            p += length
        if p < end:
            out[k]["byte_off"], out[k]["skip"] = p, P - px
        else:
            out[k]["byte_off"], out[k]["skip"] = end, 0
        # (a later write to an index wins: the last pixel per slot)
        table[slots[done:P]] = words[done:P]
        done = P
        out[k]["prev"] = words[P - 1]
        out[k]["table"] = table
    return out


def points_from_pixels(data: bytes, w: int, h: int, K: int, pixels, channels: int, size: Optional[int] = None) -> np.ndarray:
    """The normative statement of ``qoimi_seek_index_from_pixels``: ``points(data, w, h, K, D, size)`` with D the caller's `pixels` - uint8 of
    h * w * channels values in any shape, channels 3 or 4 - at 4 channels, alpha 255 where channels == 3.  ``byte_off`` and ``skip`` are the walk
    of the STREAM, ``prev`` and ``table`` come from the PIXELS; that the stream decodes to them is not looked at.  Whenever it does - every
    stream an encoder wrote from them - this is ``points`` over the stream's decode."""
    if channels not in (3, 4):
        raise ValueError("points_from_pixels: channels is 3 or 4")
    px = np.asarray(pixels, dtype=np.uint8).reshape(h * w, channels)
    D = np.full((h * w, 4), 255, dtype=np.uint8)
    D[:, :channels] = px
    return points(data, w, h, K, D, size)


def _loads(point) -> List[int]:
    prev = int(point["prev"])
    vals = [int(v) for v in point["table"] if int(v) != 0 and int(v) != prev]
    return vals + [prev]


def pad_rows_of(point, w: int) -> int:
    """``pad_rows`` of a band that starts at `point`."""
    return max(1, -(-(len(_loads(point)) + int(point["skip"])) // w))


def _band_points(pts, K: int, h: int, first_row: int, rows: int):
    if rows < 1 or first_row < 0 or first_row + rows > h or first_row % K or (first_row and first_row // K > len(pts)):
        raise ValueError("band: first_row is 0 or a seek row, rows >= 1, first_row + rows <= h")
    e = pts[first_row // K - 1] if first_row else None
    k2 = -(-(first_row + rows) // K) - 1
    e2 = pts[k2] if 0 <= k2 < len(pts) else None
    return e, e2


def _prefix(e, w: int, rows: int, channels: int, colorspace: int) -> Tuple[bytes, int]:
    """(header, loads and pad run; pad_rows)"""
    if e is None:
        pad_rows, body = 0, b""
    else:
        loads = _loads(e)
        if len(loads) > 64:
            raise ValueError("band: a seek point with more than 64 loads (its table does not hold prev)")
        n, skip = len(loads), int(e["skip"])
        pad_rows = max(1, -(-(n + skip) // w))
        R = pad_rows * w - skip - n
        body = b"".join(b"\xff" + int(v).to_bytes(4, "little") for v in loads) + b"\xfd" * (R // 62)
        if R % 62:
            body += bytes([0xC0 | (R % 62 - 1)])
    head = b"qoif" + w.to_bytes(4, "big") + (pad_rows + rows).to_bytes(4, "big") + bytes([channels, colorspace])
    return head + body, pad_rows


def _tail(e, e2, size: int) -> Tuple[int, int]:
    lo = int(e["byte_off"]) if e is not None else 14
    hi = min(int(e2["byte_off"]) + 13, size) if e2 is not None else size
    if not 14 <= lo <= size - 8 or hi < lo:
        raise ValueError("band: the points do not belong to this stream")
    return lo, hi


def band_stream(data: bytes, w: int, h: int, channels: int, colorspace: int, K: int, pts, first_row: int, rows: int,
                size: Optional[int] = None) -> Tuple[bytes, int]:
    """(the band stream of rows [first_row, first_row + rows), pad_rows).  pts: ``points`` of the stream."""
    size = len(data) if size is None else int(size)
    e, e2 = _band_points(pts, K, h, first_row, rows)
    prefix, pad_rows = _prefix(e, w, rows, channels, colorspace)
    lo, hi = _tail(e, e2, size)
    return prefix + bytes(data[lo:hi]), pad_rows


def band_info(size: int, w: int, h: int, channels: int, colorspace: int, K: int, pts, first_row: int, rows: int) -> Dict[str, object]:
    """What ``qoimi_band_plan`` gives, from the points alone: {"size", "desc": (w, pad_rows + rows, channels, colorspace), "pad_rows"}."""
    e, e2 = _band_points(pts, K, h, first_row, rows)
    prefix, pad_rows = _prefix(e, w, rows, channels, colorspace)
    lo, hi = _tail(e, e2, size)
    return {"size": len(prefix) + hi - lo, "desc": (w, pad_rows + rows, channels, colorspace), "pad_rows": pad_rows}


def bands_for_crops(descs: Sequence, crops: Sequence, intervals: Sequence[int], pts: Optional[Sequence] = None):
    """(bands, rebased): per referenced image, ascending, the band ``(image, first_row, rows)`` that ``qoimi_decode_crops_indexed`` decodes -
    it starts at the last seek row at or above the image's topmost crop (0 if there is none) and reaches the largest y + height - and the
    crops as the inner ``qoimi_decode_crops`` call gets them: ``image`` the band's number, ``y - first_row + pad_rows``.  pts[i]: the points
    of image i (unreferenced images are not looked at); without pts only the bands are made and rebased is None."""
    top: Dict[int, int] = {}
    for c in crops:
        image, _, y, _, _, _ = _crops.fields(c)
        top[image] = min(top.get(image, y), y)
    bottom = _crops.rows_needed(descs, crops)
    bands = []
    for image in sorted(bottom):
        K = int(intervals[image])
        w = int(descs[image].width) if hasattr(descs[image], "width") else int(descs[image][0])
        if n_points(w, 1, K) < 0:
            raise ValueError("bands_for_crops: K * w >= 128")
        first_row = top[image] // K * K
        bands.append((image, first_row, bottom[image] - first_row))
    if pts is None:
        return bands, None
    number = {b[0]: k for k, b in enumerate(bands)}
    rebased = []
    for c in crops:
        image, x, y, cw, ch, flags = _crops.fields(c)
        _, first_row, _ = bands[number[image]]
        w = int(descs[image].width) if hasattr(descs[image], "width") else int(descs[image][0])
        pad = pad_rows_of(pts[image][first_row // int(intervals[image]) - 1], w) if first_row else 0
        rebased.append((number[image], x, y - first_row + pad, cw, ch, flags))
    return bands, rebased
