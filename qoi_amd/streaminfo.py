"""The normative model of ``qoimi_inspect_streams`` in plain Python (no torch, no GPU): the chunk walk of a QOI stream without pixel
state, its counts and the strict-conformance flags.  It plays the role ``synth.stream_hash64`` plays for the stream hash: the GPU tests
compare the kernels with it field for field.

The walk (tag rules of qoi.h:547-575, bounded by the BYTES and not by width*height as the reference's decode loop is)::

    p = 14; end = size - 8
    while p < end:
        b = s[p]
        0xFE -> RGB, 4 bytes      0xFF -> RGBA, 5 bytes
        b >> 6 == 0 -> INDEX, 1   == 1 -> DIFF, 1   == 2 -> LUMA, 2   == 3 -> RUN, 1 byte, (b & 63) + 1 pixels
        every other chunk is 1 pixel; count the chunk, add its pixels, p += its length
    walk_end = p
"""
from __future__ import annotations

import numpy as np

OP_INDEX, OP_DIFF, OP_LUMA, OP_RUN, OP_RGB, OP_RGBA = range(6)
OP_NAMES = ("INDEX", "DIFF", "LUMA", "RUN", "RGB", "RGBA")

SI_TOO_SHORT = 1         # size < 22: nothing was read, every other field is 0
SI_HEADER_BAD = 2        # fails the rules of qoi.h:497-521
SI_PIXELS_SHORT = 4      # pixels < width*height
SI_PIXELS_OVER = 8       # pixels > width*height
SI_LAST_CHUNK_CUT = 16   # walk_end > size - 8
SI_NO_END_MARKER = 32    # the final 8 bytes are not 0,0,0,0,0,0,0,1
SI_REPEATED_INDEX = 64   # repeat_index != 0 (qoi.h:118-119)
FLAG_NAMES = {SI_TOO_SHORT: "TOO_SHORT", SI_HEADER_BAD: "HEADER_BAD", SI_PIXELS_SHORT: "PIXELS_SHORT", SI_PIXELS_OVER: "PIXELS_OVER",
              SI_LAST_CHUNK_CUT: "LAST_CHUNK_CUT", SI_NO_END_MARKER: "NO_END_MARKER", SI_REPEATED_INDEX: "REPEATED_INDEX"}

END_MARKER = bytes([0, 0, 0, 0, 0, 0, 0, 1])   # qoi.h:339
PIXELS_MAX = 400000000                         # qoi.h:311

# qoimi_stream_info: 64 bytes, offsets 0/8/16/40/44/48/52
INFO_DTYPE = np.dtype([("pixels", "<u8"), ("run_pixels", "<u8"), ("ops", "<u4", (6,)), ("repeat_index", "<u4"),
                       ("walk_end", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (3,))])


def flag_names(flags: int) -> list:
    return [name for bit, name in FLAG_NAMES.items() if flags & bit]


def header_ok(s: bytes) -> bool:
    """qoi.h:505-521 on the 14 header bytes."""
    w, h = int.from_bytes(s[4:8], "big"), int.from_bytes(s[8:12], "big")
    return s[0:4] == b"qoif" and w != 0 and h != 0 and s[12] in (3, 4) and s[13] <= 1 and h < PIXELS_MAX // w


def inspect_stream(data: bytes, size=None) -> dict:
    """The fields of ``qoimi_stream_info`` for the first `size` bytes of `data` (default: all of it)."""
    size = len(data) if size is None else int(size)
    info = {"pixels": 0, "run_pixels": 0, "ops": [0] * 6, "repeat_index": 0, "walk_end": 0, "flags": 0}
    if size < 22:
        info["flags"] = SI_TOO_SHORT
        return info
    s = bytes(data[:size])
    ops = info["ops"]
    p, end, prev = 14, size - 8, -1
    pixels = run_pixels = repeat = 0
    while p < end:
        b = s[p]
        if b == 0xFE:
            ops[OP_RGB] += 1; pixels += 1; p += 4
        elif b == 0xFF:
            ops[OP_RGBA] += 1; pixels += 1; p += 5
        elif b >> 6 == 0:
            ops[OP_INDEX] += 1; pixels += 1; p += 1
            if b == prev:
                repeat += 1
        elif b >> 6 == 1:
            ops[OP_DIFF] += 1; pixels += 1; p += 1
        elif b >> 6 == 2:
            ops[OP_LUMA] += 1; pixels += 1; p += 2
        else:
            ops[OP_RUN] += 1; pixels += (b & 63) + 1; run_pixels += (b & 63) + 1; p += 1
        prev = b                      # the tag byte of the chunk in front: equal to an INDEX byte only if that chunk was the same INDEX
    flags = 0
    if not header_ok(s):
        flags |= SI_HEADER_BAD
    else:
        want = int.from_bytes(s[4:8], "big") * int.from_bytes(s[8:12], "big")
        flags |= SI_PIXELS_SHORT if pixels < want else 0
        flags |= SI_PIXELS_OVER if pixels > want else 0
    flags |= SI_LAST_CHUNK_CUT if p > end else 0
    flags |= SI_NO_END_MARKER if s[end:] != END_MARKER else 0
    flags |= SI_REPEATED_INDEX if repeat else 0
    info.update(pixels=pixels, run_pixels=run_pixels, repeat_index=repeat, walk_end=p, flags=flags)
    return info


def info_record(info: dict) -> np.ndarray:
    """An ``inspect_stream`` dict as one INFO_DTYPE record (what ``Context.inspect_streams`` returns per stream)."""
    r = np.zeros((), dtype=INFO_DTYPE)
    for k in ("pixels", "run_pixels", "repeat_index", "walk_end", "flags"):
        r[k] = info[k]
    r["ops"] = info["ops"]
    return r
