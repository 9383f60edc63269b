"""Inputs and small models that CPU tests and GPU tests share and that belong to no one call's case module: the layout of a pack, the
seek-index images, the gradient image of the resampling models, the argument builders of the qoimi_encode_tiles rejections and the
streams of the line-fetch tests."""
import ctypes
import struct

import numpy as np
import pytest

from qoi_amd import api, bicubic


def pack_offsets(lens, align):
    """d_packed_off of qoimi_pack_streams: uint64[n + 1] - the exclusive scan of the lengths, every start rounded up to `align`
    (a power of two); the last entry is the END of the last stream, not rounded."""
    lens = np.asarray(lens, dtype=np.uint64)
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    a = np.uint64(align)
    for i in range(lens.size):
        if i:
            off[i] = (off[i - 1] + lens[i - 1] + a - np.uint64(1)) // a * a
    off[-1] = off[-2] + lens[-1]
    return off


END = bytes([0, 0, 0, 0, 0, 0, 0, 1])


def header(w, h, ch, cs=0):
    return b"qoif" + w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([ch, cs])


def index_image(w, h, ch, seed):
    """five colours in random order: INDEX chunks, short runs, slots last written many rows back"""
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, size=(5, ch), dtype=np.uint8)
    px = palette[rng.integers(0, 5, size=w * h)]
    px[: w * h // 3] = palette[rng.integers(0, 2, size=w * h // 3)]          # colours 2..4 not seen for the first third
    return px


def runs_image(w, h, ch, seed):
    """runs of 1 to 200 pixels that cross row ends, some longer than 62 (several RUN chunks in a row)"""
    rng = np.random.default_rng(seed)
    px = np.zeros((w * h, ch), dtype=np.uint8)
    at = 0
    while at < w * h:
        n = int(rng.integers(1, 200))
        px[at:at + n] = rng.integers(0, 256, size=ch, dtype=np.uint8)
        at += n
    return px


def alpha_image(w, h, ch, seed):
    """noise with changing alpha (RGBA chunks where ch == 4)"""
    return np.random.default_rng(seed).integers(0, 256, size=(w * h, ch), dtype=np.uint8)


def gradient_image(w, h, och, seed):
    """random pixels, a quarter of them with alpha 0 and - at 4 channels - one all-transparent block in the lower left"""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 256, size=(h, w, och), dtype=np.uint8)
    if och == 4:
        D[:, :, 3][rng.integers(0, 4, size=(h, w)) == 0] = 0
        D[h // 2:, :w // 2, 3] = 0
    return D


E_ARG = -1


@pytest.fixture()
def args():
    class A:
        pass
    a = A()
    a.lib = api.load_library()
    a.fake_ctx = (ctypes.c_ubyte * (1 << 20))()                  # never looked at: every rejection comes first
    a.ctx = ctypes.addressof(a.fake_ctx)
    a.buf = (ctypes.c_ubyte * 8192)()                            # stands in for d_pixels, the device tables and the pack
    ctypes.memset(a.buf, 0x5A, 8192)
    a.p = ctypes.addressof(a.buf)
    a.pack, a.off, a.len = a.p + 4096, a.p + 6144, a.p + 7168
    a.po = (ctypes.c_size_t * 3)(1, 1024, 2051)
    a.descs = (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(5, 3, 3, 1))   # image 1 is named by no tile: garbage
    a.tiles = tl((0, 1, 1, 2, 2, 1, 0, 0), (2, 0, 0, 5, 3, 2, 3, 0))
    a.h_off = (ctypes.c_ulonglong * 3)(7, 7, 7)
    a.h_len = (ctypes.c_int * 2)(7, 7)
    a.h_desc = (api.QoiDesc * 2)(api.QoiDesc(7, 7, 7, 7), api.QoiDesc(7, 7, 7, 7))
    return a


def tl(*rows):
    return (api.QoimiTile * len(rows))(*[api.QoimiTile(*r) for r in rows])


def untouched(a):
    return (bytes(a.buf) == b"\x5A" * 8192 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096 and list(a.h_off) == [7] * 3 and list(a.h_len) == [7] * 2
            and all((d.width, d.height, d.channels, d.colorspace) == (7, 7, 7, 7) for d in a.h_desc))


def line_stream(w, h, body):
    return b"qoif" + struct.pack(">II", w, h) + bytes([4, 0]) + bytes(body) + bytes([0, 0, 0, 0, 0, 0, 0, 1])


def line_walk(w, h, seed, alpha=False):
    rng = np.random.default_rng(seed)
    px = np.cumsum(rng.integers(-3, 4, size=(w * h, 4)), axis=0).astype(np.uint8)
    if not alpha:
        px[:, 3] = 255
    return px


# the items of tests/test_gpu_bicubic.py, by image
SOFT, RGB, ONE, STRIP, CHECK, TALL = 0, 1, 2, 3, 4, 5
# identity; 5 x 3 -> 17 x 11 (the borders truncate the kernel); 64 x 64 -> 4 x 4 (64 taps, 16 lanes); 37 x 29 -> 5 x 7; 1 x 1 -> 9 x 9;
# rectangles at the image's edges; the whole strip at 58 taps; the checkerboard enlarged to five tiles; the flips take turns
IDENTITY = (SOFT, 3, 2, 40, 30, 40, 30, 2)
CHECK_UP = (CHECK, 5, 4, 9, 7, 40, 30, 0)
CHECK_DOWN = (CHECK, 2, 1, 64, 64, 4, 4, 0)
CAP = (STRIP, 0, 0, 128, 3, 8, 1, 0)                 # exactly 16 : 1 - 64 taps, sixteen lanes of four columns
NEAR_CAP = (STRIP, 3, 1, 127, 33, 8, 3, 1)           # 64 taps in x, 44 in y
BORDERS = (SOFT, 30, 20, 3, 3, 19, 11, 0)            # 3 x 3 enlarged: the kernel is cut at all four borders of every output pixel
CORNER = (SOFT, 64, 42, 3, 3, 5, 7, 3)               # ... at the image's corner
WRAP = (SOFT, 5, 4, 5, 3, 300, 2, 1)                 # 600 pixels of one lane: three tiles, each narrower than a row
WRAP_TWO = (STRIP, 0, 30, 130, 3, 129, 2, 0)         # 5 taps, two lanes: tiles of 128 pixels under rows of 129
ROWS = (TALL, 1, 0, 1, 4160, 1, 260, 2)              # tiles of 256 rows of 64 entries: the row table full
WIDE_ROW = (TALL, 0, 17, 4, 256, 256, 16, 0)         # a tile is one row of 256 pixels (the column table full) whose row has 64 entries
BICUBIC_ADDED = [CAP, NEAR_CAP, BORDERS, CORNER, WRAP, WRAP_TWO]
BICUBIC_ITEMS = [IDENTITY, (SOFT, 10, 7, 5, 3, 17, 11, 1), CHECK_DOWN, (SOFT, 20, 10, 37, 29, 5, 7, 3), (ONE, 0, 0, 1, 1, 9, 9, 0),
                 (SOFT, 55, 36, 12, 9, 7, 5, 0), (SOFT, 0, 0, 67, 45, 20, 13, 1), (STRIP, 0, 0, 130, 3, 9, 5, 2), CHECK_UP, (RGB, 60, 0, 7, 45, 3, 50, 3)] + BICUBIC_ADDED
BICUBIC_TABLES = [ROWS, WIDE_ROW]


def assert_bicubic_paths():
    """what the items make of the kernel, from the model alone (no GPU)"""
    assert {bicubic.split(it[3], it[5])[0] for it in BICUBIC_ITEMS} == {0, 1, 2, 3, 4}, ({bicubic.split(it[3], it[5])[0] for it in BICUBIC_ITEMS})
    assert bicubic.taps(64, 4) == 64 and bicubic.split(64, 4) == (4, 4), (bicubic.taps(64, 4), bicubic.split(64, 4))
    assert bicubic.tiles(9, 40, 30) == 5, (bicubic.tiles(9, 40, 30))
    assert [bicubic.split(it[3], it[5])[0] for it in (BORDERS, CORNER, WRAP, WRAP_TWO, CAP, NEAR_CAP, ROWS, WIDE_ROW)] == [0, 0, 0, 1, 4, 4, 0, 0], ([bicubic.split(it[3], it[5])[0] for it in (BORDERS, CORNER, WRAP, WRAP_TWO, CAP, NEAR_CAP, ROWS, WIDE_ROW)])
    assert bicubic.taps(128, 8) == 64 and bicubic.split(128, 8) == (4, 4) and bicubic.split(127, 8) == (4, 4) and bicubic.taps(33, 3) == 44, (bicubic.taps(128, 8), bicubic.split(128, 8), bicubic.split(127, 8), bicubic.taps(33, 3))
    assert int(np.count_nonzero(bicubic.kernel(128, 8)[3])) >= 62, (int(np.count_nonzero(bicubic.kernel(128, 8)[3])))
    # the 3 x 3 rectangles have fewer samples than the kernel has taps: it is cut for every output pixel, in both axes
    assert bicubic.taps(3, 19) == bicubic.taps(3, 11) == bicubic.taps(3, 5) == bicubic.taps(3, 7) == 4 > 3 and bicubic.first(0, 3, 19) == 0, (bicubic.taps(3, 19), bicubic.first(0, 3, 19))
    # the two forms of the column table; three tiles of one item; both tables full
    assert bicubic.tiles(5, 300, 2) == 3 and len(bicubic.tile(1, 5, 300, 2)[0]) == 256 and bicubic.tile(1, 5, 300, 2)[0][44] == 0, (bicubic.tiles(5, 300, 2), len(bicubic.tile(1, 5, 300, 2)[0]), bicubic.tile(1, 5, 300, 2)[0][44])
    assert bicubic.tile(1, 5, 300, 2) == (list(range(256, 300)) + list(range(212)), [0, 1]), (bicubic.tile(1, 5, 300, 2))
    assert bicubic.split(130, 129) == (1, 3) and len(bicubic.tile(0, 130, 129, 2)[0]) == 128 < 129, (bicubic.split(130, 129), len(bicubic.tile(0, 130, 129, 2)[0]))
    assert bicubic.tile(1, 130, 129, 2) == (list(range(128, 129)) + list(range(127)), [0, 1]), (bicubic.tile(1, 130, 129, 2))
    assert all(bicubic.tile(0, it[3], it[5], it[6])[0] == list(range(it[5])) for it in (BORDERS, CORNER, CAP, NEAR_CAP)), "all(bicubic.tile(0, it[3], it[5], it[6])[0] == list(range(it[5])) for it in (BORDERS, CORNER, CAP, NEAR_CAP))"
    assert bicubic.tiles(1, 1, 260) == 2 and len(bicubic.tile(0, 1, 1, 260)[1]) == 256 and bicubic.taps(4160, 260) == 64 and 256 * 64 == 16384, (bicubic.tiles(1, 1, 260), len(bicubic.tile(0, 1, 1, 260)[1]), bicubic.taps(4160, 260), 256 * 64)
    assert bicubic.tile(3, 4, 256, 16) == (list(range(256)), [3]) and bicubic.taps(256, 16) == 64 and 256 * (bicubic.split(4, 256)[1] << 0) == 1024, (bicubic.tile(3, 4, 256, 16), bicubic.taps(256, 16), 256 * (bicubic.split(4, 256)[1] << 0))
    # the kernel forms qy * qx in 32 bits: the added items reach 2^30 and stay below 2^31
    largest = {it: int(np.abs(bicubic.weights(it[4], it[6])).max()) * int(np.abs(bicubic.weights(it[3], it[5])).max()) for it in BICUBIC_ADDED + BICUBIC_TABLES}
    assert all(largest[it] >= 1 << 30 for it in (BORDERS, CORNER)) and max(largest.values()) < 1 << 31, (max(largest.values()))
    assert int(bicubic.weights(3, 19)[0, 0]) > 1 << 15 and int(bicubic.weights(3, 11)[10, 2]) > 1 << 15, (int(bicubic.weights(3, 19)[0, 0]), int(bicubic.weights(3, 11)[10, 2]))      # (the corner pixels: one pixel, both)
