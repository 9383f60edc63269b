"""The item arithmetic the GPU kernel of qoimi_encode_tiles runs (qoi_amd/csrc/qoi_tile_core.h) compiled with g++ (tests/host/tile_host.cpp)
and compared with the Python model qoi_amd/tiles.py on the CPU: every item of every tile of small sources at odd byte offsets, both channel
counts in and out, both modes, all four flips, factors with every lane split.  The host's memory functor checks every address: a 4-byte load
is aligned and holds a byte of the image, a 16-byte load lies inside it, a store is an aligned word of the slot.  Every comparison is exact.
The same file with a main of its own is built with the address and undefined-behaviour sanitizers and run directly over the same cases."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, i64, u32, u64, u8p
from qoi_amd import tiles

SRC = "tile_host.cpp"
FACTORS = (1, 2, 3, 4, 5, 8, 13, 16, 33, 64)
# (w, h, sch, byte offset of the image from a 16-aligned address)
SOURCES = [(1, 1, 3, 0), (1, 1, 4, 2), (1, 130, 3, 2), (1, 130, 4, 0), (37, 29, 3, 1), (70, 45, 4, 3), (64, 40, 4, 0)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "tile_host_run": (i64, [ctypes.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, cint, u8p]),
        "tile_host_tiles": (u64, [u32, u32, u32, u32])})


def aligned(nbytes, align=256):
    raw = np.zeros(nbytes + align, dtype=np.uint8)
    shift = (-raw.ctypes.data) % align
    return raw[shift:shift + nbytes]


def source(w, h, sch, off, seed):
    """the image as uint8[h, w, sch] inside a buffer of random bytes, its first byte at a 16-aligned address + off"""
    rng = np.random.default_rng(seed)
    nbytes = w * h * sch
    buf = aligned(nbytes + 64, 16)
    buf[:] = rng.integers(0, 256, size=buf.size, dtype=np.uint8)
    img = buf[16 + off:16 + off + nbytes].reshape(h, w, sch)
    if sch == 4:
        img[:, :, 3] = rng.choice(np.array([0, 1, 128, 255], dtype=np.uint8), size=(h, w))
        img[: h // 2, : w // 3, 3] = 0                          # blocks whose alphas add up to 0: the plain value
    return buf, img


def rects(w, h):
    out = [(0, 0, w, h)]
    if w > 8 and h > 12:
        out += [(3, 5, w - 7, h - 9), (4, 8, w - 4, h - 8), (1, 0, 13, 11), (w - 5, h - 3, 5, 3)]       # edge blocks on both sides, odd corners
    elif h > 12:
        out += [(0, 5, w, h - 9), (0, 127, 1, 3)]
    return out


def run(lib, img, rect, f, flags, och, weighted):
    h, w, sch = img.shape
    x, y, cw, ch = rect
    nbytes, tw, th = tiles.size(w, h, sch, (0, x, y, cw, ch, f, flags), och)
    assert nbytes == tw * th * och > 0
    out = aligned((nbytes + 255) & ~255)
    out[:] = 0xEE
    rc = lib.tile_host_run(img.ctypes.data, w, h, sch, x, y, cw, ch, f, flags, och, int(weighted), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return rc, out[:nbytes].reshape(th, tw, och)


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "%dx%dx%d+%d" % s)
def test_every_item_of_every_tile_reproduces_the_model(host_lib, src):
    w, h, sch, off = src
    buf, img = source(w, h, sch, off, seed=w * 131 + h * 7 + sch)
    assert img.ctypes.data % 16 == off
    before = buf.copy()
    checked = 0
    for rect in rects(w, h):
        for f in FACTORS:
            for flags in range(4):
                for och in (3, 4):
                    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED):
                        rc, got = run(host_lib, img, rect, f, flags, och, mode == tiles.ALPHA_WEIGHTED)
                        what = (src, rect, f, flags, och, mode)
                        assert rc >= 0, (what, "an address was wrong", -rc)
                        cw, ch = rect[2], rect[3]
                        assert rc == host_lib.tile_host_tiles(cw, ch, f, och) >= 1, what
                        want = tiles.tile(img, (0,) + rect + (f, flags), och, mode)
                        assert np.array_equal(got, want), what
                        checked += 1
    assert np.array_equal(buf, before)                          # the source is only read
    assert checked >= 160


def test_items_and_tiles(host_lib):
    """f == 1: one item per aligned 16-byte word of the pixels; f >= 2: thumb_reduce's count over the rectangle; 256 items a tile"""
    for cw, ch in [(1, 1), (5, 1), (6, 1), (64, 64), (257, 129), (4096, 1), (1365, 3), (1366, 3)]:
        for och in (3, 4):
            assert host_lib.tile_host_tiles(cw, ch, 1, och) == -(-(-(-cw * ch * och // 16)) // 256)
        for f in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64):
            lanes = 1
            while -(-f // lanes) > 4:
                lanes *= 2
            assert host_lib.tile_host_tiles(cw, ch, f, 4) == -(-(-(-cw // f) * -(-ch // f) * lanes) // 256), (cw, ch, f)


def test_sum_extremes(host_lib):
    """64 x 64 blocks of 0xFF at factor 64: every sum at the limit qoi_thumb_core.h documents (64 * 64 * 255 * 255 < 2^32), and alpha 0"""
    img = aligned(128 * 64 * 4, 16).reshape(64, 128, 4)
    img[:] = 255
    img[:, 64:, 3] = 0
    img[:, 64:, 0] = 200
    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED):
        for och in (3, 4):
            rc, got = run(host_lib, img, (0, 0, 128, 64), 64, 0, och, mode == tiles.ALPHA_WEIGHTED)
            assert rc >= 0 and np.array_equal(got, tiles.tile(img, (0, 0, 0, 128, 64, 64), och, mode))
            assert got[0, 0].tolist() == [255] * och and got[0, 1].tolist() == [200, 255, 255, 0][:och]


def test_standalone_program_under_sanitizers(tmp_path):
    """tile_host.cpp with its own main and its own double-loop model, built with AddressSanitizer and UndefinedBehaviorSanitizer, run directly"""
    assert hostbuild.sanitized(SRC, "TILE_HOST_MAIN", tmp_path) == "tile_host: 3360 tiles ok\n"
