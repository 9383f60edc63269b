"""The item loop the GPU kernel tile_select runs for qoimi_encode_tiles in QOIMI_TILE_NEAREST / QOIMI_TILE_MODE (qoi_amd/csrc/qoi_tile_core.h
and the vote of qoi_mode_core.h) compiled with g++ (tests/host/tile_select_host.cpp: the lanes of a tile walked in a loop) and compared
with the Python model qoi_amd/tiles.py on the CPU: label images at every byte offset 0..3, both channel counts in and out, all four
flips, every factor with a lane split of its own.  The memory functor checks every access: a 4-byte load is aligned and holds a byte of the
image, a 16-byte load lies inside it, a store is naturally aligned and inside the slot, and every byte of the tile is stored exactly once.
Every comparison is exact.  The same file with a main of its own is built with the address and undefined-behaviour sanitizers and run
directly over such cases."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import i64, u32, u64, u8p
from labelimg import label_image
from qoi_amd import tiles

SRC = "tile_select_host.cpp"
KIND = {tiles.NEAREST: 1, tiles.MODE: 2}
FACTORS = {tiles.NEAREST: (1, 2, 3, 4, 5, 8, 13, 16, 33, 64), tiles.MODE: (1, 2, 3, 4, 5, 8, 13, 16)}
# (w, h, sch, byte offset of the image from a 16-aligned address)
SOURCES = [(1, 1, 3, 0), (1, 1, 4, 2), (1, 130, 3, 2), (1, 130, 4, 1), (37, 29, 3, 1), (37, 29, 3, 3), (70, 45, 4, 3), (70, 45, 4, 2), (64, 40, 4, 0)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "tile_select_host_run": (i64, [ctypes.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u64, u64, u8p, u8p, u64]),
        "tile_select_host_tiles": (u64, [u32, u32, u32, u32, u32]),
        "tile_select_host_cfg": (u32, [u32, u32, u32, u32, u32]),
        "tile_select_host_max_factor": (u32, [])})


def source(w, h, sch, off, seed):
    """the label image as uint8[h, w, sch] inside a buffer, its first byte at a 16-aligned address + off"""
    nbytes = w * h * sch
    raw = np.full(nbytes + 64 + 16, 0x5A, dtype=np.uint8)
    shift = (-raw.ctypes.data) % 16
    buf = raw[shift:shift + nbytes + 64]
    img = buf[16 + off:16 + off + nbytes].reshape(h, w, sch)
    img[:] = label_image(w, h, sch, seed)
    return buf, img


def rects(w, h):
    out = [(0, 0, w, h)]
    if w > 8 and h > 12:
        out += [(3, 5, w - 7, h - 9), (4, 8, w - 4, h - 8), (w - 5, h - 3, 5, 3)]       # edge blocks on both sides, odd corners
    elif h > 12:
        out += [(0, 5, w, h - 9), (0, 127, 1, 3)]
    return out


def run(lib, img, rect, f, flags, och, mode):
    h, w, sch = img.shape
    x, y, cw, ch = rect
    nbytes, tw, th = tiles.size(w, h, sch, (0, x, y, cw, ch, f, flags), och)
    assert nbytes == tw * th * och > 0
    slot = (nbytes + 255) & ~255
    b = hostbuild.Banded(slot, 0)
    assert b.q % 16 == 0
    rc = lib.tile_select_host_run(img.ctypes.data, w, h, sch, x, y, cw, ch, f, flags, och, KIND[mode], b.q, hostbuild.BASE, b.out.ctypes.data_as(u8p),
                                  b.writes.ctypes.data_as(u8p), b.hi)            # (a store behind the slot is a bad access)
    stored = (nbytes + 15) & ~15 if f == 1 else nbytes                           # the copy stores whole 16-byte words of the slot
    what = (img.shape, rect, f, flags, och, mode)
    assert np.all(b.writes[b.lo:b.lo + stored] == 1) and not b.writes[:b.lo].any() and not b.writes[b.lo + stored:].any(), what
    assert np.all(b.out[:b.lo] == hostbuild.GUARD) and np.all(b.out[b.lo + stored:] == hostbuild.GUARD), what
    return rc, b.out[b.lo:b.lo + nbytes].reshape(th, tw, och)


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "%dx%dx%d+%d" % s)
def test_every_item_of_every_tile_reproduces_the_model(host_lib, src):
    w, h, sch, off = src
    buf, img = source(w, h, sch, off, seed=w * 131 + h * 7 + sch + off)
    assert img.ctypes.data % 16 == off
    before = buf.copy()
    checked = 0
    for rect in rects(w, h):
        for mode in (tiles.NEAREST, tiles.MODE):
            for f in FACTORS[mode]:
                want0 = tiles.tile(img, (0,) + rect + (f, 0), 4, mode)            # the flips and och follow the reduction
                for flags in range(4):
                    for och in (3, 4):
                        rc, got = run(host_lib, img, rect, f, flags, och, mode)
                        what = (src, rect, f, flags, och, mode)
                        assert rc >= 0, (what, "bad accesses", -1 - rc)
                        assert rc == host_lib.tile_select_host_tiles(KIND[mode], rect[2], rect[3], f, och) == tiles.select_tiles(rect[2], rect[3], f, och, mode) >= 1, what
                        want = want0[::-1] if flags & 2 else want0
                        want = want[:, ::-1] if flags & 1 else want
                        assert np.array_equal(got, want[:, :, :och]), what
                        checked += 1
                assert np.array_equal(tiles.tile(img, (0,) + rect + (f, 3), 3, mode), want0[::-1, ::-1, :3])
    assert np.array_equal(buf, before)                          # the source is only read
    assert checked >= 18 * 8


def test_the_entry_and_the_limit(host_lib):
    assert host_lib.tile_select_host_max_factor() == tiles.MODE_MAX_FACTOR == 16
    for mode in (tiles.NEAREST, tiles.MODE):
        for f in FACTORS[mode]:
            lg, c = tiles.select_split(f, mode)
            for sch in (3, 4):
                for och in (3, 4):
                    for flags in range(4):
                        # bits 0..15: the vote's split; 16..19 sch; 20..23 och; 24: the box filter's alone; 25..27 the kind; 28.. the flags
                        assert host_lib.tile_select_host_cfg(KIND[mode], f, sch, och, flags) == lg | c << 8 | sch << 16 | och << 20 | KIND[mode] << 25 | flags << 28


def test_standalone_program_under_sanitizers(tmp_path):
    """tile_select_host.cpp with its own main and its own counting loop, built with AddressSanitizer and UndefinedBehaviorSanitizer, run directly"""
    assert hostbuild.sanitized(SRC, "TILE_SELECT_HOST_MAIN", tmp_path) == "tile_select_host: 3888 tiles ok\n"
