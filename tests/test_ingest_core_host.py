"""The item arithmetic the GPU kernel tensor_ingest runs (qoi_amd/csrc/qoi_ingest_core.h) compiled with g++ (tests/host/ingest_host.cpp) and
compared with the Python model qoi_amd/tiles.py on the CPU: every item of every tile of small tensors at odd element offsets - every dtype,
both layouts, both channel counts in and out, every legal range, all four flips, rectangles at x = 1 and at the right edge.  The host's
memory functor checks every address: a load is whole, naturally aligned elements of the image (u8: an aligned dword that holds one of its
bytes), a store is aligned dwords of the slot.  Every comparison is exact.  The same file with a main of its own is built with the address
and undefined-behaviour sanitizers and run directly over the same walk."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import i64, u32, u32p, u64, u8p
from qoi_amd import tiles

SRC = "ingest_host.cpp"
# (w, h, elements the image begins behind a 16-aligned address)
SHAPES = [(1, 1, 1), (5, 3, 3), (37, 23, 1), (70, 9, 5)]
FORMATS = [(d, l, r) for d in (tiles.U8, tiles.F16, tiles.BF16, tiles.F32) for l in (tiles.HWC, tiles.CHW)
           for r in ((tiles.UNIT,) if d == tiles.U8 else (tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES))]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "ingest_host_run": (i64, [ctypes.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u8p]),
        "ingest_host_tiles": (u64, [u32, u32]), "ingest_host_items": (u64, [u32, u32]),
        "ingest_host_bytes": (None, [u32p, u32, u32, u32, u8p])})


def aligned(nbytes, align=256):
    raw = np.zeros(nbytes + align, dtype=np.uint8)
    shift = (-raw.ctypes.data) % align
    return raw[shift:shift + nbytes]


def elements(rng, count, dtype, rng_bits):
    """random elements over [-0.25, 1.25] scaled to the range (both clamps occur), as the dtype's array"""
    if dtype == tiles.U8:
        return rng.integers(0, 256, size=count, dtype=np.uint8)
    x = rng.uniform(-0.25, 1.25, size=count).astype(np.float32)
    x = {tiles.UNIT: x, tiles.SYMMETRIC: x * 2 - 1, tiles.BYTES: x * 255}[rng_bits]
    if dtype == tiles.F32:
        return x
    if dtype == tiles.F16:
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def source(w, h, sch, off, fmt, seed):
    """the tensor inside a buffer of random bytes, its first element `off` elements behind a 16-aligned address"""
    dtype, layout, rng_bits = fmt
    rng = np.random.default_rng(seed)
    elem = tiles.ELEM[dtype]
    nbytes = w * h * sch * elem
    buf = aligned(nbytes + 96, 16)
    buf[:] = rng.integers(0, 256, size=buf.size, dtype=np.uint8)
    view = buf[16 + off * elem:16 + off * elem + nbytes].view(tiles.SOURCE_ARRAYS[dtype])
    view[:] = elements(rng, w * h * sch, dtype, rng_bits)
    return buf, view.reshape((sch, h, w) if layout == tiles.CHW else (h, w, sch))


def rects(w, h):
    out = [(0, 0, w, h)]
    if w > 4:
        out += [(1, 0, w - 2, h), (w - 4, 1, 4, h - 1), (1, h - 1, w - 1, 1)]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d+%d" % s)
def test_every_item_of_every_tile_reproduces_the_model(host_lib, shape):
    w, h, off = shape
    checked = 0
    for fmt in FORMATS:
        flags = tiles.source_flags(*fmt)
        for sch in (3, 4):
            buf, T = source(w, h, sch, off, fmt, seed=w * 131 + h * 7 + sch + flags)
            assert T.ctypes.data % 16 == (off * tiles.ELEM[fmt[0]]) % 16
            before = buf.copy()
            B = tiles.convert(T, flags)
            if fmt[0] != tiles.U8 and w * h > 64:
                assert B.min() == 0 and B.max() == 255             # both clamps
            for rect in rects(w, h):
                x, y, cw, ch = rect
                for flips in range(4):
                    for och in (3, 4):
                        nbytes = cw * ch * och
                        out = aligned((nbytes + 255) & ~255)
                        out[:] = 0xEE
                        rc = host_lib.ingest_host_run(T.ctypes.data, w, h, sch, flags, x, y, cw, ch, flips, och, out.ctypes.data_as(u8p))
                        what = (shape, fmt, sch, rect, flips, och)
                        assert rc >= 0, (what, "an address was wrong", -rc)
                        assert rc == host_lib.ingest_host_tiles(cw, ch) == tiles.ingest_tiles(cw, ch) >= 1, what
                        want = tiles.tile(T, (0, x, y, cw, ch, 1, flags | flips), och)
                        assert np.array_equal(out[:nbytes].reshape(ch, cw, och), want), what
                        assert np.array_equal(want, tiles.tile(B, (0, x, y, cw, ch, 1, flips), och)), what
                        if och == 3:                                   # behind the last dword that holds a byte of the tile nothing is stored
                            assert np.all(out[(nbytes + 3) & ~3:] == 0xEE), what
                        checked += 1
            assert np.array_equal(buf, before)                      # the source is only read
    assert checked >= 20 * 2 * 8


def test_items_and_tiles(host_lib):
    """an item is four consecutive output pixels, 256 items a tile"""
    for cw, ch in [(1, 1), (3, 1), (4, 1), (5, 1), (64, 64), (257, 129), (1024, 1), (1025, 1), (2200, 2000), (19999, 20000)]:
        assert host_lib.ingest_host_items(cw, ch) == tiles.ingest_items(cw, ch) == -(-cw * ch // 4)
        assert host_lib.ingest_host_tiles(cw, ch) == tiles.ingest_tiles(cw, ch) == -(-(-(-cw * ch // 4)) // 256)


@pytest.mark.parametrize("dtype", [tiles.F16, tiles.BF16])
def test_every_16_bit_pattern(host_lib, dtype):
    """all 65536 elements of binary16 and of bfloat16 - NaNs, infinities, subnormals - in every range: the conversion alone"""
    bits = np.arange(65536, dtype=np.uint32)
    a = bits.astype(np.uint16)
    x = tiles.widen(a.view(np.float16) if dtype == tiles.F16 else a, dtype)
    for k, rng in enumerate((tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES)):
        out = np.zeros(65536, np.uint8)
        host_lib.ingest_host_bytes(bits.ctypes.data_as(u32p), 65536, dtype, k, out.ctypes.data_as(u8p))
        assert np.array_equal(out, tiles.to_bytes(x, rng)), (dtype, rng)


def test_float_patterns(host_lib):
    """binary32: the special values, the neighbourhood of every tie and of both clamps, and random bit patterns"""
    r = np.random.default_rng(5)
    t = (np.arange(-2, 258, dtype=np.float32)[:, None] + np.array([0.0, 0.5], np.float32)[None, :]).reshape(-1)
    near = np.concatenate([t, np.nextafter(t, np.float32(1e9)), np.nextafter(t, np.float32(-1e9))])
    x = np.concatenate([near, near / np.float32(255), near / np.float32(127.5) - np.float32(1),
                        np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30, 65504.0, 1e-45, -1e-45, 1.17549435e-38], np.float32),
                        r.integers(0, 2 ** 32, size=20000, dtype=np.uint32).view(np.float32)])
    bits = np.ascontiguousarray(x).view(np.uint32)
    for k, rng in enumerate((tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES)):
        out = np.zeros(bits.size, np.uint8)
        host_lib.ingest_host_bytes(bits.ctypes.data_as(u32p), bits.size, tiles.F32, k, out.ctypes.data_as(u8p))
        assert np.array_equal(out, tiles.to_bytes(x, rng)), rng


def test_standalone_program_under_sanitizers(tmp_path):
    """ingest_host.cpp with its own main and its own double-loop model, built with AddressSanitizer and UndefinedBehaviorSanitizer, run directly"""
    assert hostbuild.sanitized(SRC, "INGEST_HOST_MAIN", tmp_path) == "ingest_host: 3840 tiles ok\n"
