"""The item arithmetic the GPU kernel label_ingest runs (qoi_amd/csrc/qoi_label_core.h) compiled with g++ (tests/host/label_host.cpp) and
compared with the Python model qoi_amd/tiles.py on the CPU: every item of every tile of small planes - every dtype, both och, all four
flips, the copy at factor 1, the centre element and the vote above it, rectangles at odd x and y, partial edge blocks, every alignment of
the plane's address at which the kernel takes another load.  The host's memory functor checks every address: a load is whole, naturally
aligned elements of the plane (u8: an aligned dword that holds one of its bytes), a store lies in the slot and no byte is stored twice.
Every comparison is exact.  The same file with a main of its own is built with the address and undefined-behaviour sanitizers and run
directly against a plain counting loop."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import Banded, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import tiles

SRC = "label_host.cpp"
DTYPES = (tiles.L_U8, tiles.L_I32, tiles.L_I64)
# the residues of the plane's address modulo 16 at which the loads differ
RESIDUES = {tiles.L_U8: (0, 1, 2, 3), tiles.L_I32: (0, 4, 8, 12), tiles.L_I64: (0, 8)}
WILD = [256, -1, -100, 2 ** 31 - 1, -2 ** 31, 2 ** 32, 2 ** 32 + 5, -2 ** 32 + 7, 2 ** 63 - 1, -2 ** 63]
# (w, h) of the plane and the rectangle (x, y, cw, ch) in it: the issue's rectangles at odd x, y
RECTS = [((4, 4), (1, 1, 1, 1)), ((6, 4), (1, 3, 3, 1)), ((7, 4), (3, 1, 4, 1)), ((8, 4), (1, 1, 5, 1)), ((41, 27), (3, 1, 37, 23)), ((1030, 3), (5, 1, 1024, 1)),
         ((1030, 3), (3, 1, 1025, 1)), ((37, 23), (0, 0, 37, 23))]
# (mode, factor): the copy in every mode's name, the vote at 2, 3 and 16, the centre at 2 and 64
REDUCTIONS = [(tiles.PLAIN, 1), (tiles.MODE, 1), (tiles.MODE, 2), (tiles.MODE, 3), (tiles.MODE, 16), (tiles.NEAREST, 2), (tiles.NEAREST, 64)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "label_host_run": (i64, [ctypes.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u64, u64, u8p, u8p, u64, i64p]),
        "label_host_tiles": (u64, [u32, u32, u32, u32, u32]), "label_host_cfg": (u32, [u32, u32, u32, u32]), "label_host_kind": (u32, []),
        "label_host_bytes": (None, [u32p, u32, u8p, u8p])})


def plane(w, h, dtype, res, seed):
    """classes 0, 85, 170 and 255 in short runs - votes, ties and constants all happen - with every sixteenth element, where the dtype can
    hold it, far outside 0..255; inside a buffer of other bytes, its first element `res` bytes behind a 16-aligned address"""
    rng = np.random.default_rng(seed)
    elem = tiles.LABEL_ELEM[dtype]
    raw = np.full(w * h * elem + 96, 0x5A, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16 + 16 + res
    A = raw[at:at + w * h * elem].view(tiles.LABEL_ARRAYS[dtype]).reshape(h, w)
    v = np.repeat(rng.integers(0, 4, size=w * h), rng.integers(1, 4, size=w * h))[:w * h] * 85
    if dtype != tiles.L_U8:
        lo, hi = (-2 ** 31, 2 ** 31 - 1) if dtype == tiles.L_I32 else (-2 ** 63, 2 ** 63 - 1)
        wild = np.array([x for x in WILD if lo <= x <= hi], dtype=np.int64)
        v = np.where(rng.integers(0, 16, size=w * h) == 0, wild[rng.integers(0, wild.size, size=w * h)], v)
    A[:] = v.reshape(h, w).astype(tiles.LABEL_ARRAYS[dtype])
    assert A.ctypes.data % 16 == res
    return raw, A


def stored_bytes(P, och, f):
    """bytes of the slot a tile of P output pixels stores: whole 16-byte items at och 4 and the dwords that hold a byte at och 3 (factor 1),
    the pixels themselves above"""
    return P * och if f != 1 else 16 * -(-P // 4) if och == 4 else 4 * -(-3 * P // 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_item_of_every_tile_reproduces_the_model(host_lib, dtype):
    checked, wide = 0, 0
    for (w, h), (x, y, cw, ch) in RECTS:
        for res in RESIDUES[dtype]:
            raw, A = plane(w, h, dtype, res, seed=w * 131 + h * 7 + res)
            before = raw.copy()
            for mode, f in REDUCTIONS:
                if f > 1 and cw * ch > 2000 and f != 2:
                    continue                                           # (the long rows: the copy and one reduction of each kind are enough)
                tw, th = -(-cw // f), -(-ch // f)
                for flips in range(4):
                    for och in (3, 4):
                        flags = tiles.label_flags(dtype) | flips
                        want = tiles.tile(A, (0, x, y, cw, ch, f, flags), och, mode)
                        nbytes = tw * th * och
                        band = Banded(stored_bytes(tw * th, och, f), 0, band=256)
                        loads = (ctypes.c_longlong * 4)()
                        rc = host_lib.label_host_run(A.ctypes.data, w, h, dtype, x, y, cw, ch, f, flips, och, 1 if mode == tiles.MODE else 0, *band.args, loads)
                        what = ((w, h), (x, y, cw, ch), res, mode, f, flips, och)
                        assert rc >= 0, (what, "bad accesses", -1 - rc)
                        assert rc == host_lib.label_host_tiles(cw, ch, f, 1 if mode == tiles.MODE else 0, och) == tiles.label_tiles(cw, ch, f, och, mode if f > 1 else tiles.PLAIN) >= 1, what
                        got = band.inside(what)                        # every stored byte once, none beside them, none behind the slot
                        assert np.array_equal(got[:nbytes].reshape(th, tw, och), want), what
                        if f == 1 and cw >= 4:
                            wide += loads[2] if dtype != tiles.L_U8 else 0
                            if dtype == tiles.L_I32 and cw * ch >= 1024 and ch == 1:
                                # a row of 1024 or 1025 elements: the runs are 16-aligned or none is
                                aligned = (A.ctypes.data + (y * w + (x + cw - 4 if flips & 1 else x)) * 4) % 16 == 0
                                assert (loads[2] > 0) == aligned, (what, list(loads))
                        checked += 1
            assert np.array_equal(raw, before)                          # the source is only read
    assert checked >= 8 * len(RESIDUES[dtype]) * 5 * 8
    if dtype != tiles.L_U8:
        assert wide > 0                                                 # the 16-byte loads were taken somewhere


def test_the_entry(host_lib):
    assert host_lib.label_host_kind() == 4
    for dtype in DTYPES:
        for f, vote in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (16, 1), (64, 0)):
            for och in (3, 4):
                for flips in range(4):
                    cfg = host_lib.label_host_cfg(tiles.label_flags(dtype) | flips, f, vote, och)
                    lg, c = tiles.select_split(f, tiles.MODE if vote else tiles.NEAREST) if f > 1 else (0, 1)
                    assert cfg == lg | c << 8 | dtype << 16 | och << 20 | (1 if vote and f > 1 else 0) << 24 | 4 << 25 | flips << 28, (dtype, f, vote, och, flips)


def test_the_saturation_alone(host_lib):
    """int64 values as their two dwords: the listed ones, the neighbourhood of every power of two and random patterns"""
    r = np.random.default_rng(8)
    near = [s * 2 ** k + d for k in range(64) for s in (1, -1) for d in (-1, 0, 1)]
    v = np.array([x for x in WILD + [0, 1, 254, 255] + near if -2 ** 63 <= x <= 2 ** 63 - 1], dtype=np.int64)
    v = np.concatenate([v, r.integers(-2 ** 63, 2 ** 63 - 1, size=20000, dtype=np.int64), r.integers(-600, 600, size=5000, dtype=np.int64)])
    words = np.ascontiguousarray(v).view(np.uint32)
    out64, out32 = np.zeros(v.size, np.uint8), np.zeros(v.size, np.uint8)
    host_lib.label_host_bytes(words.ctypes.data_as(u32p), v.size, out64.ctypes.data_as(u8p), out32.ctypes.data_as(u8p))
    assert np.array_equal(out64, tiles.labels_to_bytes(v[None, :], tiles.label_flags(tiles.L_I64))[0, :, 0])
    low = words[0::2].view(np.int32)
    assert np.array_equal(out32, tiles.labels_to_bytes(low[None, :], tiles.label_flags(tiles.L_I32))[0, :, 0])
    for value, byte in ((2 ** 32, 255), (2 ** 32 + 5, 255), (-2 ** 32 + 7, 0), (-2 ** 63, 0), (2 ** 63 - 1, 255)):
        assert (v == value).any() and np.all(out64[v == value] == byte), value


def test_standalone_program_under_sanitizers(tmp_path):
    """label_host.cpp with its own main and its own counting-loop model, built with AddressSanitizer and UndefinedBehaviorSanitizer, run directly"""
    out = hostbuild.sanitized(SRC, "LABEL_HOST_MAIN", tmp_path)
    assert out.startswith("label_host: ") and out.endswith(" tiles ok\n") and int(out.split()[1]) == 5 * 10 * 2 * (7 + 5) * 4 * 2, out
