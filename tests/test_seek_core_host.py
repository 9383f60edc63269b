"""The arithmetic of the row seek index (qoi_amd/csrc/qoi_seek_core.h) compiled with g++ (tests/host/seek_host.cpp) and compared with the Python
model qoi_amd/seekindex.py on the CPU: band streams written item by item as band_assemble writes them - at every alignment, between guard
bytes, over a memory functor that counts every load outside the tail and every store outside the band stream - equal seekindex.band_stream
byte for byte; the walk of one 64-byte piece that seek_locate runs equals the chunk walk of the model at every entry phase and every target.
The same source is built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a program of its own: nothing
sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import GUARD, cuint, i64, u32, u32p, u64
from qoi_amd import seekindex as si
from model_cases import END, alpha_image, header, index_image, runs_image

SRC = "seek_host.cpp"


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    bp, vp = ctypes.c_char_p, ctypes.c_void_p
    return hostbuild.shared(SRC, tmp_path_factory, {
        "seek_host_points": (i64, [u32, u32, u32]),
        "seek_host_piece": (cuint, [bp, u32, u32, u32, u32p, u32p]),
        "seek_host_band": (i64, [vp, u32, u32, u32, u32, bp, u32, vp, u64, u64, u32p])})


def test_point_counts(host_lib):
    for w, h, K in [(1, 128, 128), (1, 129, 128), (1, 389, 128), (64, 13, 2), (64, 13, 1), (129, 8, 1), (16384, 16384, 256), (5, 100, 25), (5, 100, 26), (7, 3, 0)]:
        assert host_lib.seek_host_points(w, h, K) == si.n_points(w, h, K), (w, h, K)


def model_piece(piece, p, target):
    """the model's walk over one piece entered at byte p: (pixels, pos, before)"""
    px, pos, before = 0, 64, 0
    while p < len(piece):
        cnt, length = si.chunk_at(piece, p)
        if pos == 64 and px + cnt > target:
            pos, before = p, px
        px += cnt
        p += length
    return px, pos, before


def test_piece_walk(host_lib):
    rng = np.random.default_rng(5)
    pieces = [bytes([0xFF] * 64), bytes([0xFD] * 64), bytes([0xC0] * 64), bytes([0xFE, 1, 2, 3] * 16), bytes([0x80, 0xFF] * 32)]
    pieces += [rng.integers(0, 256, size=64, dtype=np.uint8).tobytes() for _ in range(40)]
    pieces += [rng.choice(np.array([0xFD, 0xC1, 0x00, 0xFF, 0xFE, 0x95], dtype=np.uint8), size=64).tobytes() for _ in range(20)]
    checked = 0
    for piece in pieces:
        for plen in (64, 63, 5, 1):
            for p in range(5):
                total = model_piece(piece[:plen], p, 1 << 40)[0]
                for target in sorted({0, 1, total // 2, total - 1, total, total + 5, 0xFFFFFFFF} - {-1}):
                    pos, before = ctypes.c_uint32(0), ctypes.c_uint32(0)
                    got = host_lib.seek_host_piece(piece, plen, p, target, ctypes.byref(pos), ctypes.byref(before))
                    want = model_piece(piece[:plen], p, target)
                    assert (got, pos.value) == want[:2] and (pos.value == 64 or before.value == want[2]), (piece.hex(), plen, p, target)
                    checked += 1
    assert checked > 5000


def bands_of(port):
    """(stream, w, h, ch, K, points, first_row, rows)"""
    out = []
    for w, h, ch, make, K in [(1, 400, 4, runs_image, 128), (2, 200, 3, index_image, 64), (61, 20, 4, alpha_image, 3), (64, 13, 4, index_image, 2),
                              (129, 9, 3, runs_image, 1), (333, 11, 4, index_image, 2)]:
        s = port.encode(make(w, h, ch, w), w, h, ch)
        for stream in (s, s[:len(s) // 2], header(w, h, ch) + b"\xfd" * (w * h // 40 + 3) + END):
            full4, _ = port.decode(stream, 4)
            pts = si.points(stream, w, h, K, full4)
            for first in [0] + [(k + 1) * K for k in range(len(pts))][:4] + [len(pts) * K]:
                for rows in sorted({1, min(K, h - first), h - first}):
                    out.append((stream, w, h, ch, K, pts, first, rows))
    return out


def test_band_streams_item_by_item(host_lib, port):
    checked = 0
    for n, (stream, w, h, ch, K, pts, first, rows) in enumerate(bands_of(port)):
        want, pad = si.band_stream(stream, w, h, ch, 0, K, pts, first, rows)
        e = pts[first // K - 1] if first else None
        lo = int(e["byte_off"]) if first else 14
        k2 = -(-(first + rows) // K) - 1
        hi = min(int(pts[k2]["byte_off"]) + 13, len(stream)) if k2 < len(pts) else len(stream)
        tail = stream[lo:hi]
        assert want.endswith(tail) and len(want) - len(tail) >= 14
        point = np.array(e).tobytes() if first else None
        for at in sorted({0, 1 + n % 15, 16}):
            buf = np.full(64 + at + len(want) + 64, GUARD, dtype=np.uint8)
            pad_rows = ctypes.c_uint32(99)
            rc = host_lib.seek_host_band(point, w, rows, ch, 0, tail, len(tail), buf.ctypes.data, buf.size, 64 + at, ctypes.byref(pad_rows))
            assert rc == len(want) and pad_rows.value == pad, (rc, len(want), w, first, rows)
            assert buf[64 + at:64 + at + len(want)].tobytes() == want, (w, K, first, rows, at)
            assert np.all(buf[:64 + at] == GUARD) and np.all(buf[64 + at + len(want):] == GUARD)
            checked += 1
    assert checked > 300


def test_a_point_with_64_distinct_table_words(host_lib):
    """An index is the caller's data.  64 non-zero table words that all differ from prev would be 65 loads and a head of 339 bytes: the core
    counts them, the head is not written (the library rejects the point before).  With prev in one slot it is the largest head there is, 334
    bytes, and equals the model's."""
    point = np.zeros((), dtype=si.POINT_DTYPE)
    point["byte_off"], point["skip"], point["prev"] = 14, 61, 0x7F7F7F7F
    point["table"] = np.arange(64, dtype=np.uint32) + 0x01000000
    tail = bytes(range(40))
    buf = np.full(1024, GUARD, dtype=np.uint8)
    pad_rows = ctypes.c_uint32(99)
    assert host_lib.seek_host_band(point.tobytes(), 64, 3, 4, 0, tail, len(tail), buf.ctypes.data, buf.size, 64, ctypes.byref(pad_rows)) == -1000065
    assert np.all(buf == GUARD) and pad_rows.value == 99
    with pytest.raises(ValueError):
        si._prefix(point, 64, 3, 4, 0)
    point["table"][33] = 0x7F7F7F7F
    want, pad = si._prefix(point, 64, 3, 4, 0)
    assert pad == 2 and len(want) == 14 + 5 * 64 + 1                       # 64 loads and skip 61 in rows of 64: a pad run of 3 pixels
    for at in (0, 5, 16):
        buf = np.full(64 + at + len(want) + len(tail) + 64, GUARD, dtype=np.uint8)
        rc = host_lib.seek_host_band(point.tobytes(), 64, 3, 4, 0, tail, len(tail), buf.ctypes.data, buf.size, 64 + at, ctypes.byref(pad_rows))
        assert rc == len(want) + len(tail) and pad_rows.value == 2
        assert buf[64 + at:64 + at + rc].tobytes() == want + tail and np.all(buf[:64 + at] == GUARD) and np.all(buf[64 + at + rc:] == GUARD)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "SEEK_HOST_MAIN", tmp_path) == "seek_host: 7344 bands ok\n"
