"""The pixel fetch of qoimi_seek_index_from_pixels (qoi_amd/csrc/qoi_seekpx_core.h) compiled with g++ (tests/host/seekpx_host.cpp) and compared
with the Python model qoi_amd/seekindex.py on the CPU: the tiles of seekpx_last lane by lane and the single-pixel reads of seekpx_carry, over
images of 3 and 4 bytes per pixel at the base alignments 0 to 3 and intervals of 1, 3, 255, 256, 1023, 1024 and 1025 pixels (and 2064: two
tiles and a tail), through a memory functor that counts every load of a dword that holds no byte of the image.  The same source is built as a
stand-alone program with the address and undefined-behaviour sanitizers over heap buffers of exactly the image's dwords and run (a program
of its own: nothing sanitized is loaded into this process)."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cuint, i64, u32, u64
from qoi_amd import seekindex as si
from model_cases import END, header

SRC = "seekpx_host.cpp"
INTERVALS = [1, 3, 255, 256, 1023, 1024, 1025, 2064]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    vp = ctypes.c_void_p
    return hostbuild.shared(SRC, tmp_path_factory, {
        "seekpx_host_points": (i64, [vp, u64, u32, u32, u32, u32, vp, vp, vp, vp]),
        "seekpx_host_dwords": (cuint, [u64, u32])})


def image(ipx, np_, ch, seed):
    """np_ * ipx pixels: a few colours in short runs (equal neighbours at every lane and wavefront edge), some never seen again"""
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, size=(9, ch), dtype=np.uint8)
    pick = rng.integers(0, 9, size=np_ * ipx)
    hold = rng.integers(0, 3, size=np_ * ipx) != 0                          # two of three pixels repeat the one in front
    for p in range(1, pick.size):
        if hold[p]:
            pick[p] = pick[p - 1]
    px = palette[pick]
    px[: min(4, len(px))] = rng.integers(0, 256, size=(min(4, len(px)), ch), dtype=np.uint8)   # colours of the first lane only
    return px


def model(px, ipx, np_, ch):
    """(words, prev[np_], table[np_][64]) as qoi_amd/seekindex.py: points takes them from D"""
    D = np.full((len(px), 4), 255, dtype=np.uint8)
    D[:, :ch] = px
    words = np.ascontiguousarray(D).view("<u4").reshape(-1)
    slots = si.hash_slot(D)
    table = np.zeros(64, dtype=np.uint32)
    prev, tables = [], []
    for k in range(np_):
        table[slots[k * ipx:(k + 1) * ipx]] = words[k * ipx:(k + 1) * ipx]
        prev.append(int(words[(k + 1) * ipx - 1]))
        tables.append(table.copy())
    return words, np.array(prev, dtype=np.uint32), np.array(tables)


def run(host_lib, px, ipx, np_, ch, align):
    nbytes = px.size
    ndw = (align + nbytes + 3) // 4
    buf = np.full(ndw * 4, 0xEE, dtype=np.uint8)                             # exactly the aligned dwords that hold the image
    buf[align:align + nbytes] = px.reshape(-1)
    last = np.zeros((np_, 64), dtype=np.uint32)
    seen = np.full(np_ * ipx, 0x5A5A5A5A, dtype=np.uint32)
    prev = np.zeros(np_, dtype=np.uint32)
    table = np.zeros((np_, 64), dtype=np.uint32)
    rc = host_lib.seekpx_host_points(buf.ctypes.data, buf.size, align, ch, ipx, np_, last.ctypes.data, seen.ctypes.data, prev.ctypes.data, table.ctypes.data)
    return rc, last, seen, prev, table


@pytest.mark.parametrize("ch", [3, 4])
def test_fetch_equals_the_model_at_every_alignment(host_lib, ch):
    checked = 0
    for ipx in INTERVALS:
        for np_ in (1, 3):
            px = image(ipx, np_, ch, 100 * ipx + np_ + ch)
            words, want_prev, want_table = model(px, ipx, np_, ch)
            for align in range(4):
                rc, last, seen, prev, table = run(host_lib, px, ipx, np_, ch, align)
                assert rc >= 0, (ipx, np_, align, rc)                        # no dword outside the image's was asked for
                assert np.array_equal(seen, words), (ipx, np_, align)
                assert np.array_equal(prev, want_prev) and np.array_equal(table, want_table), (ipx, np_, align)
                # a lane reads at most five dwords, a single pixel at most two: nothing is fetched byte by byte
                lanes = np_ * -(-ipx // 4)
                assert rc <= 5 * lanes + 2 * 65 * np_, (ipx, np_, align, rc)
                # the words of `last` are positions + 1 of pixels of their interval and slot
                for k in range(np_):
                    for s in np.flatnonzero(last[k]):
                        pos = int(last[k][s]) - 1
                        assert k * ipx <= pos < (k + 1) * ipx and int(si.hash_slot(np.frombuffer(words[pos:pos + 1].tobytes(), dtype=np.uint8))) == s
                checked += 1
    assert checked == 64


def test_equals_points_from_pixels(host_lib):
    """... and the model's own entry point: prev and table of points_from_pixels for images of w x h, K rows per interval"""
    stream = lambda w, h, ch: header(w, h, ch) + b"\xfd" * 3 + END         # (byte_off and skip are the stream's: not looked at here)
    for w, h, K, ch in [(129, 40, 16, 3), (64, 13, 2, 4), (1, 400, 128, 4), (65, 20, 3, 3), (300, 30, 5, 4)]:
        np_ = si.n_points(w, h, K)
        px = image(w * h, 1, ch, w + h)
        if w == 300:                                                        # constant stripes 70 pixels wide
            px = np.repeat(np.arange(-(-w * h // 70), dtype=np.uint8)[:, None] % 5 * 50 + 3, 70, axis=0)[:w * h].repeat(ch, axis=1)
        want = si.points_from_pixels(stream(w, h, ch), w, h, K, px, ch)
        for align in range(4):
            rc, _, _, prev, table = run(host_lib, px[:np_ * K * w], K * w, np_, ch, align)
            assert rc >= 0 and np.array_equal(prev, want["prev"]) and np.array_equal(table, want["table"]), (w, h, K, ch, align)


def test_dword_counts(host_lib):
    for addr in range(8):
        for nbytes in range(17):
            want = 0 if nbytes == 0 else (addr + nbytes - 1) // 4 - addr // 4 + 1
            assert host_lib.seekpx_host_dwords(0x1000 + addr, nbytes) == want, (addr, nbytes)


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "SEEKPX_HOST_MAIN", tmp_path) == "seekpx_host: 352 tiles ok\n"
