"""qoi_amd/imagediff.py: diff - the normative statement of qoimi_compare_images' comparison - on hand-made cases (no GPU)."""
import numpy as np

from qoi_amd import api, imagediff
from qoi_amd.imagediff import NONE, diff, pixel_word

N = 10


def rgba():
    px = np.arange(N * 4, dtype=np.uint8).reshape(N, 4) * 3 + 1
    px[:, 3] = 200 + np.arange(N)
    return px


def test_equal_images():
    a = rgba()
    for ca, cb in ((4, 4), (3, 3), (4, 3), (3, 4)):
        assert diff(a[:, :ca], a[:, :cb].copy(), N, ca, cb) == (0, NONE, 0, 0)
    assert diff(np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, 4, 3) == (0, NONE, 0, 0)


def test_first_pixel_only():
    a, b = rgba(), rgba()
    b[0, 1] ^= 0x40
    assert diff(a, b, N, 4, 4) == (1, 0, pixel_word(a, 0, 4), pixel_word(b, 0, 4))
    assert pixel_word(a, 0, 4) == 1 | 4 << 8 | 7 << 16 | 200 << 24
    assert pixel_word(b, 0, 4) == 1 | (4 ^ 0x40) << 8 | 7 << 16 | 200 << 24


def test_last_pixel_only():
    a, b = rgba(), rgba()
    b[N - 1, 2] += 1
    for ca, cb in ((4, 4), (3, 3), (4, 3), (3, 4)):
        m, first, want, got = diff(a[:, :ca], b[:, :cb], N, ca, cb)
        assert (m, first) == (1, N - 1)
        assert want == pixel_word(a[:, :ca], N - 1, ca) and got == pixel_word(b[:, :cb], N - 1, cb)


def test_alpha_only_is_seen_where_both_sides_hold_it():
    a, b = rgba(), rgba()
    b[4, 3] = 7
    m, first, want, got = diff(a, b, N, 4, 4)
    assert (m, first) == (1, 4) and want >> 24 == 204 and got >> 24 == 7 and want & 0xFFFFFF == got & 0xFFFFFF
    assert diff(a, b[:, :3], N, 4, 3) == (0, NONE, 0, 0)
    assert diff(a[:, :3], b, N, 3, 4) == (0, NONE, 0, 0)


def test_missing_alpha_reads_ff():
    a, b = rgba(), rgba()
    b[6, 0] ^= 1
    _, first, want, got = diff(a, b[:, :3], N, 4, 3)
    assert first == 6 and want >> 24 == 206 and got >> 24 == 0xFF
    _, first, want, got = diff(a[:, :3], b, N, 3, 4)
    assert first == 6 and want >> 24 == 0xFF and got >> 24 == 206
    _, first, want, got = diff(a[:, :3], b[:, :3], N, 3, 3)
    assert first == 6 and want >> 24 == 0xFF and got >> 24 == 0xFF and (want ^ got) == 1


def test_every_pixel():
    a = rgba()
    b = a ^ 0x10
    for ca, cb in ((4, 4), (3, 3), (4, 3), (3, 4)):
        m, first, want, got = diff(a[:, :ca], b[:, :cb], N, ca, cb)
        assert (m, first) == (N, 0) and (want ^ got) & 0xFFFFFF == 0x101010


def test_flat_buffers_and_longer_buffers_are_taken():
    a, b = rgba(), rgba()
    b[2] = 0
    flat_a, flat_b = np.concatenate([a.reshape(-1), [9, 9]]).astype(np.uint8), np.concatenate([b.reshape(-1), [1]]).astype(np.uint8)
    assert diff(flat_a, flat_b, N, 4, 4) == diff(a, b, N, 4, 4)


def test_record_layout_matches_the_c_struct():
    import ctypes
    assert imagediff.DIFF_DTYPE.itemsize == ctypes.sizeof(api.ImageDiff) == 32
    for name, _ in api.ImageDiff._fields_:
        assert imagediff.DIFF_DTYPE.fields[name][1] == getattr(api.ImageDiff, name).offset, name
    assert (imagediff.DIFF_PIXELS, imagediff.DIFF_HEADER) == (1, 2)
