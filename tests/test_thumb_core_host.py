"""The block arithmetic the GPU kernel runs (qoi_amd/csrc/qoi_thumb_core.h: sums of a block -> output pixel, both modes) compiled with g++
(tests/host/thumb_host.cpp) and compared with the Python model qoi_amd/thumbs.py on the CPU: every cnt the factors 1..64 can produce, the
extremes of the sums, random weighted blocks.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import cint, i64, u32, u32p, u8p
from qoi_amd import thumbs
from qoi_amd.thumbs import ALPHA_WEIGHTED, PLAIN


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared("thumb_host.cpp", tmp_path_factory, {
        "thumb_host_pixels": (None, [u32p, u32p, ctypes.c_size_t, cint, u32p]),
        "thumb_host_div_round": (None, [u32p, u32p, ctypes.c_size_t, u32p]),
        "thumb_host_extent": (u32, [u32, u32]),
        "thumb_host_split": (None, [u32, u32p, u32p]),
        "thumb_host_cover": (i64, [u32, u32, u32, u8p, u32p, u32p])})


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def core_pixels(lib, sums, cnt, weighted):
    """sums uint32[n, 7] (S_r, S_g, S_b, S_a, W_r, W_g, W_b), cnt uint32[n] -> uint8[n, 4]"""
    sums = np.ascontiguousarray(sums, dtype=np.uint32)
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    out = np.zeros(len(cnt), dtype=np.uint32)
    lib.thumb_host_pixels(ptr(sums), ptr(cnt), len(cnt), int(weighted), ptr(out))
    return out.view(np.uint8).reshape(-1, 4)


def model_pixels(sums, cnt, weighted):
    """the definition over the same sums, in Python ints"""
    out = np.zeros((len(cnt), 4), dtype=np.uint8)
    for i, (s, n) in enumerate(zip(sums.tolist(), cnt.tolist())):
        res = [(s[c] + n // 2) // n for c in range(4)]
        if weighted and s[3] > 0:
            res[:3] = [(s[4 + c] + s[3] // 2) // s[3] for c in range(3)]
        out[i] = res
    return out


def all_counts():
    """every cnt a factor 1..64 can produce: whole blocks f * f, edge blocks a * f (a < f columns or rows), corner blocks a * b"""
    counts = set()
    for f in range(1, 65):
        for a in range(1, f + 1):
            counts.add(a * f)
            for b in range(1, f + 1):
                counts.add(a * b)
    return sorted(counts)


def test_extent(host_lib):
    for f in range(1, 65):
        for n in (1, f - 1, f, f + 1, 2 * f, 2 * f + 1, 399999999, 4294967295):
            if n >= 1:
                assert host_lib.thumb_host_extent(n, f) == -(-n // f) == (thumbs.size(n, 1, f)[0]), (n, f)


def test_div_round_every_count(host_lib):
    """(s + d/2) / d for every cnt and every sum a channel of such a block can reach at the edges of each quotient, and at the extremes"""
    s_list, d_list = [], []
    for d in all_counts():
        top = 255 * d
        cands = {0, 1, d // 2 - 1, d // 2, d // 2 + 1, d - 1, d, d + d // 2 - 1, d + d // 2, top - d // 2 - 1, top - d // 2, top - 1, top}
        for q in (1, 2, 127, 128, 254):
            cands |= {q * d + d // 2 - 1, q * d + d // 2, q * d - d // 2 - 1, q * d - d // 2, q * d - (d + 1) // 2, q * d + (d - 1) // 2, q * d + (d + 1) // 2}
        for s in cands:
            if 0 <= s <= top:
                s_list.append(s); d_list.append(d)
    s = np.array(s_list, dtype=np.uint32)
    d = np.array(d_list, dtype=np.uint32)
    out = np.zeros(len(s), dtype=np.uint32)
    host_lib.thumb_host_div_round(ptr(s), ptr(d), len(s), ptr(out))
    want = (s.astype(np.int64) + d.astype(np.int64) // 2) // d.astype(np.int64)
    assert np.array_equal(out, want)
    assert out.max() == 255
    # division by a sum of alphas: numerators up to 64 * 64 * 255 * 255
    rng = np.random.default_rng(11)
    A = np.concatenate([rng.integers(1, 64 * 64 * 255 + 1, size=200000), np.array([1, 2, 3, 255, 256, 64 * 64 * 255, 64 * 64 * 255 - 1])]).astype(np.int64)
    c = rng.integers(0, 256, size=len(A))
    num = np.minimum(A * c + rng.integers(0, 2, size=len(A)) * rng.integers(0, 255, size=len(A)), A * 255)
    out = np.zeros(len(A), dtype=np.uint32)
    host_lib.thumb_host_div_round(ptr(num.astype(np.uint32)), ptr(A.astype(np.uint32)), len(A), ptr(out))
    assert np.array_equal(out, (num + A // 2) // A)


@pytest.mark.parametrize("weighted", [False, True])
def test_pixels_every_count_and_the_extremes(host_lib, weighted):
    """whole-block sums: for every cnt, all channels at 0, at the top (255 * cnt; weighted 255 * 255 * cnt), and random sums a block of that
    many pixels can have"""
    rng = np.random.default_rng(3 + weighted)
    rows, cnts = [], []
    for n in all_counts():
        for _ in range(6):
            px = rng.integers(0, 256, size=(min(n, 64), 4))            # up to 64 distinct pixels, repeated to n
            reps = np.full(len(px), n // len(px)); reps[: n % len(px)] += 1
            S = (px * reps[:, None]).sum(axis=0)
            Wt = (px[:, :3] * px[:, 3:4] * reps[:, None]).sum(axis=0)
            rows.append(list(S) + list(Wt)); cnts.append(n)
        rows.append([0] * 7); cnts.append(n)
        rows.append([255 * n] * 4 + [255 * 255 * n] * 3); cnts.append(n)
        rows.append([255 * n, 0, 17 * n, 0, 0, 0, 0]); cnts.append(n)                       # transparent: the plain value in both modes
        rows.append([n, n, n, 1, 1, 1, 1] if n > 1 else [1, 1, 1, 1, 1, 1, 1]); cnts.append(n)   # one faint pixel carries the colour
    sums, cnt = np.array(rows, dtype=np.uint32), np.array(cnts, dtype=np.uint32)
    assert sums.max() == 64 * 64 * 255 * 255
    assert np.array_equal(core_pixels(host_lib, sums, cnt, weighted), model_pixels(sums, cnt, weighted))


def test_random_weighted_blocks_against_the_model(host_lib):
    """More than 10^5 random blocks: pixels -> sums (numpy) -> the core, against thumbs.thumbnail of the same pixels.  An image of height
    bh <= f whose width is a multiple of f is one row of blocks of f x bh pixels, so every (f, bh) below gives blocks of cnt = f * bh."""
    rng = np.random.default_rng(2024)
    total = 0
    differ = False
    shapes = [(f, 1, 1600) for f in range(1, 65)] + [(64, bh, 24) for bh in (2, 3, 5, 17, 33, 63, 64)] + [(7, 5, 300), (8, 8, 300), (3, 2, 300)]
    for k, (f, bh, blocks) in enumerate(shapes):
        px = rng.integers(0, 256, size=(bh, f * blocks, 4), dtype=np.uint8)
        kind = k % 4
        if kind == 0:
            px[:, :, 3] = rng.choice(np.array([0, 255], dtype=np.uint8), size=px.shape[:2])
        elif kind == 1:
            px[:, :, 3] = rng.integers(0, 3, size=px.shape[:2])
        elif kind == 2:
            px[:, : f * (blocks // 2), 3] = 0                                # all-transparent blocks: the plain value
        a = px.astype(np.int64).reshape(bh, blocks, f, 4)
        sums = np.zeros((blocks, 7), dtype=np.uint32)
        sums[:, :4] = a.sum(axis=(0, 2))
        sums[:, 4:] = (a[..., :3] * a[..., 3:4]).sum(axis=(0, 2))
        cnt = np.full(blocks, f * bh, dtype=np.uint32)
        want_plain, want_weighted = thumbs.thumbnail(px, f, PLAIN)[0], thumbs.thumbnail(px, f, ALPHA_WEIGHTED)[0]
        assert want_plain.shape == (blocks, 4)
        assert np.array_equal(core_pixels(host_lib, sums, cnt, False), want_plain), (f, bh)
        assert np.array_equal(core_pixels(host_lib, sums, cnt, True), want_weighted), (f, bh)
        differ |= not np.array_equal(want_plain, want_weighted)
        total += blocks
    assert total >= 100000 and differ


def test_split_of_a_block_over_lanes(host_lib):
    """L = 1, 2, 4, 8 or 16 lanes, at most 4 columns each, together at least f; 16 bytes a lane for f = 4, 8, 16, 32, 64 and 8 for f = 2"""
    for f in range(1, 65):
        lg, c = ctypes.c_uint32(99), ctypes.c_uint32(99)
        host_lib.thumb_host_split(f, ctypes.byref(lg), ctypes.byref(c))
        L = 1 << lg.value
        assert lg.value <= 4 and 1 <= c.value <= 4 and L * c.value >= f > (L // 2) * 4 * (L > 1), (f, L, c.value)
        assert c.value == -(-f // L)
        if f in (4, 8, 16, 32, 64):
            assert c.value == 4 and L == f // 4
        if f == 2:
            assert (L, c.value) == (1, 2)


def test_items_cover_every_source_pixel_once(host_lib):
    """the item numbering thumb_reduce uses (thumb_share, tile by tile): for all 64 factors every source pixel is read by exactly one lane, no
    share leaves the image, and the lanes of an output pixel read exactly the cnt pixels it divides by - on shapes with partial edge blocks,
    w < f, h < f, one pixel, and more than one tile"""
    shapes = [(1, 1), (1, 97), (131, 1), (37, 23), (257, 9), (64, 48), (130, 70), (63, 65), (128, 128)]
    for f in range(1, 65):
        lg, c = ctypes.c_uint32(), ctypes.c_uint32()
        host_lib.thumb_host_split(f, ctypes.byref(lg), ctypes.byref(c))
        for w, h in shapes:
            tw, th = thumbs.size(w, h, f)
            reads = np.zeros(w * h, dtype=np.uint8)
            share, cnt = np.zeros(tw * th, dtype=np.uint32), np.zeros(tw * th, dtype=np.uint32)
            tiles = host_lib.thumb_host_cover(w, h, f, reads.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ptr(share), ptr(cnt))
            assert tiles == -(-((tw * th) << lg.value) // 256), (w, h, f, tiles)
            assert np.all(reads == 1), (w, h, f)
            bw = np.minimum(f, w - f * np.arange(tw))
            bh = np.minimum(f, h - f * np.arange(th))
            assert np.array_equal(cnt.reshape(th, tw), bh[:, None] * bw[None, :]) and np.array_equal(share, cnt), (w, h, f)
