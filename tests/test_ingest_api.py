"""Tensors as the source of qoimi_encode_tiles (QOIMI_TILE_SRC*), what can be checked without a GPU: the constants in every layer,
qoimi_tile_size with the bits, and every QOIMI_E_ARG case of the source format in the order the header gives - all of them are reported
before the context or the device is looked at, so a block of zeroed host memory stands in for a context and host arrays for device buffers
(the idiom of test_tiles_api.py); the outputs keep their bytes and qoimi_last_error names the cause."""
import ctypes
import os
import re

import pytest

from qoi_amd import api, tensors, tiles
from model_cases import E_ARG, tl, untouched
from model_cases import args  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = tiles.source_flags(tiles.F16)
F32_CHW = tiles.source_flags(tiles.F32, tiles.CHW, tiles.SYMMETRIC)


def test_constants_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    want = {"QOIMI_TILE_SRC": tiles.SRC, "QOIMI_TILE_SRC_CHW": tiles.SRC_CHW, "QOIMI_TILE_SRC_F16": tiles.SRC_F16, "QOIMI_TILE_SRC_BF16": tiles.SRC_BF16,
            "QOIMI_TILE_SRC_F32": tiles.SRC_F32, "QOIMI_TILE_SRC_SYMMETRIC": tiles.SRC_SYMMETRIC, "QOIMI_TILE_SRC_BYTES": tiles.SRC_BYTES}
    assert list(want.values()) == [16, 32, 64, 128, 192, 256, 512]
    for name, value in want.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (tiles.U8, tiles.F16, tiles.BF16, tiles.F32) == (tensors.U8, tensors.F16, tensors.BF16, tensors.F32)      # the dtype field holds QOIMI_TENSOR_*
    assert (tiles.SRC_F16, tiles.SRC_BF16, tiles.SRC_F32) == (tensors.F16 << 6, tensors.BF16 << 6, tensors.F32 << 6)
    assert tiles.SRC_MASK == 0x3F0 and tiles.SRC_MASK & (tiles.FLIP_X | tiles.FLIP_Y | 4 | 8) == 0
    core = open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_ingest_core.h")).read()
    assert re.search(r"kIngestPixels\s*=\s*4\b", core) and tiles.INGEST_PIXELS == 4
    mk = open(os.path.join(ROOT, "qoi_amd", "csrc", "sources.mk")).read()
    assert "qoi_ingest.hip" in mk
    # the header, the model and the kernel state the same conversion
    for text in (header, core, tiles.__doc__):
        flat = " ".join(re.sub(r"(?m)^\s*(/?\*|//)", " ", text).split())           # (the comment leaders of the two C files)
        assert "x * 255" in flat and "x * 127.5" in flat and "+ 127.5" in flat and "ties to even" in flat and "roundings" in flat and "t >= 255" in flat
    assert "|t| < 0.5 gives 0 either way" in " ".join(re.sub(r"(?m)^\s*\*", " ", header).split())


def test_the_ingest_kernel_has_no_timer_entry():
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert not any("ingest" in n for n in names)


def test_tile_size_with_the_bits():
    lib = api.load_library()
    legal = [tiles.source_flags(d, l, r) for d in (tiles.U8, tiles.F16, tiles.BF16, tiles.F32) for l in (tiles.HWC, tiles.CHW)
             for r in ((tiles.UNIT,) if d == tiles.U8 else (tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES))]
    assert len(set(legal)) == 20
    for src in legal:
        for flips in range(4):
            for ch_in in (3, 4):
                for ch in (0, 3, 4):
                    t = (7, 3, 2, 30, 17, 1, src | flips)
                    assert api.tile_size(37, 23, ch_in, t, ch) == tiles.size(37, 23, ch_in, t, ch) == (30 * 17 * (ch or ch_in), 30, 17)   # no size changes
    bad = [tiles.SRC_CHW, tiles.SRC_F16, tiles.SRC_BF16, tiles.SRC_F32, tiles.SRC_SYMMETRIC, tiles.SRC_BYTES, tiles.SRC_F16 | tiles.SRC_BYTES,   # no SRC
           tiles.SRC | 768, tiles.SRC | tiles.SRC_F32 | 768,                                                                                      # 768
           tiles.SRC | tiles.SRC_SYMMETRIC, tiles.SRC | tiles.SRC_CHW | tiles.SRC_BYTES,                                                           # a range with u8
           tiles.SRC | 4, tiles.SRC | 8, F16 | 1 << 10, F16 | 1 << 31]                                                                             # bits that stay unknown
    for flags in bad:
        tw, th = ctypes.c_uint(77), ctypes.c_uint(78)
        t = api.QoimiTile(0, 0, 0, 4, 4, 1, flags, 0)
        assert lib.qoimi_tile_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), ctypes.byref(t), 0, ctypes.byref(tw), ctypes.byref(th)) == 0, flags
        assert (tw.value, th.value) == (77, 78) and tiles.size(4, 4, 4, t, 0) == (0, 0, 0)
    for f in (2, 64):                                                # factor 1 only
        assert api.tile_size(8, 8, 4, (0, 0, 0, 8, 8, f, F16), 0) == tiles.size(8, 8, 4, (0, 0, 0, 8, 8, f, F16), 0) == (0, 0, 0)
        assert api.tile_size(8, 8, 4, (0, 0, 0, 8, 8, f, 0), 0)[0] > 0


def test_rejections_in_order(args):  # noqa: F811
    a = args
    # images: 0 is 4 x 4 x 4, 2 is 5 x 3 x 3 (1 is named by no tile); a.p is 8-aligned at least (ctypes), offsets chosen per case

    def call(po=(0, 1024, 2048), tiles_=None, mode=0, pack=a.pack, cap=1024, px=a.p, staging=0):
        return a.lib.qoimi_encode_tiles(a.ctx, px, (ctypes.c_size_t * 3)(*po), a.descs, 3, 0, tiles_, len(tiles_), mode, 1, pack, cap, a.off, a.len, staging,
                                        a.h_off, a.h_len, a.h_desc, None)

    assert a.p % 4 == 0
    t0 = (0, 1, 1, 2, 2, 1, F16, 0)
    t2 = (2, 0, 0, 5, 3, 1, F32_CHW | 3, 0)
    cases = [
        # 1: a SRC_* bit without QOIMI_TILE_SRC - and it comes behind the existing per-tile checks
        ("CHW without SRC", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.SRC_CHW, 0))), "without QOIMI_TILE_SRC"),
        ("F32 without SRC", lambda: call(tiles_=tl((0, 1, 1, 2, 2, 1, tiles.SRC_F32 | 1, 0), t2)), "without QOIMI_TILE_SRC"),
        ("BYTES without SRC, at factor 2 and range 768", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, 768, 0))), "without QOIMI_TILE_SRC"),
        ("an unknown bit comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.SRC_CHW | 4, 0))), "unknown flag bit"),
        ("bit 10 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, F16 | 1 << 10, 0))), "unknown flag bit"),
        ("reserved comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.SRC_CHW, 1))), "reserved"),
        ("the rectangle comes first", lambda: call(tiles_=tl(t0, (2, 1, 0, 5, 3, 1, tiles.SRC_CHW, 0))), "leaves"),
        # 2: range 768
        ("range 768", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, F16 | 768, 0))), "768"),
        ("range 768 with u8 and factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, tiles.SRC | 768, 0))), "768"),
        # 3: a range with u8
        ("SYMMETRIC with u8", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.SRC | tiles.SRC_SYMMETRIC, 0))), "range with a u8"),
        ("BYTES with u8 CHW at factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, tiles.SRC | tiles.SRC_CHW | tiles.SRC_BYTES, 0))), "range with a u8"),
        # 4: factor != 1
        ("factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, F32_CHW, 0))), "factor 1 only"),
        ("factor 64 with SRC alone, in a mixed call", lambda: call(tiles_=tl((0, 0, 0, 4, 4, 1, 0, 0), (2, 0, 0, 5, 3, 64, tiles.SRC, 0))), "factor 1 only"),
        ("factor 2 in QOIMI_TILE_MODE", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, F32_CHW, 0)), mode=tiles.MODE), "factor 1 only"),
        # 5: some but not all tiles carry SRC (before 6 and 7: image 0 would be misaligned and in two formats)
        ("a byte tile in a tensor call", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, (0, 0, 0, 4, 4, 1, 0, 0), t2)), "byte call or a tensor call"),
        ("a tensor tile in a byte call", lambda: call(tiles_=tl((0, 0, 0, 4, 4, 2, 0, 0), (2, 0, 0, 5, 3, 1, tiles.SRC, 0))), "byte call or a tensor call"),
        # 6: one image in two formats (before 7: image 0 at an odd address)
        ("image 0 as f16 and as u8", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, (0, 0, 0, 1, 1, 1, tiles.SRC, 0))), "two different source formats"),
        ("image 2 in two ranges", lambda: call(tiles_=tl(t2, t0, (2, 0, 0, 1, 1, 1, F32_CHW ^ tiles.SRC_SYMMETRIC, 0))), "two different source formats"),
        ("image 2 in two layouts", lambda: call(tiles_=tl(t2, (2, 0, 0, 1, 1, 1, F32_CHW ^ tiles.SRC_CHW, 0))), "two different source formats"),
        # 7: the address is not a multiple of the element size (before 8: the image would wrap the address space)
        ("f16 at an odd offset", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("f32 at offset 2", lambda: call(po=(0, 1024, 2050), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("f32 at an aligned offset of an odd d_pixels", lambda: call(px=a.p + 1, po=(1, 1024, 2048), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("f32 at an odd offset that also wraps", lambda: call(po=(0, 1024, 2 ** 64 - 9), tiles_=tl(t0, t2)), "multiple of the element size"),
        # 8: extents in BYTES.  Image 2 is 5 x 3 x 3 f32 = 180 bytes (45 as bytes), image 0 is 4 x 4 x 4 f16 = 128 bytes (64 as bytes)
        ("image end wraps the address space, counted in bytes", lambda: call(po=(0, 1024, 2 ** 64 - a.p - 176), tiles_=tl(t0, t2)), "address space"),
        ("image 2's last element lies in the pack", lambda: call(po=(0, 1024, 4096 - 176), tiles_=tl(t0, t2)), "overlap"),
        ("image 0's last element reaches into the pack", lambda: call(po=(4096 - 126, 1024, 2048), tiles_=tl(t0, t2)), "overlap"),
        ("the pack behind image 2's 45th byte", lambda: call(pack=a.p + 2048 + 45, cap=8, tiles_=tl(t0, t2)), "overlap"),
    ]
    for name, c, cause in cases:
        assert c() == E_ARG, name
        assert cause in api.last_error(), (name, api.last_error())
        assert untouched(a), name


def test_what_is_not_rejected_is_not_rejected_for_the_wrong_reason(args):  # noqa: F811
    """images that end one byte in front of the pack - in bytes of their dtype - pass the overlap check, and every legal format passes the
    format checks: such calls get as far as the context, which this test must not do, so it is the tile limit (9) that stops them.  The
    limit counts the new kernel's items: four output pixels each."""
    a = args
    w, h = 19999, 20000
    per = tiles.ingest_tiles(w, h)
    n = -(-(2 ** 31 - 1) // per)
    assert per * n >= 2 ** 31 - 1 > per * (n - 1) and n < 6000
    many_ok = n - 1
    descs = (api.QoiDesc * 1)(api.QoiDesc(w, h, 3, 0))
    for src in (tiles.SRC, tiles.source_flags(tiles.F16, tiles.CHW, tiles.BYTES), tiles.source_flags(tiles.BF16, tiles.HWC, tiles.SYMMETRIC), tiles.source_flags(tiles.F32, tiles.CHW)):
        nbytes = tiles.source_bytes(w, h, 3, src)
        many = (api.QoimiTile * n)(*[api.QoimiTile(0, 0, 0, w, h, 1, src | (j & 3), 0) for j in range(n)])
        for pack, cap in ((a.p - 64, 64), (a.p + nbytes, 64), (None, 0)):
            for mode in (0, 1, 4, 5):                                 # at factor 1 every mode is accepted
                rc = a.lib.qoimi_encode_tiles(a.ctx, a.p, (ctypes.c_size_t * 1)(0), descs, 1, 0, many, n, mode, 1, pack, cap, a.off, a.len, 1 << 60, a.h_off, a.h_len, a.h_desc, None)
                assert rc == E_ARG and "tiles of work items" in api.last_error(), api.last_error()
                assert untouched(a)
    # the count is the new kernel's: with tile_gather's items (16 bytes of och 3 each, fewer than four pixels' 12) the same n tiles stay below
    # the limit, and a byte call of them reaches the context - which is why this test does not make it
    assert per * many_ok < 2 ** 31 - 1
    gather = -(-(-(-w * h * 3 // 16)) // 256)
    assert gather * n < 2 ** 31 - 1 <= per * n
