"""qoimi_encode_tiles / qoimi_tile_size / qoimi_tile_pyramid / qoimi_tile_stats, what can be checked without a GPU: the entry points in every
layer, the structure's layout, the host arithmetic against qoi_amd/tiles.py, and every QOIMI_E_ARG case - all of them are reported before the
context or the device is looked at, so a block of zeroed host memory stands in for a context here and host arrays for device buffers; the
outputs keep their bytes and qoimi_last_error names the cause."""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, tiles
from model_cases import E_ARG, tl, untouched
from model_cases import args  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_encode_tiles", "qoimi_tile_size", "qoimi_tile_pyramid", "qoimi_tile_stats")


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_encode_tiles\s*\(", header) and re.search(r"\bsize_t\s+qoimi_tile_size\s*\(", header)
    assert re.search(r"\bint\s+qoimi_tile_pyramid\s*\(", header) and re.search(r"\bvoid\s+qoimi_tile_stats\s*\(", header)
    assert re.search(r"\}\s*qoimi_tile\s*;", header)
    assert (tiles.FLIP_X, tiles.FLIP_Y, tiles.PLAIN, tiles.ALPHA_WEIGHTED) == (1, 2, 0, 1)
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("encode_tiles", "tile_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.tile_size) and callable(api.tile_pyramid)
    mk = open(os.path.join(ROOT, "qoi_amd", "csrc", "sources.mk")).read()
    assert "qoi_tile.hip" in mk and os.path.exists(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_tile_core.h"))


def test_the_gather_kernel_has_no_timer_entry():
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert not any("tile" in n for n in names)


def test_struct_layout():
    assert ctypes.sizeof(api.QoimiTile) == 32
    assert [(f, getattr(api.QoimiTile, f).offset) for f, _ in api.QoimiTile._fields_] == [
        ("image", 0), ("x", 4), ("y", 8), ("width", 12), ("height", 16), ("factor", 20), ("flags", 24), ("reserved", 28)]
    t = api.QoimiTile(1, 2, 3, 4, 5, 6, 3, 0)
    assert bytes(t) == b"".join(v.to_bytes(4, "little") for v in (1, 2, 3, 4, 5, 6, 3, 0))
    assert tiles.fields(t) == (1, 2, 3, 4, 5, 6, 3, 0)


def test_tile_size():
    lib = api.load_library()
    for (w, h) in [(1, 1), (37, 23), (3840, 2160), (19999, 20000)]:
        for rect in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, w, h), (w // 2, h // 3, w - w // 2, h - h // 3)]:
            for f in (1, 2, 3, 13, 64):
                for ch_in in (3, 4):
                    for ch in (0, 3, 4):
                        t = (7,) + rect + (f, 3)                         # (tile.image is not looked at)
                        want = tiles.size(w, h, ch_in, t, ch)
                        assert want[0] == -(-rect[2] // f) * -(-rect[3] // f) * (ch or ch_in)
                        assert api.tile_size(w, h, ch_in, t, ch) == want, (w, h, rect, f, ch_in, ch)
    good = (0, 1, 1, 2, 2, 1, 0, 0)
    zero = [((0, 4, 4, 0), good, 4), ((4, 0, 4, 0), good, 4), ((4, 4, 2, 0), good, 4), ((4, 4, 5, 0), good, 0), ((4, 4, 4, 2), good, 4), ((20000, 20000, 4, 0), good, 4),
            ((4, 4, 4, 0), (0, 0, 0, 0, 1, 1, 0, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 0, 1, 0, 0), 4), ((4, 4, 4, 0), (0, 3, 0, 2, 1, 1, 0, 0), 4),
            ((4, 4, 4, 0), (0, 0, 3, 1, 2, 1, 0, 0), 4), ((4, 4, 4, 0), (0, 4294967295, 0, 2, 1, 1, 0, 0), 4), ((4, 4, 4, 0), (0, 0, 2, 1, 4294967295, 1, 0, 0), 4),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 0, 0, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 65, 0, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 4, 0), 4),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 0x80000001, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 0, 1), 4),
            ((4, 4, 4, 0), good, 1), ((4, 4, 4, 0), good, 2), ((4, 4, 4, 0), good, 5), ((4, 4, 4, 0), good, -3)]
    for d, t, ch in zero:
        tw, th = ctypes.c_uint(77), ctypes.c_uint(78)
        assert lib.qoimi_tile_size(ctypes.byref(api.QoiDesc(*d)), ctypes.byref(api.QoimiTile(*t)), ch, ctypes.byref(tw), ctypes.byref(th)) == 0, (d, t, ch)
        assert (tw.value, th.value) == (77, 78)
        assert tiles.size(d[0], d[1], d[2], t, ch)[0] == 0 or d[3] == 2
    assert lib.qoimi_tile_size(None, ctypes.byref(api.QoimiTile(*good)), 4, None, None) == 0
    assert lib.qoimi_tile_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), None, 4, None, None) == 0
    assert lib.qoimi_tile_size(ctypes.byref(api.QoiDesc(4, 4, 3, 1)), ctypes.byref(api.QoimiTile(*good)), 0, None, None) == 12
    assert api.tile_size(4, 4, 4, (0, -1, 0, 1, 1, 1), 4) == (0, 0, 0)
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_tile_stats(None, out)                                      # no context: zeros
    assert list(out) == [0, 0, 0, 0]


def test_tile_pyramid():
    lib = api.load_library()
    for (w, h, tw, th, levels) in [(300, 200, 64, 48, 4), (1, 1, 1, 1, 7), (257, 129, 64, 48, 4), (16384, 16384, 256, 256, 4), (5, 3, 1 << 24, 1 << 24, 7),
                                   (150, 90, 64, 64, 3), (37, 29, 7, 5, 1)]:
        got = api.tile_pyramid(w, h, 4, tw, th, levels)
        assert [tiles.fields(t) for t in got] == tiles.pyramid(w, h, tw, th, levels), (w, h, tw, th, levels)
    d = api.QoiDesc(300, 200, 3, 0)
    n = lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 48, 4, None, 0)
    assert n == len(tiles.pyramid(300, 200, 64, 48, 4)) == 25 + 9 + 4 + 1
    arr = (api.QoimiTile * (n + 1))()
    ctypes.memset(arr, 0x5A, ctypes.sizeof(arr))
    bad = {"rejected descriptor": lambda: lib.qoimi_tile_pyramid(ctypes.byref(api.QoiDesc(0, 200, 3, 0)), 64, 48, 4, None, 0),
           "NULL descriptor": lambda: lib.qoimi_tile_pyramid(None, 64, 48, 4, None, 0),
           "pixel cap": lambda: lib.qoimi_tile_pyramid(ctypes.byref(api.QoiDesc(20000, 20000, 3, 0)), 64, 48, 4, None, 0),
           "tile_w 0": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 0, 48, 4, None, 0),
           "tile_h 0": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 0, 4, None, 0),
           "tile_w above 2^24": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), (1 << 24) + 1, 48, 4, None, 0),
           "tile_h above 2^24": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 0xFFFFFFFF, 4, None, 0),
           "levels 0": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 48, 0, None, 0),
           "levels 8": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 48, 8, None, 0),
           "cap too small": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 48, 4, arr, n - 1),
           "cap negative": lambda: lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 48, 4, arr, -1)}
    for name, f in bad.items():
        assert f() == E_ARG, name
        assert api.last_error() != "", name
    assert bytes(arr) == b"\x5A" * ctypes.sizeof(arr)
    assert lib.qoimi_tile_pyramid(ctypes.byref(d), 64, 48, 4, arr, n) == n
    assert bytes(arr[n]) == b"\x5A" * 32 and tiles.fields(arr[n - 1]) == (0, 0, 0, 300, 200, 8, 0, 0)
    with pytest.raises(api.QoiError):
        api.tile_pyramid(300, 200, 3, 64, 48, 9)
    # 19999 x 20000 in tiles of 1 x 1 over two levels: 2^31 - 1 tiles or fewer? 399 980 000 + 100 000 000 - far below; the limit cannot be
    # reached by an accepted descriptor (fewer than 400 000 000 pixels a level, 7 levels at most), so the count always fits an int
    assert lib.qoimi_tile_pyramid(ctypes.byref(api.QoiDesc(19999, 20000, 3, 0)), 1, 1, 7, None, 0) == sum(
        -(-19999 // (1 << l)) * -(-20000 // (1 << l)) for l in range(7))


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


def test_rejections(args):
    a = args

    def call(ctx=a.ctx, px=a.p, po=a.po, descs=a.descs, n=3, ch=0, tiles_=a.tiles, nt=2, mode=0, align=1, pack=a.pack, cap=1024, off=a.off, ln=a.len, staging=0):
        return a.lib.qoimi_encode_tiles(ctx, px, po, descs, n, ch, tiles_, nt, mode, align, pack, cap, off, ln, staging, a.h_off, a.h_len, a.h_desc, None)

    def d3(*last):
        return (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(*last))

    ok0 = (0, 1, 1, 2, 2, 1, 0, 0)
    calls = {
        "NULL ctx": (lambda: call(ctx=None), "NULL"), "NULL d_pixels": (lambda: call(px=None), "NULL"), "NULL pixel_offsets": (lambda: call(po=None), "NULL"),
        "NULL descs": (lambda: call(descs=None), "NULL"), "NULL tiles": (lambda: call(tiles_=None), "NULL"),
        "NULL d_packed_off": (lambda: call(off=None), "NULL"), "NULL d_stream_len": (lambda: call(ln=None), "NULL"),
        "n_images 0": (lambda: call(n=0), "empty"), "n_images -1": (lambda: call(n=-1), "empty"), "n_tiles 0": (lambda: call(nt=0), "empty"), "n_tiles -1": (lambda: call(nt=-1), "empty"),
        "NULL d_packed with a capacity": (lambda: call(pack=None), "NULL"),
        "align 0": (lambda: call(align=0), "align"), "align 3": (lambda: call(align=3), "align"), "align 512": (lambda: call(align=512), "align"),
        "channels 1": (lambda: call(ch=1), "channels"), "channels 2": (lambda: call(ch=2), "channels"), "channels 5": (lambda: call(ch=5), "channels"), "channels -3": (lambda: call(ch=-3), "channels"),
        "mode 2": (lambda: call(mode=2), "mode"), "mode -1": (lambda: call(mode=-1), "mode"),
        "image == n_images": (lambda: call(tiles_=tl(ok0, (3, 0, 0, 1, 1, 1, 0, 0))), "no image 3"),
        "image 2^32-1": (lambda: call(tiles_=tl(ok0, (4294967295, 0, 0, 1, 1, 1, 0, 0))), "no image"),
        "image beyond a shorter n_images": (lambda: call(n=2), "no image 2"),
        "now image 1 is named": (lambda: call(tiles_=tl(ok0, (1, 0, 0, 1, 1, 1, 0, 0))), "descriptor 1"),
        "width 0": (lambda: call(tiles_=tl(ok0, (2, 0, 0, 0, 1, 1, 0, 0))), "zero"), "height 0": (lambda: call(tiles_=tl((0, 0, 0, 1, 0, 1, 0, 0), ok0)), "zero"),
        "one column outside": (lambda: call(tiles_=tl(ok0, (2, 1, 0, 5, 1, 1, 0, 0))), "leaves"), "one row outside": (lambda: call(tiles_=tl(ok0, (2, 0, 1, 5, 3, 1, 0, 0))), "leaves"),
        "x == width": (lambda: call(tiles_=tl(ok0, (2, 5, 0, 1, 1, 1, 0, 0))), "leaves"),
        "x + width wraps in 32 bits": (lambda: call(tiles_=tl(ok0, (2, 4294967295, 0, 2, 1, 1, 0, 0))), "leaves"),
        "y + height wraps in 32 bits": (lambda: call(tiles_=tl(ok0, (2, 0, 2, 1, 4294967295, 1, 0, 0))), "leaves"),
        "factor 0": (lambda: call(tiles_=tl(ok0, (2, 0, 0, 5, 3, 0, 0, 0))), "factor"), "factor 65": (lambda: call(tiles_=tl((0, 0, 0, 4, 4, 65, 0, 0), ok0)), "factor"),
        "flag bit 2": (lambda: call(tiles_=tl(ok0, (2, 0, 0, 5, 1, 1, 4, 0))), "flag"), "flag bit 31": (lambda: call(tiles_=tl((0, 1, 1, 2, 2, 1, 0x80000000, 0), ok0)), "flag"),
        "reserved 1": (lambda: call(tiles_=tl(ok0, (2, 0, 0, 5, 1, 1, 0, 1))), "reserved"),
        "image offset wraps the address space": (lambda: call(po=(ctypes.c_size_t * 3)(1, 0, 2 ** 64 - 8)), "address space"),
        "image end wraps the address space": (lambda: call(po=(ctypes.c_size_t * 3)(1, 0, 2 ** 64 - a.p - 44)), "address space"),
        "image 0 overlaps the pack's first byte": (lambda: call(po=(ctypes.c_size_t * 3)(4096 - 63, 0, 2051)), "overlap"),
        "image 2 overlaps the pack's last byte": (lambda: call(po=(ctypes.c_size_t * 3)(1, 0, 4096 + 1023)), "overlap"),
        "the pack inside image 0": (lambda: call(pack=a.p + 17, cap=8), "overlap"),
    }
    for name, f in REJECTED_DESCS.items():
        calls["descriptor: " + name] = ((lambda f_: lambda: call(descs=d3(*f_), staging=1))(f), "descriptor 2")
        calls["descriptor with channels given: " + name] = ((lambda f_: lambda: call(descs=d3(*f_), ch=3))(f), "descriptor 2")
    for name, (c, cause) in calls.items():
        assert c() == E_ARG, name
        assert cause in api.last_error(), (name, api.last_error())
        assert untouched(a), name


def test_what_is_not_rejected_is_not_rejected_for_the_wrong_reason(args):
    """an image that ends one byte in front of the pack, or begins right behind it, does not overlap it: such calls get as far as the
    context - which this test must not do, so it is the tile limit below that stops them"""
    a = args
    w, h = 19999, 20000
    n = 5600
    tiles_per = -(-(-(-w * h * 4 // 16)) // 256)
    assert tiles_per * n >= 2 ** 31 - 1 > tiles_per * 5400
    descs = (api.QoiDesc * 1)(api.QoiDesc(w, h, 4, 0))
    many = (api.QoimiTile * n)(*[api.QoimiTile(0, 0, 0, w, h, 1, j & 3, 0) for j in range(n)])
    for pack, cap in ((a.p - 64, 64), (a.p + w * h * 4, 64), (None, 0)):
        # (staging of 2^60 bytes: the plan puts all 5600 tiles into one sub-batch)
        rc = a.lib.qoimi_encode_tiles(a.ctx, a.p, (ctypes.c_size_t * 1)(0), descs, 1, 0, many, n, 0, 1, pack, cap, a.off, a.len, 1 << 60, a.h_off, a.h_len, a.h_desc, None)
        assert rc == E_ARG and "tiles" in api.last_error() and "overlap" not in api.last_error()
        assert untouched(a)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    with pytest.raises(api.QoiError):
        ctx.encode_tiles(1, [0], d, 0, [(0, 0, 0, 1, 1, 1)], 0, 1, 1, 64, 1, 1)
    with pytest.raises(api.QoiError):
        ctx.encode_tiles(1, [0, 16], d, 0, [(0, 0, 0, 1, 1)], 0, 1, 1, 64, 1, 1)
    with pytest.raises(api.QoiError):
        ctx.encode_tiles(1, [0, 16], d, 0, [(0, 0, 0, 1, 1, -1)], 0, 1, 1, 64, 1, 1)
