"""qoimi_pixel_stats / qoimi_pixel_stats_counters, what can be checked without a GPU: the two entry points in every layer, the structure's
layout, and every QOIMI_E_ARG case - all of them are reported before the context or the device is looked at, so a block of zeroed host memory
stands in for a context here and host arrays for device buffers; stats_out keeps its bytes."""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, pixelstats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_pixel_stats", "qoimi_pixel_stats_counters")
E_ARG = -1


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_pixel_stats\s*\(", header)
    assert re.search(r"\bvoid\s+qoimi_pixel_stats_counters\s*\(", header)
    assert re.search(r"\}\s*qoimi_pixel_stat\s*;", header)
    for name, value in (("CONSTANT", 1), ("OPAQUE", 2), ("TRANSPARENT", 4), ("GREY", 8)):
        assert f"QOIMI_PS_{name} = {value}" in header and getattr(pixelstats, name) == value
    assert header.index("qoimi_resize_stats(") < header.index("qoimi_pixel_stat;")
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("pixel_stats", "pixel_stats_counters"):
        assert callable(getattr(api.Context, method))


def test_the_reduction_kernel_has_no_timer_entry():
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert not any("stats" in n for n in names)


def test_struct_layout():
    S = api.QoimiPixelStat
    assert ctypes.sizeof(S) == 128
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("pixels", 0), ("sum", 8), ("sum_sq", 40), ("min", 72), ("max", 76), ("first", 80),
                                                                  ("flags", 84), ("opaque_pixels", 88), ("transparent_pixels", 96), ("grey_pixels", 104),
                                                                  ("reserved", 112)]
    s = S()
    s.pixels, s.first, s.flags, s.grey_pixels = 6, 0x04030201, 10, 5
    s.sum[2], s.sum_sq[3], s.min[1], s.max[0] = 7, 2 ** 44, 9, 250
    f = pixelstats.of_struct(s)
    assert set(f) == set(pixelstats.FIELDS)
    assert (f["pixels"], f["first"], f["flags"], f["grey_pixels"], f["sum"], f["sum_sq"][3], f["min"], f["max"]) == (6, 0x04030201, 10, 5, (0, 0, 7, 0), 2 ** 44, (0, 9, 0, 0), (250, 0, 0, 0))
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    api.load_library().qoimi_pixel_stats_counters(None, out)            # no context: zeros
    assert list(out) == [0, 0, 0, 0]


@pytest.fixture()
def args():
    class A:
        pass
    a = A()
    a.lib = api.load_library()
    a.fake_ctx = (ctypes.c_ubyte * (1 << 20))()                  # never looked at: every rejection comes first
    a.ctx = ctypes.addressof(a.fake_ctx)
    a.buf = (ctypes.c_ubyte * 4096)()
    a.p = ctypes.addressof(a.buf)
    a.out = (api.QoimiPixelStat * 8)()
    ctypes.memset(a.out, 0x5A, ctypes.sizeof(a.out))
    a.hist = (ctypes.c_ubyte * 8192)()
    ctypes.memset(a.hist, 0x5A, 8192)
    a.h = ctypes.addressof(a.hist)
    a.n = 3
    a.so = (ctypes.c_size_t * 3)(0, 1024, 2048)
    a.sizes = (ctypes.c_int * 3)(40, 0, 40)                      # image 1 is named by no region: its size and descriptor are garbage
    a.descs = (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(5, 3, 3, 1))   # (3 and 4 channels mix)
    a.regions = cr((0, 1, 1, 2, 2, 0), (2, 0, 0, 5, 1, 3))
    return a


def cr(*rows):
    return (api.QoimiCrop * len(rows))(*[api.QoimiCrop(*r) for r in rows])


def untouched(a):
    return (bytes(a.out) == b"\x5A" * ctypes.sizeof(a.out) and bytes(a.hist) == b"\x5A" * 8192 and bytes(a.buf) == b"\0" * 4096 and
            bytes(a.fake_ctx[:4096]) == b"\0" * 4096)


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


def test_rejections(args):
    a = args

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, regions=a.regions, nr=2, out=a.out, hist=None, staging=0):
        return a.lib.qoimi_pixel_stats(ctx, streams, so, sizes, descs, n, regions, nr, out, hist, staging, None)

    def d3(*last):
        return (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(*last))

    ok0 = (0, 1, 1, 2, 2, 0)
    calls = {
        "NULL ctx": lambda: call(ctx=None), "NULL d_streams": lambda: call(streams=None), "NULL stream_offsets": lambda: call(so=None),
        "NULL sizes": lambda: call(sizes=None), "NULL descs": lambda: call(descs=None), "NULL regions": lambda: call(regions=None),
        "NULL stats_out": lambda: call(out=None), "NULL ctx with a histogram": lambda: call(ctx=None, hist=a.h),
        "n_images 0": lambda: call(n=0), "n_images -1": lambda: call(n=-1), "n_regions 0": lambda: call(nr=0), "n_regions -1": lambda: call(nr=-1),
        "image == n_images": lambda: call(regions=cr(ok0, (3, 0, 0, 1, 1, 0))), "image 2^32-1": lambda: call(regions=cr(ok0, (4294967295, 0, 0, 1, 1, 0))),
        "image beyond a shorter n_images": lambda: call(n=2),
        "width 0": lambda: call(regions=cr(ok0, (2, 0, 0, 0, 1, 0))), "height 0": lambda: call(regions=cr((0, 0, 0, 1, 0, 0), (2, 0, 0, 5, 1, 0))),
        "one column outside": lambda: call(regions=cr(ok0, (2, 1, 0, 5, 1, 0))), "one row outside": lambda: call(regions=cr(ok0, (2, 0, 1, 5, 3, 0))),
        "x == width": lambda: call(regions=cr(ok0, (2, 5, 0, 1, 1, 0))), "y == height": lambda: call(regions=cr((0, 0, 4, 1, 1, 0), (2, 0, 0, 5, 1, 0))),
        "x + width wraps in 32 bits": lambda: call(regions=cr(ok0, (2, 4294967295, 0, 2, 1, 0))),
        "y + height wraps in 32 bits": lambda: call(regions=cr(ok0, (2, 0, 2, 1, 4294967295, 0))),
        "flag bit 2": lambda: call(regions=cr(ok0, (2, 0, 0, 5, 1, 4)), hist=a.h), "flag bit 31": lambda: call(regions=cr((0, 1, 1, 2, 2, 0x80000000), (2, 0, 0, 5, 1, 0))),
        "referenced size 21": lambda: call(sizes=(ctypes.c_int * 3)(40, 0, 21)), "referenced size 0": lambda: call(sizes=(ctypes.c_int * 3)(0, 40, 40)),
        "referenced size negative": lambda: call(sizes=(ctypes.c_int * 3)(40, 40, -1), hist=a.h),
        "now image 1 is named": lambda: call(regions=cr(ok0, (1, 0, 0, 1, 1, 0))),
    }
    for name, f in REJECTED_DESCS.items():
        calls["descriptor: " + name] = (lambda f_: lambda: call(descs=d3(*f_), staging=1))(f)
        calls["descriptor with a histogram: " + name] = (lambda f_: lambda: call(descs=d3(*f_), hist=a.h))(f)
    for name, c in calls.items():
        assert c() == E_ARG, name
        assert api.last_error() != "", name
        assert untouched(a), name


def test_tile_limit_of_a_sub_batch(args):
    """5600 whole-image regions of a 19999 x 20000 image: 390 606 tiles each, 2^31 - 1 or more in the one sub-batch; 5400 of them stay below the
    limit, so that call would get as far as the context - which this test must not do"""
    a = args
    w, h = 19999, 20000
    tiles = pixelstats.tiles(w, h)
    n = 5600
    assert tiles == 390606 and tiles * n >= 2 ** 31 - 1 > tiles * 5400
    descs = (api.QoiDesc * 1)(api.QoiDesc(w, h, 4, 0))
    many = (api.QoimiCrop * n)(*[api.QoimiCrop(0, 0, 0, w, h, j & 3) for j in range(n)])
    out = (api.QoimiPixelStat * n)()
    rc = a.lib.qoimi_pixel_stats(a.ctx, a.p, (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(40), descs, 1, many, n, out, None, 0, None)
    assert rc == E_ARG and "tiles" in api.last_error()
    assert bytes(out) == b"\0" * ctypes.sizeof(out) and untouched(a)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    with pytest.raises(api.QoiError):
        ctx.pixel_stats(1, [0], [40, 40], d, [(0, 0, 0, 1, 1, 0)])
    with pytest.raises(api.QoiError):
        ctx.pixel_stats(1, [0, 40], [40, 40], d, [(0, 0, 0, 1, 1, -1)])
    with pytest.raises(api.QoiError):
        ctx.pixel_stats(1, [0, 40], [40, 40], d, [(0, 0, 0, 1, 1)])
