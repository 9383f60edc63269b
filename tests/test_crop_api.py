"""qoimi_decode_crops / qoimi_crop_size / qoimi_crop_stats, what can be checked without a GPU: the three entry points in every layer, the
structure's layout, the size arithmetic, and every QOIMI_E_ARG case - all of them are reported before the context or the device is looked at,
so a block of zeroed host memory stands in for a context here and host arrays for device buffers; the output keeps its bytes.  And the tile
grid of tools/qoitile_mi355x.py."""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, crops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_decode_crops", "qoimi_crop_size", "qoimi_crop_stats")
E_ARG = -1


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_decode_crops\s*\(", header)
    assert re.search(r"\bsize_t\s+qoimi_crop_size\s*\(", header)
    assert re.search(r"\bvoid\s+qoimi_crop_stats\s*\(", header)
    assert "QOIMI_CROP_FLIP_X = 1" in header and "QOIMI_CROP_FLIP_Y = 2" in header and re.search(r"\}\s*qoimi_crop\s*;", header)
    assert (crops.FLIP_X, crops.FLIP_Y) == (1, 2)
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("decode_crops", "crop_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.crop_size)


def test_the_gather_kernel_has_no_timer_entry():
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert not any("crop" in n for n in names)


def test_struct_layout():
    assert ctypes.sizeof(api.QoimiCrop) == 24
    assert [(f, getattr(api.QoimiCrop, f).offset) for f, _ in api.QoimiCrop._fields_] == [("image", 0), ("x", 4), ("y", 8), ("width", 12), ("height", 16), ("flags", 20)]
    c = api.QoimiCrop(1, 2, 3, 4, 5, 3)
    assert bytes(c) == b"".join(v.to_bytes(4, "little") for v in (1, 2, 3, 4, 5, 3))
    assert crops.fields(c) == (1, 2, 3, 4, 5, 3)


def test_crop_size():
    lib = api.load_library()
    for (w, h) in [(1, 1), (37, 23), (3840, 2160), (19999, 20000), (4, 99999999)]:
        for rect in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, w, h), (w // 2, h // 3, w - w // 2, h - h // 3), (0, h - 1, w, 1)]:
            for flags in range(4):
                for ch_in in (3, 4):
                    for ch in (3, 4):
                        want = crops.size(w, h, rect, flags, ch)
                        assert want == rect[2] * rect[3] * ch
                        assert api.crop_size(w, h, ch_in, (7,) + rect + (flags,), ch) == want, (w, h, rect, flags, ch)      # (crop.image is not looked at)
    assert api.crop_size(19999, 20000, 4, api.QoimiCrop(0, 0, 0, 19999, 20000, 0), 4) == 19999 * 20000 * 4 > 2 ** 32 // 4
    # the zero returns: a rejected descriptor, an empty rectangle, one that leaves the image (also where 32-bit sums would wrap), an
    # unknown flag bit, channels not 3 / 4 (0 is not an output channel count here)
    good = (0, 1, 1, 2, 2, 0)
    zero = [((0, 4, 4, 0), good, 4), ((4, 0, 4, 0), good, 4), ((4, 4, 2, 0), good, 4), ((4, 4, 5, 0), good, 4), ((4, 4, 4, 2), good, 4), ((20000, 20000, 4, 0), good, 4),
            ((4, 4, 4, 0), (0, 0, 0, 0, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 0, 0), 4), ((4, 4, 4, 0), (0, 3, 0, 2, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 3, 1, 2, 0), 4),
            ((4, 4, 4, 0), (0, 4, 0, 1, 1, 0), 4), ((4, 4, 4, 0), (0, 4294967295, 0, 2, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 2, 1, 4294967295, 0), 4),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 4), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 0x80000001), 4),
            ((4, 4, 4, 0), good, 0), ((4, 4, 4, 0), good, 2), ((4, 4, 4, 0), good, 5), ((4, 4, 4, 0), good, -3)]
    for d, c, ch in zero:
        assert lib.qoimi_crop_size(ctypes.byref(api.QoiDesc(*d)), ctypes.byref(api.QoimiCrop(*c)), ch) == 0, (d, c, ch)
    assert lib.qoimi_crop_size(None, ctypes.byref(api.QoimiCrop(*good)), 4) == 0
    assert lib.qoimi_crop_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), None, 4) == 0
    assert lib.qoimi_crop_size(ctypes.byref(api.QoiDesc(4, 4, 3, 1)), ctypes.byref(api.QoimiCrop(*good)), 3) == 12
    assert api.crop_size(4, 4, 4, (0, -1, 0, 1, 1, 0), 4) == 0
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_crop_stats(None, out)                                      # no context: zeros
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
    a.out = (ctypes.c_ubyte * 4096)()
    ctypes.memset(a.out, 0x5A, 4096)
    a.o = ctypes.addressof(a.out)
    a.n = 3
    a.so = (ctypes.c_size_t * 3)(0, 1024, 2048)
    a.sizes = (ctypes.c_int * 3)(40, 0, 40)                      # image 1 is named by no crop: its size and descriptor are garbage
    a.descs = (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(5, 3, 4, 1))
    a.crops = cr((0, 1, 1, 2, 2, 0), (2, 0, 0, 5, 1, 3))         # 16 and 20 bytes at 4 channels
    a.oo = (ctypes.c_size_t * 2)(0, 1024)
    return a


def cr(*rows):
    return (api.QoimiCrop * len(rows))(*[api.QoimiCrop(*r) for r in rows])


def untouched(a):
    return bytes(a.out) == b"\x5A" * 4096 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


def test_rejections(args):
    a = args

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, ch=0, crops_=a.crops, nc=2, out=a.o, oo=a.oo, staging=0):
        return a.lib.qoimi_decode_crops(ctx, streams, so, sizes, descs, n, ch, crops_, nc, out, oo, staging, None)

    def o2(x, y):
        return (ctypes.c_size_t * 2)(x, y)

    def d3(*last):
        return (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(*last))

    ok0 = (0, 1, 1, 2, 2, 0)
    calls = {
        "NULL ctx": lambda: call(ctx=None), "NULL d_streams": lambda: call(streams=None), "NULL stream_offsets": lambda: call(so=None),
        "NULL sizes": lambda: call(sizes=None), "NULL descs": lambda: call(descs=None), "NULL crops": lambda: call(crops_=None),
        "NULL d_out": lambda: call(out=None), "NULL out_offsets": lambda: call(oo=None),
        "n_images 0": lambda: call(n=0), "n_images -1": lambda: call(n=-1), "n_crops 0": lambda: call(nc=0), "n_crops -1": lambda: call(nc=-1),
        "channels 1": lambda: call(ch=1), "channels 2": lambda: call(ch=2), "channels 5": lambda: call(ch=5), "channels -3": lambda: call(ch=-3),
        "image == n_images": lambda: call(crops_=cr(ok0, (3, 0, 0, 1, 1, 0))), "image 2^32-1": lambda: call(crops_=cr(ok0, (4294967295, 0, 0, 1, 1, 0))),
        "image beyond a shorter n_images": lambda: call(n=2),
        "width 0": lambda: call(crops_=cr(ok0, (2, 0, 0, 0, 1, 0))), "height 0": lambda: call(crops_=cr((0, 0, 0, 1, 0, 0), (2, 0, 0, 5, 1, 0))),
        "one column outside": lambda: call(crops_=cr(ok0, (2, 1, 0, 5, 1, 0))), "one row outside": lambda: call(crops_=cr(ok0, (2, 0, 1, 5, 3, 0))),
        "x == width": lambda: call(crops_=cr(ok0, (2, 5, 0, 1, 1, 0))), "y == height": lambda: call(crops_=cr((0, 0, 4, 1, 1, 0), (2, 0, 0, 5, 1, 0))),
        "x + width wraps in 32 bits": lambda: call(crops_=cr(ok0, (2, 4294967295, 0, 2, 1, 0))),
        "y + height wraps in 32 bits": lambda: call(crops_=cr(ok0, (2, 0, 2, 1, 4294967295, 0))),
        "flag bit 2": lambda: call(crops_=cr(ok0, (2, 0, 0, 5, 1, 4))), "flag bit 31": lambda: call(crops_=cr((0, 1, 1, 2, 2, 0x80000000), (2, 0, 0, 5, 1, 0))),
        "referenced size 21": lambda: call(sizes=(ctypes.c_int * 3)(40, 0, 21)), "referenced size 0": lambda: call(sizes=(ctypes.c_int * 3)(0, 40, 40)),
        "referenced size negative": lambda: call(sizes=(ctypes.c_int * 3)(40, 40, -1)),
        "mixed channels": lambda: call(descs=d3(5, 3, 3, 0)), "mixed channels, 3 first": lambda: call(descs=(api.QoiDesc * 3)(api.QoiDesc(4, 4, 3, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(5, 3, 4, 0))),
        "outputs overlap by one byte": lambda: call(oo=o2(0, 15)), "outputs coincide": lambda: call(oo=o2(64, 64)),
        "outputs overlap, crop 1 in front": lambda: call(oo=o2(119, 100)),
        "outputs overlap with channels 3": lambda: call(ch=3, oo=o2(0, 11)),
        "output offset wraps the address space": lambda: call(oo=o2(0, 2 ** 64 - 8)), "output end wraps the address space": lambda: call(oo=o2(0, 2 ** 64 - a.o - 19)),
        "now image 1 is named": lambda: call(crops_=cr(ok0, (1, 0, 0, 1, 1, 0))),
    }
    for name, f in REJECTED_DESCS.items():
        calls["descriptor: " + name] = (lambda f_: lambda: call(descs=d3(*f_), staging=1))(f)
        calls["descriptor with channels given: " + name] = (lambda f_: lambda: call(descs=d3(*f_), ch=3))(f)
    for name, c in calls.items():
        assert c() == E_ARG, name
        assert api.last_error() != "", name
        assert untouched(a), name


def test_tile_limit_of_a_sub_batch(args):
    """5600 whole-image crops of a 19999 x 20000 image: 390 606 tiles each, 2^31 - 1 or more in the one sub-batch; 5400 of them stay
    below the limit, so that call would get as far as the context - which this test must not do"""
    a = args
    w, h = 19999, 20000
    B = w * h * 4
    tiles = -(-(-(-B // 16)) // 256)
    n = 5600
    assert tiles * n >= 2 ** 31 - 1 > tiles * 5400
    descs = (api.QoiDesc * 1)(api.QoiDesc(w, h, 4, 0))
    many = (api.QoimiCrop * n)(*[api.QoimiCrop(0, 0, 0, w, h, j & 3) for j in range(n)])
    oo = (ctypes.c_size_t * n)(*[j * B for j in range(n)])
    aligned = (a.o + 15) & ~15
    rc = a.lib.qoimi_decode_crops(a.ctx, a.p, (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(40), descs, 1, 4, many, n, aligned, oo, 0, None)
    assert rc == E_ARG and "tiles" in api.last_error()
    assert untouched(a)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    with pytest.raises(api.QoiError):
        ctx.decode_crops(1, [0], [40, 40], d, 0, [(0, 0, 0, 1, 1, 0)], 1, [0])
    with pytest.raises(api.QoiError):
        ctx.decode_crops(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1, 0)], 1, [0, 4])
    with pytest.raises(api.QoiError):
        ctx.decode_crops(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1, -1)], 1, [0])
    with pytest.raises(api.QoiError):
        ctx.decode_crops(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1)], 1, [0])


def test_tile_grid():
    from tools.qoitile_mi355x import tile_grid
    assert tile_grid(70, 50, 32) == [(0, 0, 0, 0, 32, 32), (0, 1, 32, 0, 32, 32), (0, 2, 64, 0, 6, 32),
                                     (1, 0, 0, 32, 32, 18), (1, 1, 32, 32, 32, 18), (1, 2, 64, 32, 6, 18)]
    assert tile_grid(64, 32, 32) == [(0, 0, 0, 0, 32, 32), (0, 1, 32, 0, 32, 32)]
    assert tile_grid(5, 3, 256) == [(0, 0, 0, 0, 5, 3)]
    assert tile_grid(3, 2, 1) == [(r, c, c, r, 1, 1) for r in range(2) for c in range(3)]
    for (w, h, t) in [(130, 70, 32), (16384, 16384, 256), (257, 9, 7)]:
        g = tile_grid(w, h, t)
        assert len(g) == -(-w // t) * -(-h // t) and sum(tw * th for (_, _, _, _, tw, th) in g) == w * h
        assert all(x == c * t and y == r * t and 1 <= tw <= t and 1 <= th <= t and x + tw <= w and y + th <= h for (r, c, x, y, tw, th) in g)
    with pytest.raises(ValueError):
        tile_grid(4, 4, 0)
