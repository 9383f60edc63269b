"""qoimi_decode_thumbnails / qoimi_thumbnail_size / qoimi_thumbnail_stats, what can be checked without a GPU: the three entry points in every
layer, the size arithmetic, and every QOIMI_E_ARG case - all of them are reported before the context or the device is looked at, so a block
of zeroed host memory stands in for a context here and host arrays for device buffers; the output keeps its bytes."""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, thumbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_decode_thumbnails", "qoimi_thumbnail_size", "qoimi_thumbnail_stats")
E_ARG = -1


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_decode_thumbnails\s*\(", header)
    assert re.search(r"\bsize_t\s+qoimi_thumbnail_size\s*\(", header)
    assert re.search(r"\bvoid\s+qoimi_thumbnail_stats\s*\(", header)
    assert "QOIMI_THUMB_PLAIN = 0" in header and "QOIMI_THUMB_ALPHA_WEIGHTED = 1" in header
    assert (thumbs.PLAIN, thumbs.ALPHA_WEIGHTED) == (0, 1)
    for name in NEW:
        assert name in api.EXPORTS, name
        assert re.fullmatch(r"qoimi_[a-z_]+", name)
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("decode_thumbnails", "thumbnail_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.thumbnail_size)


def test_kernel_name_table_still_ends_behind_cmp_first():
    """the reduction kernel has no entry in the timer and name table: qoimi_thumbnail_stats counts its launches instead"""
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert names.index("cmp_first") == names.index("cmp_pixels") + 1 == names.index("decode_total") + 2
    assert all(n == "" for n in names[names.index("cmp_first") + 1:])
    assert not any("thumb" in n for n in names)


def test_thumbnail_size():
    lib = api.load_library()
    for (w, h, f) in [(1, 1, 1), (1, 1, 64), (5, 3, 2), (64, 64, 64), (65, 64, 64), (3840, 2160, 15), (3840, 2160, 1), (19999, 20000, 7), (4, 99999999, 64)]:
        tw, th = thumbs.size(w, h, f)
        for ch_in in (3, 4):
            for ch in (3, 4):
                assert api.thumbnail_size(w, h, ch_in, f, ch) == (tw * th * ch, tw, th), (w, h, f, ch_in, ch)
    # the zero returns: a rejected descriptor, a factor outside 1..64, channels not 3 / 4 (0 is not an output channel count here); tw / th keep their values
    zero = [((0, 4, 4, 0), 2, 4), ((4, 0, 4, 0), 2, 4), ((4, 4, 2, 0), 2, 4), ((4, 4, 5, 0), 2, 4), ((4, 4, 4, 2), 2, 4), ((20000, 20000, 4, 0), 2, 4),
            ((4, 4, 4, 0), 0, 4), ((4, 4, 4, 0), 65, 4), ((4, 4, 4, 0), 4294967295, 4), ((4, 4, 4, 0), 2, 0), ((4, 4, 4, 0), 2, 2), ((4, 4, 4, 0), 2, 5), ((4, 4, 4, 0), 2, -3)]
    for fields, f, ch in zero:
        tw, th = ctypes.c_uint(77), ctypes.c_uint(78)
        assert lib.qoimi_thumbnail_size(ctypes.byref(api.QoiDesc(*fields)), f, ch, ctypes.byref(tw), ctypes.byref(th)) == 0, (fields, f, ch)
        assert (tw.value, th.value) == (77, 78)
    assert lib.qoimi_thumbnail_size(None, 2, 4, None, None) == 0
    assert lib.qoimi_thumbnail_size(ctypes.byref(api.QoiDesc(5, 3, 3, 1)), 2, 3, None, None) == 3 * 2 * 3          # tw / th may be NULL
    assert api.thumbnail_size(0, 4, 4, 2, 4) == (0, 0, 0)
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_thumbnail_stats(None, out)                                 # no context: zeros
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
    a.n = 2
    a.so = (ctypes.c_size_t * 2)(0, 1024)
    a.to = (ctypes.c_size_t * 2)(0, 1024)
    a.sizes = (ctypes.c_int * 2)(40, 40)
    a.descs = (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(5, 3, 4, 1))
    a.factors = (ctypes.c_uint * 2)(2, 3)
    return a


def bad_descs(*fields):
    return (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(*fields))


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


def untouched(a):
    return bytes(a.out) == b"\x5A" * 4096 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096


def test_rejections(args):
    a = args

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, ch=0, factors=a.factors, mode=0, out=a.o, to=a.to, staging=0):
        return a.lib.qoimi_decode_thumbnails(ctx, streams, so, sizes, descs, n, ch, factors, mode, out, to, staging, None)

    def f2(x, y):
        return (ctypes.c_uint * 2)(x, y)

    def o2(x, y):
        return (ctypes.c_size_t * 2)(x, y)

    calls = {
        "NULL ctx": lambda: call(ctx=None), "NULL d_streams": lambda: call(streams=None), "NULL stream_offsets": lambda: call(so=None),
        "NULL sizes": lambda: call(sizes=None), "NULL descs": lambda: call(descs=None), "NULL factors": lambda: call(factors=None),
        "NULL d_thumbs": lambda: call(out=None), "NULL thumb_offsets": lambda: call(to=None),
        "n 0": lambda: call(n=0), "n -1": lambda: call(n=-1),
        "size 21": lambda: call(sizes=(ctypes.c_int * 2)(40, 21)), "size 0 first": lambda: call(sizes=(ctypes.c_int * 2)(0, 40)),
        "negative size": lambda: call(sizes=(ctypes.c_int * 2)(40, -1)),
        "channels 1": lambda: call(ch=1), "channels 2": lambda: call(ch=2), "channels 5": lambda: call(ch=5), "channels -3": lambda: call(ch=-3),
        "mixed output channels": lambda: call(descs=(api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(5, 3, 3, 0))),
        "mixed output channels, 3 first": lambda: call(descs=(api.QoiDesc * 2)(api.QoiDesc(4, 4, 3, 0), api.QoiDesc(5, 3, 4, 0))),
        "factor 0": lambda: call(factors=f2(2, 0)), "factor 65": lambda: call(factors=f2(65, 2)), "factor 2^32-1": lambda: call(factors=f2(2, 4294967295)),
        "mode 2": lambda: call(mode=2), "mode -1": lambda: call(mode=-1),
        # 4 x 4 x 4 at f = 2 is 2 x 2 x 4 = 16 bytes, 5 x 3 x 4 at f = 3 is 2 x 1 x 4 = 8 bytes
        "outputs overlap by one byte": lambda: call(to=o2(0, 15)), "outputs coincide": lambda: call(to=o2(64, 64)),
        "outputs overlap, image 1 in front": lambda: call(to=o2(107, 100)),
        "outputs overlap with channels 3": lambda: call(ch=3, to=o2(0, 11)),
    }
    for name, fields in REJECTED_DESCS.items():
        calls["descriptor: " + name] = (lambda f: lambda: call(descs=bad_descs(*f), staging=1))(fields)
        calls["descriptor with channels given: " + name] = (lambda f: lambda: call(descs=bad_descs(*f), ch=3))(fields)
    for name, c in calls.items():
        assert c() == E_ARG, name
        assert api.last_error() != "", name
        assert untouched(a), name
    # the same ranges side by side are no overlap: those calls get as far as the context (a zeroed block - not a GPU), which this test
    # must not do; that they are accepted is shown on the GPU (tests/test_gpu_thumbnails.py: placement)


def test_python_wrapper_checks_its_lengths():
    """one offset, size, descriptor, factor per image: the wrapper says so before the C call reads past a short array"""
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    with pytest.raises(api.QoiError):
        ctx.decode_thumbnails(1, [0], [40, 40], d, 0, 2, 0, 1, [0, 16])
    with pytest.raises(api.QoiError):
        ctx.decode_thumbnails(1, [0, 40], [40, 40], d, 0, [2], 0, 1, [0, 16])
    with pytest.raises(api.QoiError):
        ctx.decode_thumbnails(1, [0, 40], [40, 40], d, 0, [2, 2], 0, 1, [0])
    with pytest.raises(api.QoiError):
        ctx.decode_thumbnails(1, [0, 40], [40, 40], d, 0, [2, -1], 0, 1, [0, 16])
