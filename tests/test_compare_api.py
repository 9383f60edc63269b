"""qoimi_compare_images / qoimi_verify_images, what can be checked without a GPU: the record layout, both entry points in every layer, and
every QOIMI_E_ARG case - all of them are reported before the context or the device is looked at, so a block of zeroed host memory stands in
for a context here and host arrays for device buffers; the output array keeps its bytes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from qoi_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_compare_images", "qoimi_verify_images")
E_ARG = -1


def test_record_layout():
    assert ctypes.sizeof(api.ImageDiff) == 32
    D = api.ImageDiff
    assert (D.mismatched.offset, D.first.offset, D.want.offset, D.got.offset, D.flags.offset, D.reserved.offset) == (0, 8, 16, 20, 24, 28)
    assert (D.mismatched.size, D.first.size, D.want.size, D.got.size, D.flags.size) == (8, 8, 4, 4, 4)


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    for name in NEW:
        assert name in api.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert "QOIMI_DIFF_PIXELS = 1" in header and "QOIMI_DIFF_HEADER = 2" in header
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("compare_images", "verify_images"):
        assert callable(getattr(api.Context, method))
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert names.index("cmp_first") == names.index("cmp_pixels") + 1 == names.index("decode_total") + 2      # appended: earlier indices stay
    assert names[names.index("cmp_first") + 1] == ""


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
    a.n = 2
    a.offs = (ctypes.c_size_t * 2)(0, 1024)
    a.sizes = (ctypes.c_int * 2)(40, 40)
    a.descs = (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(5, 3, 3, 1))
    a.out = (api.ImageDiff * 2)()
    ctypes.memset(a.out, 0x5A, ctypes.sizeof(a.out))
    a.first = ctypes.c_int(7)
    return a


def bad_descs(*fields):
    return (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(*fields))


REJECTED_DESCS = {"width 0": (0, 3, 3, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


def untouched(a):
    return bytes(a.out) == b"\x5A" * ctypes.sizeof(a.out) and a.first.value == 7 and bytes(a.buf) == b"\0" * 4096


def test_compare_rejections(args):
    a = args

    def call(ctx=a.ctx, da=a.p, ao=a.offs, ach=0, db=a.p, bo=a.offs, bch=0, descs=a.descs, n=a.n, out=a.out):
        return a.lib.qoimi_compare_images(ctx, da, ao, ach, db, bo, bch, descs, n, out, ctypes.byref(a.first), None)

    calls = {
        "NULL ctx": lambda: call(ctx=None), "NULL d_a": lambda: call(da=None), "NULL d_b": lambda: call(db=None),
        "NULL a_offsets": lambda: call(ao=None), "NULL b_offsets": lambda: call(bo=None), "NULL descs": lambda: call(descs=None),
        "NULL diffs_out": lambda: call(out=None), "n 0": lambda: call(n=0), "n -1": lambda: call(n=-1),
        "a_channels 1": lambda: call(ach=1), "a_channels 2": lambda: call(ach=2), "a_channels 5": lambda: call(ach=5), "a_channels -3": lambda: call(ach=-3),
        "b_channels 1": lambda: call(bch=1), "b_channels 2": lambda: call(bch=2), "b_channels 5": lambda: call(bch=5), "b_channels -4": lambda: call(bch=-4),
    }
    for name, fields in REJECTED_DESCS.items():
        calls["descriptor: " + name] = (lambda f: lambda: call(descs=bad_descs(*f)))(fields)
        calls["descriptor with channels given: " + name] = (lambda f: lambda: call(descs=bad_descs(*f), ach=4, bch=3))(fields)
    for name, c in calls.items():
        assert c() == E_ARG, name
        assert api.last_error() != "", name
        assert untouched(a), name


def test_verify_rejections(args):
    a = args

    def call(ctx=a.ctx, px=a.p, po=a.offs, descs=a.descs, n=a.n, streams=a.p, so=a.offs, sizes=a.sizes, staging=0, out=a.out):
        return a.lib.qoimi_verify_images(ctx, px, po, descs, n, streams, so, sizes, staging, out, ctypes.byref(a.first), None)

    calls = {
        "NULL ctx": lambda: call(ctx=None), "NULL d_pixels": lambda: call(px=None), "NULL pixel_offsets": lambda: call(po=None),
        "NULL descs": lambda: call(descs=None), "NULL d_streams": lambda: call(streams=None), "NULL stream_offsets": lambda: call(so=None),
        "NULL sizes": lambda: call(sizes=None), "NULL diffs_out": lambda: call(out=None), "n 0": lambda: call(n=0), "n -5": lambda: call(n=-5),
        "negative size": lambda: call(sizes=(ctypes.c_int * 2)(40, -1)), "negative size first": lambda: call(sizes=(ctypes.c_int * 2)(-2147483648, 40)),
    }
    for name, fields in REJECTED_DESCS.items():
        calls["descriptor: " + name] = (lambda f: lambda: call(descs=bad_descs(*f), staging=1))(fields)
    for name, c in calls.items():
        assert c() == E_ARG, name
        assert api.last_error() != "", name
        assert untouched(a), name


def test_python_wrappers_check_their_lengths():
    """one offset per side / stream and descriptor: the wrapper says so before the C call reads past a short array"""
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    with pytest.raises(api.QoiError):
        ctx.compare_images(1, [0], 0, 1, [0, 16], 0, d)
    with pytest.raises(api.QoiError):
        ctx.verify_images(1, [0, 16], d, 1, [0, 40], [40])
    assert np.dtype(np.uintp).itemsize == ctypes.sizeof(ctypes.c_size_t)
