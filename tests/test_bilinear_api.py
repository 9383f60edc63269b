"""qoimi_decode_bilinear / qoimi_decode_bilinear_indexed / qoimi_bilinear_size / qoimi_bilinear_stats, what can be checked without a GPU: the
four entry points in every layer, the header's statement of the definition, the reuse of qoimi_resize, the size arithmetic against
qoi_amd/bilinear.py: size, and every QOIMI_E_ARG case with the word qoimi_last_error names it by - all of them are reported before the context
or the device is looked at, so a block of zeroed host memory stands in for a context here and host arrays for device buffers; the output keeps
its bytes.  (What the library does behind the rejections needs a device: tests/test_gpu_bilinear.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, bilinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_decode_bilinear", "qoimi_decode_bilinear_indexed", "qoimi_bilinear_size", "qoimi_bilinear_stats")
E_ARG = -1


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_decode_bilinear\s*\(", header) and re.search(r"\bint\s+qoimi_decode_bilinear_indexed\s*\(", header)
    assert re.search(r"\bsize_t\s+qoimi_bilinear_size\s*\(", header) and re.search(r"\bvoid\s+qoimi_bilinear_stats\s*\(", header)
    # the definition in full, the model named as normative, the two limits
    for text in ("qoi_amd/bilinear.py", "normative", "(2k + 1) * n_out", "(2X + 1) * n_src", "rad = 2 * max(n_src, n_out)", "renormalised", "D(X, Y) = Wx(X) * Wy(Y)",
                 "(N_c + D/2) / D", "width <= 32 * out_width", "< 2^30", "antialias=True", "SYNCHRONOUS"):
        assert text in header, text
    # the item structure, the flags and the modes are those of qoimi_decode_resized: nothing new is declared
    assert len(re.findall(r"\}\s*qoimi_resize\s*;", header)) == 1 and "QOIMI_BILINEAR_" not in header and "qoimi_bilinear;" not in header
    lib = api.load_library()
    assert lib.qoimi_decode_bilinear.argtypes == lib.qoimi_decode_resized.argtypes
    assert lib.qoimi_decode_bilinear_indexed.argtypes == lib.qoimi_decode_resized_indexed.argtypes
    assert lib.qoimi_bilinear_size.argtypes == lib.qoimi_resize_size.argtypes
    assert (bilinear.FLIP_X, bilinear.FLIP_Y, bilinear.PLAIN, bilinear.ALPHA_WEIGHTED, bilinear.MAX_RATIO) == (1, 2, 0, 1, 32)
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("decode_bilinear", "decode_bilinear_indexed", "bilinear_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.bilinear_size)


def test_the_filter_kernel_is_built_without_scratch_and_has_no_timer_entry():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "bilinear_filter" in k]
    assert len(hits) == 1, hits
    assert ks[hits[0]]["scratch"] == 0 and ks[hits[0]]["vgpr_spills"] == 0 and ks[hits[0]]["lds"] == 0, ks[hits[0]]
    lib = api.load_library()
    assert not any("bilinear" in lib.qoimi_kernel_name(i).decode() for i in range(64))


def test_bilinear_size():
    lib = api.load_library()
    for (w, h) in [(1, 1), (37, 23), (3840, 2160), (19999, 20000), (4, 99999999)]:
        for rect in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, min(w, 64), min(h, 128)), (w // 2, h // 3, min(w - w // 2, 50), min(h - h // 3, 7))]:
            for out in [(1, 2), (2, 4), (224, 224), (rect[2], rect[3]), (32768, 32767), (32768, 32768), (1 << 23, 127), (1 << 23, 128)]:
                for flags in range(4):
                    for ch in (3, 4):
                        want = bilinear.size(w, h, rect, out, flags, ch)
                        assert api.bilinear_size(w, h, 7 - ch, (7,) + rect + out + (flags,), ch) == want, (w, h, rect, out, flags, ch)   # (item.image is not looked at)
    # the ratio limit, exactly and one beyond, per axis; the product limit, just below and exactly
    assert api.bilinear_size(4096, 4096, 4, (0, 0, 0, 2048, 2048, 64, 64, 0), 4) == 64 * 64 * 4
    assert api.bilinear_size(4096, 4096, 4, (0, 0, 0, 2049, 64, 64, 2, 0), 4) == 0 and api.bilinear_size(4096, 4096, 4, (0, 0, 0, 64, 2049, 2, 64, 0), 4) == 0
    assert api.bilinear_size(130, 70, 4, (0, 0, 0, 33, 1, 1, 1, 0), 4) == 0 and api.bilinear_size(130, 70, 4, (0, 0, 0, 32, 1, 1, 1, 0), 4) == 4
    assert api.bilinear_size(4, 4, 4, (0, 0, 0, 1, 1, 32768, 32767, 0), 3) == 32768 * 32767 * 3 and api.bilinear_size(4, 4, 4, (0, 0, 0, 1, 1, 32768, 32768, 0), 3) == 0
    assert api.bilinear_size(40000, 9000, 4, (0, 0, 0, 40000, 9000, 40000, 26843, 0), 3) == 40000 * 26843 * 3      # 40000 * 26843 < 2^30 <= 40000 * 26844
    assert api.bilinear_size(40000, 9000, 4, (0, 0, 0, 40000, 9000, 40000, 26844, 0), 3) == 0 and api.bilinear_size(40000, 27000, 4, (0, 0, 0, 40000, 26844, 1250, 839, 0), 3) == 0
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    zero = [((0, 4, 4, 0), good, 4), ((4, 4, 2, 0), good, 4), ((4, 4, 4, 2), good, 4), ((20000, 20000, 4, 0), good, 4),
            ((4, 4, 4, 0), (0, 0, 0, 0, 1, 1, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 0, 1, 0), 4), ((4, 4, 4, 0), (0, 3, 0, 2, 1, 2, 1, 0), 4),
            ((4, 4, 4, 0), (0, 4294967295, 0, 2, 1, 2, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 1, 4), 4), ((4, 4, 4, 0), good, 0), ((4, 4, 4, 0), good, 5),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 4294967295, 4294967295, 0), 4)]
    for d, r, ch in zero:
        assert lib.qoimi_bilinear_size(ctypes.byref(api.QoiDesc(*d)), ctypes.byref(api.QoimiResize(*r)), ch) == 0, (d, r, ch)
    assert lib.qoimi_bilinear_size(None, ctypes.byref(api.QoimiResize(*good)), 4) == 0
    assert lib.qoimi_bilinear_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), None, 4) == 0
    assert lib.qoimi_bilinear_size(ctypes.byref(api.QoiDesc(4, 4, 3, 1)), ctypes.byref(api.QoimiResize(*good)), 3) == 45
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_bilinear_stats(None, out)                                  # no context: zeros
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
    a.sizes = (ctypes.c_int * 3)(40, 0, 40)                      # image 1 is named by no item: its size and descriptor are garbage
    a.descs = (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(130, 3, 4, 1))
    a.items = rs((0, 1, 1, 2, 2, 2, 2, 0), (2, 0, 0, 130, 1, 5, 1, 3))     # 16 and 20 bytes at 4 channels
    a.oo = (ctypes.c_size_t * 2)(0, 1024)
    a.ks = (ctypes.c_uint * 3)(32, 0, 1)
    a.points = (ctypes.c_ubyte * 4096)()
    a.pf = (ctypes.c_size_t * 3)(0, 0, 0)
    return a


def rs(*rows):
    return (api.QoimiResize * len(rows))(*[api.QoimiResize(*r) for r in rows])


def untouched(a):
    return bytes(a.out) == b"\x5A" * 4096 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


@pytest.mark.parametrize("indexed", [False, True])
def test_rejections(args, indexed):
    a = args

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, ch=0, items=a.items, ni=2, mode=0, out=a.o, oo=a.oo, staging=0, ks=a.ks, points=a.points, pf=a.pf):
        if indexed:
            return a.lib.qoimi_decode_bilinear_indexed(ctx, streams, so, sizes, descs, n, ch, items, ni, mode, out, oo, staging, None, ks, None if points is None else ctypes.cast(points, a.lib.qoimi_decode_bilinear_indexed.argtypes[15]), pf)
        return a.lib.qoimi_decode_bilinear(ctx, streams, so, sizes, descs, n, ch, items, ni, mode, out, oo, staging, None)

    def o2(x, y):
        return (ctypes.c_size_t * 2)(x, y)

    def d3(*last):
        return (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(*last))

    ok0 = (0, 1, 1, 2, 2, 2, 2, 0)
    ok2 = (2, 0, 0, 130, 1, 5, 1, 0)
    calls = {
        "NULL ctx": (lambda: call(ctx=None), "NULL"), "NULL d_streams": (lambda: call(streams=None), "NULL"), "NULL stream_offsets": (lambda: call(so=None), "NULL"),
        "NULL sizes": (lambda: call(sizes=None), "NULL"), "NULL descs": (lambda: call(descs=None), "NULL"), "NULL items": (lambda: call(items=None), "NULL"),
        "NULL d_out": (lambda: call(out=None), "NULL"), "NULL out_offsets": (lambda: call(oo=None), "NULL"),
        "n_images 0": (lambda: call(n=0), "empty"), "n_images -1": (lambda: call(n=-1), "empty"), "n_items 0": (lambda: call(ni=0), "empty"), "n_items -1": (lambda: call(ni=-1), "empty"),
        "channels 1": (lambda: call(ch=1), "channels"), "channels 5": (lambda: call(ch=5), "channels"), "channels -3": (lambda: call(ch=-3), "channels"),
        "mode 2": (lambda: call(mode=2), "mode"), "mode -1": (lambda: call(mode=-1), "mode"),
        "image == n_images": (lambda: call(items=rs(ok0, (3, 0, 0, 1, 1, 1, 1, 0))), "no image"), "image 2^32-1": (lambda: call(items=rs(ok0, (4294967295, 0, 0, 1, 1, 1, 1, 0))), "no image"),
        "image beyond a shorter n_images": (lambda: call(n=2), "no image"),
        "width 0": (lambda: call(items=rs(ok0, (2, 0, 0, 0, 1, 1, 1, 0))), "zero"), "height 0": (lambda: call(items=rs((0, 0, 0, 1, 0, 1, 1, 0), ok2)), "zero"),
        "out_width 0": (lambda: call(items=rs(ok0, (2, 0, 0, 5, 1, 0, 1, 0))), "zero"), "out_height 0": (lambda: call(items=rs((0, 0, 0, 1, 1, 1, 0, 0), ok2)), "zero"),
        "one column outside": (lambda: call(items=rs(ok0, (2, 1, 0, 130, 1, 130, 1, 0))), "leaves"), "one row outside": (lambda: call(items=rs(ok0, (2, 0, 1, 5, 3, 5, 3, 0))), "leaves"),
        "x == width": (lambda: call(items=rs(ok0, (2, 130, 0, 1, 1, 1, 1, 0))), "leaves"), "y == height": (lambda: call(items=rs((0, 0, 4, 1, 1, 1, 1, 0), ok2)), "leaves"),
        "x + width wraps in 32 bits": (lambda: call(items=rs(ok0, (2, 4294967295, 0, 2, 1, 2, 1, 0))), "leaves"),
        "y + height wraps in 32 bits": (lambda: call(items=rs(ok0, (2, 0, 2, 1, 4294967295, 1, 4294967295, 0))), "leaves"),
        "the ratio in x: 65 to 2": (lambda: call(items=rs(ok0, (2, 0, 0, 65, 1, 2, 1, 0))), "32"), "the ratio in x: 33 to 1": (lambda: call(items=rs(ok0, (2, 3, 0, 33, 3, 1, 3, 0))), "32"),
        "the ratio in y: 33 to 1": (lambda: call(descs=d3(5, 33, 4, 0), items=rs(ok0, (2, 0, 0, 5, 33, 5, 1, 0))), "32"),
        "the ratio of 64 the area filter takes": (lambda: call(items=rs(ok0, (2, 0, 0, 128, 1, 2, 1, 0))), "32"),
        "the product: 2^15 x 2^15": (lambda: call(items=rs(ok0, (2, 0, 0, 1, 1, 32768, 32768, 0))), "2^30"),
        "the product: 2^23 x 128": (lambda: call(items=rs((0, 0, 0, 4, 4, 1 << 23, 128, 0), ok2)), "2^30"),
        "the product by the source width": (lambda: call(descs=d3(40000, 3, 4, 0), items=rs(ok0, (2, 0, 0, 40000, 1, 1250, 26844, 0))), "2^30"),
        "flag bit 2": (lambda: call(items=rs(ok0, (2, 0, 0, 5, 1, 5, 1, 4))), "flag"), "flag bit 31": (lambda: call(items=rs((0, 1, 1, 2, 2, 2, 2, 0x80000000), ok2)), "flag"),
        "referenced size 21": (lambda: call(sizes=(ctypes.c_int * 3)(40, 0, 21)), "shorter"), "referenced size 0": (lambda: call(sizes=(ctypes.c_int * 3)(0, 40, 40)), "shorter"),
        "referenced size negative": (lambda: call(sizes=(ctypes.c_int * 3)(40, 40, -1)), "shorter"),
        "mixed channels": (lambda: call(descs=d3(130, 3, 3, 0)), "channel"),
        "outputs overlap by one byte": (lambda: call(oo=o2(0, 15)), "overlap"), "outputs coincide": (lambda: call(oo=o2(64, 64)), "overlap"),
        "outputs overlap, item 1 in front": (lambda: call(oo=o2(119, 100)), "overlap"), "outputs overlap with channels 3": (lambda: call(ch=3, oo=o2(0, 11)), "overlap"),
        "output offset wraps the address space": (lambda: call(oo=o2(0, 2 ** 64 - 8)), "address space"),
        "output end wraps the address space": (lambda: call(oo=o2(0, 2 ** 64 - a.o - 19)), "address space"),
        "now image 1 is named": (lambda: call(items=rs(ok0, (1, 0, 0, 1, 1, 1, 1, 0))), "shorter"),
    }
    if indexed:
        calls.update({"NULL interval_rows": (lambda: call(ks=None), "NULL"), "NULL points": (lambda: call(points=None), "NULL"), "NULL point_firsts": (lambda: call(pf=None), "NULL"),
                      "interval_rows * width below 128": (lambda: call(ks=(ctypes.c_uint * 3)(31, 0, 1)), "128")})
    for name, f in REJECTED_DESCS.items():
        calls["descriptor: " + name] = ((lambda f_: lambda: call(descs=d3(*f_), staging=1))(f), "descriptor")
        calls["descriptor with channels given: " + name] = ((lambda f_: lambda: call(descs=d3(*f_), ch=3))(f), "descriptor")
    for name, (c, word) in calls.items():
        assert c() == E_ARG, name
        assert word in api.last_error(), (name, api.last_error())
        assert untouched(a), name
    # the limits exactly are no rejection of the items: 64 to 2, 32 to 1 and 32768 x 32767 get as far as the output ranges
    assert call(items=rs((2, 0, 0, 64, 1, 2, 1, 0), (2, 1, 0, 32, 3, 1, 1, 0)), oo=o2(0, 7)) == E_ARG and "overlap" in api.last_error()
    assert call(items=rs(ok0, (2, 0, 0, 1, 1, 32768, 32767, 0)), oo=o2(16, 0)) == E_ARG and "overlap" in api.last_error()
    assert untouched(a)
    # (an accepted call goes on to the context and the device: tests/test_gpu_bilinear.py)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    ok = (0, 0, 0, 1, 1, 1, 1, 0)
    for f, tail in ((ctx.decode_bilinear, ()), (ctx.decode_bilinear_indexed, ([1, 1], None, [0, 0]))):
        with pytest.raises(api.QoiError):
            f(1, [0], [40, 40], d, 0, [ok], 0, 1, [0], *tail)
        with pytest.raises(api.QoiError):
            f(1, [0, 40], [40, 40], d, 0, [ok], 0, 1, [0, 4], *tail)
        with pytest.raises(api.QoiError):
            f(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1, 1, 1, -1)], 0, 1, [0], *tail)
        with pytest.raises(api.QoiError):
            f(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1, 0)], 0, 1, [0], *tail)
