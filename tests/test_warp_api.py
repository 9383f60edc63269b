"""qoimi_decode_warped / qoimi_decode_warped_indexed / qoimi_warp_size / qoimi_warp_stats / qoimi_warp_orient, what can be checked without a
GPU: the entry points in every layer, the header's statement of the definition, the structure's size and offsets, the size and orientation
arithmetic against qoi_amd/warp.py, and every QOIMI_E_ARG case with the word qoimi_last_error names it by, in the order the header gives -
all of them are reported before the context or the device is looked at, so a block of zeroed host memory stands in for a context here and
host arrays for device buffers; the output keeps its bytes.  (What the library does behind the rejections needs a device:
tests/test_gpu_warp.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, warp
from qoi_amd.warp import ONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_decode_warped", "qoimi_decode_warped_indexed", "qoimi_warp_size", "qoimi_warp_stats", "qoimi_warp_orient")
E_ARG = -1


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_decode_warped\s*\(", header) and re.search(r"\bint\s+qoimi_decode_warped_indexed\s*\(", header)
    assert re.search(r"\bsize_t\s+qoimi_warp_size\s*\(", header) and re.search(r"\bvoid\s+qoimi_warp_stats\s*\(", header) and re.search(r"\bint\s+qoimi_warp_orient\s*\(", header)
    for text in ("qoi_amd/warp.py", "normative", "(2k + 1) << 16", "Px = a * U + b * V + c", "k0 = px >> 17", "131072 - fx", "(N_c + 2^33) >> 34", "NO ANTIALIASING",
                 "qoimi_decode_resized", "2^31 * 2^21 = 2^52", "2^57: both positions fit 64 bits", "tight around", "in this order", "SYNCHRONOUS"):
        assert text in header, text
    assert len(re.findall(r"\}\s*qoimi_warp\s*;", header)) == 1 and re.search(r"QOIMI_WARP_REPLICATE\s*=\s*1\b", header)
    lib = api.load_library()
    assert lib.qoimi_decode_warped_indexed.argtypes[:14] == lib.qoimi_decode_warped.argtypes and lib.qoimi_decode_warped_indexed.argtypes[14:] == lib.qoimi_decode_bilinear_indexed.argtypes[14:]
    assert (warp.REPLICATE, warp.PLAIN, warp.ALPHA_WEIGHTED, warp.ONE, warp.TILE) == (1, 0, 1, 65536, 16)
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("decode_warped", "decode_warped_indexed", "warp_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.warp_size) and callable(api.warp_orient)


def test_struct_layout():
    assert ctypes.sizeof(api.QoimiWarp) == 72
    names = ["image", "x", "y", "width", "height", "out_width", "out_height", "flags", "a", "b", "d", "e", "fill", "reserved", "c", "f"]
    assert [f for f, _ in api.QoimiWarp._fields_] == names
    assert [getattr(api.QoimiWarp, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64]
    it = api.QoimiWarp(*range(1, 17))
    assert warp.fields(it) == tuple(range(1, 17))
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert "72 bytes, offsets 0/4/8/12/16/20/24/28/32/36/40/44/48/52/56/64" in header


def test_the_kernel_is_built_without_scratch_and_has_no_timer_entry():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "warp_gather" in k]
    assert len(hits) == 1, hits
    assert ks[hits[0]]["scratch"] == 0 and ks[hits[0]]["vgpr_spills"] == 0 and ks[hits[0]]["lds"] == 0, ks[hits[0]]
    lib = api.load_library()
    assert not any("warp" in lib.qoimi_kernel_name(i).decode() for i in range(64))


LIMIT_MAP = (-2 ** 31, 2 ** 31 - 1, (1 << 56) - 1, 2 ** 31 - 1, -2 ** 31, 1 - (1 << 56))


def test_warp_size():
    lib = api.load_library()
    for (w, h) in [(1, 1), (37, 23), (3840, 2160), (19999, 20000)]:
        for rect in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, min(w, 64), min(h, 128)), (0, 0, w + 1, 1), (0, 1, 1, h)]:
            for out in [(1, 2), (224, 224), ((1 << 20) - 1, 381), (1 << 20, 1), (1, 1 << 20), (20000, 19999), (20000, 20000), (0, 5)]:
                for flags in (0, 1, 2, 3):
                    for m in (warp.IDENTITY, LIMIT_MAP, (ONE, 0, 1 << 56, 0, ONE, 0), (ONE, 0, 0, 0, ONE, -(1 << 56))):
                        for ch in (3, 4):
                            it = warp.item(7, rect, out, m, flags, 0xFFFFFFFF)          # (item.image is not looked at)
                            assert api.warp_size(w, h, 7 - ch, it, ch) == warp.size(w, h, it, ch), (w, h, it, ch)
    good = warp.item(0, (1, 1, 2, 2), (5, 3))
    assert api.warp_size(4, 4, 4, good, 4) == 60 and api.warp_size(4, 4, 4, good, 3) == 45
    assert api.warp_size(4, 4, 4, good[:13] + (1,) + good[14:], 4) == 0                   # reserved
    for d in [(0, 4, 4, 0), (4, 4, 2, 0), (4, 4, 4, 2), (20000, 20000, 4, 0)]:
        assert lib.qoimi_warp_size(ctypes.byref(api.QoiDesc(*d)), ctypes.byref(api.QoimiWarp(*good)), 4) == 0, d
    for ch in (0, 5, -3):
        assert lib.qoimi_warp_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), ctypes.byref(api.QoimiWarp(*good)), ch) == 0
    assert lib.qoimi_warp_size(None, ctypes.byref(api.QoimiWarp(*good)), 4) == 0
    assert lib.qoimi_warp_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), None, 4) == 0
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_warp_stats(None, out)                                      # no context: zeros
    assert list(out) == [0, 0, 0, 0]


def test_warp_orient():
    for (w, h) in [(1, 1), (37, 23), (130, 70)]:
        for rect in [(0, 0, w, h), (w - 1, h - 1, 1, 1), (w // 2, h // 3, w - w // 2, 1), (0, 0, w + 1, 1), (0, 1, 1, h), (0, 0, 0, 1), (1, 0, 0xFFFFFFFF, 1)]:
            for o in range(-1, 11):
                got, want = api.warp_orient(w, h, 4, rect, o), warp.orient(w, h, rect, o)
                assert (got is None) == (want is None), (w, h, rect, o)
                if got is not None:
                    assert warp.fields(got) == want, (w, h, rect, o)
                    assert api.warp_size(w, h, 4, got, 3) == rect[2] * rect[3] * 3
    lib = api.load_library()
    out = api.QoimiWarp()
    assert lib.qoimi_warp_orient(None, 0, 0, 1, 1, 1, ctypes.byref(out)) == E_ARG
    assert lib.qoimi_warp_orient(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), 0, 0, 1, 1, 1, None) == E_ARG
    assert lib.qoimi_warp_orient(ctypes.byref(api.QoiDesc(4, 4, 5, 0)), 0, 0, 1, 1, 1, ctypes.byref(out)) == E_ARG
    assert lib.qoimi_warp_orient(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), 0, 0, 1, 1, 9, ctypes.byref(out)) == E_ARG and "1..8" in api.last_error()


def ws(*rows):
    return (api.QoimiWarp * len(rows))(*[api.QoimiWarp(*r) for r in rows])


def it(image, rect, out, m=warp.IDENTITY, flags=0, reserved=0):
    t = warp.item(image, rect, out, m, flags, 0x11223344)
    return t[:13] + (reserved,) + t[14:]


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
    a.items = ws(it(0, (1, 1, 2, 2), (2, 2)), it(2, (0, 0, 130, 1), (5, 1), LIMIT_MAP, 1))     # 16 and 20 bytes at 4 channels
    a.oo = (ctypes.c_size_t * 2)(0, 1024)
    a.ks = (ctypes.c_uint * 3)(32, 0, 1)
    a.points = (ctypes.c_ubyte * 4096)()
    a.pf = (ctypes.c_size_t * 3)(0, 0, 0)
    return a


def untouched(a):
    return bytes(a.out) == b"\x5A" * 4096 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


@pytest.mark.parametrize("indexed", [False, True])
def test_rejections(args, indexed):
    a = args

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, ch=0, items=a.items, ni=2, mode=0, out=a.o, oo=a.oo, staging=0, ks=a.ks, points=a.points, pf=a.pf):
        if indexed:
            return a.lib.qoimi_decode_warped_indexed(ctx, streams, so, sizes, descs, n, ch, items, ni, mode, out, oo, staging, None, ks, None if points is None else ctypes.cast(points, a.lib.qoimi_decode_warped_indexed.argtypes[15]), pf)
        return a.lib.qoimi_decode_warped(ctx, streams, so, sizes, descs, n, ch, items, ni, mode, out, oo, staging, None)

    def o2(x, y):
        return (ctypes.c_size_t * 2)(x, y)

    def d3(*last):
        return (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(*last))

    ok0 = it(0, (1, 1, 2, 2), (2, 2))
    ok2 = it(2, (0, 0, 130, 1), (5, 1))
    big_c, big_f = (ONE, 0, 1 << 56, 0, ONE, 0), (ONE, 0, 0, 0, ONE, -(1 << 56))
    calls = {
        "NULL ctx": (lambda: call(ctx=None), "NULL"), "NULL d_streams": (lambda: call(streams=None), "NULL"), "NULL stream_offsets": (lambda: call(so=None), "NULL"),
        "NULL sizes": (lambda: call(sizes=None), "NULL"), "NULL descs": (lambda: call(descs=None), "NULL"), "NULL items": (lambda: call(items=None), "NULL"),
        "NULL d_out": (lambda: call(out=None), "NULL"), "NULL out_offsets": (lambda: call(oo=None), "NULL"),
        "n_images 0": (lambda: call(n=0), "empty"), "n_images -1": (lambda: call(n=-1), "empty"), "n_items 0": (lambda: call(ni=0), "empty"), "n_items -1": (lambda: call(ni=-1), "empty"),
        "channels 1": (lambda: call(ch=1), "channels"), "channels 5": (lambda: call(ch=5), "channels"), "channels -3": (lambda: call(ch=-3), "channels"),
        "mode 2": (lambda: call(mode=2), "mode"), "mode -1": (lambda: call(mode=-1), "mode"),
        "image == n_images": (lambda: call(items=ws(ok0, it(3, (0, 0, 1, 1), (1, 1)))), "no image"), "image 2^32-1": (lambda: call(items=ws(ok0, it(4294967295, (0, 0, 1, 1), (1, 1)))), "no image"),
        "image beyond a shorter n_images": (lambda: call(n=2), "no image"),
        "width 0": (lambda: call(items=ws(ok0, it(2, (0, 0, 0, 1), (1, 1)))), "zero"), "height 0": (lambda: call(items=ws(it(0, (0, 0, 1, 0), (1, 1)), ok2)), "zero"),
        "out_width 0": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (0, 1)))), "zero"), "out_height 0": (lambda: call(items=ws(it(0, (0, 0, 1, 1), (1, 0)), ok2)), "zero"),
        "one column outside": (lambda: call(items=ws(ok0, it(2, (1, 0, 130, 1), (130, 1)))), "leaves"), "one row outside": (lambda: call(items=ws(ok0, it(2, (0, 1, 5, 3), (5, 3)))), "leaves"),
        "x == width": (lambda: call(items=ws(ok0, it(2, (130, 0, 1, 1), (1, 1)))), "leaves"), "y == height": (lambda: call(items=ws(it(0, (0, 4, 1, 1), (1, 1)), ok2)), "leaves"),
        "x + width wraps in 32 bits": (lambda: call(items=ws(ok0, it(2, (4294967295, 0, 2, 1), (2, 1)))), "leaves"),
        "y + height wraps in 32 bits": (lambda: call(items=ws(ok0, it(2, (0, 2, 1, 4294967295), (1, 1)))), "leaves"),
        "out_width 2^20": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (1 << 20, 1)))), "2^20"), "out_height 2^20": (lambda: call(items=ws(it(0, (0, 0, 1, 1), (1, 1 << 20)), ok2)), "2^20"),
        "out_width 2^32-1": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (4294967295, 1)))), "2^20"),
        "20000 x 20000 output pixels": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (20000, 20000)))), "400 000 000"),
        "c 2^56": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (5, 1), big_c))), "2^56"), "f -2^56": (lambda: call(items=ws(it(0, (0, 0, 1, 1), (1, 1), big_f), ok2)), "2^56"),
        "c -2^63": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (5, 1), (ONE, 0, -2 ** 63, 0, ONE, 0)))), "2^56"),
        "flag bit 1": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (5, 1), flags=2))), "flag"), "flag bit 31": (lambda: call(items=ws(it(0, (1, 1, 2, 2), (2, 2), flags=0x80000001), ok2)), "flag"),
        "reserved 1": (lambda: call(items=ws(ok0, it(2, (0, 0, 5, 1), (5, 1), reserved=1))), "reserved"),
        "referenced size 21": (lambda: call(sizes=(ctypes.c_int * 3)(40, 0, 21)), "shorter"), "referenced size 0": (lambda: call(sizes=(ctypes.c_int * 3)(0, 40, 40)), "shorter"),
        "referenced size negative": (lambda: call(sizes=(ctypes.c_int * 3)(40, 40, -1)), "shorter"),
        "mixed channels": (lambda: call(descs=d3(130, 3, 3, 0)), "channel"),
        "outputs overlap by one byte": (lambda: call(oo=o2(0, 15)), "overlap"), "outputs coincide": (lambda: call(oo=o2(64, 64)), "overlap"),
        "outputs overlap, item 1 in front": (lambda: call(oo=o2(119, 100)), "overlap"), "outputs overlap with channels 3": (lambda: call(ch=3, oo=o2(0, 11)), "overlap"),
        "output offset wraps the address space": (lambda: call(oo=o2(0, 2 ** 64 - 8)), "address space"),
        "output end wraps the address space": (lambda: call(oo=o2(0, 2 ** 64 - a.o - 19)), "address space"),
        "now image 1 is named": (lambda: call(items=ws(ok0, it(1, (0, 0, 1, 1), (1, 1)))), "shorter"),
        # the order inside an item: each fault in front of all the later ones
        "order: zero first": (lambda: call(items=ws(ok0, it(2, (200, 0, 0, 1), (1 << 20, 20000), big_c, 2, 1))), "zero"),
        "order: leaves second": (lambda: call(items=ws(ok0, it(2, (200, 0, 1, 1), (1 << 20, 20000), big_c, 2, 1))), "leaves"),
        "order: the sides third": (lambda: call(items=ws(ok0, it(2, (0, 0, 1, 1), (1 << 20, 20000), big_c, 2, 1))), "2^20"),
        "order: the pixels fourth": (lambda: call(items=ws(ok0, it(2, (0, 0, 1, 1), (20000, 20000), big_c, 2, 1))), "400 000 000"),
        "order: the offsets fifth": (lambda: call(items=ws(ok0, it(2, (0, 0, 1, 1), (5, 1), big_c, 2, 1))), "2^56"),
        "order: the flags sixth": (lambda: call(items=ws(ok0, it(2, (0, 0, 1, 1), (5, 1), warp.IDENTITY, 2, 1))), "flag"),
        "order: an earlier item's fault first": (lambda: call(items=ws(it(0, (1, 1, 2, 2), (2, 2), reserved=7), it(2, (0, 0, 0, 1), (1, 1)))), "reserved"),
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
    # the limits exactly are no rejection of the items: they get as far as the output ranges
    assert call(items=ws(it(2, (0, 0, 5, 1), ((1 << 20) - 1, 381), LIMIT_MAP, 1), ok0), oo=o2(0, 7)) == E_ARG and "overlap" in api.last_error()
    assert call(items=ws(ok0, it(2, (0, 0, 5, 1), (20000, 19999), LIMIT_MAP, 1)), oo=o2(16, 0)) == E_ARG and "overlap" in api.last_error()
    assert untouched(a)
    # (an accepted call goes on to the context and the device: tests/test_gpu_warp.py)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    ok = warp.item(0, (0, 0, 1, 1), (1, 1))
    for f, tail in ((ctx.decode_warped, ()), (ctx.decode_warped_indexed, ([1, 1], None, [0, 0]))):
        with pytest.raises(api.QoiError):
            f(1, [0], [40, 40], d, 0, [ok], 0, 1, [0], *tail)
        with pytest.raises(api.QoiError):
            f(1, [0, 40], [40, 40], d, 0, [ok], 0, 1, [0, 4], *tail)
        with pytest.raises(api.QoiError):
            f(1, [0, 40], [40, 40], d, 0, [ok[:8] + (2 ** 31,) + ok[9:]], 0, 1, [0], *tail)
        with pytest.raises(api.QoiError):
            f(1, [0, 40], [40, 40], d, 0, [ok[:8]], 0, 1, [0], *tail)
