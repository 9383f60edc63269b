"""qoimi_decode_resized / qoimi_resize_size / qoimi_resize_stats, what can be checked without a GPU: the three entry points in every layer, the
structure's layout, the size arithmetic, and every QOIMI_E_ARG case - all of them are reported before the context or the device is looked at,
so a block of zeroed host memory stands in for a context here and host arrays for device buffers; the output keeps its bytes.  (What the
library does behind the rejections needs a device: tests/test_gpu_resize.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

from qoi_amd import api, resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_decode_resized", "qoimi_resize_size", "qoimi_resize_stats")
E_ARG = -1


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_decode_resized\s*\(", header)
    assert re.search(r"\bsize_t\s+qoimi_resize_size\s*\(", header)
    assert re.search(r"\bvoid\s+qoimi_resize_stats\s*\(", header)
    assert "QOIMI_RESIZE_FLIP_X = 1" in header and "QOIMI_RESIZE_FLIP_Y = 2" in header and re.search(r"\}\s*qoimi_resize\s*;", header)
    assert "QOIMI_RESIZE_PLAIN = 0" in header and "QOIMI_RESIZE_ALPHA_WEIGHTED = 1" in header
    assert (resize.FLIP_X, resize.FLIP_Y, resize.PLAIN, resize.ALPHA_WEIGHTED, resize.MAX_RATIO) == (1, 2, 0, 1, 64)
    assert "qoimi_*" in open(os.path.join(ROOT, "qoi_amd", "csrc", "exports.map")).read()
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("decode_resized", "resize_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.resize_size)


def test_the_filter_kernel_is_built_without_scratch_and_has_no_timer_entry():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "resize_filter" in k]
    assert len(hits) == 1, hits
    assert ks[hits[0]]["scratch"] == 0 and ks[hits[0]]["vgpr_spills"] == 0 and ks[hits[0]]["lds"] == 0, ks[hits[0]]
    lib = api.load_library()
    assert not any("resize" in lib.qoimi_kernel_name(i).decode() for i in range(64))


def test_struct_layout():
    assert ctypes.sizeof(api.QoimiResize) == 32
    assert [(f, getattr(api.QoimiResize, f).offset) for f, _ in api.QoimiResize._fields_] == [
        ("image", 0), ("x", 4), ("y", 8), ("width", 12), ("height", 16), ("out_width", 20), ("out_height", 24), ("flags", 28)]
    r = api.QoimiResize(1, 2, 3, 4, 5, 6, 7, 3)
    assert bytes(r) == b"".join(v.to_bytes(4, "little") for v in (1, 2, 3, 4, 5, 6, 7, 3))
    assert resize.fields(r) == (1, 2, 3, 4, 5, 6, 7, 3) and resize.as_crop(r) == (1, 2, 3, 4, 5, 3)
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*qoimi_resize\s*;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == ["image", "x", "y", "width", "height", "out_width", "out_height", "flags"]
    assert body.count("unsigned int") == 5


def test_resize_size():
    lib = api.load_library()
    for (w, h) in [(1, 1), (37, 23), (3840, 2160), (19999, 20000), (4, 99999999)]:
        for rect in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, min(w, 64), min(h, 128)), (w // 2, h // 3, min(w - w // 2, 50), min(h - h // 3, 7))]:
            for out in [(1, 2), (224, 224), (rect[2], rect[3]), (65536, 65536)]:
                for flags in range(4):
                    for ch_in in (3, 4):
                        for ch in (3, 4):
                            want = resize.size(w, h, rect, out, flags, ch)
                            assert want == out[0] * out[1] * ch
                            assert api.resize_size(w, h, ch_in, (7,) + rect + out + (flags,), ch) == want, (w, h, rect, out, flags, ch)   # (item.image is not looked at)
    # the cap, exactly and one beyond, per axis
    assert api.resize_size(4096, 4096, 4, (0, 0, 0, 4096, 4096, 64, 64, 0), 4) == 64 * 64 * 4
    assert api.resize_size(4096, 4096, 4, (0, 0, 0, 4096, 4095, 64, 64, 0), 3) == 64 * 64 * 3
    assert api.resize_size(4097, 4096, 4, (0, 0, 0, 4097, 64, 64, 1, 0), 4) == 0
    assert api.resize_size(4096, 4097, 4, (0, 0, 0, 64, 4097, 1, 64, 0), 4) == 0
    assert api.resize_size(130, 70, 4, (0, 0, 0, 65, 1, 1, 1, 0), 4) == 0 and api.resize_size(130, 70, 4, (0, 0, 0, 64, 1, 1, 1, 0), 4) == 4
    # the zero returns: a rejected descriptor, an empty rectangle or output, a rectangle that leaves the image (also where 32-bit sums would
    # wrap), an unknown flag bit, channels not 3 / 4 (0 is not an output channel count here), a product beyond a size_t
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    zero = [((0, 4, 4, 0), good, 4), ((4, 0, 4, 0), good, 4), ((4, 4, 2, 0), good, 4), ((4, 4, 5, 0), good, 4), ((4, 4, 4, 2), good, 4), ((20000, 20000, 4, 0), good, 4),
            ((4, 4, 4, 0), (0, 0, 0, 0, 1, 1, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 0, 1, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 0, 1, 0), 4),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 0, 0), 4), ((4, 4, 4, 0), (0, 3, 0, 2, 1, 2, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 3, 1, 2, 1, 2, 0), 4),
            ((4, 4, 4, 0), (0, 4, 0, 1, 1, 1, 1, 0), 4), ((4, 4, 4, 0), (0, 4294967295, 0, 2, 1, 2, 1, 0), 4), ((4, 4, 4, 0), (0, 0, 2, 1, 4294967295, 1, 4294967295, 0), 4),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 1, 4), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 1, 1, 0x80000001), 4),
            ((4, 4, 4, 0), good, 0), ((4, 4, 4, 0), good, 2), ((4, 4, 4, 0), good, 5), ((4, 4, 4, 0), good, -3),
            ((4, 4, 4, 0), (0, 0, 0, 1, 1, 4294967295, 4294967295, 0), 4), ((4, 4, 4, 0), (0, 0, 0, 1, 1, 4294967295, 4294967295, 0), 3)]
    for d, r, ch in zero:
        assert lib.qoimi_resize_size(ctypes.byref(api.QoiDesc(*d)), ctypes.byref(api.QoimiResize(*r)), ch) == 0, (d, r, ch)
    assert lib.qoimi_resize_size(None, ctypes.byref(api.QoimiResize(*good)), 4) == 0
    assert lib.qoimi_resize_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), None, 4) == 0
    assert lib.qoimi_resize_size(ctypes.byref(api.QoiDesc(4, 4, 3, 1)), ctypes.byref(api.QoimiResize(*good)), 3) == 45
    assert api.resize_size(4, 4, 4, (0, -1, 0, 1, 1, 1, 1, 0), 4) == 0
    assert api.resize_size(4, 4, 4, (0, 0, 0, 1, 1, 1 << 31, 1 << 31, 0), 4) == 0 == resize.size(4, 4, (0, 0, 1, 1), (1 << 31, 1 << 31), 0, 4)
    assert api.resize_size(4, 4, 4, (0, 0, 0, 1, 1, 1 << 31, 1 << 30, 0), 4) == 1 << 63 == resize.size(4, 4, (0, 0, 1, 1), (1 << 31, 1 << 30), 0, 4)
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_resize_stats(None, out)                                    # no context: zeros
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
    return a


def rs(*rows):
    return (api.QoimiResize * len(rows))(*[api.QoimiResize(*r) for r in rows])


def untouched(a):
    return bytes(a.out) == b"\x5A" * 4096 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096


REJECTED_DESCS = {"width 0": (0, 3, 4, 0), "height 0": (3, 0, 4, 0), "channels 2": (3, 3, 2, 0), "channels 5": (3, 3, 5, 0),
                  "colorspace 2": (3, 3, 4, 2), "pixel cap": (20000, 20000, 4, 0)}


def test_rejections(args):
    a = args

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, ch=0, items=a.items, ni=2, mode=0, out=a.o, oo=a.oo, staging=0):
        return a.lib.qoimi_decode_resized(ctx, streams, so, sizes, descs, n, ch, items, ni, mode, out, oo, staging, None)

    def o2(x, y):
        return (ctypes.c_size_t * 2)(x, y)

    def d3(*last):
        return (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(*last))

    ok0 = (0, 1, 1, 2, 2, 2, 2, 0)
    ok2 = (2, 0, 0, 130, 1, 5, 1, 0)
    calls = {
        "NULL ctx": lambda: call(ctx=None), "NULL d_streams": lambda: call(streams=None), "NULL stream_offsets": lambda: call(so=None),
        "NULL sizes": lambda: call(sizes=None), "NULL descs": lambda: call(descs=None), "NULL items": lambda: call(items=None),
        "NULL d_out": lambda: call(out=None), "NULL out_offsets": lambda: call(oo=None),
        "n_images 0": lambda: call(n=0), "n_images -1": lambda: call(n=-1), "n_items 0": lambda: call(ni=0), "n_items -1": lambda: call(ni=-1),
        "channels 1": lambda: call(ch=1), "channels 2": lambda: call(ch=2), "channels 5": lambda: call(ch=5), "channels -3": lambda: call(ch=-3),
        "mode 2": lambda: call(mode=2), "mode -1": lambda: call(mode=-1),
        "image == n_images": lambda: call(items=rs(ok0, (3, 0, 0, 1, 1, 1, 1, 0))), "image 2^32-1": lambda: call(items=rs(ok0, (4294967295, 0, 0, 1, 1, 1, 1, 0))),
        "image beyond a shorter n_images": lambda: call(n=2),
        "width 0": lambda: call(items=rs(ok0, (2, 0, 0, 0, 1, 1, 1, 0))), "height 0": lambda: call(items=rs((0, 0, 0, 1, 0, 1, 1, 0), ok2)),
        "out_width 0": lambda: call(items=rs(ok0, (2, 0, 0, 5, 1, 0, 1, 0))), "out_height 0": lambda: call(items=rs((0, 0, 0, 1, 1, 1, 0, 0), ok2)),
        "one column outside": lambda: call(items=rs(ok0, (2, 1, 0, 130, 1, 130, 1, 0))), "one row outside": lambda: call(items=rs(ok0, (2, 0, 1, 5, 3, 5, 3, 0))),
        "x == width": lambda: call(items=rs(ok0, (2, 130, 0, 1, 1, 1, 1, 0))), "y == height": lambda: call(items=rs((0, 0, 4, 1, 1, 1, 1, 0), ok2)),
        "x + width wraps in 32 bits": lambda: call(items=rs(ok0, (2, 4294967295, 0, 2, 1, 2, 1, 0))),
        "y + height wraps in 32 bits": lambda: call(items=rs(ok0, (2, 0, 2, 1, 4294967295, 1, 4294967295, 0))),
        "the cap in x: 129 to 2": lambda: call(items=rs(ok0, (2, 0, 0, 129, 1, 2, 1, 0))), "the cap in x: 65 to 1": lambda: call(items=rs(ok0, (2, 3, 0, 65, 3, 1, 3, 0))),
        "the cap in y: 65 to 1": lambda: call(descs=d3(5, 65, 4, 0), items=rs(ok0, (2, 0, 0, 5, 65, 5, 1, 0))),
        "flag bit 2": lambda: call(items=rs(ok0, (2, 0, 0, 5, 1, 5, 1, 4))), "flag bit 31": lambda: call(items=rs((0, 1, 1, 2, 2, 2, 2, 0x80000000), ok2)),
        "referenced size 21": lambda: call(sizes=(ctypes.c_int * 3)(40, 0, 21)), "referenced size 0": lambda: call(sizes=(ctypes.c_int * 3)(0, 40, 40)),
        "referenced size negative": lambda: call(sizes=(ctypes.c_int * 3)(40, 40, -1)),
        "mixed channels": lambda: call(descs=d3(130, 3, 3, 0)), "mixed channels, 3 first": lambda: call(descs=(api.QoiDesc * 3)(api.QoiDesc(4, 4, 3, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(130, 3, 4, 0))),
        "outputs overlap by one byte": lambda: call(oo=o2(0, 15)), "outputs coincide": lambda: call(oo=o2(64, 64)),
        "outputs overlap, item 1 in front": lambda: call(oo=o2(119, 100)),
        "outputs overlap with channels 3": lambda: call(ch=3, oo=o2(0, 11)),
        "output offset wraps the address space": lambda: call(oo=o2(0, 2 ** 64 - 8)), "output end wraps the address space": lambda: call(oo=o2(0, 2 ** 64 - a.o - 19)),
        "output beyond a size_t": lambda: call(items=rs(ok0, (2, 0, 0, 1, 1, 1 << 31, 1 << 31, 0))),
        "now image 1 is named": lambda: call(items=rs(ok0, (1, 0, 0, 1, 1, 1, 1, 0))),
    }
    for name, f in REJECTED_DESCS.items():
        calls["descriptor: " + name] = (lambda f_: lambda: call(descs=d3(*f_), staging=1))(f)
        calls["descriptor with channels given: " + name] = (lambda f_: lambda: call(descs=d3(*f_), ch=3))(f)
    for name, c in calls.items():
        assert c() == E_ARG, name
        assert api.last_error() != "", name
        assert untouched(a), name
    # the cap exactly is no rejection of the items: 128 to 2 and 64 to 1 get as far as the output ranges
    assert call(items=rs((2, 0, 0, 128, 1, 2, 1, 0), (2, 1, 0, 64, 3, 1, 1, 0)), oo=o2(0, 7)) == E_ARG and "overlap" in api.last_error()
    assert untouched(a)
    # (an accepted call goes on to the context and the device: tests/test_gpu_resize.py)


def test_tile_limit_of_a_sub_batch(args):
    """items of 2^20 x 2^19 output pixels of one lane: 2^31 tiles each - one is too many, whatever the image; at 65536 x 65536 pixels an item
    stays below the limit with 2^24 tiles, 128 of them reach 2^31 - 1 or more and 127 would get as far as the context - which this test
    must not do"""
    a = args
    descs = (api.QoiDesc * 1)(api.QoiDesc(4, 4, 4, 0))
    one = rs((0, 0, 0, 1, 1, 1 << 20, 1 << 19, 0))
    assert resize.tiles(1, 1 << 20, 1 << 19) == 2 ** 31
    aligned = (a.o + 15) & ~15
    rc = a.lib.qoimi_decode_resized(a.ctx, a.p, (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(40), descs, 1, 3, one, 1, 0, aligned, (ctypes.c_size_t * 1)(0), 0, None)
    assert rc == E_ARG and "tiles" in api.last_error()
    n, B = 128, 65536 * 65536 * 3
    per = resize.tiles(1, 65536, 65536)
    assert per * n >= 2 ** 31 - 1 > per * (n - 1)
    many = (api.QoimiResize * n)(*[api.QoimiResize(0, 0, 0, 1, 1, 65536, 65536, j & 3) for j in range(n)])
    oo = (ctypes.c_size_t * n)(*[j * B for j in range(n)])
    rc = a.lib.qoimi_decode_resized(a.ctx, a.p, (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(40), descs, 1, 3, many, n, 0, aligned, oo, 0, None)
    assert rc == E_ARG and "tiles" in api.last_error()
    assert untouched(a)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    ok = (0, 0, 0, 1, 1, 1, 1, 0)
    with pytest.raises(api.QoiError):
        ctx.decode_resized(1, [0], [40, 40], d, 0, [ok], 0, 1, [0])
    with pytest.raises(api.QoiError):
        ctx.decode_resized(1, [0, 40], [40, 40], d, 0, [ok], 0, 1, [0, 4])
    with pytest.raises(api.QoiError):
        ctx.decode_resized(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1, 1, 1, -1)], 0, 1, [0])
    with pytest.raises(api.QoiError):
        ctx.decode_resized(1, [0, 40], [40, 40], d, 0, [(0, 0, 0, 1, 1, 0)], 0, 1, [0])
