"""qoimi_decode_tensors / qoimi_decode_warped_tensors / qoimi_tensor_size / qoimi_warp_tensor_size / qoimi_tensor_stats, what can be checked
without a GPU: the entry points in every layer, the header's statement of the definition, the structure's size and offsets, the size arithmetic
against qoi_amd/tensors.py, the three kernels in the built library, and every QOIMI_E_ARG case with the word qoimi_last_error names it by, in
the order the header gives - all of them are reported before the context or the device is looked at, so a block of zeroed host memory stands in
for a context here and host arrays for device buffers; the output keeps its bytes.  (What the library does behind the rejections needs a device:
tests/test_gpu_tensors.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from qoi_amd import api, bilinear, resize, tensors, warp
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_AREA, FILTER_BILINEAR, HWC, U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_decode_tensors", "qoimi_decode_warped_tensors", "qoimi_tensor_size", "qoimi_warp_tensor_size", "qoimi_tensor_stats")
E_ARG = -1
ONE4, ZERO4 = (1.0,) * 4, (0.0,) * 4
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def test_symbols_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"\bint\s+qoimi_decode_tensors\s*\(", header) and re.search(r"\bint\s+qoimi_decode_warped_tensors\s*\(", header)
    assert re.search(r"\bsize_t\s+qoimi_tensor_size\s*\(", header) and re.search(r"\bsize_t\s+qoimi_warp_tensor_size\s*\(", header)
    assert re.search(r"\bvoid\s+qoimi_tensor_stats\s*\(", header)
    for text in ("qoi_amd/tensors.py", "normative", "byte for byte, flips included", "TWO roundings, never a fused multiply-add", "round to nearest even",
                 "Subnormals are kept", "becomes infinity", "(Y * ow + X) * och + c", "(c * oh + Y) * ow + X", "looked for in this order", "a multiple of the element size",
                 "SYNCHRONOUS", "Not here: indexed forms"):
        assert text in header, text
    assert len(re.findall(r"\}\s*qoimi_tensor_format\s*;", header)) == 1
    for name, value in (("QOIMI_TENSOR_U8", 0), ("QOIMI_TENSOR_F16", 1), ("QOIMI_TENSOR_BF16", 2), ("QOIMI_TENSOR_F32", 3), ("QOIMI_TENSOR_HWC", 0), ("QOIMI_TENSOR_CHW", 1),
                        ("QOIMI_FILTER_AREA", 0), ("QOIMI_FILTER_BILINEAR", 1)):
        assert re.search(name + r"\s*=\s*%d\b" % value, header), name
    assert (tensors.U8, tensors.F16, tensors.BF16, tensors.F32, tensors.HWC, tensors.CHW, tensors.FILTER_AREA, tensors.FILTER_BILINEAR) == (0, 1, 2, 3, 0, 1, 0, 1)
    assert tensors.ELEM == {0: 1, 1: 2, 2: 2, 3: 4}
    for name in NEW:
        assert name in api.EXPORTS, name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("decode_tensors", "decode_warped_tensors", "tensor_stats"):
        assert callable(getattr(api.Context, method))
    assert callable(api.tensor_size) and callable(api.warp_tensor_size)
    import qoi_amd
    pkg = os.path.dirname(qoi_amd.__file__)
    assert not any(re.search(r"^\s*(import|from)\s+torch\b", open(os.path.join(pkg, f)).read(), re.M) for f in ("tensors.py", "api.py"))


def test_struct_layout():
    assert ctypes.sizeof(api.QoimiTensorFormat) == 48
    names = ["dtype", "layout", "scale", "bias", "reserved"]
    assert [f for f, _ in api.QoimiTensorFormat._fields_] == names
    assert [getattr(api.QoimiTensorFormat, f).offset for f in names] == [0, 4, 8, 24, 40]
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert "48 bytes, offsets 0/4/8/24/40" in header
    t = api.tensor_format((F16, CHW, IMAGENET[0], IMAGENET[1]))
    assert (t.dtype, t.layout) == (1, 1) and list(t.reserved) == [0, 0]
    assert np.array_equal(np.array(list(t.scale), np.float32), IMAGENET[0]) and np.array_equal(np.array(list(t.bias), np.float32), IMAGENET[1])


def test_the_kernels_are_built_without_scratch_and_have_no_timer_entry():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("tensor_area", "tensor_tent", "tensor_warp"):
        hits = [k for k in ks if name in k]
        assert len(hits) == 1, (name, hits)
        assert ks[hits[0]]["scratch"] == 0 and ks[hits[0]]["vgpr_spills"] == 0 and ks[hits[0]]["lds"] == 0, ks[hits[0]]
        assert not any(old in hits[0] for old in ("resize_filter", "bilinear_filter", "warp_gather", "crop_gather"))
    lib = api.load_library()
    assert not any("tensor" in lib.qoimi_kernel_name(i).decode() for i in range(64))


BAD_FORMATS = [(4, HWC, ONE4, ZERO4), (2 ** 32 - 1, HWC, ONE4, ZERO4), (F16, 2, ONE4, ZERO4), (F32, HWC, (1.0, float("inf"), 1.0, 1.0), ZERO4),
               (BF16, CHW, ONE4, (0.0, 0.0, float("nan"), 0.0)), (U8, HWC, (1.0, 1.0, 1.0, 0.5), ZERO4), (U8, CHW, ONE4, (-0.0, 0.0, 0.0, 0.0)), (U8, HWC, ONE4, (0.0, 1.0, 0.0, 0.0))]
GOOD_FORMATS = [(U8, HWC, ONE4, ZERO4), (U8, CHW, ONE4, ZERO4), (F16, CHW, *IMAGENET), (BF16, HWC, (-1e30, 0.0, 1e-45, 3e38), (-0.0, 1e38, -1e-45, 0.0)), (F32, CHW, *IMAGENET)]


def test_tensor_size():
    lib = api.load_library()
    for (w, h) in [(1, 1), (37, 23), (3840, 2160)]:
        for rect in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, min(w, 64), min(h, 128)), (0, 0, w + 1, 1)]:
            for out in [(1, 2), (224, 224), (0, 5), (40000, 40000)]:
                for flags in (0, 3, 4):
                    for ch in (3, 4):
                        it = (7,) + rect + out + (flags,)
                        for f in GOOD_FORMATS:
                            assert api.tensor_size(w, h, 3, it, FILTER_AREA, ch, f) == tensors.size(resize.size(w, h, rect, out, flags, ch), f[0]), (w, h, it, ch, f[0])
                            assert api.tensor_size(w, h, 3, it, FILTER_BILINEAR, ch, f) == tensors.size(bilinear.size(w, h, rect, out, flags, ch), f[0]), (w, h, it, ch, f[0])
                        for f in BAD_FORMATS:
                            assert api.tensor_size(w, h, 3, it, FILTER_AREA, ch, f) == 0 and tensors.wrong(tensors.fmt(*f))
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    gw = warp.item(0, (1, 1, 2, 2), (5, 3))
    f16 = (F16, CHW, *IMAGENET)
    assert api.tensor_size(4, 4, 4, good, FILTER_AREA, 4, f16) == 120 and api.tensor_size(4, 4, 4, good, FILTER_BILINEAR, 3, (F32, HWC, *IMAGENET)) == 180
    assert api.warp_tensor_size(4, 4, 4, gw, 4, f16) == 120 and api.warp_tensor_size(4, 4, 4, gw, 3, GOOD_FORMATS[0]) == 45 == warp.size(4, 4, gw, 3)
    assert api.warp_tensor_size(4, 4, 4, gw[:13] + (1,) + gw[14:], 4, f16) == 0 and api.warp_tensor_size(4, 4, 4, warp.item(0, (1, 1, 4, 2), (5, 3)), 4, f16) == 0
    for filt in (2, -1):
        assert api.tensor_size(4, 4, 4, good, filt, 4, f16) == 0
    for f in BAD_FORMATS:
        assert api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0
    d, r, t = ctypes.byref(api.QoiDesc(4, 4, 4, 0)), ctypes.byref(api.QoimiResize(*good)), ctypes.byref(api.tensor_format(f16))
    assert lib.qoimi_tensor_size(d, r, 0, 4, t) == 120
    assert lib.qoimi_tensor_size(None, r, 0, 4, t) == 0 and lib.qoimi_tensor_size(d, None, 0, 4, t) == 0 and lib.qoimi_tensor_size(d, r, 0, 4, None) == 0
    assert lib.qoimi_tensor_size(d, r, 0, 5, t) == 0 and lib.qoimi_tensor_size(ctypes.byref(api.QoiDesc(4, 4, 5, 0)), r, 0, 4, t) == 0
    assert lib.qoimi_warp_tensor_size(d, ctypes.byref(api.QoimiWarp(*gw)), 4, None) == 0
    res = api.tensor_format(f16)
    res.reserved[1] = 1
    assert lib.qoimi_tensor_size(d, r, 0, 4, ctypes.byref(res)) == 0
    out = (ctypes.c_longlong * 4)(5, 6, 7, 8)
    lib.qoimi_tensor_stats(None, out)                                    # no context: zeros
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
    a.out = (ctypes.c_ubyte * 8192)()
    ctypes.memset(a.out, 0x5A, 8192)
    a.o = (ctypes.addressof(a.out) + 15) & ~15                   # a multiple of 16: the offsets are the alignment
    a.n = 3
    a.so = (ctypes.c_size_t * 3)(0, 1024, 2048)
    a.sizes = (ctypes.c_int * 3)(40, 0, 40)                      # image 1 is named by no item: its size and descriptor are garbage
    a.descs = (api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(130, 3, 4, 1))
    a.items = (api.QoimiResize * 2)(api.QoimiResize(0, 1, 1, 2, 2, 2, 2, 0), api.QoimiResize(2, 0, 0, 130, 1, 5, 1, 1))     # 4 and 5 pixels
    a.warps = (api.QoimiWarp * 2)(api.QoimiWarp(*warp.item(0, (1, 1, 2, 2), (2, 2))), api.QoimiWarp(*warp.item(2, (0, 0, 130, 1), (5, 1), flags=1)))
    a.oo = (ctypes.c_size_t * 2)(0, 1024)
    return a


def untouched(a):
    return bytes(a.out) == b"\x5A" * 8192 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx[:4096]) == b"\0" * 4096


def fm(f, reserved=(0, 0)):
    t = api.tensor_format(f)
    return api.QoimiTensorFormat(t.dtype, t.layout, t.scale, t.bias, (ctypes.c_uint * 2)(*reserved))


@pytest.mark.parametrize("warped", [False, True])
def test_rejections(args, warped):
    a = args
    f16 = (F16, CHW, *IMAGENET)

    def call(ctx=a.ctx, streams=a.p, so=a.so, sizes=a.sizes, descs=a.descs, n=a.n, ch=0, items=None, ni=2, filter=FILTER_BILINEAR, mode=0, f=fm(f16), out=a.o, oo=a.oo, staging=0):
        fp = None if f is None else ctypes.byref(f)
        if warped:
            return a.lib.qoimi_decode_warped_tensors(ctx, streams, so, sizes, descs, n, ch, a.warps if items is None else items, ni, mode, fp, out, oo, staging, None)
        return a.lib.qoimi_decode_tensors(ctx, streams, so, sizes, descs, n, ch, a.items if items is None else items, ni, filter, mode, fp, out, oo, staging, None)

    def o2(x, y):
        return (ctypes.c_size_t * 2)(x, y)

    def leaves():
        if warped:
            return (api.QoimiWarp * 2)(a.warps[0], api.QoimiWarp(*warp.item(2, (1, 0, 130, 1), (5, 1))))
        return (api.QoimiResize * 2)(a.items[0], api.QoimiResize(2, 1, 0, 130, 1, 5, 1, 0))

    def huge():
        """an output of 2^62 bytes as u8: four times that does not fit a size_t (the resampling items only: a warp's output stays small)"""
        return (api.QoimiResize * 2)(a.items[0], api.QoimiResize(2, 0, 0, 1, 1, 2 ** 31 - 1, 2 ** 31 + 1, 0))

    inf, nan = float("inf"), float("nan")
    calls = {
        "NULL ctx": (lambda: call(ctx=None), "NULL"), "NULL d_streams": (lambda: call(streams=None), "NULL"), "NULL stream_offsets": (lambda: call(so=None), "NULL"),
        "NULL sizes": (lambda: call(sizes=None), "NULL"), "NULL descs": (lambda: call(descs=None), "NULL"), "NULL d_out": (lambda: call(out=None), "NULL"),
        "NULL out_offsets": (lambda: call(oo=None), "NULL"), "n_images 0": (lambda: call(n=0), "empty"), "n_items 0": (lambda: call(ni=0), "empty"), "n_items -1": (lambda: call(ni=-1), "empty"),
        "channels 1": (lambda: call(ch=1), "channels"), "channels 5": (lambda: call(ch=5), "channels"), "mode 2": (lambda: call(mode=2), "mode"), "mode -1": (lambda: call(mode=-1), "mode"),
        "NULL format": (lambda: call(f=None), "format is NULL"),
        "dtype 4": (lambda: call(f=fm((4, HWC, ONE4, ZERO4))), "dtype"), "dtype 2^32-1": (lambda: call(f=fm((2 ** 32 - 1, HWC, ONE4, ZERO4))), "dtype"),
        "layout 2": (lambda: call(f=fm((F16, 2, ONE4, ZERO4))), "layout"), "layout 2^31": (lambda: call(f=fm((F32, 2 ** 31, ONE4, ZERO4))), "layout"),
        "reserved[0]": (lambda: call(f=fm(f16, (1, 0))), "reserved"), "reserved[1]": (lambda: call(f=fm(f16, (0, 2 ** 31))), "reserved"),
        "scale inf": (lambda: call(f=fm((F32, HWC, (1.0, 1.0, 1.0, inf), ZERO4))), "finite"), "scale -inf": (lambda: call(f=fm((F16, HWC, (-inf, 1.0, 1.0, 1.0), ZERO4))), "finite"),
        "scale nan": (lambda: call(f=fm((BF16, CHW, (1.0, nan, 1.0, 1.0), ZERO4))), "finite"), "bias inf": (lambda: call(f=fm((F32, HWC, ONE4, (0.0, inf, 0.0, 0.0)))), "finite"),
        "bias nan": (lambda: call(f=fm((F32, HWC, ONE4, (0.0, 0.0, 0.0, nan)))), "finite"), "U8 with a nan": (lambda: call(f=fm((U8, HWC, (nan, 1.0, 1.0, 1.0), ZERO4))), "finite"),
        "U8 scale 2": (lambda: call(f=fm((U8, HWC, (1.0, 2.0, 1.0, 1.0), ZERO4))), "QOIMI_TENSOR_U8"), "U8 bias 1": (lambda: call(f=fm((U8, CHW, ONE4, (0.0, 0.0, 1.0, 0.0)))), "QOIMI_TENSOR_U8"),
        "U8 bias -0": (lambda: call(f=fm((U8, HWC, ONE4, (0.0, 0.0, 0.0, -0.0)))), "QOIMI_TENSOR_U8"), "U8 alpha scale with 3 channels": (lambda: call(ch=3, f=fm((U8, HWC, (1.0, 1.0, 1.0, 0.0), ZERO4))), "QOIMI_TENSOR_U8"),
        "image == n_images": (lambda: call(n=2), "no image"), "the rectangle leaves": (lambda: call(items=leaves()), "leaves"),
        "referenced size 21": (lambda: call(sizes=(ctypes.c_int * 3)(40, 0, 21)), "shorter"), "descriptor": (lambda: call(descs=(api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(130, 3, 5, 0))), "descriptor"),
        "mixed channels": (lambda: call(descs=(api.QoiDesc * 3)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(0, 0, 9, 9), api.QoiDesc(130, 3, 3, 0))), "channel"),
        # sizes in bytes: item 0 is 4 pixels x 4 channels x 2 bytes = 32 bytes at f16, 64 at f32, 16 as u8
        "outputs overlap by one element": (lambda: call(oo=o2(0, 30)), "overlap"), "outputs overlap at f32 only": (lambda: call(oo=o2(0, 32), f=fm((F32, HWC, ONE4, ZERO4))), "overlap"),
        "outputs coincide": (lambda: call(oo=o2(64, 64)), "overlap"), "outputs overlap, item 1 in front": (lambda: call(oo=o2(100, 62)), "overlap"),
        "output offset wraps the address space": (lambda: call(oo=o2(0, 2 ** 64 - 8)), "address space"),
        "output end wraps at f16 only": (lambda: call(oo=o2(0, 2 ** 64 - a.o - 30)), "address space"),
        "item 0 at an odd address": (lambda: call(oo=o2(1, 1024)), "multiple of the element size"), "item 1 at an odd address": (lambda: call(oo=o2(0, 1023)), "multiple of the element size"),
        "f32 at 2 mod 4": (lambda: call(oo=o2(0, 1026), f=fm((F32, CHW, ONE4, ZERO4))), "multiple of the element size"),
        "bf16 at an odd address": (lambda: call(oo=o2(2049, 0), f=fm((BF16, HWC, ONE4, ZERO4))), "multiple of the element size"),
        # the order: each fault in front of all the later ones
        "order: mode before the format": (lambda: call(mode=3, f=None), "mode"), "order: NULL format before its fields and the items": (lambda: call(f=None, items=leaves(), oo=o2(1, 1)), "format is NULL"),
        "order: dtype before layout": (lambda: call(f=fm((9, 9, (nan,) * 4, ZERO4), (1, 1))), "dtype"), "order: layout before reserved": (lambda: call(f=fm((F16, 9, (nan,) * 4, ZERO4), (1, 1))), "layout"),
        "order: reserved before finite": (lambda: call(f=fm((U8, HWC, (nan,) * 4, ZERO4), (1, 1))), "reserved"), "order: the format before the items": (lambda: call(f=fm((F16, 2, ONE4, ZERO4)), items=leaves()), "layout"),
        "order: the items before the alignment": (lambda: call(items=leaves(), oo=o2(1, 1025)), "leaves"), "order: overlap before the alignment": (lambda: call(oo=o2(1, 3)), "overlap"),
    }
    if not warped:
        calls.update({"filter 2": (lambda: call(filter=2), "filter"), "filter -1": (lambda: call(filter=-1), "filter"), "order: the filter first": (lambda: call(filter=7, ctx=None, f=None), "filter"),
                      "reduced by 33 under the tents": (lambda: call(items=(api.QoimiResize * 2)(a.items[0], api.QoimiResize(2, 0, 0, 130, 1, 3, 1, 0))), "32"),
                      "... by 65 under the area filter": (lambda: call(filter=FILTER_AREA, items=(api.QoimiResize * 2)(a.items[0], api.QoimiResize(2, 0, 0, 130, 1, 2, 1, 0))), "64"),
                      "bytes that do not fit a size_t": (lambda: call(filter=FILTER_AREA, items=huge(), f=fm((F32, HWC, ONE4, ZERO4))), "address space")})
    for name, (c, word) in calls.items():
        assert c() == E_ARG, name
        assert word in api.last_error(), (name, api.last_error())
        assert untouched(a), name
    # U8 with scale 1 and bias +0, and every accepted format, get as far as the output ranges
    for f in GOOD_FORMATS:
        assert call(f=fm(f), oo=o2(64, 64)) == E_ARG and "overlap" in api.last_error(), f[:2]
    # as u8 the outputs stand side by side at 16 bytes; element-aligned offsets of every size get as far as the plan's sub-batches ... which need a context: not called here
    assert untouched(a)
    # (an accepted call goes on to the context and the device: tests/test_gpu_tensors.py)


def test_python_wrapper_checks_its_lengths():
    ctx = api.Context.__new__(api.Context)                      # no device: the length checks come first
    ctx._h = None
    d = [api.QoiDesc(2, 2, 4, 0)] * 2
    f = (F16, CHW, *IMAGENET)
    ok, okw = (0, 0, 0, 1, 1, 1, 1, 0), warp.item(0, (0, 0, 1, 1), (1, 1))
    with pytest.raises(api.QoiError):
        ctx.decode_tensors(1, [0], [40, 40], d, 0, [ok], FILTER_AREA, 0, f, 1, [0])
    with pytest.raises(api.QoiError):
        ctx.decode_tensors(1, [0, 40], [40, 40], d, 0, [ok], FILTER_AREA, 0, f, 1, [0, 4])
    with pytest.raises(api.QoiError):
        ctx.decode_warped_tensors(1, [0, 40], [40, 40], d, 0, [okw[:8]], 0, f, 1, [0])
    with pytest.raises(api.QoiError):
        api.tensor_format((F16, CHW, (1.0, 1.0, 1.0), ZERO4))
