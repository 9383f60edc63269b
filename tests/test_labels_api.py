"""QOIMI_FILTER_NEAREST, QOIMI_TENSOR_I32 / _I64 and QOIMI_TENSOR_HW in every layer, what can be checked without a GPU: the enum values in the
header, the models and the host; the header's statement of the definitions; qoimi_tensor_size and qoimi_warp_tensor_size against
qoi_amd/tensors.py over qoi_amd/nearest.py and the other models; the values that stay no filter, no dtype and no layout; the kernel in the
built library, without scratch, spills and LDS and without a timer name; the rejections the host reports before it looks at the context (a
block of zeroed host memory stands in for one, host arrays for device buffers; the output keeps its bytes) and their order.  (What the
library does behind the rejections needs a device: tests/test_gpu_labels.py.)"""
import ctypes
import os
import re

import pytest

from qoi_amd import api, bilinear, nearest, resize, tensors, warp
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_AREA, FILTER_BICUBIC, FILTER_BILINEAR, FILTER_LANCZOS, FILTER_NEAREST, HW, HWC, I32, I64, U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
ONE4, ZERO4 = (1.0,) * 4, (0.0,) * 4
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FORMATS = [(U8, HWC, ONE4, ZERO4), (U8, HW, ONE4, ZERO4), (F16, CHW, *IMAGENET), (BF16, HW, *IMAGENET), (F32, HW, *IMAGENET), (I32, HWC, ONE4, ZERO4), (I32, CHW, ONE4, ZERO4),
           (I32, HW, ONE4, ZERO4), (I64, HWC, ONE4, ZERO4), (I64, CHW, ONE4, ZERO4), (I64, HW, ONE4, ZERO4)]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def model_size(u8_bytes, och, f):
    return tensors.size_hw(u8_bytes, och, f[0]) if f[1] == HW else tensors.size(u8_bytes, f[0])


def test_the_values_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    for name, value in (("QOIMI_FILTER_NEAREST", 9), ("QOIMI_TENSOR_I32", 5), ("QOIMI_TENSOR_I64", 6), ("QOIMI_TENSOR_HW", 3)):
        assert re.search(name + r"\s*=\s*%d\b" % value, header), name
    assert (FILTER_NEAREST, I32, I64, HW) == (9, 5, 6, 3)
    for text in ("8 is not a filter", "4 is not a dtype", "2 is not a layout", "qoi_amd/nearest.py", "k = ((2X + 1) * cw) / (2 * ow),  r = ((2Y + 1) * rh) / (2 * oh)",
                 "k < cw always holds", "Both modes give the same bytes", "it is qoimi_decode_crops", "column X * f + f / 2", "a = 65536 * cw / ow, e = 65536 * rh / oh",
                 "NO ratio limit", "little-endian two's-complement integer of 4 / 8 bytes", "only the FIRST channel (r) of each pixel is stored", "element\n * index Y * ow + X",
                 "the others are ignored but must still be finite", "or QOIMI_FILTER_NEAREST", "Not here: indexed forms, a majority (mode) filter",
                 "QOIMI_TENSOR_U8, QOIMI_TENSOR_I32 or QOIMI_TENSOR_I64 with a scale other than 1"):
        assert text in header, text
    assert "a nearest-neighbour FILTER of qoimi_decode_tensors" not in header and "integer class-index dtypes (int32, int64) for label maps" not in header
    host = read("qoi_amd", "csrc", "qoi_host_tensor.hip")
    assert "kNearestKind" in host and '"tensor_nearest"' in host and "launch_tensor_nearest" in host and "2, 4, 5, 7 and 8 are not filters" in host
    assert "launch_tensor_nearest" in read("qoi_amd", "csrc", "qoi_kernels.h") and "qoi_nearest.hip" in read("qoi_amd", "csrc", "sources.mk")
    core = read("qoi_amd", "csrc", "qoi_tensor_core.h")
    assert re.search(r"kTensorI32\s*=\s*5\b", core) and re.search(r"kTensorI64\s*=\s*6\b", core) and re.search(r"kTensorHW\s*=\s*3\b", core)
    kernel = read("qoi_amd", "csrc", "qoi_nearest.hip")
    assert "walk_tiles" in kernel and "__shared__" not in kernel and "nearest_work" in kernel


def test_the_kernel_is_built_without_scratch_and_has_no_timer_name():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "tensor_nearest" in k]
    assert len(hits) == 1, hits
    k = ks[hits[0]]
    assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["lds"] == 0 and k["agpr"] == 0, k
    lib = api.load_library()
    assert not any("nearest" in lib.qoimi_kernel_name(i).decode() for i in range(64))


def test_tensor_size_for_the_nearest_filter():
    w, h = 20000, 17000
    rects = [(0, 0, 1, 1), (3, 2, 16, 32), (0, 0, 16384, 1), (0, 0, 1, 16384), (0, 0, 16384, 16384), (0, 0, 16385, 1), (0, 0, 1, 16385), (w - 16384, h - 1, 16384, 1),
             (w - 16383, 0, 16384, 1), (0, 0, 0, 1)]
    outs = [(1, 1), (2, 1), (224, 224), (16384, 16384), (16385, 1), (1, 16385), (0, 1)]
    seen = set()
    for rect in rects:
        for out in outs:
            for flags in (0, 3, 4):
                for ch in (3, 4):
                    it = (5,) + rect + out + (flags,)
                    u8 = nearest.size(w, h, rect, out, flags, ch)
                    seen.add((u8 != 0, rect[2] > 64 * out[0] > 0, max(rect[2:] + out) > 16384))
                    for f in FORMATS:
                        assert api.tensor_size(w, h, 4, it, FILTER_NEAREST, ch, f) == model_size(u8, ch, f), (it, ch, f[:2])
    assert {(True, True, False), (True, False, False), (False, False, True), (False, True, True)} <= seen
    assert api.tensor_size(w, h, 4, (0, 0, 0, 16384, 16384, 1, 1, 0), FILTER_NEAREST, 4, FORMATS[-1]) == 8                     # 16384 to 1: no ratio limit
    assert api.tensor_size(w, h, 4, (0, 0, 0, 16384, 1, 1, 1, 0), FILTER_AREA, 4, FORMATS[-1]) == 0
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 4, (I64, HW, ONE4, ZERO4)) == 120 and api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 3, (I64, HW, ONE4, ZERO4)) == 120
    assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 3, (I32, CHW, ONE4, ZERO4)) == 180 and api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 4, (U8, HW, ONE4, ZERO4)) == 15
    assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 5, FORMATS[-1]) == 0


def test_the_new_formats_under_the_other_filters_and_the_warp():
    gw = warp.item(0, (1, 1, 2, 2), (5, 3), flags=warp.NEAREST)
    for (w, h) in [(4, 4), (37, 23)]:
        for rect in [(0, 0, 1, 1), (1, 1, 2, 2), (0, 0, w + 1, 1)]:
            for out in [(5, 3), (224, 224), (0, 5)]:
                for ch in (3, 4):
                    it = (7,) + rect + out + (1,)
                    wi = warp.item(7, rect, out)
                    for f in FORMATS:
                        for filt, model in ((FILTER_AREA, resize), (FILTER_BILINEAR, bilinear)):
                            assert api.tensor_size(w, h, 3, it, filt, ch, f) == model_size(model.size(w, h, rect, out, 1, ch), ch, f), (w, h, it, ch, f[:2])
                        assert api.warp_tensor_size(w, h, 3, wi, ch, f) == model_size(warp.size(w, h, wi, ch), ch, f), (w, h, wi, ch, f[:2])
    assert api.warp_tensor_size(4, 4, 4, gw, 4, (I64, HW, ONE4, ZERO4)) == 120 and api.warp_tensor_size(4, 4, 4, gw, 3, (I32, HWC, ONE4, ZERO4)) == 180
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    for filt in (FILTER_BICUBIC, FILTER_LANCZOS):
        assert api.tensor_size(4, 4, 4, good, filt, 4, (I64, HW, ONE4, ZERO4)) == 120 and api.tensor_size(4, 4, 4, good, filt, 4, (I32, CHW, ONE4, ZERO4)) == 240


def test_what_stays_rejected():
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    gw = warp.item(0, (1, 1, 2, 2), (5, 3))
    for filt in (2, 4, 5, 7, 8, 10, -1):
        assert api.tensor_size(4, 4, 4, good, filt, 4, (I64, HW, ONE4, ZERO4)) == 0, filt
    for dtype in (4, 7, 2 ** 32 - 1):
        f = (dtype, HWC, ONE4, ZERO4)
        assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 4, f) == 0 and api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0 and "dtype" in tensors.wrong(f), dtype
    for layout in (2, 4, 2 ** 31):
        f = (I64, layout, ONE4, ZERO4)
        assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 4, f) == 0 and api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0 and "layout" in tensors.wrong(f), layout
    for dtype in (I32, I64):
        for f in [(dtype, HW, (1.0, 1.0, 1.0, 0.5), ZERO4), (dtype, HWC, ONE4, (-0.0, 0.0, 0.0, 0.0)), (dtype, CHW, ONE4, (0.0, 1.0, 0.0, 0.0)), (dtype, HW, (float("nan"),) + ONE4[1:], ZERO4)]:
            assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 4, f) == 0 and api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0 and tensors.wrong(tensors.fmt(*f)), f
    assert api.tensor_size(4, 4, 4, good, FILTER_NEAREST, 4, (F32, HW, (1.0, 1.0, 1.0, float("inf")), ZERO4)) == 0        # ignored under HW, but finite


@pytest.fixture()
def args():
    class A:
        pass
    a = A()
    a.lib = api.load_library()
    a.fake_ctx = (ctypes.c_ubyte * (1 << 16))()                  # never looked at: every rejection comes first
    a.ctx = ctypes.addressof(a.fake_ctx)
    a.buf = (ctypes.c_ubyte * 4096)()
    a.p = ctypes.addressof(a.buf)
    a.out = (ctypes.c_ubyte * 8192)()
    ctypes.memset(a.out, 0x5A, 8192)
    a.o = (ctypes.addressof(a.out) + 15) & ~15                   # a multiple of 16: the offsets are the alignment
    a.so = (ctypes.c_size_t * 2)(0, 1024)
    a.sizes = (ctypes.c_int * 2)(40, 40)
    a.descs = (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(20000, 17000, 4, 1))
    a.items = [(0, 1, 1, 2, 2, 2, 2, 0), (1, 0, 0, 16384, 1, 5, 1, 1)]                  # 4 and 5 pixels; the second reduced by 3276
    a.warps = [warp.item(0, (1, 1, 2, 2), (2, 2), flags=warp.NEAREST), warp.item(1, (0, 0, 130, 1), (5, 1), flags=1)]
    return a


def untouched(a):
    return bytes(a.out) == b"\x5A" * 8192 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx) == b"\0" * (1 << 16)


def fm(f, reserved=(0, 0)):
    t = api.tensor_format(f)
    return api.QoimiTensorFormat(t.dtype, t.layout, t.scale, t.bias, (ctypes.c_uint * 2)(*reserved))


@pytest.mark.parametrize("warped", [False, True])
def test_rejections_and_their_order(args, warped):
    a = args
    i64hw = (I64, HW, ONE4, ZERO4)

    def call(ctx=a.ctx, ch=0, items=None, filter=FILTER_NEAREST, mode=0, f=fm(i64hw), oo=(0, 1024)):
        fp = None if f is None else ctypes.byref(f)
        o2 = (ctypes.c_size_t * 2)(*oo)
        if warped:
            arr = (api.QoimiWarp * 2)(*[api.QoimiWarp(*it) for it in (a.warps if items is None else items)])
            return a.lib.qoimi_decode_warped_tensors(ctx, a.p, a.so, a.sizes, a.descs, 2, ch, arr, 2, mode, fp, a.o, o2, 0, None)
        arr = (api.QoimiResize * 2)(*[api.QoimiResize(*it) for it in (a.items if items is None else items)])
        return a.lib.qoimi_decode_tensors(ctx, a.p, a.so, a.sizes, a.descs, 2, ch, arr, 2, filter, mode, fp, a.o, o2, 0, None)

    nan = float("nan")
    # item 0 is 4 pixels: 32 bytes as I64 HW, 16 as I32 HW, 128 as I64 HWC (4 channels), 4 as U8 HW
    calls = {
        "dtype 4": (lambda: call(f=fm((4, HW, ONE4, ZERO4))), "dtype"), "dtype 7": (lambda: call(f=fm((7, HWC, ONE4, ZERO4))), "dtype"),
        "layout 2": (lambda: call(f=fm((I64, 2, ONE4, ZERO4))), "layout"), "layout 4": (lambda: call(f=fm((I32, 4, ONE4, ZERO4))), "layout"),
        "I32 scale 2": (lambda: call(f=fm((I32, HW, (2.0, 1.0, 1.0, 1.0), ZERO4))), "QOIMI_TENSOR_I32 takes scale 1 and bias +0 only"),
        "I64 scale of an ignored channel": (lambda: call(f=fm((I64, HW, (1.0, 1.0, 1.0, 0.5), ZERO4))), "QOIMI_TENSOR_I64 takes scale 1 and bias +0 only"),
        "I64 bias 1": (lambda: call(f=fm((I64, CHW, ONE4, (0.0, 0.0, 1.0, 0.0)))), "QOIMI_TENSOR_I64"), "I32 bias -0": (lambda: call(f=fm((I32, HWC, ONE4, (-0.0, 0.0, 0.0, 0.0)))), "QOIMI_TENSOR_I32"),
        "HW with an infinite ignored scale": (lambda: call(f=fm((F32, HW, (1.0, 1.0, 1.0, float("inf")), ZERO4))), "finite"),
        "I64 at 4 mod 8": (lambda: call(oo=(4, 1024)), "multiple of the element size"), "I64, item 1 at 4 mod 8": (lambda: call(oo=(0, 1028)), "multiple of the element size"),
        "I32 at 2 mod 4": (lambda: call(oo=(0, 1026), f=fm((I32, HW, ONE4, ZERO4))), "multiple of the element size"),
        # overlap in bytes under HW: 32 bytes, not the 128 of HWC nor the 4 of u8 HW
        "I64 HW overlaps by one element": (lambda: call(oo=(0, 24)), "overlap"), "I64 HWC overlaps where HW does not": (lambda: call(ch=4, oo=(0, 120), f=fm((I64, HWC, ONE4, ZERO4))), "overlap"),
        "I64 HW side by side gets as far as the alignment": (lambda: call(oo=(0, 36)), "multiple of the element size"),
        "I32 HW side by side gets as far as the alignment": (lambda: call(oo=(0, 18), f=fm((I32, HW, ONE4, ZERO4))), "multiple of the element size"),
        "U8 HW overlaps by one byte": (lambda: call(oo=(0, 3), f=fm((U8, HW, ONE4, ZERO4))), "overlap"),
        "output end wraps at I64 only": (lambda: call(oo=(0, 2 ** 64 - a.o - 32)), "address space"),
        # the order
        "order: mode before the format": (lambda: call(mode=3, f=None), "mode"), "order: dtype before layout": (lambda: call(f=fm((7, 4, (nan,) * 4, ZERO4), (1, 1))), "dtype"),
        "order: layout before reserved": (lambda: call(f=fm((I64, 4, (nan,) * 4, ZERO4), (1, 1))), "layout"), "order: reserved before finite": (lambda: call(f=fm((I64, HW, (nan,) * 4, ZERO4), (1, 0))), "reserved"),
        "order: finite before the integer rule": (lambda: call(f=fm((I64, HW, (2.0, nan, 1.0, 1.0), ZERO4))), "finite"),
        "order: overlap before the alignment": (lambda: call(oo=(4, 12)), "overlap"),
    }
    if not warped:
        big = lambda it: [a.items[0], it]                          # noqa: E731
        calls.update({
            "filter 8": (lambda: call(filter=8), "filter"), "filter 10": (lambda: call(filter=10), "filter"), "order: the filter first": (lambda: call(filter=10, ctx=None, f=None), "filter"),
            "width 16385": (lambda: call(items=big((1, 0, 0, 16385, 1, 5, 1, 0))), "16384"), "height 16385": (lambda: call(items=big((1, 0, 0, 1, 16385, 1, 1, 0))), "16384"),
            "out_width 16385": (lambda: call(items=big((1, 0, 0, 1, 1, 16385, 1, 0))), "16384"), "out_height 16385": (lambda: call(items=big((1, 0, 0, 1, 1, 1, 16385, 0))), "16384"),
            "order: zero before the size": (lambda: call(items=big((1, 0, 0, 16385, 0, 1, 1, 4))), "zero"), "order: the flag before the size": (lambda: call(items=big((1, 0, 0, 16385, 1, 1, 1, 4))), "flag"),
            "order: leaves before the size": (lambda: call(items=big((1, 19999, 0, 16385, 1, 1, 1, 0))), "leaves"),
            "order: the format before the items": (lambda: call(f=fm((I64, 2, ONE4, ZERO4)), items=big((1, 0, 0, 16385, 1, 1, 1, 0))), "layout"),
            "order: the items before the alignment": (lambda: call(items=big((1, 0, 0, 16385, 1, 1, 1, 0)), oo=(4, 1028)), "16384"),
            "reduced by 3276 under the area filter": (lambda: call(filter=FILTER_AREA), "64"),
        })
    for name, (c, word) in calls.items():
        assert c() == E_ARG, name
        assert word in api.last_error(), (name, api.last_error())
        assert untouched(a), name
    if not warped:
        assert "QOIMI_FILTER_NEAREST" in (call(filter=8), api.last_error())[1] and "QOIMI_FILTER_LANCZOS" in api.last_error()
    # every new format - and 16384 to 5 under the nearest filter: no ratio limit - gets as far as the output ranges
    for f in FORMATS:
        assert call(f=fm(f), oo=(64, 64)) == E_ARG and "overlap" in api.last_error(), f[:2]
    assert untouched(a)
