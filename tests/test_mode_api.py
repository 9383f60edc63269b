"""QOIMI_FILTER_MODE in every layer, what can be checked without a GPU: the value in the header, the model and the host; the header's
statement of the definition; qoimi_tensor_size against qoi_amd/mode.py, and 0 just past each limit; the values that stay no filter; the
kernel in the built library - exactly one tensor_mode, without scratch, spills, AGPRs and with the LDS DESIGN.md states (none); the
rejections the host reports before it looks at the context (a block of zeroed host memory stands in for one, host arrays for device
buffers; the output keeps its bytes) and their order.  (What the library does behind the rejections needs a device:
tests/test_gpu_mode.py.)"""
import ctypes
import os
import re

import pytest

from qoi_amd import api, mode, tensors
from qoi_amd.tensors import CHW, F16, FILTER_MODE, FILTER_NEAREST, HW, HWC, I32, I64, U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
ONE4, ZERO4 = (1.0,) * 4, (0.0,) * 4
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FORMATS = [(U8, HWC, ONE4, ZERO4), (U8, HW, ONE4, ZERO4), (F16, CHW, *IMAGENET), (I32, CHW, ONE4, ZERO4), (I64, HWC, ONE4, ZERO4), (I64, HW, ONE4, ZERO4)]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def model_size(u8_bytes, och, f):
    return tensors.size_hw(u8_bytes, och, f[0]) if f[1] == HW else tensors.size(u8_bytes, f[0])


def test_the_value_in_every_layer_and_the_headers_statement():
    header = read("include", "qoi_mi355x.h")
    assert re.search(r"QOIMI_FILTER_MODE\s*=\s*11\b", header) and "/* 10 is not a filter */" in header
    assert FILTER_MODE == 11 and tensors._FILTERS[FILTER_MODE] is mode.mode
    for text in ("qoi_amd/mode.py", "first(Z) = (2 * Z * n_src + n_out - 1) / (2 * n_out)", "[first(Z), first(Z + 1))", "A pixel votes as a whole", "all four bytes as decoded",
                 "the winners are the values with the\n * largest count", "key = r << 24 | g << 16 | b << 8 | a", "the pixel QOIMI_FILTER_NEAREST would take",
                 "it is QOIMI_FILTER_NEAREST byte for byte", "all distinct gives QOIMI_FILTER_NEAREST at any size", "a constant\n * rectangle gives the constant",
                 "the cells are the f x g blocks", "width <= 16 * out_width and\n * height <= 16 * out_height (a cell is at most 16 x 16 pixels)",
                 "or QOIMI_FILTER_MODE (qoimi_decode_tensors only)", "Not here: indexed forms, a majority (mode) filter per channel",
                 "QOIMI_FILTER_NEAREST or QOIMI_FILTER_MODE with that filter", "after the vote"):
        assert text in header, text
    assert "a majority (mode) filter for REDUCING label maps (QOIMI_FILTER_NEAREST takes" not in header
    host = read("qoi_amd", "csrc", "qoi_host_tensor.hip")
    assert "kModeKind = {mode_item_wrong, mode_split, mode_tiles, nullptr, &qoimi_ctx::tensor_stats, \"tensor_mode\"}" in host and "launch_tensor_mode" in host
    assert "QOIMI_FILTER_MODE == 11" in host and "2, 4, 5, 7 and 8 are not filters, nor is 10" in host
    assert "launch_tensor_mode" in read("qoi_amd", "csrc", "qoi_kernels.h") and "qoi_mode.hip" in read("qoi_amd", "csrc", "sources.mk")
    core = read("qoi_amd", "csrc", "qoi_mode_core.h")
    assert re.search(r"kModeMaxRatio\s*=\s*16\b", core) and re.search(r"kModeMaxSize\s*=\s*16384\b", core) and re.search(r"kModeHold\s*=\s*4\b", core)
    assert (mode.MAX_RATIO, mode.MAX_SIZE, mode.HOLD, mode.MAX_LG) == (16, 16384, 4, 6) and re.search(r"kModeMaxLg\s*=\s*6\b", core)
    kernel = read("qoi_amd", "csrc", "qoi_mode.hip")
    assert "walk_tiles" in kernel and "__shared__" not in kernel and "mode_meet" in kernel and "TensorSink" in kernel


def test_the_kernel_is_built_once_without_scratch_agprs_and_lds():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "tensor_mode" in k]
    assert len(hits) == 1, hits
    k = ks[hits[0]]
    assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
    assert k["lds"] == 0 and "tensor_mode uses no LDS" in read("DESIGN.md")                 # the LDS figure DESIGN.md states
    lib = api.load_library()
    assert not any("mode" in lib.qoimi_kernel_name(i).decode() for i in range(64))


def test_tensor_size_agrees_with_the_model_and_is_0_past_each_limit():
    w, h = 20000, 17000
    rects = [(0, 0, 1, 1), (3, 2, 16, 32), (0, 0, 16384, 1), (0, 0, 1, 16384), (0, 0, 16384, 16384), (0, 0, 16385, 1), (0, 0, 1, 16385), (w - 16384, h - 1, 16384, 1),
             (w - 16383, 0, 16384, 1), (0, 0, 0, 1), (5, 5, 3584, 3584)]
    outs = [(1, 1), (2, 1), (1, 2), (224, 224), (1024, 1024), (1024, 1), (1, 1024), (16384, 16384), (16385, 1), (1, 16385), (1025, 1025), (0, 1)]
    seen = set()
    for rect in rects:
        for out in outs:
            for flags in (0, 3, 4):
                for ch in (3, 4):
                    it = (5,) + rect + out + (flags,)
                    u8 = mode.size(w, h, rect, out, flags, ch)
                    seen.add((u8 != 0, min(out) > 0 and (rect[2] > 16 * out[0] or rect[3] > 16 * out[1]), max(rect[2:] + out) > 16384))
                    for f in FORMATS:
                        assert api.tensor_size(w, h, 4, it, FILTER_MODE, ch, f) == model_size(u8, ch, f), (it, ch, f[:2])
    assert {(True, False, False), (False, True, False), (False, False, True), (False, True, True)} <= seen
    i64hw = FORMATS[-1]
    size = lambda rect, out: api.tensor_size(w, h, 4, (0,) + rect + out + (0,), FILTER_MODE, 4, i64hw)      # noqa: E731
    # just inside and just past each limit
    assert size((0, 0, 16, 16), (1, 1)) == 8 and size((0, 0, 17, 16), (1, 1)) == 0 and size((0, 0, 16, 17), (1, 1)) == 0
    assert size((0, 0, 32, 48), (2, 3)) == 48 and size((0, 0, 33, 48), (2, 3)) == 0 and size((0, 0, 32, 49), (2, 3)) == 0
    assert size((0, 0, 16384, 3), (1024, 3)) == 8 * 3072 and size((0, 0, 16385, 3), (1025, 3)) == 0 and size((0, 0, 3, 16384), (3, 1024)) == 8 * 3072
    assert size((0, 0, 3, 16385), (3, 1025)) == 0 and size((0, 0, 1, 1), (16384, 1)) == 8 * 16384 and size((0, 0, 1, 1), (16385, 1)) == 0 and size((0, 0, 1, 1), (1, 16385)) == 0
    assert size((0, 0, 17, 1), (1, 1)) == 0 and api.tensor_size(w, h, 4, (0, 0, 0, 17, 1, 1, 1, 0), FILTER_NEAREST, 4, i64hw) == 8      # the nearest filter has no ratio limit
    assert size((w - 3, 0, 4, 1), (1, 1)) == 0 and size((0, 0, 4, 4), (2, 2)) == 32
    assert api.tensor_size(w, h, 4, (0, 0, 0, 4, 4, 2, 2, 0), FILTER_MODE, 5, i64hw) == 0


def test_what_stays_rejected():
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    for filt in (2, 4, 5, 7, 8, 10, 12, 13, -1, 11 + 256, 2 ** 31 - 1):
        assert api.tensor_size(4, 4, 4, good, filt, 4, (I64, HW, ONE4, ZERO4)) == 0, filt
        with pytest.raises(ValueError):
            tensors.tensors(None, good[1:5], good[5:7], 0, filt)
    assert api.tensor_size(4, 4, 4, good, FILTER_MODE, 4, (I64, HW, ONE4, ZERO4)) == 120


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
    a.items = [(0, 1, 1, 2, 2, 2, 2, 0), (1, 0, 0, 80, 16, 5, 1, 1)]                    # 4 and 5 pixels; the second reduced by exactly 16 in both axes
    return a


def untouched(a):
    return bytes(a.out) == b"\x5A" * 8192 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx) == b"\0" * (1 << 16)


def test_rejections_and_their_order(args):
    a = args
    fmt = api.tensor_format((I64, HW, ONE4, ZERO4))

    def call(ctx=a.ctx, ch=0, items=None, filter=FILTER_MODE, mode_=0, f=fmt, oo=(0, 1024)):
        fp = None if f is None else ctypes.byref(f)
        arr = (api.QoimiResize * 2)(*[api.QoimiResize(*it) for it in (a.items if items is None else items)])
        return a.lib.qoimi_decode_tensors(ctx, a.p, a.so, a.sizes, a.descs, 2, ch, arr, 2, filter, mode_, fp, a.o, (ctypes.c_size_t * 2)(*oo), 0, None)

    big = lambda it: [a.items[0], it]                              # noqa: E731
    calls = {
        "filter 10": (lambda: call(filter=10), "filter"), "filter 12": (lambda: call(filter=12), "filter"), "order: the filter first": (lambda: call(filter=12, ctx=None, f=None), "filter"),
        "width 81 to 5": (lambda: call(items=big((1, 0, 0, 81, 16, 5, 1, 0))), "16 in an axis"), "height 17 to 1": (lambda: call(items=big((1, 0, 0, 80, 17, 5, 1, 0))), "16 in an axis"),
        "width 16385": (lambda: call(items=big((1, 0, 0, 16385, 1, 1025, 1, 0))), "16384"), "height 16385": (lambda: call(items=big((1, 0, 0, 1, 16385, 1, 1025, 0))), "16384"),
        "out_width 16385": (lambda: call(items=big((1, 0, 0, 1, 1, 16385, 1, 0))), "16384"), "out_height 16385": (lambda: call(items=big((1, 0, 0, 1, 1, 1, 16385, 0))), "16384"),
        # the order: the rectangle rules (zero, flag, leaves), the ratio, the size
        "order: zero before the flag": (lambda: call(items=big((1, 19999, 0, 16385, 0, 1, 1, 4))), "zero"), "order: the flag before leaves": (lambda: call(items=big((1, 19999, 0, 16385, 1, 1, 1, 4))), "flag"),
        "order: leaves before the ratio": (lambda: call(items=big((1, 19999, 0, 16385, 1, 1, 1, 0))), "leaves"),
        "order: the ratio before the size": (lambda: call(items=big((1, 0, 0, 16385, 1, 1, 1, 0))), "16 in an axis"),
        "order: item by item": (lambda: call(items=[(1, 0, 0, 1, 1, 16385, 1, 0), (1, 0, 0, 81, 16, 5, 1, 0)]), "16384"),
        "order: mode before the items": (lambda: call(mode_=3, items=big((1, 0, 0, 81, 16, 5, 1, 0))), "mode"),
        "order: the format before the items": (lambda: call(f=api.tensor_format((I64, 2, ONE4, ZERO4)), items=big((1, 0, 0, 81, 16, 5, 1, 0))), "layout"),
        "order: the items before the overlap": (lambda: call(items=big((1, 0, 0, 81, 16, 5, 1, 0)), oo=(0, 8)), "16 in an axis"),
        "order: the items before the alignment": (lambda: call(items=big((1, 0, 0, 81, 16, 5, 1, 0)), oo=(4, 1028)), "16 in an axis"),
        "I64 at 4 mod 8": (lambda: call(oo=(4, 1024)), "multiple of the element size"),
    }
    for name, (c, word) in calls.items():
        assert c() == E_ARG, name
        assert word in api.last_error(), (name, api.last_error())
        assert untouched(a), name
    assert "QOIMI_FILTER_MODE" in (call(filter=10), api.last_error())[1] and "QOIMI_FILTER_NEAREST" in api.last_error()
    # a reduction by exactly 16 in both axes gets as far as the output ranges
    assert call(oo=(64, 64)) == E_ARG and "overlap" in api.last_error()
    assert untouched(a)
