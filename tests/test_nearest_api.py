"""QOIMI_WARP_NEAREST in every layer, what can be checked without a GPU: the value 4 in the header, the model, the core and the host's
static_assert; the header's statement of the definition; qoimi_warp_size and qoimi_warp_tensor_size with and without the flag, 2 and every
bit from 8 on stay no flags; the warp kernels in the built library, still without scratch; the rejections the host reports before it looks
at the context (a block of zeroed host memory stands in for one); the option of the tool."""
import ctypes
import os
import re

from qoi_amd import api, tensors, warp
from qoi_amd.tensors import CHW, F16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
F16_CHW = (F16, CHW, *IMAGENET)


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_value_is_4_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    assert re.search(r"QOIMI_WARP_NEAREST\s*=\s*4\b", header) and re.search(r"QOIMI_WARP_REPLICATE\s*=\s*1\b", header)
    assert warp.NEAREST == 4 and warp.REPLICATE == 1
    for text in ("column k = Px >> 17 and row r = Py >> 17", "[k << 17, (k + 1) << 17)", "with its centre at (2k + 1) << 16",
                 "a bit other than QOIMI_WARP_REPLICATE and QOIMI_WARP_NEAREST", "both modes give the same bytes", "every position is a pixel centre",
                 "qoimi_decode_warped_tensors and qoimi_decode_warped_indexed", "in this order", "integer class-index dtypes"):
        assert text in header, text
    staged = read("qoi_amd", "csrc", "qoi_host_staged.hip")
    assert re.search(r"static_assert\([^;]*QOIMI_WARP_NEAREST == \(int\)kWarpNearest", staged)
    assert "QOIMI_WARP_REPLICATE | QOIMI_WARP_NEAREST" in read("qoi_amd", "csrc", "qoi_staged.h")
    assert re.search(r"kWarpNearest\s*=\s*4\b", read("qoi_amd", "csrc", "qoi_warp_core.h"))


def test_the_warp_kernels_are_still_built_without_scratch():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("warp_gather", "tensor_warp"):                         # they carry the new branch
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0 and k["vgpr"] <= 64, (name, k)   # eight wavefronts per SIMD by registers


def test_warp_size_takes_the_flag():
    def it(flags):
        return warp.item(0, (1, 1, 6, 5), (9, 7), warp.rotation((6, 5), (9, 7), 30.0), flags, 0x01020304)

    for flags in (0, 1, 4, 5):
        for ch in (3, 4):
            assert api.warp_size(8, 8, 4, it(flags), ch) == 63 * ch == warp.size(8, 8, it(flags), ch), flags
            assert api.warp_tensor_size(8, 8, 4, it(flags), ch, F16_CHW) == 126 * ch
    for flags in (2, 3, 6, 7, 8, 12, 0x80000004, 0x80000000, 1 << 16):
        assert api.warp_size(8, 8, 4, it(flags), 4) == 0 == warp.size(8, 8, it(flags), 4), flags
        assert api.warp_tensor_size(8, 8, 4, it(flags), 4, F16_CHW) == 0
    # the other limits stay in front of the flag and hold with it
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 6, 5), (2 ** 20, 1), flags=4), 4) == 0
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 6, 5), (20000, 20000), flags=4), 4) == 0
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 8, 5), (9, 7), flags=4), 4) == 0
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 6, 5), (2 ** 20 - 1, 381), flags=4), 3) == (2 ** 20 - 1) * 381 * 3


def test_rejections_before_the_context_is_looked_at():
    lib = api.load_library()
    fake = ctypes.create_string_buffer(1 << 16)                      # stands in for a context: a rejected call never looks at it
    streams = ctypes.create_string_buffer(64)
    out = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))
    so, sz, ds = (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(64), (api.QoiDesc * 1)(api.QoiDesc(20000, 17000, 4, 0))
    fmt = api.tensor_format(F16_CHW)

    def warped(item, tensor=False):
        arr = (api.QoimiWarp * 1)(api.QoimiWarp(*item))
        head = (ctypes.cast(fake, ctypes.c_void_p), streams, so, sz, ds, 1, 4, arr, 1, 0)
        tail = (out, (ctypes.c_size_t * 1)(0), 0, None)
        return lib.qoimi_decode_warped_tensors(*head, ctypes.byref(fmt), *tail) if tensor else lib.qoimi_decode_warped(*head, *tail)

    for tensor in (False, True):
        for flags in (2, 6, 8, 0x80000004):
            assert warped(warp.item(0, (0, 0, 4, 4), (4, 4), flags=flags), tensor) == E_ARG and "item 0: unknown flag bit" in api.last_error(), flags
        # the order stays: sizes, rectangle, output limits and offsets in front of the flags, reserved behind them - with the flag set too
        for item, word in [(warp.item(0, (0, 0, 0, 4), (4, 4), flags=6), "zero"), (warp.item(0, (19999, 0, 4, 4), (4, 4), flags=6), "leaves"),
                           (warp.item(0, (0, 0, 4, 4), (2 ** 20, 4), flags=6), "2^20"), (warp.item(0, (0, 0, 4, 4), (20000, 20000), flags=6), "400 000 000"),
                           (warp.item(0, (0, 0, 4, 4), (4, 4), (warp.ONE, 0, 2 ** 56, 0, warp.ONE, 0), flags=6), "2^56"),
                           (warp.item(0, (0, 0, 4, 4), (2 ** 20, 4), flags=4), "2^20"), (warp.item(0, (0, 0, 4, 4), (4, 4), flags=4)[:13] + (1,) + (0, 0), "reserved")]:
            assert warped(item, tensor) == E_ARG and word in api.last_error(), (item, api.last_error())
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)


def test_tool_option(tmp_path):
    """--sample is a choice of the warp tool (an empty directory ends it behind the arguments: "no .qoi files"); the default stays"""
    from tools import qoiwarp_mi355x as warp_tool
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    for sample in ("nearest", "bilinear"):
        assert warp_tool.main([str(empty), "--rotate", "30", "--sample", sample, "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    assert warp_tool.main([str(empty), "--orient", "6", "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    n = len(lines)
    assert warp_tool.main([str(empty), "--rotate", "30", "--sample", "cubic", "-o", str(tmp_path / "o")], out=lines.append) == 2 and len(lines) == n
    assert "--sample bilinear|nearest" in warp_tool.__doc__ and not os.path.exists(tmp_path / "o")
