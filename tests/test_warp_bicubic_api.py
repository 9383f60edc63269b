"""QOIMI_WARP_BICUBIC in every layer, what can be checked without a GPU: the value 16 in the header, the model, the core and the host's
static_assert; the header's statement of the definition; qoimi_warp_size and qoimi_warp_tensor_size with and without the flag, 8 stays no
flag and NEAREST | BICUBIC is rejected; the two new kernels in the built library - no scratch, no LDS, 64 VGPRs at most - and the two old ones
with the registers they had; the rejections the host reports before it looks at the context (a block of zeroed host memory stands in for
one), in their order; the option of the tool."""
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


def test_the_value_is_16_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    assert re.search(r"QOIMI_WARP_BICUBIC\s*=\s*16\b", header) and re.search(r"QOIMI_WARP_NEAREST\s*=\s*4\b", header)
    assert warp.BICUBIC == 16
    for text in ("k0 - 1, k0, k0 + 1, k0 + 2", "d = u + fr, fr, u - fr, 2u - fr", "W = 2u^3 = 2^52", "q_j = (c_j + 2^36) >> 37", "(0, 2^15, 0, 0)",
                 "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together", "a = -3/4", "clamp((N_c + 2^29) >> 30, 0, 255)", "keeps its weight",
                 "QOIMI_FILTER_BICUBIC", "differs by at most 1", "Lanczos in the warp", "antialiasing of reducing maps"):
        assert text in header, text
    staged = read("qoi_amd", "csrc", "qoi_host_staged.hip")
    assert re.search(r"static_assert\([^;]*QOIMI_WARP_BICUBIC == \(int\)kWarpBicubic", staged)
    assert "QOIMI_WARP_REPLICATE | QOIMI_WARP_NEAREST | QOIMI_WARP_BICUBIC" in read("qoi_amd", "csrc", "qoi_staged.h")
    core = read("qoi_amd", "csrc", "qoi_warp_cubic_core.h")
    assert re.search(r"kWarpBicubic\s*=\s*16\b", core) and "cubic_weight(" in core and "cubic_pixel(" in core
    assert "qoi_warp_cubic.hip" in read("qoi_amd", "csrc", "sources.mk")
    # the bilinear work item has no new branch
    assert "kWarpBicubic" not in read("qoi_amd", "csrc", "qoi_warp_core.h") and "kWarpBicubic" not in read("qoi_amd", "csrc", "qoi_gather_tiles.h")


def test_the_kernels_in_the_built_library():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("warp_bicubic_bytes", "warp_bicubic_tensor"):
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] <= 64, (name, k)                                  # eight wavefronts per SIMD by registers
        assert not any(s in hit for s in ("warp_gather", "tensor_warp", "tensor_cubic", "tensor_nearest"))
    for name in ("warp_gather", "tensor_warp"):                             # as they were: 42 VGPRs each before the flag existed
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["vgpr"] == 42 and k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
    # no entry in the name table
    table = re.search(r"qoimi_kernel_name\(int i\) \{(.*?)\};", read("qoi_amd", "csrc", "qoi_host.hip"), re.S).group(1)
    assert "enc_slabs" in table and "warp" not in table and "tensor" not in table


def test_warp_size_takes_the_flag():
    def it(flags):
        return warp.item(0, (1, 1, 6, 5), (9, 7), warp.rotation((6, 5), (9, 7), 30.0), flags, 0x01020304)

    for flags in (16, 17):
        for ch in (3, 4):
            assert api.warp_size(8, 8, 4, it(flags), ch) == 63 * ch == warp.size(8, 8, it(flags), ch), flags
            assert api.warp_tensor_size(8, 8, 4, it(flags), ch, F16_CHW) == 126 * ch
    for flags in (20, 21, 8, 24, 18, 32, 48, 0x80000010):
        assert api.warp_size(8, 8, 4, it(flags), 4) == 0 == warp.size(8, 8, it(flags), 4), flags
        assert api.warp_tensor_size(8, 8, 4, it(flags), 4, F16_CHW) == 0
    # the other limits stay in front of the flag and hold with it
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 6, 5), (2 ** 20, 1), flags=16), 4) == 0
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 6, 5), (20000, 20000), flags=16), 4) == 0
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 8, 5), (9, 7), flags=16), 4) == 0
    assert api.warp_size(8, 8, 4, warp.item(0, (1, 1, 6, 5), (2 ** 20 - 1, 381), flags=17), 3) == (2 ** 20 - 1) * 381 * 3


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
        for flags in (8, 24, 18, 32, 0x80000010):
            assert warped(warp.item(0, (0, 0, 4, 4), (4, 4), flags=flags), tensor) == E_ARG and "item 0: unknown flag bit" in api.last_error(), flags
        for flags in (20, 21):
            assert warped(warp.item(0, (0, 0, 4, 4), (4, 4), flags=flags), tensor) == E_ARG
            assert "item 0: QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together" in api.last_error(), flags
        assert warped(warp.item(0, (0, 0, 4, 4), (4, 4), flags=20 | 32), tensor) == E_ARG and "unknown flag bit" in api.last_error()
        # the order stays: sizes, rectangle, output limits and offsets in front of the flag rule, reserved behind it - with the flag set too
        for item, word in [(warp.item(0, (0, 0, 0, 4), (4, 4), flags=20), "zero"), (warp.item(0, (19999, 0, 4, 4), (4, 4), flags=20), "leaves"),
                           (warp.item(0, (0, 0, 4, 4), (2 ** 20, 4), flags=20), "2^20"), (warp.item(0, (0, 0, 4, 4), (20000, 20000), flags=20), "400 000 000"),
                           (warp.item(0, (0, 0, 4, 4), (4, 4), (warp.ONE, 0, 2 ** 56, 0, warp.ONE, 0), flags=20), "2^56"),
                           (warp.item(0, (0, 0, 4, 4), (2 ** 20, 4), flags=16), "2^20"), (warp.item(0, (0, 0, 4, 4), (4, 4), flags=20)[:13] + (1,) + (0, 0), "together"),
                           (warp.item(0, (0, 0, 4, 4), (4, 4), flags=16)[:13] + (1,) + (0, 0), "reserved")]:
            assert warped(item, tensor) == E_ARG and word in api.last_error(), (item, api.last_error())
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)


def test_tool_option(tmp_path):
    """--sample bicubic is a choice of the warp tool (an empty directory ends it behind the arguments: "no .qoi files"); cubic is none"""
    from tools import qoiwarp_mi355x as warp_tool
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    for sample in ("bicubic", "nearest", "bilinear"):
        assert warp_tool.main([str(empty), "--rotate", "30", "--sample", sample, "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    n = len(lines)
    assert warp_tool.main([str(empty), "--rotate", "30", "--sample", "cubic", "-o", str(tmp_path / "o")], out=lines.append) == 2 and len(lines) == n
    assert "--sample bilinear|nearest|bicubic" in warp_tool.__doc__ and not os.path.exists(tmp_path / "o")
