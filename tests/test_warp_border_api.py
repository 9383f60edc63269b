"""QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP in every layer, what can be checked without a GPU: the values 64, 128 and
256 in the header, the model, the core and the host's static_assert; the header's statement of the definition; qoimi_warp_size and
qoimi_warp_tensor_size with the flags, 0 for two borders, 2, 8 and 32 still no flags; the two new kernels in the built library - no scratch,
no spills, no LDS - and the four old ones with the registers they had; the rejections the host reports before it looks at the context (a
block of zeroed host memory stands in for one), in their order, for the u8 and the tensor call; the option of the tool."""
import ctypes
import os
import re

from qoi_amd import api, tensors, warp
from qoi_amd.tensors import CHW, F16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
F16_CHW = (F16, CHW, *IMAGENET)
BORDERS = (warp.REFLECT, warp.REFLECT_101, warp.WRAP)
TWO_BORDERS = "more than one border of QOIMI_WARP_REPLICATE, QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_values_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    for name, value in (("REFLECT", 64), ("REFLECT_101", 128), ("WRAP", 256)):
        assert re.search(r"QOIMI_WARP_%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(warp, name) == value
    for text in ("dcba|abcd|dcba", "dcb|abcd|cba", "abcd|abcd|abcd", "P = 2n, m = k mod P", "m < n ? m : P - 1 - m", "P = 2n - 2", "m < n ? m : P - m",
                 "k mod n", "EACH TAP IS FOLDED ON ITS OWN", "nothing outside R is ever read", "cv2.BORDER_REFLECT_101", "2, 8 and 32 are not flags",
                 "a border per axis", "mixing reflect with a fill", "numpy.pad"):
        assert text in header, text
    staged = read("qoi_amd", "csrc", "qoi_host_staged.hip")
    assert re.search(r"static_assert\([^;]*QOIMI_WARP_REFLECT == \(int\)kWarpReflect[^;]*QOIMI_WARP_REFLECT_101 == \(int\)kWarpReflect101[^;]*QOIMI_WARP_WRAP == \(int\)kWarpWrap", staged)
    assert TWO_BORDERS in read("qoi_amd", "csrc", "qoi_staged.h")
    core = read("qoi_amd", "csrc", "qoi_warp_border_core.h")
    assert re.search(r"kWarpReflect = 64, kWarpReflect101 = 128, kWarpWrap = 256", core)
    assert "warp_blend<WEIGHTED>(" in core and "warp_cubic_blend<WEIGHTED>(" in core and "warp_cubic_weights(" in core      # shared, not restated
    assert " % " not in re.sub(r"//.*", "", core) and " / (double)" in core              # no integer division: the quotient estimate is a double's
    assert "qoi_warp_border.hip" in read("qoi_amd", "csrc", "sources.mk")
    # the other work items have no new branch
    for name in ("qoi_warp_core.h", "qoi_warp_cubic_core.h", "qoi_gather_tiles.h", "qoi_warp.hip", "qoi_warp_cubic.hip", "qoi_tensor.hip"):
        assert "kWarpReflect" not in read("qoi_amd", "csrc", name) and "kWarpWrap" not in read("qoi_amd", "csrc", name), name


def test_the_kernels_in_the_built_library():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("warp_border_bytes", "warp_border_tensor"):
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
        print(name, k)                                                     # (DESIGN.md 4i-3 records the VGPR count)
    for name, vgpr in (("warp_gather", 42), ("tensor_warp", 42), ("warp_bicubic_bytes", 56), ("warp_bicubic_tensor", 56)):   # as they were
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["vgpr"] == vgpr and k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
    table = re.search(r"qoimi_kernel_name\(int i\) \{(.*?)\};", read("qoi_amd", "csrc", "qoi_host.hip"), re.S).group(1)
    assert "warp" not in table


def item(flags, rect=(1, 1, 6, 5), out=(9, 7)):
    return warp.item(0, rect, out, warp.rotation(rect[2:], out, 30.0), flags, 0x01020304)


def test_the_size_functions_take_the_flags():
    for border in BORDERS:
        for sampling in (0, warp.NEAREST, warp.BICUBIC):
            for ch in (3, 4):
                assert api.warp_size(8, 8, 4, item(border | sampling), ch) == 63 * ch == warp.size(8, 8, item(border | sampling), ch), (border, sampling)
                assert api.warp_tensor_size(8, 8, 4, item(border | sampling), ch, F16_CHW) == 126 * ch
    for flags in (1 | 64, 1 | 128, 1 | 256, 64 | 128, 64 | 256, 128 | 256, 1 | 64 | 128 | 256, 4 | 64 | 256, 16 | 1 | 128,      # two borders
                  2 | 64, 8 | 128, 32 | 256, 32, 512, 0x80000040, 4 | 16 | 64):                                                # no flag; two samplings
        assert api.warp_size(8, 8, 4, item(flags), 4) == 0 == warp.size(8, 8, item(flags), 4), flags
        assert api.warp_tensor_size(8, 8, 4, item(flags), 4, F16_CHW) == 0
    # the other limits stay in front of the flag rule and hold with the flags
    assert api.warp_size(8, 8, 4, item(64, out=(2 ** 20, 1)), 4) == 0 and api.warp_size(8, 8, 4, item(128, rect=(1, 1, 8, 5)), 4) == 0
    assert api.warp_size(8, 8, 4, item(256 | 16, out=(2 ** 20 - 1, 381)), 3) == (2 ** 20 - 1) * 381 * 3


def test_rejections_before_the_context_is_looked_at():
    lib = api.load_library()
    fake = ctypes.create_string_buffer(1 << 16)                      # stands in for a context: a rejected call never looks at it
    streams = ctypes.create_string_buffer(64)
    out = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))
    so, sz, ds = (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(64), (api.QoiDesc * 1)(api.QoiDesc(20000, 17000, 4, 0))
    fmt = api.tensor_format(F16_CHW)

    def warped(it, tensor):
        arr = (api.QoimiWarp * 1)(api.QoimiWarp(*it))
        head = (ctypes.cast(fake, ctypes.c_void_p), streams, so, sz, ds, 1, 4, arr, 1, 0)
        tail = (out, (ctypes.c_size_t * 1)(0), 0, None)
        return lib.qoimi_decode_warped_tensors(*head, ctypes.byref(fmt), *tail) if tensor else lib.qoimi_decode_warped(*head, *tail)

    def plain(flags, reserved=0, rect=(0, 0, 4, 4), out_size=(4, 4), matrix=warp.IDENTITY):
        it = warp.item(0, rect, out_size, matrix, flags)
        return it[:13] + (reserved,) + it[14:]

    for tensor in (False, True):
        def says(it, text):
            assert warped(it, tensor) == E_ARG and "item 0: " + text in api.last_error(), (it, api.last_error())

        for flags in (2, 8, 32, 512, 0x80000040, 64 | 2, 128 | 8, 256 | 32, 64 | 128 | 32, 4 | 16 | 2, 4 | 16 | 64 | 128 | 32):     # 1. an unknown bit
            says(plain(flags), "unknown flag bit")
            says(plain(flags, reserved=1), "unknown flag bit")
        for flags in (4 | 16 | 64, 4 | 16 | 64 | 128, 4 | 16 | 1 | 256):                                                              # 2. the two samplings
            says(plain(flags), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
            says(plain(flags, reserved=1), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
        for flags in (1 | 64, 1 | 128, 1 | 256, 64 | 128, 64 | 256, 128 | 256, 1 | 64 | 128 | 256, 4 | 64 | 128, 16 | 1 | 256):         # 3. two borders
            says(plain(flags), TWO_BORDERS)
            says(plain(flags, reserved=1), TWO_BORDERS)
        for flags in (64, 128 | 4, 256 | 16):                                                                                         # 4. reserved
            says(plain(flags, reserved=1), "reserved is not 0")
        # sizes, rectangle, output limits and offsets stay in front of the flag rule
        for it, word in [(plain(64 | 128, rect=(0, 0, 0, 4)), "zero"), (plain(64 | 128, rect=(19999, 0, 4, 4)), "leaves"), (plain(1 | 256, out_size=(2 ** 20, 4)), "2^20"),
                         (plain(64 | 256, out_size=(20000, 20000)), "400 000 000"), (plain(1 | 64, matrix=(warp.ONE, 0, 2 ** 56, 0, warp.ONE, 0)), "2^56")]:
            assert warped(it, tensor) == E_ARG and word in api.last_error(), (it, api.last_error())
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)


def test_tool_option(tmp_path):
    """--border reflect | reflect101 | wrap are choices of the warp tool beside fill and replicate (an empty directory ends it behind the
    arguments: "no .qoi files"); mirror is none; the choices are the model's flags"""
    from tools import qoiwarp_mi355x as warp_tool
    assert warp_tool.BORDERS == {"fill": 0, "replicate": warp.REPLICATE, "reflect": warp.REFLECT, "reflect101": warp.REFLECT_101, "wrap": warp.WRAP}
    assert warp_tool.SAMPLES == {"bilinear": 0, "nearest": warp.NEAREST, "bicubic": warp.BICUBIC}
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    for border in warp_tool.BORDERS:
        for sample in ("bilinear", "nearest", "bicubic"):
            assert warp_tool.main([str(empty), "--rotate", "30", "--border", border, "--sample", sample, "-o", str(tmp_path / "o")], out=lines.append) == 2
            assert lines[-1] == "no .qoi files"
    n = len(lines)
    assert warp_tool.main([str(empty), "--rotate", "30", "--border", "mirror", "-o", str(tmp_path / "o")], out=lines.append) == 2 and len(lines) == n
    assert "--border fill|replicate|reflect|reflect101|wrap" in warp_tool.__doc__ and not os.path.exists(tmp_path / "o")
