"""QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 in every layer, what can be checked without a GPU: the values 1024 and 2048 in the header, the model,
the core and the host's static_assert; the header's statement of the definition; qoimi_warp_size and qoimi_warp_tensor_size with the flags
and each border, 0 for the two new rejections, 512 still no flag; the two new kernels in the built library - no scratch, no spills, no AGPRs,
no LDS - and the six older warp kernels with the registers they had; the rejections the host reports before it looks at the context (a block
of zeroed host memory stands in for one), in their order, for the u8 and the tensor call; the option of the tool and its argument check."""
import ctypes
import os
import re

from qoi_amd import api, tensors, warp
from qoi_amd.tensors import CHW, F16
from qoi_amd.warp import BICUBIC, NEAREST, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, WRAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
F16_CHW = (F16, CHW, *IMAGENET)
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
TWO_BORDERS = "more than one border of QOIMI_WARP_REPLICATE, QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP"
BOTH = "QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 together"
BILINEAR_ONLY = "supersampling is defined for the bilinear sampling only"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_values_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    for name, value in (("SUPER2", 1024), ("SUPER4", 2048)):
        assert re.search(r"QOIMI_WARP_%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(warp, name) == value
    for text in ("Us = s * U + 2i + 1 - s", "Vs = s * V + 2j + 1 - s", "Px = ((a * Us + b * Vs) >> L) + c", "Py = ((d * Us + e * Vs) >> L) + f",
                 "(N_c + 2^(33 + 2L)) >> (34 + 2L)", "(M_c + A / 2) / A", "with ONE rounding", "Each tap is treated on its own", "Us, Vs < 2^23",
                 "|a * Us + b * Vs| < 2^55", "N_c <= 255 * 2^38 < 2^46", "M_c < 2^54", "the exact s x s box average with one rounding",
                 "qoimi_decode_thumbnails at factor s", "There is NO", "adaptivity", "Beyond 4 : 1 the result still aliases", "512 are not",
                 "1, 4, 16, 64, 128, 256, 1024 and 2048", "supersampling is defined for the bilinear", "qoi_amd/csrc/qoi_warp_super_core.h",
                 "NO ANTIALIASING", "antialiasing of reducing maps", "supersampling beyond 4 x 4", "supersampled bicubic or nearest"):
        assert text in header, text
    staged = read("qoi_amd", "csrc", "qoi_host_staged.hip")
    assert re.search(r"static_assert\([^;]*QOIMI_WARP_SUPER2 == \(int\)kWarpSuper2[^;]*QOIMI_WARP_SUPER4 == \(int\)kWarpSuper4", staged)
    rules = read("qoi_amd", "csrc", "qoi_staged.h")
    assert BOTH in rules and BILINEAR_ONLY in rules and "kWarpKernelSuper" in rules
    assert rules.index("unknown flag bit") < rules.index("QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together") < rules.index(TWO_BORDERS) < rules.index('"' + BOTH) \
        < rules.index('"' + BILINEAR_ONLY) < rules.index('"reserved is not 0"', rules.index(TWO_BORDERS))
    core = read("qoi_amd", "csrc", "qoi_warp_super_core.h")
    assert re.search(r"kWarpSuper2 = 1024, kWarpSuper4 = 2048", core)
    assert "warp_axis(" in core and "warp_border_axis(" in core and "resize_pixel(" in core and "warp_border_work<WEIGHTED>(" in core    # shared, not restated
    code = re.sub(r"//.*", "", core)
    assert " % " not in code and " / " not in code                     # no division of its own: resize_pixel's resize_div only
    assert "qoi_warp_super.hip" in read("qoi_amd", "csrc", "sources.mk") and "qoi_warp_super.hip" in read("DESIGN.md")
    kernels = read("qoi_amd", "csrc", "qoi_kernels.h")
    assert "launch_warp_super(" in kernels and "launch_tensor_warp_super(" in kernels
    assert "launch_warp_super" in staged and "launch_tensor_warp_super" in read("qoi_amd", "csrc", "qoi_host_tensor.hip")
    # the other work items have no new branch
    for name in ("qoi_warp_core.h", "qoi_warp_cubic_core.h", "qoi_warp_border_core.h", "qoi_gather_tiles.h", "qoi_warp.hip", "qoi_warp_cubic.hip", "qoi_warp_border.hip",
                 "qoi_tensor.hip"):
        assert "kWarpSuper" not in read("qoi_amd", "csrc", name) and "warp_super" not in read("qoi_amd", "csrc", name), name


def test_the_kernels_in_the_built_library():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("warp_super_bytes", "warp_super_tensor"):
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
        print(name, k)                                                     # (DESIGN.md 4i-4 records the VGPR count)
    for name, vgpr in (("warp_gather", 42), ("tensor_warp", 42), ("warp_bicubic_bytes", 56), ("warp_bicubic_tensor", 56), ("warp_border_bytes", 59),
                       ("warp_border_tensor", 59)):                        # as they were
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["vgpr"] == vgpr and k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
    table = re.search(r"qoimi_kernel_name\(int i\) \{(.*?)\};", read("qoi_amd", "csrc", "qoi_host.hip"), re.S).group(1)
    assert "warp" not in table


def item(flags, rect=(1, 1, 6, 5), out=(9, 7)):
    return warp.item(0, rect, out, warp.rotation(rect[2:], out, 30.0, 0.5), flags, 0x01020304)


def test_the_size_functions_take_the_flags():
    for flag in (SUPER2, SUPER4):
        for border in BORDERS:
            for ch in (3, 4):
                assert api.warp_size(8, 8, 4, item(border | flag), ch) == 63 * ch == warp.size(8, 8, item(border | flag), ch), (border, flag)
                assert api.warp_tensor_size(8, 8, 4, item(border | flag), ch, F16_CHW) == 126 * ch
    for flags in (SUPER2 | SUPER4, SUPER2 | SUPER4 | WRAP, SUPER2 | NEAREST, SUPER4 | NEAREST | REPLICATE, SUPER2 | BICUBIC, SUPER4 | BICUBIC | REFLECT,     # the new rejections
                  512, 512 | SUPER2, 4096 | SUPER4, SUPER2 | 1 | 64, SUPER4 | NEAREST | BICUBIC, 1 << 16, 1 << 31):                                        # no flag; the older ones
        assert api.warp_size(8, 8, 4, item(flags), 4) == 0 == warp.size(8, 8, item(flags), 4), flags
        assert api.warp_tensor_size(8, 8, 4, item(flags), 4, F16_CHW) == 0
    # the other limits stay in front of the flag rule and hold with the flags
    assert api.warp_size(8, 8, 4, item(SUPER2, out=(2 ** 20, 1)), 4) == 0 and api.warp_size(8, 8, 4, item(SUPER4, rect=(1, 1, 8, 5)), 4) == 0
    assert api.warp_size(8, 8, 4, item(SUPER4 | WRAP, out=(2 ** 20 - 1, 381)), 3) == (2 ** 20 - 1) * 381 * 3


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

        for flags in (512, 1 << 16, 1 << 31, 4096, 512 | SUPER2, SUPER2 | SUPER4 | 512, SUPER4 | NEAREST | BICUBIC | 2, SUPER2 | 1 | 64 | 32):     # 1. an unknown bit
            says(plain(flags), "unknown flag bit")
            says(plain(flags, reserved=1), "unknown flag bit")
        for flags in (SUPER2 | NEAREST | BICUBIC, SUPER2 | SUPER4 | NEAREST | BICUBIC | 1 | 64):                                               # 2. the two samplings
            says(plain(flags), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
            says(plain(flags, reserved=1), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
        for flags in (SUPER2 | 1 | 64, SUPER2 | SUPER4 | 128 | 256, SUPER4 | NEAREST | 1 | 256):                                               # 3. two borders
            says(plain(flags), TWO_BORDERS)
            says(plain(flags, reserved=1), TWO_BORDERS)
        for flags in (SUPER2 | SUPER4, SUPER2 | SUPER4 | REFLECT, SUPER2 | SUPER4 | NEAREST, SUPER2 | SUPER4 | BICUBIC | REPLICATE):             # 4. both SUPER flags
            says(plain(flags), BOTH)
            says(plain(flags, reserved=1), BOTH)
        for flags in (SUPER2 | NEAREST, SUPER4 | BICUBIC, SUPER4 | NEAREST | WRAP, SUPER2 | BICUBIC | REPLICATE):                             # 5. not the bilinear sampling
            says(plain(flags), BILINEAR_ONLY)
            says(plain(flags, reserved=1), BILINEAR_ONLY)
        for flags in (SUPER2, SUPER4 | REPLICATE, SUPER2 | REFLECT_101, SUPER4 | WRAP):                                                       # 6. reserved
            says(plain(flags, reserved=1), "reserved is not 0")
        # sizes, rectangle, output limits and offsets stay in front of the flag rule
        for it, word in [(plain(SUPER2 | SUPER4, rect=(0, 0, 0, 4)), "zero"), (plain(SUPER2 | NEAREST, rect=(19999, 0, 4, 4)), "leaves"),
                         (plain(SUPER2 | SUPER4, out_size=(2 ** 20, 4)), "2^20"), (plain(SUPER4 | BICUBIC, out_size=(20000, 20000)), "400 000 000"),
                         (plain(SUPER2 | SUPER4, matrix=(warp.ONE, 0, 2 ** 56, 0, warp.ONE, 0)), "2^56")]:
            assert warped(it, tensor) == E_ARG and word in api.last_error(), (it, api.last_error())
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)


def test_tool_option(tmp_path):
    """--supersample 1 | 2 | 4 is an option of the warp tool (an empty directory ends it behind the arguments: "no .qoi files"); 3 is no
    choice; 2 and 4 go with --sample bilinear only, by the tool's own check; the choices are the model's flags"""
    from tools import qoiwarp_mi355x as warp_tool
    assert warp_tool.SUPERSAMPLES == {1: 0, 2: warp.SUPER2, 4: warp.SUPER4}
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    base = [str(empty), "--rotate", "30", "--scale", "0.3", "-o", str(tmp_path / "o")]
    for s in ("1", "2", "4"):
        for border in warp_tool.BORDERS:
            assert warp_tool.main(base + ["--supersample", s, "--border", border], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    for sample in ("nearest", "bicubic"):
        assert warp_tool.main(base + ["--supersample", "1", "--sample", sample], out=lines.append) == 2 and lines[-1] == "no .qoi files"
        for s in ("2", "4"):
            assert warp_tool.main(base + ["--supersample", s, "--sample", sample], out=lines.append) == 2
            assert lines[-1] == "--supersample 2 or 4 goes with --sample bilinear only"
    n = len(lines)
    assert warp_tool.main(base + ["--supersample", "3"], out=lines.append) == 2 and len(lines) == n
    assert "--supersample 1|2|4" in warp_tool.__doc__ and not os.path.exists(tmp_path / "o")
