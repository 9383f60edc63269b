"""QOIMI_WARP_VOTE2 and QOIMI_WARP_VOTE4 in every layer, what can be checked without a GPU: the values 8192 and 16384 in the header, the model,
the core and the host's static_assert; the header's statement of the definition; qoimi_warp_size and qoimi_warp_tensor_size with the flags
and each border, 0 for the two new rejections, 4096 still no flag; the two new kernels in the built library - no scratch, no spills, no
AGPRs, no LDS; the rejections the host reports before it looks at the context (a block of zeroed host memory stands in for one), in their
order and with their messages, for the u8 and the tensor call; the new choices of the tool."""
import ctypes
import os
import re

from qoi_amd import api, tensors, warp
from qoi_amd.tensors import HW, I64
from qoi_amd.warp import BICUBIC, NEAREST, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4, WRAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
I64_HW = tensors.fmt(I64, HW)                                          # the N x H x W a loss function takes
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
TWO_BORDERS = "more than one border of QOIMI_WARP_REPLICATE, QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP"
BOTH_SUPERS = "QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 together"
BILINEAR_ONLY = "supersampling is defined for the bilinear sampling only"
BOTH = "QOIMI_WARP_VOTE2 and QOIMI_WARP_VOTE4 together"
OWN = "the vote is a sampling of its own: QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4 with QOIMI_WARP_NEAREST, QOIMI_WARP_BICUBIC, QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_values_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    for name, value in (("VOTE2", 8192), ("VOTE4", 16384)):
        assert re.search(r"QOIMI_WARP_%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(warp, name) == value
    for text in ("MAJORITY VOTE", "The flags are a fourth sampling", "4096 is not a flag", "the 64-bit index tested before it is narrowed",
                 "the value is the dword `fill` as given", "Nothing outside R is ever read", "a value votes as a whole dword",
                 "the centre value if it is a winner", "r << 24 | g << 16 | b << 8 | a", "it does not", "och 3 drops alpha after the vote",
                 "No invented value", "49152 < 65536", "QOIMI_FILTER_MODE of qoimi_decode_tensors (U8, HWC)", "QOIMI_TILE_MODE at factor s",
                 "A constant rectangle stays the constant under any map with any of the four borders", "still skips pixels",
                 "1, 4, 16, 64, 128, 256, 1024, 2048, 8192 and 16384", "qoi_amd/csrc/qoi_warp_vote_core.h", "QOIMI_TENSOR_I64 with QOIMI_TENSOR_HW"):
        assert text in header, text
    assert "the mode filter in the warp" not in header
    staged = read("qoi_amd", "csrc", "qoi_host_staged.hip")
    assert re.search(r"static_assert\([^;]*QOIMI_WARP_VOTE2 == \(int\)kWarpVote2[^;]*QOIMI_WARP_VOTE4 == \(int\)kWarpVote4", staged)
    rules = read("qoi_amd", "csrc", "qoi_staged.h")
    assert BOTH in rules and OWN in rules and "kWarpKernelVote = 4" in rules and "(&kernels)[5]" in rules
    assert rules.index("unknown flag bit") < rules.index("QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together") < rules.index(TWO_BORDERS) < rules.index('"' + BOTH_SUPERS) \
        < rules.index('"' + BILINEAR_ONLY) < rules.index('"' + BOTH) < rules.index('"' + OWN) < rules.index('"reserved is not 0"', rules.index(TWO_BORDERS))
    core = read("qoi_amd", "csrc", "qoi_warp_vote_core.h")
    assert re.search(r"kWarpVote2 = 8192, kWarpVote4 = 16384", core) and "kWarpVotes = kWarpVote2 | kWarpVote4" in core
    for shared in ("warp_super_position(", "warp_fold_of(", "mode_word(", "mode_pick(", "warp_place(", "warp_super_work<WEIGHTED>("):    # shared, not restated
        assert shared in core, shared
    code = re.sub(r"//.*", "", core)
    assert " % " not in code and " / " not in code and "__shared__" not in code and "atomic" not in code
    assert "qoi_warp_vote.hip" in read("qoi_amd", "csrc", "sources.mk") and "qoi_warp_vote.hip" in read("DESIGN.md")
    kernels = read("qoi_amd", "csrc", "qoi_kernels.h")
    assert "launch_warp_vote(" in kernels and "launch_tensor_warp_vote(" in kernels
    assert "launch_warp_vote" in staged and '"warp_vote_bytes"' in staged
    tensor = read("qoi_amd", "csrc", "qoi_host_tensor.hip")
    assert "launch_tensor_warp_vote" in tensor and '"warp_vote_tensor"' in tensor
    # the other work items have no new branch
    for name in ("qoi_warp_core.h", "qoi_warp_cubic_core.h", "qoi_warp_border_core.h", "qoi_warp_super_core.h", "qoi_mode_core.h", "qoi_gather_tiles.h", "qoi_warp.hip",
                 "qoi_warp_cubic.hip", "qoi_warp_border.hip", "qoi_warp_super.hip", "qoi_tensor.hip", "qoi_mode.hip"):
        assert "kWarpVote" not in read("qoi_amd", "csrc", name) and "warp_vote" not in read("qoi_amd", "csrc", name), name


def test_the_kernels_in_the_built_library():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("warp_vote_bytes", "warp_vote_tensor"):
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, (name, k)
        print(name, k)                                                     # (DESIGN.md 4i-5 records the VGPR count)
    table = re.search(r"qoimi_kernel_name\(int i\) \{(.*?)\};", read("qoi_amd", "csrc", "qoi_host.hip"), re.S).group(1)
    assert "warp" not in table


def item(flags, rect=(1, 1, 6, 5), out=(9, 7)):
    return warp.item(0, rect, out, warp.rotation(rect[2:], out, 30.0, 0.5), flags, 0x01020304)


def test_the_size_functions_take_the_flags():
    for flag in (VOTE2, VOTE4):
        for border in BORDERS:
            for ch in (3, 4):
                assert api.warp_size(8, 8, 4, item(border | flag), ch) == 63 * ch == warp.size(8, 8, item(border | flag), ch), (border, flag)
                assert api.warp_tensor_size(8, 8, 4, item(border | flag), ch, I64_HW) == 63 * 8
    for flags in (VOTE2 | VOTE4, VOTE2 | VOTE4 | WRAP, VOTE2 | NEAREST, VOTE4 | NEAREST | REPLICATE, VOTE2 | BICUBIC, VOTE4 | BICUBIC | REFLECT, VOTE2 | SUPER2,      # the new rejections
                  VOTE4 | SUPER4 | WRAP, VOTE2 | SUPER4, VOTE4 | SUPER2 | REFLECT_101,
                  4096, 4096 | VOTE2, 4096 | VOTE4, 1 << 15, VOTE2 | 1 | 64, VOTE4 | NEAREST | BICUBIC, VOTE2 | SUPER2 | SUPER4, 1 << 16, 1 << 31):        # no flag; the older ones
        assert api.warp_size(8, 8, 4, item(flags), 4) == 0 == warp.size(8, 8, item(flags), 4), flags
        assert api.warp_tensor_size(8, 8, 4, item(flags), 4, I64_HW) == 0
    # the other limits stay in front of the flag rule and hold with the flags
    assert api.warp_size(8, 8, 4, item(VOTE2, out=(2 ** 20, 1)), 4) == 0 and api.warp_size(8, 8, 4, item(VOTE4, rect=(1, 1, 8, 5)), 4) == 0
    assert api.warp_size(8, 8, 4, item(VOTE4 | WRAP, out=(2 ** 20 - 1, 381)), 3) == (2 ** 20 - 1) * 381 * 3


def test_rejections_before_the_context_is_looked_at():
    lib = api.load_library()
    fake = ctypes.create_string_buffer(1 << 16)                      # stands in for a context: a rejected call never looks at it
    streams = ctypes.create_string_buffer(64)
    out = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))
    so, sz, ds = (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(64), (api.QoiDesc * 1)(api.QoiDesc(20000, 17000, 4, 0))
    fmt = api.tensor_format(I64_HW)

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
            assert warped(it, tensor) == E_ARG and api.last_error().endswith("item 0: " + text), (it, api.last_error())

        for flags in (4096, 1 << 15, 1 << 16, 1 << 31, 512, 4096 | VOTE2, VOTE2 | VOTE4 | 4096, VOTE4 | NEAREST | BICUBIC | 2, VOTE2 | 1 | 64 | 32, VOTE2 | SUPER2 | 512):   # 1. an unknown bit
            says(plain(flags), "unknown flag bit")
            says(plain(flags, reserved=1), "unknown flag bit")
        for flags in (VOTE2 | NEAREST | BICUBIC, VOTE2 | VOTE4 | SUPER2 | SUPER4 | NEAREST | BICUBIC | 1 | 64):                               # 2. the two samplings
            says(plain(flags), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
            says(plain(flags, reserved=1), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
        for flags in (VOTE2 | 1 | 64, VOTE2 | VOTE4 | 128 | 256, VOTE4 | NEAREST | 1 | 256, VOTE2 | SUPER2 | SUPER4 | 64 | 128):                 # 3. two borders
            says(plain(flags), TWO_BORDERS)
            says(plain(flags, reserved=1), TWO_BORDERS)
        for flags in (VOTE2 | SUPER2 | SUPER4, VOTE2 | VOTE4 | SUPER2 | SUPER4 | WRAP):                                                       # 4. both SUPER flags
            says(plain(flags), BOTH_SUPERS)
            says(plain(flags, reserved=1), BOTH_SUPERS)
        for flags in (VOTE2 | SUPER2 | NEAREST, VOTE2 | VOTE4 | SUPER4 | BICUBIC | REPLICATE):                                               # 5. a SUPER flag, not bilinear
            assert warped(plain(flags), tensor) == E_ARG and "item 0: " + BILINEAR_ONLY in api.last_error(), (flags, api.last_error())
            assert warped(plain(flags, reserved=1), tensor) == E_ARG and "item 0: " + BILINEAR_ONLY in api.last_error(), (flags, api.last_error())
        for flags in (VOTE2 | VOTE4, VOTE2 | VOTE4 | REFLECT, VOTE2 | VOTE4 | NEAREST, VOTE2 | VOTE4 | SUPER2, VOTE2 | VOTE4 | BICUBIC | REPLICATE):   # 6. both VOTE flags
            says(plain(flags), BOTH)
            says(plain(flags, reserved=1), BOTH)
        for flags in (VOTE2 | NEAREST, VOTE4 | BICUBIC, VOTE4 | NEAREST | WRAP, VOTE2 | SUPER2, VOTE4 | SUPER4 | REPLICATE, VOTE2 | SUPER4 | REFLECT_101):   # 7. not a sampling of its own
            says(plain(flags), OWN)
            says(plain(flags, reserved=1), OWN)
        for flags in (VOTE2, VOTE4 | REPLICATE, VOTE2 | REFLECT_101, VOTE4 | WRAP):                                                           # 8. reserved
            says(plain(flags, reserved=1), "reserved is not 0")
        # sizes, rectangle, output limits and offsets stay in front of the flag rule
        for it, word in [(plain(VOTE2 | VOTE4, rect=(0, 0, 0, 4)), "zero"), (plain(VOTE2 | NEAREST, rect=(19999, 0, 4, 4)), "leaves"),
                         (plain(VOTE2 | VOTE4, out_size=(2 ** 20, 4)), "2^20"), (plain(VOTE4 | BICUBIC, out_size=(20000, 20000)), "400 000 000"),
                         (plain(VOTE2 | VOTE4, matrix=(warp.ONE, 0, 2 ** 56, 0, warp.ONE, 0)), "2^56")]:
            assert warped(it, tensor) == E_ARG and word in api.last_error(), (it, api.last_error())
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)


def test_tool_option(tmp_path):
    """--sample vote2 | vote4 are choices of the warp tool beside bilinear, nearest and bicubic (an empty directory ends it behind the
    arguments: "no .qoi files"); vote3 is none; they go with every border; the existing --supersample check holds for them; the choices are
    the model's flags"""
    from tools import qoiwarp_mi355x as warp_tool
    assert warp_tool.VOTE_SAMPLES == {"vote2": warp.VOTE2, "vote4": warp.VOTE4}
    assert warp_tool.SAMPLES == {"bilinear": 0, "nearest": warp.NEAREST, "bicubic": warp.BICUBIC}
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    base = [str(empty), "--rotate", "30", "--scale", "0.3", "-o", str(tmp_path / "o")]
    for sample in ("vote2", "vote4"):
        for border in warp_tool.BORDERS:
            assert warp_tool.main(base + ["--sample", sample, "--border", border], out=lines.append) == 2 and lines[-1] == "no .qoi files"
        assert warp_tool.main(base + ["--sample", sample, "--supersample", "1"], out=lines.append) == 2 and lines[-1] == "no .qoi files"
        for s in ("2", "4"):
            assert warp_tool.main(base + ["--sample", sample, "--supersample", s], out=lines.append) == 2
            assert lines[-1] == "--supersample 2 or 4 goes with --sample bilinear only"
    n = len(lines)
    assert warp_tool.main(base + ["--sample", "vote3"], out=lines.append) == 2 and len(lines) == n
    assert "--sample bilinear|nearest|bicubic|vote2|vote4" in warp_tool.__doc__ and not os.path.exists(tmp_path / "o")
