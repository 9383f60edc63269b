"""QOIMI_WARP_PROJECTIVE in every layer, what can be checked without a GPU: the value 131072 in the header, the model, the core and the host's
static_assert; the header's statement of the definition; qoimi_warp_size and qoimi_warp_tensor_size with the flag, each sampling and each
border, 0 for the three new rejections, 32768 and 65536 still no flags; the two new kernels in the built library - no scratch, no spills,
no AGPRs, no LDS; the rejections the host reports before it looks at the context (a block of zeroed host memory stands in for one), in
their order and with their messages, for the u8 and the tensor call; reserved != 0 without the flag still rejected."""
import ctypes
import os
import re

from qoi_amd import api, tensors, warp
from qoi_amd.tensors import CHW, F16
from qoi_amd.warp import BICUBIC, NEAREST, PROJECTIVE, REFLECT, REFLECT_101, REPLICATE, SUPER2, SUPER4, VOTE2, VOTE4, WRAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
F16_CHW = tensors.fmt(F16, CHW)
BORDERS = (0, REPLICATE, REFLECT, REFLECT_101, WRAP)
SAMPLINGS = (0, NEAREST, BICUBIC)
TWO_BORDERS = "more than one border of QOIMI_WARP_REPLICATE, QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP"
OWN = "the vote is a sampling of its own"
WITH = ("the projective map is defined for the bilinear, nearest and bicubic samplings: QOIMI_WARP_PROJECTIVE with QOIMI_WARP_SUPER2, QOIMI_WARP_SUPER4, "
        "QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4")
OFFSETS = "|c| or |f| is 2^53 or more with QOIMI_WARP_PROJECTIVE"
HORIZON = "the denominator of QOIMI_WARP_PROJECTIVE falls below 1/8 inside the output"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_value_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    assert re.search(r"QOIMI_WARP_PROJECTIVE\s*=\s*131072\b", header) and warp.PROJECTIVE == 131072 == 1 << 17
    for text in ("QOIMI_WARP_PROJECTIVE = 131072 (1 << 17)", "32768 and 65536 are not", "g = (int16)(reserved & 0xFFFF) and h = (int16)(reserved >> 16)",
                 "without the flag reserved != 0 is rejected exactly as before", "every division and shift floors", "F = 14 + L, so F is 14..34",
                 "Uc = U - ow, Vc = V - oh", "W  = 2^F + g * Uc + h * Vc", "Px = floor(Nx * 2^F / W),  Py = floor(Ny * 2^F / W)", "From Px and Py on nothing changes",
                 "the useful range of g is 1 / ow", "|c| or |f| of 2^53 or more", "2^F - |g| * (ow - 1) - |h| * (oh - 1) < 2^(F - 3)", "at or above 1/8 inside the output",
                 "|Nx| < 2^52 + 2^52 + 2^53 =", "2^(F-3) <= W < 5 * 2^F < 2^37", "|Px| <= 8 * |Nx| < 2^57", "the bytes of the same item without the flag",
                 "so lines stay lines", "differs by at most 1", "less than 2^-17 of a pixel", "A constant rectangle stays the constant under",
                 "projective SUPER and VOTE items", "a free denominator at the origin", "coefficients wider than 16 bits", "a horizon inside the output",
                 "qoi_amd/csrc/qoi_warp_proj_core.h", "return 0 for the three new rejections"):
        assert text in header, text
    assert "supersampled bicubic or nearest, projective maps, a border" not in header           # no longer a gap as such
    staged = read("qoi_amd", "csrc", "qoi_host_staged.hip")
    assert re.search(r"static_assert\([^;]*QOIMI_WARP_PROJECTIVE == \(int\)kWarpProjective", staged)
    rules = read("qoi_amd", "csrc", "qoi_staged.h")
    assert WITH in rules and OFFSETS in rules and HORIZON in rules and "kWarpKernelProj = 5" in rules
    assert rules.index('"' + OWN) < rules.index('"' + WITH) < rules.index('"' + OFFSETS) < rules.index('"' + HORIZON) < rules.index('"reserved is not 0"', rules.index(TWO_BORDERS))
    core = read("qoi_amd", "csrc", "qoi_warp_proj_core.h")
    assert "kWarpProjective = 1u << 17" in core and "kWarpProjMaxOffset = 1ll << 53" in core
    for shared in ("warp_vote_work<WEIGHTED>(", "warp_place(", "warp_position(", "warp_border_pixel_at<WEIGHTED>(", "warp_cubic_pixel_at<WEIGHTED>(", "warp_nearest_at(",
                   "warp_pixel_at<WEIGHTED>("):                                                              # shared, not restated
        assert shared in core, shared
    code = re.sub(r"//.*", "", core)
    assert "__int128" not in code and " % " not in code and "__shared__" not in code and "atomic" not in code and "__syncthreads" not in code
    assert code.count(" / ") == 2 and code.count("1.0 / (double)W") == 2                                     # the reciprocal, nothing else divides
    assert "qoi_warp_proj.hip" in read("qoi_amd", "csrc", "sources.mk") and "qoi_warp_proj.hip" in read("DESIGN.md")
    kernels = read("qoi_amd", "csrc", "qoi_kernels.h")
    assert "launch_warp_proj(" in kernels and "launch_tensor_warp_proj(" in kernels and "int32_t g, h; };" in kernels
    assert "launch_warp_proj" in staged and '"warp_proj_bytes"' in staged
    tensor = read("qoi_amd", "csrc", "qoi_host_tensor.hip")
    assert "launch_tensor_warp_proj" in tensor and '"warp_proj_tensor"' in tensor
    # the other work items have no new branch
    for name in ("qoi_warp_core.h", "qoi_warp_cubic_core.h", "qoi_warp_border_core.h", "qoi_warp_super_core.h", "qoi_warp_vote_core.h", "qoi_gather_tiles.h", "qoi_warp.hip",
                 "qoi_warp_cubic.hip", "qoi_warp_border.hip", "qoi_warp_super.hip", "qoi_warp_vote.hip", "qoi_tensor.hip"):
        assert "kWarpProj" not in read("qoi_amd", "csrc", name) and "warp_proj" not in read("qoi_amd", "csrc", name), name


def test_the_kernels_in_the_built_library():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    for name in ("warp_proj_bytes", "warp_proj_tensor"):
        (hit,) = [k for k in ks if name in k]
        k = ks[hit]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0 and k["vgpr"] <= 64, (name, k)   # eight wavefronts per SIMD by registers
        print(name, k)                                                     # (DESIGN.md 4i-6 records the VGPR count)
    table = re.search(r"qoimi_kernel_name\(int i\) \{(.*?)\};", read("qoi_amd", "csrc", "qoi_host.hip"), re.S).group(1)
    assert "warp" not in table


def item(flags, proj=None, rect=(1, 1, 6, 5), out=(9, 7), matrix=None):
    return warp.item(0, rect, out, matrix or warp.rotation(rect[2:], out, 30.0, 0.5), flags, 0x01020304, proj=proj)


def test_the_size_functions_take_the_flag():
    # out 9 x 7: L = 4, F = 18; 2^18 - 8 |g| - 6 |h| >= 2^15
    for proj in ((0, 0), (1000, -2000), (-28672, 0), (0, 32767), (14336, -19114)):
        assert 2 ** 18 - 8 * abs(proj[0]) - 6 * abs(proj[1]) >= 2 ** 15
        for sampling in SAMPLINGS:
            for border in BORDERS:
                for ch in (3, 4):
                    it = item(sampling | border, proj)
                    assert api.warp_size(8, 8, 4, it, ch) == 63 * ch == warp.size(8, 8, it, ch), (proj, sampling, border)
                    assert api.warp_tensor_size(8, 8, 4, it, ch, F16_CHW) == 63 * ch * 2
    far = (warp.ONE, 0, 2 ** 53, 0, warp.ONE, 0)
    rejected = [item(SUPER2, (0, 0)), item(SUPER4 | WRAP, (1, 1)), item(VOTE2, (0, 0)), item(VOTE4 | REPLICATE, (5, 5)),                    # with a SUPER or VOTE flag
                item(0, (0, 0), matrix=far), item(NEAREST, (3, 4), matrix=(warp.ONE, 0, 0, 0, warp.ONE, -2 ** 53)),                         # the offsets
                item(0, (-28673, 0)), item(BICUBIC | REFLECT, (-20000, -12000)), item(NEAREST, (14337, -19114)), item(0, (32767, 32767)),          # the least denominator
                item(32768, (0, 0)), item(65536, (0, 0)), item(32768), item(65536), item(PROJECTIVE | (1 << 18)), item(1 << 18)]              # no flags
    for it in rejected:
        assert api.warp_size(8, 8, 4, it, 4) == 0 == warp.size(8, 8, it, 4), it
        assert api.warp_tensor_size(8, 8, 4, it, 4, F16_CHW) == 0
    # without the flag the offsets may reach 2^56 and reserved must be 0, as before
    assert api.warp_size(8, 8, 4, item(0, matrix=far), 4) == 63 * 4
    plain = item(BICUBIC)
    assert api.warp_size(8, 8, 4, plain[:13] + (1,) + plain[14:], 4) == 0 == api.warp_size(8, 8, 4, plain[:13] + (0x00010000,) + plain[14:], 4)
    # the other limits stay in front and hold with the flag
    assert api.warp_size(8, 8, 4, item(0, (0, 0), out=(2 ** 20, 1)), 4) == 0 and api.warp_size(8, 8, 4, item(0, (0, 0), rect=(1, 1, 8, 5)), 4) == 0
    assert api.warp_size(8, 8, 4, item(WRAP, (-14336, 10), out=(2 ** 20 - 1, 3)), 3) == (2 ** 20 - 1) * 3 * 3                          # F = 34


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

    P = PROJECTIVE
    far = (warp.ONE, 0, 2 ** 53, 0, warp.ONE, 0)
    horizon = warp.proj_reserved(19115, 0)                           # out 4 x 4: F = 16, 2^16 - 3 * 19115 < 2^13
    for tensor in (False, True):
        def says(it, text):
            assert warped(it, tensor) == E_ARG and api.last_error().split("item 0: ")[-1].startswith(text), (it, api.last_error())

        for flags in (P | 32768, P | 65536, 32768, 65536, P | 2, P | 4096, P | (1 << 18), P | (1 << 31), P | SUPER2 | 512):                  # an unknown bit first
            says(plain(flags, horizon, matrix=far), "unknown flag bit")
        says(plain(P | NEAREST | BICUBIC | VOTE2, horizon, matrix=far), "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together")
        says(plain(P | SUPER2 | 1 | 64, horizon, matrix=far), TWO_BORDERS)
        says(plain(P | SUPER2 | SUPER4, horizon, matrix=far), "QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 together")
        says(plain(P | SUPER2 | BICUBIC, horizon, matrix=far), "supersampling is defined for the bilinear sampling only")
        says(plain(P | VOTE2 | VOTE4, horizon, matrix=far), "QOIMI_WARP_VOTE2 and QOIMI_WARP_VOTE4 together")
        says(plain(P | VOTE4 | NEAREST, horizon, matrix=far), OWN)
        for flags in (SUPER2, SUPER4 | WRAP, VOTE2, VOTE4 | REPLICATE):                                                                   # 1. with a SUPER or VOTE flag
            says(plain(P | flags, horizon, matrix=far), WITH)
            says(plain(P | flags), WITH)
        for m in (far, (warp.ONE, 0, -2 ** 53, 0, warp.ONE, 0), (warp.ONE, 0, 0, 0, warp.ONE, 2 ** 55), (warp.ONE, 0, 0, 0, warp.ONE, -2 ** 53)):   # 2. the offsets
            says(plain(P | BICUBIC | WRAP, horizon, matrix=m), OFFSETS)
            says(plain(P, 0, matrix=m), OFFSETS)
        for g, h in ((19115, 0), (0, -19115), (-9557, 9558), (32767, 32767), (-32768, -32768)):                                           # 3. the least denominator
            says(plain(P | NEAREST, warp.proj_reserved(g, h)), HORIZON)
        for flags in (0, BICUBIC | WRAP, NEAREST | REPLICATE, SUPER2, VOTE4 | REFLECT):                                                   # reserved without the flag
            says(plain(flags, 1), "reserved is not 0")
            says(plain(flags, horizon), "reserved is not 0")
        # sizes, rectangle, output limits and the wider offsets stay in front of the flag rule
        for it, word in [(plain(P | SUPER2, horizon, rect=(0, 0, 0, 4)), "zero"), (plain(P | VOTE2, horizon, rect=(19999, 0, 4, 4)), "leaves"),
                         (plain(P | SUPER2, horizon, out_size=(2 ** 20, 4)), "2^20"), (plain(P | SUPER2, horizon, out_size=(20000, 20000)), "400 000 000"),
                         (plain(P | SUPER2, horizon, matrix=(warp.ONE, 0, 2 ** 56, 0, warp.ONE, 0)), "2^56")]:
            assert warped(it, tensor) == E_ARG and word in api.last_error(), (it, api.last_error())
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)
