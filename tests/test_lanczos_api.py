"""QOIMI_FILTER_LANCZOS in every layer, what can be checked without a GPU: the enum value in the header, the model and the host; the header's
statement of the definition; qoimi_tensor_size against qoi_amd/tensors.py: size of qoi_amd/lanczos.py: size over a grid that holds every limit
on both sides; 2, 4, 5 and 7 stay no filters; the kernel in the built library, without scratch and within its LDS; the rejections the host reports before it looks at
the context (a block of zeroed host memory stands in for one); the options of the two tools."""
import ctypes
import os
import re

import numpy as np
import pytest

from qoi_amd import api, lanczos, tensors
from qoi_amd.tensors import BF16, CHW, F16, F32, FILTER_AREA, FILTER_BICUBIC, FILTER_BILINEAR, FILTER_LANCZOS, HWC, U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
ONE4, ZERO4 = (1.0,) * 4, (0.0,) * 4
IMAGENET = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FORMATS = [(U8, HWC, ONE4, ZERO4), (F16, CHW, *IMAGENET), (BF16, HWC, *IMAGENET), (F32, CHW, *IMAGENET)]


def test_the_value_is_6_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    assert re.search(r"QOIMI_FILTER_LANCZOS\s*=\s*6\b", header) and "nor are 4, 5 and 7" in header
    assert FILTER_LANCZOS == 6 and (FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC) == (0, 1, 3)
    for text in ("qoi_amd/lanczos.py", "T[i] = round(2^30 * sinc(i / 1024) * sinc(i / 3072))", "T[512] = 652756755", "T[1536] = -145057057", "-158126265",
                 "z = 1024 * d, i = z / u, r = z - i * u", "c(X, k) = T[i] * (u - r) + T[i + 1] * r", "at most 6 x 6 samples", "most 96 taps per axis",
                 "QOIMI_FILTER_LANCZOS, QOIMI_FILTER_AREA, QOIMI_FILTER_BILINEAR or QOIMI_FILTER_BICUBIC", "other Lanczos windows"):
        assert text in header, text
    assert "a = -3/4, Lanczos" not in header
    host = open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_host_tensor.hip")).read()
    assert "kLanczosKind" in host and '"tensor_lanczos"' in host and "launch_tensor_lanczos" in host
    assert "qoi_lanczos.hip" in open(os.path.join(ROOT, "qoi_amd", "csrc", "sources.mk")).read()


def test_the_kernel_is_built_without_scratch():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "tensor_lanczos" in k]
    assert len(hits) == 1, hits
    k = ks[hits[0]]
    assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
    assert k["lds"] == 2 * (1536 + 24576) <= 64 * 1024 and 3 * k["lds"] <= 160 * 1024 and k["vgpr"] <= 64, k     # three workgroups per CU by LDS, eight wavefronts per SIMD by registers


def test_tensor_size_over_the_limits():
    w, h = 20000, 17000
    rects = [(0, 0, 1, 1), (3, 2, 16, 32), (0, 0, 17, 1), (0, 0, 1, 33), (0, 0, 16384, 16384), (0, 0, 16385, 1), (0, 0, 1, 16385), (w - 16384, h - 1, 16384, 1),
             (w - 16383, 0, 16384, 1), (0, 0, 0, 1)]
    outs = [(1, 1), (1, 2), (2, 1), (1024, 1024), (1025, 1024), (16384, 16384), (16385, 1), (1, 16385), (224, 224), (0, 1)]
    seen = set()
    for rect in rects:
        for out in outs:
            for flags in (0, 3, 4):
                for ch in (3, 4):
                    it = (5,) + rect + out + (flags,)
                    u8 = lanczos.size(w, h, rect, out, flags, ch)
                    seen.add((u8 != 0, rect[2] > 16 * out[0] or rect[3] > 16 * out[1], max(rect[2:] + out) > 16384))
                    for f in FORMATS:
                        assert api.tensor_size(w, h, 4, it, FILTER_LANCZOS, ch, f) == tensors.size(u8, f[0]), (it, ch, f[0])
                    assert api.tensor_size(w, h, 4, it, 2, ch, FORMATS[1]) == 0 == api.tensor_size(w, h, 4, it, 7, ch, FORMATS[1])
    assert {(True, False, False), (False, True, False), (False, False, True)} <= seen
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    assert api.tensor_size(4, 4, 4, good, FILTER_LANCZOS, 4, FORMATS[1]) == 120 and api.tensor_size(4, 4, 4, good, FILTER_LANCZOS, 3, FORMATS[3]) == 180
    for filt in (2, 4, 5, 7, -1, 8):
        assert api.tensor_size(4, 4, 4, good, filt, 4, FORMATS[1]) == 0
    assert api.tensor_size(4, 4, 4, good, FILTER_LANCZOS, 4, (4, HWC, ONE4, ZERO4)) == 0 and api.tensor_size(4, 4, 4, good, FILTER_LANCZOS, 5, FORMATS[1]) == 0
    # where the filters differ: 17 to 32 times is the tent's alone, above 16384 the area filter's and the tent's
    assert api.tensor_size(64, 4, 4, (0, 0, 0, 64, 1, 2, 1, 0), FILTER_BILINEAR, 4, FORMATS[0]) == 8 and api.tensor_size(64, 4, 4, (0, 0, 0, 64, 1, 2, 1, 0), FILTER_LANCZOS, 4, FORMATS[0]) == 0
    assert api.tensor_size(4, 4, 4, (0, 0, 0, 1, 1, 16385, 1, 0), FILTER_AREA, 4, FORMATS[0]) == 4 * 16385 and api.tensor_size(4, 4, 4, (0, 0, 0, 1, 1, 16385, 1, 0), FILTER_LANCZOS, 4, FORMATS[0]) == 0


def test_the_model_dispatches():
    D = np.random.default_rng(3).integers(0, 256, size=(9, 11, 4), dtype=np.uint8)
    f = (F16, CHW, *IMAGENET)
    got = tensors.tensors(D, (1, 1, 9, 7), (4, 5), 1, FILTER_LANCZOS, tensors.ALPHA_WEIGHTED, f)
    assert np.array_equal(got, tensors.convert(lanczos.lanczos(D, (1, 1, 9, 7), (4, 5), 1, lanczos.ALPHA_WEIGHTED), f))
    assert np.array_equal(tensors.tensors(D, (1, 1, 9, 7), (9, 7), 0, FILTER_LANCZOS), D[1:8, 1:10])
    for filt in (2, 4, 5, 7, -1, 8):
        with pytest.raises(ValueError):
            tensors.tensors(D, (1, 1, 9, 7), (4, 5), 0, filt)


def test_rejections_before_the_context_is_looked_at():
    lib = api.load_library()
    fake = ctypes.create_string_buffer(1 << 16)                      # stands in for a context: a rejected call never looks at it
    streams = ctypes.create_string_buffer(64)
    out = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))
    so, sz, ds = (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(64), (api.QoiDesc * 1)(api.QoiDesc(20000, 17000, 4, 0))
    fmt = api.tensor_format((U8, HWC, ONE4, ZERO4))

    def call(item, filter=FILTER_LANCZOS, f=fmt):
        arr = (api.QoimiResize * 1)(api.QoimiResize(*item))
        return lib.qoimi_decode_tensors(ctypes.cast(fake, ctypes.c_void_p), streams, so, sz, ds, 1, 4, arr, 1, filter, 0, ctypes.byref(f) if f is not None else None,
                                        out, (ctypes.c_size_t * 1)(0), 0, None)

    for item, word in [((0, 0, 0, 17, 1, 1, 1, 0), "more than 16"), ((0, 0, 0, 1, 33, 1, 2, 0), "more than 16"), ((0, 0, 0, 16385, 1, 1025, 1, 0), "16384"),
                       ((0, 0, 0, 1, 1, 1, 16385, 0), "16384"), ((0, 0, 0, 1, 1, 16385, 1, 0), "16384"), ((0, 19999, 0, 2, 1, 1, 1, 0), "leaves"),
                       ((0, 0, 0, 17, 1, 1, 1, 4), "flag"), ((0, 0, 0, 0, 1, 1, 1, 0), "zero")]:
        assert call(item) == E_ARG and word in api.last_error(), (item, api.last_error())
    for filt in (2, 4, 5, 7, -1):
        assert call((0, 0, 0, 1, 1, 1, 1, 0), filter=filt) == E_ARG and "filter" in api.last_error(), filt
        assert "QOIMI_FILTER_BICUBIC" in api.last_error() and "QOIMI_FILTER_LANCZOS" in api.last_error()
    assert call((0, 0, 0, 17, 1, 1, 1, 0), f=None) == E_ARG and "format" in api.last_error()          # the format in front of the items
    assert bytes(out) == b"\xA5" * 4096 and fake.raw == b"\0" * (1 << 16)


def test_tool_options(tmp_path):
    """--filter lanczos is a choice of both tools (an empty directory ends them behind the arguments: "no .qoi files"); lanczos3 is none"""
    from tools import qoiresize_mi355x as resize_tool
    from tools import qoitensor_mi355x as tensor_tool
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    assert tensor_tool.main([str(empty), "--size", "4x4", "--filter", "lanczos", "-o", str(tmp_path / "t.npy")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    assert resize_tool.main([str(empty), "--size", "4x4", "--filter", "lanczos", "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    n = len(lines)
    assert tensor_tool.main([str(empty), "--size", "4x4", "--filter", "lanczos3", "-o", str(tmp_path / "t.npy")], out=lines.append) == 2
    assert resize_tool.main([str(empty), "--size", "4x4", "--filter", "lanczos3", "-o", str(tmp_path / "o")], out=lines.append) == 2 and len(lines) == n
    assert "lanczos" in tensor_tool.__doc__ and "lanczos" in resize_tool.__doc__ and not os.path.exists(tmp_path / "o")
