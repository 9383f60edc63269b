"""Packed streams, what can be checked without a GPU: the three entry points exist in every layer, answer a NULL context like every
other entry point, and the layout of a pack as a few lines of numpy (the model the GPU tests compare qoimi_pack_streams with)."""
import ctypes
import os
import re
import subprocess

import pytest
from model_cases import pack_offsets as offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qoimi_pack_streams", "qoimi_decode_images", "qoimi_read_descs")
QOIMI_E_ARG = -1


def test_offsets_model():
    assert offsets([22, 1, 0, 300], 1).tolist() == [0, 22, 23, 23, 323]
    assert offsets([22, 1, 0, 300], 4).tolist() == [0, 24, 28, 28, 328]
    assert offsets([22, 1, 0, 300], 256).tolist() == [0, 256, 512, 512, 812]
    assert offsets([5], 64).tolist() == [0, 5]


def test_symbols_in_every_layer():
    from qoi_amd import api
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    for name in NEW:
        assert name in api.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    for flavour in ("libqoi_mi355x.so", "libqoi_mi355x_nostdio.so", "libqoi_mi355x_test.so"):
        path = os.path.join(ROOT, "qoi_amd", "lib", flavour)
        assert os.path.exists(path), f"{flavour} not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {l.split()[-1] for l in syms.splitlines() if l.strip()}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    for method in ("pack_streams", "decode_images", "read_descs"):
        assert callable(getattr(api.Context, method))


def test_null_context_is_rejected_first():
    from qoi_amd import api
    lib = api.load_library()
    buf = (ctypes.c_ubyte * 64)()
    p = ctypes.addressof(buf)
    one = (ctypes.c_size_t * 1)(0)
    sizes = (ctypes.c_int * 1)(22)
    descs = (api.QoiDesc * 1)(api.QoiDesc(1, 1, 4, 0))
    bad = ctypes.c_int(7)
    calls = {
        "qoimi_pack_streams": lambda: lib.qoimi_pack_streams(None, p, 32, p, 1, 1, p, 32, p, None),
        "qoimi_decode_images": lambda: lib.qoimi_decode_images(None, p, one, sizes, descs, 1, 4, p, one, None),
        "qoimi_read_descs": lambda: lib.qoimi_read_descs(None, p, one, sizes, 1, descs, ctypes.byref(bad), None),
    }
    for name, call in calls.items():
        assert call() == QOIMI_E_ARG, name
        assert api.last_error() != "", name
    assert bytes(buf) == b"\0" * 64 and bad.value == 7
