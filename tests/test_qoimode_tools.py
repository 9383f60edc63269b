"""--filter mode of tools/qoitensor_mi355x.py and tools/qoiresize_mi355x.py.  Without a GPU: the argument handling.  On the GPU (-m gpu):
two small label maps as .qoi files to N x H x W class indices and to PNGs whose values equal qoi_amd/mode.py: mode of the oracle's decode,
and a file beyond the filter's ratio limit left out."""
import os

import numpy as np
import pytest

import mode_cases as MC
from qoi_amd import mode, tensors
from tools import qoiresize_mi355x as resize_tool
from tools import qoitensor_mi355x as tensor_tool
from tools.qoiresize_mi355x import fit_rect


def test_arguments(tmp_path):
    """the new choice is a choice (an empty directory ends the tools behind their arguments: "no .qoi files"), its neighbours are none"""
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    o = str(tmp_path / "o" / "t.npy")
    for extra in (["--filter", "mode"], ["--filter", "mode", "--dtype", "i64", "--layout", "hw", "--channels", "4"], ["--filter", "mode", "--dtype", "u8", "--layout", "hwc"]):
        assert tensor_tool.main([str(empty), "--size", "4x4", "-o", o] + extra, out=lines.append) == 2 and lines[-1] == "no .qoi files", extra
    assert resize_tool.main([str(empty), "--size", "4x4", "--filter", "mode", "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    n = len(lines)
    for extra in (["--filter", "majority"], ["--filter", "median"], ["--filter", "Mode"]):
        assert tensor_tool.main([str(empty), "--size", "4x4", "-o", o] + extra, out=lines.append) == 2, extra
        assert resize_tool.main([str(empty), "--size", "4x4", "-o", str(tmp_path / "o")] + extra, out=lines.append) == 2 and len(lines) == n
    for doc in (tensor_tool.__doc__, resize_tool.__doc__):
        assert "area|bilinear|bicubic|lanczos|nearest|mode" in doc and "qoi_amd/mode.py" in doc
    assert not os.path.exists(tmp_path / "o")


@pytest.mark.gpu
def test_tools_on_the_gpu(ref, port, tmp_path):
    import torch  # noqa: F401  (first, so the library binds to torch's HIP runtime)
    from qoi_amd import api
    from tools import png_io
    oracle = ref or port
    images = {"a": (MC.label_map(37, 29, 3, 3, 11), 37, 29, 3), "b": (MC.label_map(70, 45, 4, 5, 12), 70, 45, 4)}
    src = tmp_path / "in"
    src.mkdir()
    for name, (px, w, h, ch) in images.items():
        assert api.qoi_write(str(src / (name + ".qoi")), px.reshape(-1), api.QoiDesc(w, h, ch, 0)) > 0
    unit = (np.ones(4, np.float32), np.zeros(4, np.float32))
    cases = [(["--dtype", "i64", "--layout", "hw"], (9, 7), tensors.I64, tensors.HW, 3, "whole"), (["--dtype", "u8", "--layout", "hwc", "--channels", "4"], (16, 11), tensors.U8, tensors.HWC, 4, "whole"),
             (["--dtype", "i32", "--layout", "chw", "--fit", "crop"], (8, 8), tensors.I32, tensors.CHW, 3, "crop")]
    for k, (extra, (ow, oh), dtype, layout, och, fit) in enumerate(cases):
        path = tmp_path / f"t{k}.npy"
        lines = []
        assert tensor_tool.main([str(src), "--size", f"{ow}x{oh}", "-o", str(path), "--filter", "mode"] + extra, out=lines.append) == 0, lines
        got = np.load(path)
        assert got.shape == {tensors.CHW: (2, och, oh, ow), tensors.HWC: (2, oh, ow, och), tensors.HW: (2, oh, ow)}[layout] and got.dtype == tensors.numpy_dtype(dtype)
        for j, (name, (px, w, h, ch)) in enumerate(sorted(images.items())):
            decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 4)
            P = mode.mode(decoded.reshape(h, w, 4), fit_rect(w, h, ow, oh, fit), (ow, oh), 0, och=och)
            assert np.array_equal(got[j], tensors.convert(P, (dtype, layout, *unit))), (k, name)
        assert any("2 images as" in l and "1 sub-batch" in l for l in lines)
    # 70 to 4 is more than 16 times: that file is left out, the other one is written
    lines = []
    assert tensor_tool.main([str(src), "--size", "4x3", "-o", str(tmp_path / "few.npy"), "--filter", "mode", "--dtype", "u8"], out=lines.append) == 1
    assert any("b.qoi" in l and "mode filter's limits" in l for l in lines) and np.load(tmp_path / "few.npy").shape == (1, 3, 3, 4)
    out_dir = tmp_path / "png"
    lines = []
    assert resize_tool.main([str(src), "--size", "9x7", "-o", str(out_dir), "--filter", "mode", "--flip", "x"], out=lines.append) == 0, lines
    for name, (px, w, h, ch) in images.items():
        decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 4)                    # one file has 4 channels: so have the outputs
        want = mode.mode(decoded.reshape(h, w, 4), (0, 0, w, h), (9, 7), mode.FLIP_X)
        got, gw, gh = png_io.read_png((out_dir / (name + ".png")).read_bytes(), 4)
        assert (gw, gh) == (9, 7) and np.array_equal(np.asarray(got).reshape(7, 9, 4), want), name
    assert any("2 images at 9x7" in l and "1 sub-batch" in l for l in lines)
    lines = []
    assert resize_tool.main([str(src), "--size", "4x3", "-o", str(tmp_path / "png2"), "--filter", "mode"], out=lines.append) == 1
    assert any("b.qoi" in l and "more than 16 times" in l for l in lines)
