"""The label-map options of the tools: tools/qoitensor_mi355x.py --filter nearest, --dtype i32|i64, --layout hw and tools/qoiresize_mi355x.py
--filter nearest.  Without a GPU: the argument handling.  On the GPU (-m gpu): two small .qoi files to N x H x W class indices and to PNGs
whose values equal qoi_amd/nearest.py: nearest of the oracle's decode - 130 to 2 wide, a reduction no other filter of the tools takes."""
import os

import numpy as np
import pytest

from qoi_amd import nearest, tensors
from tools import qoiresize_mi355x as resize_tool
from tools import qoitensor_mi355x as tensor_tool
from tools.qoiresize_mi355x import fit_rect


def test_arguments(tmp_path):
    """the new choices are choices (an empty directory ends the tools behind their arguments: "no .qoi files"), their neighbours are none"""
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    o = str(tmp_path / "o" / "t.npy")
    for extra in (["--filter", "nearest"], ["--dtype", "i32"], ["--dtype", "i64"], ["--layout", "hw"], ["--filter", "nearest", "--dtype", "i64", "--layout", "hw", "--channels", "4"],
                  ["--filter", "lanczos", "--dtype", "f16", "--layout", "hw", "--mean", "0.5", "--std", "0.25"]):
        assert tensor_tool.main([str(empty), "--size", "4x4", "-o", o] + extra, out=lines.append) == 2 and lines[-1] == "no .qoi files", extra
    assert resize_tool.main([str(empty), "--size", "4x4", "--filter", "nearest", "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    n = len(lines)
    for extra in (["--filter", "nearest-exact"], ["--dtype", "i16"], ["--dtype", "u64"], ["--layout", "h"], ["--layout", "wh"]):
        assert tensor_tool.main([str(empty), "--size", "4x4", "-o", o] + extra, out=lines.append) == 2, extra
    assert resize_tool.main([str(empty), "--size", "4x4", "--filter", "nn", "-o", str(tmp_path / "o")], out=lines.append) == 2 and len(lines) == n
    # the integer dtypes store the pixel values: no --mean / --std, as for u8
    for dtype in ("i32", "i64"):
        assert tensor_tool.main([str(empty), "--size", "4x4", "--dtype", dtype, "--mean", "0.5", "-o", o], out=lines.append) == 2 and dtype in lines[-1]
        assert tensor_tool.main([str(empty), "--size", "4x4", "--dtype", dtype, "--std", "2", "-o", o], out=lines.append) == 2 and "--mean / --std" in lines[-1]
    for word in ("nearest", "i32|i64", "chw|hwc|hw"):
        assert word in tensor_tool.__doc__, word
    assert "area|bilinear|bicubic|lanczos|nearest" in resize_tool.__doc__ and "qoi_amd/nearest.py" in resize_tool.__doc__
    assert not os.path.exists(tmp_path / "o")


@pytest.mark.gpu
def test_tools_on_the_gpu(ref, port, tmp_path):
    import torch  # noqa: F401  (first, so the library binds to torch's HIP runtime)
    from qoi_amd import api, synth
    from tools import png_io
    oracle = ref or port
    images = {"a": (synth.frame_rgba("sprite_alpha", 130, 70, 0), 130, 70, 4), "b": (synth.frame_rgb("photo", 64, 48, 1), 64, 48, 3)}
    src = tmp_path / "in"
    src.mkdir()
    for name, (px, w, h, ch) in images.items():
        assert api.qoi_write(str(src / (name + ".qoi")), px.reshape(-1), api.QoiDesc(w, h, ch, 0)) > 0
    unit = (np.ones(4, np.float32), np.zeros(4, np.float32))
    cases = [(["--filter", "nearest", "--dtype", "i64", "--layout", "hw"], (37, 23), tensors.FILTER_NEAREST, tensors.I64, tensors.HW, 3, "whole"),
             (["--filter", "nearest", "--dtype", "i32", "--layout", "chw", "--channels", "4", "--fit", "crop"], (37, 23), tensors.FILTER_NEAREST, tensors.I32, tensors.CHW, 4, "crop"),
             (["--filter", "nearest", "--dtype", "u8", "--layout", "hw"], (2, 1), tensors.FILTER_NEAREST, tensors.U8, tensors.HW, 3, "whole"),      # 130 to 2: no ratio limit
             (["--filter", "bilinear", "--dtype", "i64", "--layout", "hwc"], (37, 23), tensors.FILTER_BILINEAR, tensors.I64, tensors.HWC, 3, "whole")]
    for k, (extra, (ow, oh), filt, dtype, layout, och, fit) in enumerate(cases):
        path = tmp_path / f"t{k}.npy"
        lines = []
        assert tensor_tool.main([str(src), "--size", f"{ow}x{oh}", "-o", str(path)] + extra, out=lines.append) == 0, lines
        got = np.load(path)
        assert got.shape == {tensors.CHW: (2, och, oh, ow), tensors.HWC: (2, oh, ow, och), tensors.HW: (2, oh, ow)}[layout] and got.dtype == tensors.numpy_dtype(dtype)
        for j, (name, (px, w, h, ch)) in enumerate(sorted(images.items())):
            decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), och)
            want = tensors.tensors(decoded.reshape(h, w, och), fit_rect(w, h, ow, oh, fit), (ow, oh), 0, filt, tensors.PLAIN, (dtype, layout, *unit))
            assert np.array_equal(got[j], want), (k, name)
        assert any("2 images as" in l and "1 sub-batch" in l for l in lines)
    out_dir = tmp_path / "png"
    lines = []
    assert resize_tool.main([str(src), "--size", "41x3", "-o", str(out_dir), "--filter", "nearest", "--flip", "x"], out=lines.append) == 0, lines
    for name, (px, w, h, ch) in images.items():
        decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 4)                    # one file has 4 channels: so have the outputs
        want = nearest.nearest(decoded.reshape(h, w, 4), (0, 0, w, h), (41, 3), nearest.FLIP_X)
        got, gw, gh = png_io.read_png((out_dir / (name + ".png")).read_bytes(), 4)
        assert (gw, gh) == (41, 3) and np.array_equal(np.asarray(got).reshape(3, 41, 4), want), name
    assert any("2 images at 41x3" in l and "1 sub-batch" in l for l in lines)
