"""tools/qoitensor_mi355x.py: .qoi files as one normalised .npy tensor through one qoimi_decode_tensors call.  Without a GPU: the argument
handling and the arithmetic of scale and bias (float64, rounded once).  On the GPU (-m gpu): two small .qoi files to tensors whose bits equal
qoi_amd/tensors.py: tensors of the oracle's decode."""
import os

import numpy as np
import pytest

from qoi_amd import tensors
from tools import qoitensor_mi355x as tool
from tools.qoiresize_mi355x import fit_rect

MEAN, STD = "0.485,0.456,0.406", "0.229,0.224,0.225"


def test_parse_floats():
    assert list(tool.parse_floats("0.5", 3, 9.0)) == [0.5, 0.5, 0.5, 9.0] and list(tool.parse_floats("0.5", 4, 9.0)) == [0.5] * 4
    assert list(tool.parse_floats("1,2,3", 3, 0.0)) == [1.0, 2.0, 3.0, 0.0] and list(tool.parse_floats(" 1, 2,3 ,4", 3, 0.0)) == [1.0, 2.0, 3.0, 4.0]
    for bad, och in (("", 3), ("a", 3), ("1,2", 3), ("1,2,3,4,5", 4), ("1,2,3", 4), ("1,inf,3", 3), ("nan", 3)):
        assert tool.parse_floats(bad, och, 0.0) is None, bad


def test_scale_bias_is_rounded_once():
    mean, std = tool.parse_floats(MEAN, 3, 0.0), tool.parse_floats(STD, 3, 1.0)
    scale, bias = tool.scale_bias(mean, std)
    assert scale.dtype == bias.dtype == np.float32
    for c in range(4):
        assert scale[c] == np.float32(1.0 / (255.0 * std[c])) and bias[c] == np.float32(-mean[c] / std[c])
    assert scale[3] == np.float32(1 / 255) and bias[3] == 0.0
    n_scale, n_bias = tensors.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert np.array_equal(scale, n_scale) and np.array_equal(bias, n_bias)
    # not 1 / float32(255 * std): the double rounding differs somewhere among simple values
    assert any(np.float32(1.0 / (255.0 * s)) != np.float32(1.0) / np.float32(255.0 * s) for s in np.arange(1, 200) / 100.0)
    assert tool.scale_bias(np.zeros(4), np.array([1.0, 0.0, 1.0, 1.0])) is None
    assert tool.scale_bias(np.zeros(4), np.full(4, 1e-300)) is None and tool.scale_bias(np.full(4, 1e300), np.ones(4)) is None


def test_arguments(tmp_path):
    """everything that ends before the device is looked at"""
    lines = []
    o = str(tmp_path / "o" / "t.npy")
    assert tool.main([], out=lines.append) == 2
    assert tool.main([str(tmp_path), "-o", o], out=lines.append) == 2                                          # no --size
    assert tool.main([str(tmp_path), "--size", "32x32"], out=lines.append) == 2                                # no -o
    assert tool.main([str(tmp_path), "--size", "32", "-o", o], out=lines.append) == 2 and "WxH" in lines[-1]
    assert tool.main([str(tmp_path), "--size", "4x4", "--filter", "cubic", "-o", o], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--dtype", "f64", "-o", o], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--layout", "nchw", "-o", o], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--channels", "2", "-o", o], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--staging-mb", "-1", "-o", o], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--dtype", "u8", "--mean", "0.5", "-o", o], out=lines.append) == 2 and "u8" in lines[-1]
    assert tool.main([str(tmp_path), "--size", "4x4", "--std", "1,0,1", "-o", o], out=lines.append) == 2 and "std" in lines[-1]
    assert tool.main([str(tmp_path), "--size", "4x4", "--mean", "1,2", "-o", o], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--channels", "4", "--mean", "1,2,3", "-o", o], out=lines.append) == 2
    assert not os.path.exists(tmp_path / "o")


@pytest.mark.gpu
def test_tool_on_the_gpu(ref, port, tmp_path):
    import torch  # noqa: F401  (first, so the library binds to torch's HIP runtime)
    from qoi_amd import api, synth
    oracle = ref or port
    images = {"a": (synth.frame_rgba("sprite_alpha", 130, 70, 0), 130, 70, 4), "b": (synth.frame_rgb("photo", 64, 48, 1), 64, 48, 3)}
    src = tmp_path / "in"
    src.mkdir()
    for name, (px, w, h, ch) in images.items():
        assert api.qoi_write(str(src / (name + ".qoi")), px.reshape(-1), api.QoiDesc(w, h, ch, 0)) > 0
    sb = tool.scale_bias(tool.parse_floats(MEAN, 3, 0.0), tool.parse_floats(STD, 3, 1.0))
    unit = tool.scale_bias(np.zeros(4), np.ones(4))
    cases = [(["--dtype", "f16", "--mean", MEAN, "--std", STD], tensors.FILTER_BILINEAR, tensors.F16, tensors.CHW, 3, "whole", sb),
             (["--dtype", "bf16", "--layout", "hwc", "--filter", "area", "--fit", "crop", "--channels", "4"], tensors.FILTER_AREA, tensors.BF16, tensors.HWC, 4, "crop", unit),
             (["--mean", MEAN, "--std", STD, "--filter", "area"], tensors.FILTER_AREA, tensors.F32, tensors.CHW, 3, "whole", sb),
             (["--dtype", "u8"], tensors.FILTER_BILINEAR, tensors.U8, tensors.CHW, 3, "whole", (np.ones(4, np.float32), np.zeros(4, np.float32)))]
    for k, (extra, filt, dtype, layout, och, fit, (scale, bias)) in enumerate(cases):
        path = tmp_path / f"t{k}.npy"
        lines = []
        assert tool.main([str(src), "--size", "37x23", "-o", str(path)] + extra, out=lines.append) == 0
        got = np.load(path)
        assert got.shape == ((2, och, 23, 37) if layout == tensors.CHW else (2, 23, 37, och)) and got.dtype == tensors.numpy_dtype(dtype)
        for j, (name, (px, w, h, ch)) in enumerate(sorted(images.items())):
            decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), och)
            want = tensors.tensors(decoded.reshape(h, w, och), fit_rect(w, h, 37, 23, fit), (37, 23), 0, filt, tensors.PLAIN, (dtype, layout, scale, bias))
            assert np.array_equal(got[j].view(np.uint8), want.view(np.uint8)), (k, name)
        assert any("2 images as" in l and "1 sub-batch" in l for l in lines)
    (src / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)
    assert tool.main([str(src), "--size", "2x1", "--filter", "area", "-o", str(tmp_path / "again.npy")], out=lambda s: None) == 1     # 130 to 2 is beyond the cap as well
    assert np.load(tmp_path / "again.npy").shape == (1, 3, 1, 2)
