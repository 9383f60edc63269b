"""tools/qoiwarp_mi355x.py: .qoi files as re-oriented or turned PNGs through one qoimi_decode_warped call.  Without a GPU: the argument
handling, the fill colour and the quantised rotation matrix.  On the GPU (-m gpu): two small .qoi files to PNGs whose pixels equal
qoi_amd/warp.py: warp of the oracle's decode."""
import os

import numpy as np
import pytest

from qoi_amd import warp
from tools import qoiwarp_mi355x as tool


def test_parse_fill():
    assert tool.parse_fill("00000000") == 0 and tool.parse_fill("ff8000C0") == 0xC00080FF and tool.parse_fill(" 01020304 ") == 0x04030201
    for bad in ("", "fff", "gg000000", "0x000000", "000000000", "-1000000"):
        assert tool.parse_fill(bad) is None, bad


def test_rotation_matrix():
    assert tool.rotation_matrix(130, 70, 130, 70, 0.0, 1.0) == warp.IDENTITY
    assert tool.rotation_matrix(130, 70, 70, 130, 90.0, 1.0) == (0, -65536, 2 * 130 * 65536, 65536, 0, 0)       # orientation 8
    assert tool.rotation_matrix(130, 70, 70, 130, 90.0, 1.0) == tuple(warp.fields(warp.orient(130, 70, (0, 0, 130, 70), 8))[k] for k in (8, 9, 14, 10, 11, 15))
    assert tool.rotation_matrix(130, 70, 130, 70, 180.0, 1.0) == tuple(warp.fields(warp.orient(130, 70, (0, 0, 130, 70), 3))[k] for k in (8, 9, 14, 10, 11, 15))
    assert tool.rotation_matrix(10, 10, 20, 20, 0.0, 2.0) == (32768, 0, 0, 0, 32768, 0)
    for (w, h, ow, oh, deg, s) in [(130, 70, 37, 23, 30.0, 0.5), (64, 48, 224, 224, -77.0, 3.1), (1, 1, 5, 4, 200.0, 1.0)]:
        m = tool.rotation_matrix(w, h, ow, oh, deg, s)
        assert m == warp.rotation((w, h), (ow, oh), deg, s)
        a, b, c, d, e, f = m
        assert a * ow + b * oh + c == w * 65536 and d * ow + e * oh + f == h * 65536     # centre to centre, exactly
        assert warp.size(w, h, warp.item(0, (0, 0, w, h), (ow, oh), m), 4) == ow * oh * 4
    assert tool.rotation_matrix(10, 10, 10, 10, 0.0, 1e-6) is None                       # a factor beyond 32 bits
    for bad in [(0, 5, 1, 1, 0.0, 1.0), (5, 5, 1, 1, 0.0, 0.0), (5, 5, 1, 1, float("nan"), 1.0), (5, 5, 1, 1, 0.0, float("inf"))]:
        with pytest.raises(ValueError):
            tool.rotation_matrix(*bad)


def test_arguments(tmp_path):
    """everything that ends before the device is looked at"""
    lines = []
    o = ["-o", str(tmp_path / "o")]
    assert tool.main([], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--orient", "6"], out=lines.append) == 2                                  # no -o
    assert tool.main([str(tmp_path)] + o, out=lines.append) == 2 and "--orient" in lines[-1]                   # neither
    assert tool.main([str(tmp_path), "--orient", "6", "--rotate", "30"] + o, out=lines.append) == 2            # both
    assert tool.main([str(tmp_path), "--orient", "0"] + o, out=lines.append) == 2 and tool.main([str(tmp_path), "--orient", "9"] + o, out=lines.append) == 2
    assert tool.main([str(tmp_path), "--orient", "6", "--size", "4x4"] + o, out=lines.append) == 2
    assert tool.main([str(tmp_path), "--rotate", "30", "--size", "4"] + o, out=lines.append) == 2 and "WxH" in lines[-1]
    assert tool.main([str(tmp_path), "--rotate", "30", "--size", "1048576x1"] + o, out=lines.append) == 2
    assert tool.main([str(tmp_path), "--rotate", "30", "--scale", "0"] + o, out=lines.append) == 2
    assert tool.main([str(tmp_path), "--rotate", "nan"] + o, out=lines.append) == 2
    assert tool.main([str(tmp_path), "--rotate", "30", "--fill", "red"] + o, out=lines.append) == 2 and "RRGGBBAA" in lines[-1]
    assert tool.main([str(tmp_path), "--rotate", "30", "--border", "mirror"] + o, out=lines.append) == 2
    assert tool.main([str(tmp_path), "--rotate", "30", "--staging-mb", "-1"] + o, out=lines.append) == 2
    assert not os.path.exists(tmp_path / "o")


@pytest.mark.gpu
def test_tool_on_the_gpu(ref, port, tmp_path):
    import torch  # noqa: F401  (first, so the library binds to torch's HIP runtime)
    from qoi_amd import api, synth
    from tools import png_io
    oracle = ref or port
    images = {"a": (synth.frame_rgba("sprite_alpha", 130, 70, 0), 130, 70, 4), "b": (synth.frame_rgb("photo", 64, 48, 1), 64, 48, 3)}
    src = tmp_path / "in"
    src.mkdir()
    for name, (px, w, h, ch) in images.items():
        assert api.qoi_write(str(src / (name + ".qoi")), px.reshape(-1), api.QoiDesc(w, h, ch, 0)) > 0
    decoded = {name: oracle.decode((src / (name + ".qoi")).read_bytes(), 4)[0].reshape(h, w, 4) for name, (px, w, h, ch) in images.items()}   # one file has 4 channels: so have the outputs
    lines = []
    assert tool.main([str(src), "--orient", "6", "-o", str(tmp_path / "o6")], out=lines.append) == 0
    for name, (px, w, h, ch) in images.items():
        got, gw, gh = png_io.read_png((tmp_path / "o6" / (name + ".png")).read_bytes(), 4)
        assert (gw, gh) == (h, w) and np.array_equal(np.asarray(got).reshape(w, h, 4), np.rot90(decoded[name], -1)), name
    assert any("2 images" in l and "1 sub-batch" in l for l in lines)
    for extra, flags, fill, mode in ((["--fill", "ff8000c0"], 0, 0xC00080FF, warp.PLAIN), (["--border", "replicate", "--mode", "weighted"], warp.REPLICATE, 0, warp.ALPHA_WEIGHTED)):
        out_dir = tmp_path / ("r" + str(flags))
        assert tool.main([str(src), "--rotate", "30", "--scale", "0.8", "--size", "37x23", "-o", str(out_dir)] + extra, out=lines.append) == 0
        for name, (px, w, h, ch) in images.items():
            want = warp.warp(decoded[name], (0, 0, w, h), (37, 23), tool.rotation_matrix(w, h, 37, 23, 30.0, 0.8), flags, fill, mode)
            got, gw, gh = png_io.read_png((out_dir / (name + ".png")).read_bytes(), 4)
            assert (gw, gh) == (37, 23) and np.array_equal(np.asarray(got).reshape(23, 37, 4), want), (name, flags)
    (src / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)
    assert tool.main([str(src), "--rotate", "45", "-o", str(tmp_path / "again")], out=lambda s: None) == 1
    assert sorted(os.listdir(tmp_path / "again")) == ["a.png", "b.png"]
