"""tools/qoiresize_mi355x.py: .qoi files as PNGs of one fixed size through one qoimi_decode_resized call.  Without a GPU: the argument handling
and the rectangle arithmetic (the whole image, or the largest centred rectangle of the target's aspect).  On the GPU (-m gpu): two small .qoi
files to PNGs whose pixels equal qoi_amd/resize.py: resize of the oracle's decode."""
import os

import numpy as np
import pytest

from qoi_amd import resize
from tools import qoiresize_mi355x as tool


def test_parse_size():
    assert tool.parse_size("224x160") == (224, 160) and tool.parse_size(" 1X1 ") == (1, 1) and tool.parse_size("4294967295x2") == (4294967295, 2)
    for bad in ("", "224", "224x", "x160", "0x5", "5x0", "-3x4", "3.5x4", "3x4x5", "4294967296x1", "axb"):
        assert tool.parse_size(bad) is None, bad


def test_fit_rect():
    assert tool.fit_rect(130, 70, 32, 32, "whole") == (0, 0, 130, 70)
    assert tool.fit_rect(130, 70, 32, 32, "crop") == (30, 0, 70, 70)                 # wider than the target: full height, centred
    assert tool.fit_rect(70, 130, 32, 32, "crop") == (0, 30, 70, 70)                 # taller: full width
    assert tool.fit_rect(131, 70, 32, 32, "crop") == (30, 0, 70, 70)                 # (131 - 70) // 2
    assert tool.fit_rect(64, 48, 4, 3, "crop") == (0, 0, 64, 48)                     # the target's aspect already
    assert tool.fit_rect(100, 100, 3, 2, "crop") == (0, 17, 100, 66)                 # floor(100 * 2 / 3), (100 - 66) // 2
    assert tool.fit_rect(100, 100, 2, 3, "crop") == (17, 0, 66, 100)
    assert tool.fit_rect(1, 1, 224, 7, "crop") == (0, 0, 1, 1) and tool.fit_rect(5, 1, 1, 100, "crop") == (2, 0, 1, 1)   # never empty
    for (w, h, ow, oh) in [(130, 70, 37, 23), (257, 9, 16, 16), (9, 257, 16, 16), (3840, 2160, 224, 224), (1, 97, 5, 2), (333, 7, 1, 1)]:
        x, y, cw, rh = tool.fit_rect(w, h, ow, oh, "crop")
        assert 1 <= cw <= w and 1 <= rh <= h and x == (w - cw) // 2 and y == (h - rh) // 2 and (cw == w or rh == h)
        assert abs(cw * oh - rh * ow) < max(ow, oh)                                  # the aspect, up to the floor
        assert resize.size(w, h, (x, y, cw, rh), (max(ow, -(-cw // 64)), max(oh, -(-rh // 64))), 0, 4) > 0
    for bad in [(0, 5, 1, 1, "crop"), (5, 5, 0, 1, "whole"), (5, 5, 1, 1, "stretch")]:
        with pytest.raises(ValueError):
            tool.fit_rect(*bad)


def test_arguments(tmp_path):
    """everything that ends before the device is looked at"""
    lines = []
    assert tool.main([], out=lines.append) == 2
    assert tool.main([str(tmp_path), "-o", str(tmp_path / "o")], out=lines.append) == 2                       # no --size
    assert tool.main([str(tmp_path), "--size", "32x32"], out=lines.append) == 2                                # no -o
    assert tool.main([str(tmp_path), "--size", "32", "-o", str(tmp_path / "o")], out=lines.append) == 2 and "WxH" in lines[-1]
    assert tool.main([str(tmp_path), "--size", "0x4", "-o", str(tmp_path / "o")], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--fit", "stretch", "-o", str(tmp_path / "o")], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--mode", "cubic", "-o", str(tmp_path / "o")], out=lines.append) == 2
    assert tool.main([str(tmp_path), "--size", "4x4", "--staging-mb", "-1", "-o", str(tmp_path / "o")], out=lines.append) == 2
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
    for fit, mode, flip, flags in (("whole", "plain", "none", 0), ("crop", "weighted", "xy", 3), ("crop", "plain", "x", 1)):
        out_dir = tmp_path / (fit + mode + flip)
        lines = []
        assert tool.main([str(src), "--size", "37x23", "-o", str(out_dir), "--fit", fit, "--mode", mode, "--flip", flip], out=lines.append) == 0
        assert sorted(os.listdir(out_dir)) == ["a.png", "b.png"]
        for name, (px, w, h, ch) in images.items():
            decoded, _ = oracle.decode((src / (name + ".qoi")).read_bytes(), 4)                    # one file has 4 channels: so have the outputs
            want = resize.resize(decoded.reshape(h, w, 4), tool.fit_rect(w, h, 37, 23, fit), (37, 23), flags,
                                 resize.ALPHA_WEIGHTED if mode == "weighted" else resize.PLAIN)
            got, gw, gh = png_io.read_png((out_dir / (name + ".png")).read_bytes(), 4)
            assert (gw, gh) == (37, 23) and np.array_equal(np.asarray(got).reshape(23, 37, 4), want), (name, fit, mode, flip)
        assert any("2 images at 37x23" in l and "1 sub-batch" in l for l in lines)
    (src / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)
    assert tool.main([str(src), "--size", "2x1", "-o", str(tmp_path / "again")], out=lambda s: None) == 1      # 130 to 2 is beyond the cap as well
    assert sorted(os.listdir(tmp_path / "again")) == ["b.png"]
