"""tools/qoistats_mi355x.py: command-line errors and exit statuses without a GPU (a bad command line is 2, a file that is no QOI stream is 1 -
both before the device is looked at), and one run on the GPU over a small synthetic file, whole and in tiles."""
import numpy as np
import pytest

from qoi_amd import pixelstats
from tools import qoistats_mi355x as tool


def test_arguments(tmp_path):
    lines = []
    assert tool.main([], out=lines.append) == 2
    assert tool.main(["a.qoi", "b.qoi"], out=lines.append) == 2
    assert tool.main(["a.qoi", "--tile"], out=lines.append) == 2
    assert tool.main(["a.qoi", "--tile", "x"], out=lines.append) == 2
    assert tool.main(["a.qoi", "--tile", "0"], out=lines.append) == 2 and "--tile" in lines[-1]
    assert tool.main(["a.qoi", "--tile", "-3"], out=lines.append) == 2
    assert tool.main(["a.qoi", "--staging-mb", "-1"], out=lines.append) == 2
    assert tool.main(["a.qoi", "-o", "dir"], out=lines.append) == 2                       # no output directory: nothing is written


def test_not_a_qoi_stream(tmp_path):
    lines = []
    (tmp_path / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)                             # width 0
    assert tool.main([str(tmp_path / "junk.qoi")], out=lines.append) == 1 and "not a QOI stream" in lines[-1]
    (tmp_path / "short.qoi").write_bytes(b"qoif\0\0\0\1")
    assert tool.main([str(tmp_path / "short.qoi"), "--tile", "32"], out=lines.append) == 1
    (tmp_path / "magic.qoi").write_bytes(b"qoig" + (4).to_bytes(4, "big") * 2 + b"\4\0" + b"\0" * 16)
    assert tool.main([str(tmp_path / "magic.qoi")], out=lines.append) == 1
    assert tool.main([str(tmp_path / "missing.qoi")], out=lines.append) == 1


def test_line():
    D = np.zeros((2, 3, 4), dtype=np.uint8)
    D[..., 3] = 255
    D[0, 0, 0] = 6
    text = tool.line("image", pixelstats.stats(D, (0, 0, 3, 2)))
    assert text.startswith("image: 6 px  mean 1.000 0.000 0.000 255.000  std 2.236 0.000 0.000 0.000") and text.endswith("opaque")


@pytest.mark.gpu
def test_tool_on_the_gpu(ref, port, tmp_path):
    import torch  # noqa: F401
    from qoi_amd.packplan import slot
    oracle = ref or port
    px = np.zeros((50, 70, 4), dtype=np.uint8)
    px[..., 3] = 255
    px[:32, :32] = (9, 9, 9, 255)                                                         # tile_0_0: constant, opaque, grey
    px[40:, 64:, 3] = 0                                                                   # tile_1_2 (6 x 18): its lower part transparent
    px[33, 40, 1] = 200                                                                   # tile_1_1: one pixel off
    src = tmp_path / "t.qoi"
    src.write_bytes(oracle.encode(px.reshape(-1), 70, 50, 4))
    decoded, _ = oracle.decode(src.read_bytes(), 4)
    D = decoded.reshape(50, 70, 4)
    lines = []
    assert tool.main([str(src), "--tile", "32"], out=lines.append) == 0
    grid = tool.tile_grid(70, 50, 32)
    assert len(lines) == len(grid) + 1 == 7
    want = [pixelstats.stats(D, (x, y, tw, th)) for (_, _, x, y, tw, th) in grid]
    for text, (r, c, *_), f in zip(lines, grid, want):
        assert text == tool.line(f"tile_{r}_{c}", f)
    assert lines[0].endswith("constant|opaque|grey") and lines[4].endswith("opaque") and lines[5].endswith("grey")
    assert "6 tiles of 32x32, 4 constant, 5 opaque" in lines[-1] and f"{slot(70 * 50 * 4)} bytes staged" in lines[-1]
    lines = []
    assert tool.main([str(src), "--staging-mb", "1"], out=lines.append) == 0
    assert lines == [tool.line("image", pixelstats.stats(D, (0, 0, 70, 50))), lines[-1]] and "1 region, 0 constant, 0 opaque" in lines[-1]
