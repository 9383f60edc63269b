"""tools/qoifromlabels_mi355x.py.  Without a GPU: the plan of the call and the argument handling.  On the GPU (-m gpu): an int64 batch to
.qoi files and to a voted pyramid whose files are the reference encoder's streams of qoi_amd/tiles.py: tile, and the count of saturated
elements the tool prints."""
import numpy as np
import pytest

from qoi_amd import tiles
from tools import qoifromlabels_mi355x as tool


def test_plan_call():
    n, w, h, flags, nbytes, grid = tool.plan_call((3, 9, 37), np.int64)
    assert (n, w, h, flags, nbytes, grid) == (3, 37, 9, tiles.label_flags(tiles.L_I64), 37 * 9 * 8, [((0, 0, 0), (0, 0, 37, 9, 1))])
    assert tool.plan_call((9, 37), np.uint8)[:5] == (1, 37, 9, tiles.LABELS, 37 * 9)
    n, w, h, flags, nbytes, grid = tool.plan_call((2, 90, 150), np.int32, 3, 64, "vote")
    assert flags == tiles.label_flags(tiles.L_I32) and nbytes == 150 * 90 * 4
    assert [t for _, t in grid] == [t[1:6] for t in tiles.pyramid(150, 90, 64, 64, 3)] and [i for i, _ in grid] == tiles.pyramid_index(150, 90, 64, 64, 3)
    for shape, dtype, levels, mode, word in (((4, 4), np.float32, 0, "nearest", "not uint8, int32 or int64"), ((4, 4), np.int16, 0, "nearest", "not uint8"),
                                              ((2, 3, 4, 4), np.int64, 0, "nearest", "H x W or N x H x W"), ((4,), np.int64, 0, "nearest", "H x W or N x H x W"),
                                              ((20000, 20000), np.uint8, 0, "nearest", "400 000 000"), ((64, 64), np.int64, 6, "vote", "1..5"),
                                              ((64, 64), np.int64, 8, "nearest", "1..7"), ((64, 64), np.int64, 2, "mean", "nearest or vote")):
        assert word in tool.plan_call(shape, dtype, levels, 16, mode), (shape, dtype, levels, mode)
    assert tool.plan_call((64, 64), np.int64, 7, 16, "nearest")[5][-1][1][4] == 64 and tool.plan_call((64, 64), np.int64, 5, 16, "vote")[5][-1][1][4] == 16


def test_arguments(tmp_path):
    lines = []
    np.save(tmp_path / "f.npy", np.zeros((4, 4), np.float32))
    assert tool.main([str(tmp_path / "f.npy"), "-o", str(tmp_path / "o")], out=lines.append) == 1 and "not uint8, int32 or int64" in lines[-1]
    assert tool.main([str(tmp_path / "none.npy"), "-o", str(tmp_path / "o")], out=lines.append) == 1
    np.save(tmp_path / "l.npy", np.zeros((4, 4), np.int64))
    for extra in (["--mode", "mean"], ["--channels", "0"], ["--levels", "x"]):
        assert tool.main([str(tmp_path / "l.npy"), "-o", str(tmp_path / "o")] + extra, out=lines.append) == 2, extra
    assert tool.main([str(tmp_path / "l.npy"), "-o", str(tmp_path / "o"), "--levels", "6", "--mode", "vote"], out=lines.append) == 1 and "1..5" in lines[-1]
    assert not (tmp_path / "o").exists()
    assert "silently" in tool.__doc__ and "never averaged" in tool.__doc__


@pytest.mark.gpu
def test_the_tool_on_the_gpu(ref, port, tmp_path):
    import labelimg
    oracle = ref or port
    a = np.stack([labelimg.label_image(150, 90, 4, 70 + i)[:, :, 1].astype(np.int64) for i in range(2)])
    a[0, 3, 5], a[1, 0, 0], a[1, 89, 149] = -100, 2 ** 32 + 5, 256
    np.save(tmp_path / "maps.npy", a)
    said = []
    assert tool.main([str(tmp_path / "maps.npy"), "-o", str(tmp_path / "flat"), "--channels", "4"], out=said.append) == 0
    flags = tiles.label_flags(tiles.L_I64)
    for i in range(2):
        want = tiles.tile(a[i], (0, 0, 0, 150, 90, 1, flags), 4)
        assert (tmp_path / "flat" / ("%04d.qoi" % i)).read_bytes() == oracle.encode(want.reshape(-1), 150, 90, 4, 0), i
    assert "2 files of 4 channels" in said[-1] and "3 elements outside 0..255" in said[-1]
    assert tool.main([str(tmp_path / "maps.npy"), "-o", str(tmp_path / "pyr"), "--levels", "3", "--tile", "64", "--mode", "vote"], out=said.append) == 0
    grid = tool.plan_call(a.shape, a.dtype, 3, 64, "vote")[5]
    assert len(grid) == 9 and "3 levels by vote, 18 files of 3 channels" in said[-1]
    for i in range(2):
        for (level, row, col), t in grid:
            want = tiles.tile(a[i], (0,) + t + (flags,), 3, tiles.MODE)
            blob = (tmp_path / "pyr" / ("%04d" % i) / str(level) / f"tile_{row}_{col}.qoi").read_bytes()
            assert blob == oracle.encode(want.reshape(-1), want.shape[1], want.shape[0], 3, 0), (i, level, row, col)
