"""tools/qoipyramid_mi355x.py: a .qoi file as a tile pyramid through one qoimi_encode_tiles call.  Without a GPU: the grid and the command
line.  On the GPU (-m gpu): a 150 x 90 image at tile 64 over 3 levels, every file compared with the reference decoder's pixels."""
import os

import numpy as np
import pytest

from qoi_amd import thumbs, tiles
from tools import qoipyramid_mi355x as tool


def test_pyramid_grid():
    g = tool.pyramid_grid(150, 90, 64, 3)
    assert [(l, r, c) for (l, r, c, _) in g] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (0, 1, 1), (0, 1, 2), (1, 0, 0), (1, 0, 1), (2, 0, 0)]
    assert g[2][3] == (0, 128, 0, 22, 64, 1, 0, 0) and g[5][3] == (0, 128, 64, 22, 26, 1, 0, 0)
    assert g[7][3] == (0, 128, 0, 22, 90, 2, 0, 0) and g[8][3] == (0, 0, 0, 150, 90, 4, 0, 0)
    for (w, h, t, levels) in [(130, 70, 32, 4), (16384, 16384, 256, 4), (257, 9, 7, 7), (5, 3, 256, 2)]:
        g = tool.pyramid_grid(w, h, t, levels)
        for level in range(levels):
            f = 1 << level
            lw, lh = -(-w // f), -(-h // f)
            mine = [(r, c, tl) for (l, r, c, tl) in g if l == level]
            assert len(mine) == -(-lw // t) * -(-lh // t)
            assert sum(tiles.size(w, h, 4, tl)[1] * tiles.size(w, h, 4, tl)[2] for (_, _, tl) in mine) == lw * lh
            assert all(tl[1] == c * t * f and tl[2] == r * t * f and tl[5] == f for (r, c, tl) in mine)
    with pytest.raises(ValueError):
        tool.pyramid_grid(4, 4, 0, 1)
    with pytest.raises(ValueError):
        tool.pyramid_grid(4, 4, 4, 8)


def test_arguments(tmp_path):
    """everything that ends before the device is looked at"""
    lines = []
    f = str(tmp_path / "x.qoi")
    o = ["-o", str(tmp_path / "o")]
    assert tool.main([], out=lines.append) == 2
    assert tool.main([f, "--tile", "64", "--levels", "3"], out=lines.append) == 2                 # no -o
    assert tool.main([f, "--levels", "3"] + o, out=lines.append) == 2                               # no --tile
    assert tool.main([f, "--tile", "64"] + o, out=lines.append) == 2                                # no --levels
    assert tool.main([f, "--tile", "0", "--levels", "3"] + o, out=lines.append) == 2 and "--tile" in lines[-1]
    assert tool.main([f, "--tile", "16777217", "--levels", "3"] + o, out=lines.append) == 2
    assert tool.main([f, "--tile", "64", "--levels", "0"] + o, out=lines.append) == 2 and "--levels" in lines[-1]
    assert tool.main([f, "--tile", "64", "--levels", "8"] + o, out=lines.append) == 2
    assert tool.main([f, "--tile", "x", "--levels", "3"] + o, out=lines.append) == 2
    assert tool.main([f, "--tile", "64", "--levels", "3", "--staging-mb", "-1"] + o, out=lines.append) == 2
    assert not os.path.exists(tmp_path / "o")


@pytest.mark.gpu
def test_round_trip_on_the_gpu(ref, port, tmp_path):
    import torch  # noqa: F401  (first, so the library binds to torch's HIP runtime)
    from qoi_amd import api, synth
    oracle = ref or port
    w, h = 150, 90
    px = synth.frame_rgba("sprite_alpha", w, h, 0).reshape(h, w, 4)
    src = tmp_path / "in.qoi"
    assert api.qoi_write(str(src), px.reshape(-1), api.QoiDesc(w, h, 4, 0)) > 0
    lines = []
    assert tool.main([str(src), "--tile", "64", "--levels", "3", "-o", str(tmp_path / "p")], out=lines.append) == 0
    assert "9 tiles" in lines[-1] and "3 levels" in lines[-1]
    grid = tool.pyramid_grid(w, h, 64, 3)
    assert sorted(os.listdir(tmp_path / "p")) == ["0", "1", "2"]
    assert sum(len(os.listdir(tmp_path / "p" / d)) for d in "012") == len(grid) == 9
    for (level, row, col, tl) in grid:
        blob = (tmp_path / "p" / str(level) / f"tile_{row}_{col}.qoi").read_bytes()
        want = tiles.tile(px, tl)
        got, d = oracle.decode(blob, 4)
        assert (d.width, d.height, d.channels) == (want.shape[1], want.shape[0], 4), (level, row, col)
        assert np.array_equal(np.asarray(got).reshape(want.shape), want), (level, row, col)
        assert blob == oracle.encode(want.reshape(-1), want.shape[1], want.shape[0], 4)
        assert np.array_equal(want, thumbs.thumbnail(px, 1 << level)[row * 64:(row + 1) * 64, col * 64:(col + 1) * 64])
    (tmp_path / "junk.qoi").write_bytes(b"qoif" + b"\0" * 30)
    assert tool.main([str(tmp_path / "junk.qoi"), "--tile", "64", "--levels", "3", "-o", str(tmp_path / "q")], out=lambda s: None) == 1
