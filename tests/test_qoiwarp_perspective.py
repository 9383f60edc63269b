"""--perspective of tools/qoiwarp_mi355x.py, what can be checked without a GPU (an empty directory ends a run behind the arguments: "no .qoi
files"): eight numbers in the place of --orient / --rotate, with every border and the bilinear, nearest and bicubic sampling, not with a
supersampling, a vote or --scale; the parser; the item the tool makes of the corners is warp.perspective's and is accepted."""
import os

from qoi_amd import warp
from tools import qoiwarp_mi355x as warp_tool

CORNERS = "4,2,36.5,6,39,28,1,24.5"


def test_parse_perspective():
    assert warp_tool.parse_perspective(CORNERS) == [(4.0, 2.0), (36.5, 6.0), (39.0, 28.0), (1.0, 24.5)]
    assert warp_tool.parse_perspective(" 0, 0 ,1,0,1,1,0,1") == [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    for bad in ("", "1,2,3", "1,2,3,4,5,6,7", "1,2,3,4,5,6,7,8,9", "1,2,3,4,5,6,7,x", "1,2,3,4,5,6,7,inf", "1,2,3,4,5,6,7,nan", "1;2;3;4;5;6;7;8"):
        assert warp_tool.parse_perspective(bad) is None, bad


def test_the_option(tmp_path):
    lines = []
    empty = tmp_path / "in"
    empty.mkdir()
    base = [str(empty), "-o", str(tmp_path / "o"), "--perspective", CORNERS]
    for sample in ("bilinear", "nearest", "bicubic"):
        for border in warp_tool.BORDERS:
            assert warp_tool.main(base + ["--sample", sample, "--border", border, "--size", "33x40"], out=lines.append) == 2 and lines[-1] == "no .qoi files"
    only = "--perspective goes with --sample bilinear, nearest or bicubic and --supersample 1 only"
    for extra in (["--sample", "vote2"], ["--sample", "vote4"], ["--supersample", "2"], ["--supersample", "4"]):
        assert warp_tool.main(base + extra, out=lines.append) == 2 and lines[-1] == only, extra
    place = "--perspective takes the place of --orient and --rotate and takes no --scale"
    for extra in (["--orient", "3"], ["--rotate", "30"], ["--scale", "0.5"]):
        assert warp_tool.main(base + extra, out=lines.append) == 2 and lines[-1] == place, extra
    for bad in ("1,2,3", "a,b,c,d,e,f,g,h", "1,2,3,4,5,6,7,inf"):
        assert warp_tool.main([str(empty), "-o", str(tmp_path / "o"), "--perspective", bad], out=lines.append) == 2
        assert lines[-1] == "--perspective must be x0,y0,x1,y1,x2,y2,x3,y3: eight finite numbers"
    # without it the tool asks for one of the two older maps, as before
    assert warp_tool.main([str(empty), "-o", str(tmp_path / "o")], out=lines.append) == 2 and lines[-1] == "one of --orient N and --rotate DEG"
    assert "--perspective x0,y0,x1,y1,x2,y2,x3,y3" in warp_tool.__doc__ and "displacement" in warp_tool.__doc__ and not os.path.exists(tmp_path / "o")


def test_the_item_of_the_corners_is_accepted():
    """what the tool builds for a 44 x 33 image into 33 x 40: warp.perspective's map and coefficients in an item the model accepts"""
    corners = warp_tool.parse_perspective(CORNERS)
    m, proj, moved = warp.perspective((44, 33), (33, 40), corners)
    it = warp.item(0, (0, 0, 44, 33), (33, 40), m, warp.REFLECT_101 | warp.BICUBIC, 0, proj=proj)
    assert it[7] == warp.REFLECT_101 | warp.BICUBIC | warp.PROJECTIVE and warp.proj_of(it[13]) == proj != (0, 0)
    assert warp._wrong(44, 33, (0, 0, 44, 33), (33, 40), m, it[7], it[13]) == "" and warp.size(44, 33, it, 3) == 33 * 40 * 3
    assert 0 <= moved < 0.01
