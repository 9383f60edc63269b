"""qoi_amd/pixelstats.py against direct numpy (sum, min, bincount) on random, constant, grey and alpha-edge images; the flags as a function of the
other fields; `first` under all four flip values; the plan is crops.plan."""
import numpy as np
import pytest

from qoi_amd import crops, pixelstats as ps


def images():
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, size=(23, 37, 4), dtype=np.uint8)
    constant = np.tile(np.array([7, 200, 31, 128], dtype=np.uint8), (9, 11, 1))
    grey = np.repeat(rng.integers(0, 256, size=(8, 13, 1), dtype=np.uint8), 4, axis=2)
    grey[..., 3] = 255
    edges = rng.integers(0, 256, size=(10, 12, 4), dtype=np.uint8)
    edges[..., 3] = rng.choice(np.array([0, 1, 254, 255], dtype=np.uint8), size=(10, 12))
    clear = rng.integers(0, 256, size=(5, 6, 4), dtype=np.uint8)
    clear[..., 3] = 0
    white = np.full((6, 7, 4), 255, dtype=np.uint8)
    return {"noise": noise, "constant": constant, "grey": grey, "edges": edges, "clear": clear, "white": white}


def rects(w, h):
    out = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, 0, 1, h), (0, h // 2, w, 1)]
    if w >= 4 and h >= 5:
        out.append((1, 2, w - 2, h - 3))
    return out


@pytest.mark.parametrize("name", sorted(images()))
def test_against_numpy(name):
    D = images()[name]
    h, w, _ = D.shape
    for (x, y, cw, ch) in rects(w, h):
        R = D[y:y + ch, x:x + cw].reshape(-1, 4)
        f = ps.stats(D, (x, y, cw, ch))
        assert f["pixels"] == cw * ch == R.shape[0]
        for c in range(4):
            col = R[:, c].astype(np.uint64)
            assert f["sum"][c] == int(col.sum()) and f["sum_sq"][c] == int((col * col).sum())
            assert f["min"][c] == int(R[:, c].min()) and f["max"][c] == int(R[:, c].max())
        assert f["opaque_pixels"] == int(np.count_nonzero(R[:, 3] == 255)) and f["transparent_pixels"] == int(np.count_nonzero(R[:, 3] == 0))
        assert f["grey_pixels"] == sum(1 for p in R if p[0] == p[1] == p[2])
        H = ps.hist(D, (x, y, cw, ch))
        assert H.shape == (4, 256) and H.dtype == np.uint32
        for c in range(4):
            assert np.array_equal(H[c], np.bincount(R[:, c], minlength=256)) and int(H[c].sum()) == cw * ch
            assert int((H[c].astype(np.uint64) * np.arange(256, dtype=np.uint64)).sum()) == f["sum"][c]
        assert set(f) == set(ps.FIELDS)


def test_flags():
    im = images()
    full = lambda D: ps.stats(D, (0, 0, D.shape[1], D.shape[0]))["flags"]
    assert full(im["constant"]) == ps.CONSTANT
    assert full(im["white"]) == ps.CONSTANT | ps.OPAQUE | ps.GREY
    assert full(im["grey"]) == ps.OPAQUE | ps.GREY
    assert full(im["clear"]) == ps.TRANSPARENT
    assert full(im["noise"]) == 0 and full(im["edges"]) == 0
    assert ps.stats(im["noise"], (3, 3, 1, 1))["flags"] & ps.CONSTANT          # one pixel is constant
    black = np.zeros((3, 3, 4), dtype=np.uint8)
    assert full(black) == ps.CONSTANT | ps.TRANSPARENT | ps.GREY
    # one pixel off clears exactly its flag
    D = im["white"].copy(); D[-1, -1, 0] = 254
    assert full(D) == ps.OPAQUE
    D = im["white"].copy(); D[2, 3, 3] = 254
    assert full(D) == ps.GREY
    D = im["clear"].copy(); D[0, 0, 3] = 1
    assert full(D) == 0
    # a function of the other fields
    for D in im.values():
        f = ps.stats(D, (0, 0, D.shape[1], D.shape[0]))
        assert ps.flags_of({k: v for k, v in f.items() if k != "flags"}) == f["flags"]
    assert (ps.CONSTANT, ps.OPAQUE, ps.TRANSPARENT, ps.GREY) == (1, 2, 4, 8)
    assert ps.flag_names(0) == "-" and ps.flag_names(3) == "constant|opaque"


def test_first_under_the_flips():
    D = images()["noise"]
    x, y, cw, ch = 5, 3, 11, 7
    word = lambda p: int(p[0]) | int(p[1]) << 8 | int(p[2]) << 16 | int(p[3]) << 24
    base = ps.stats(D, (x, y, cw, ch))
    for flags in range(4):
        f = ps.stats(D, (9, x, y, cw, ch, flags))
        assert f["first"] == word(crops.crop(D, (x, y, cw, ch), flags)[0, 0])
        assert {k: v for k, v in f.items() if k != "first"} == {k: v for k, v in base.items() if k != "first"}
    assert len({ps.stats(D, (x, y, cw, ch, fl))["first"] for fl in range(4)}) == 4
    with pytest.raises(ValueError):
        ps.stats(D, (x, y, cw, ch, 4))
    with pytest.raises(ValueError):
        ps.stats(D, (30, 0, 8, 1))
    with pytest.raises(ValueError):
        ps.stats(D[..., :3], (0, 0, 1, 1))


def test_mean_std_and_tiles():
    D = images()["noise"]
    f = ps.stats(D, (0, 0, 37, 23))
    mean, std = ps.mean_std(f)
    flat = D.reshape(-1, 4).astype(np.float64)
    assert np.allclose(mean, flat.mean(axis=0)) and np.allclose(std, flat.std(axis=0))
    assert ps.TILE_PX == 1024
    assert [ps.tiles(*s) for s in ((1, 1), (1023, 1), (1024, 1), (1025, 1), (130, 70), (19999, 20000))] == [1, 1, 1, 2, 9, 390606]


def test_plan_is_the_crops_plan():
    descs = [(64, 48), (130, 70), (5, 5)]
    regions = [(1, 0, 0, 130, 35, 1), (0, 3, 3, 8, 8, 0), (1, 100, 60, 30, 10, 2)]
    for staging in (0, 1, 20000, 1 << 20):
        assert ps.plan(descs, regions, staging) == crops.plan(descs, regions, staging)
    assert ps.plan(descs, regions, 0)[0] == [0, 1]
