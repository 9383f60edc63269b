"""qoi_amd/tiles.py - the normative statement of qoimi_encode_tiles - against independent statements of the same thing: ``tile`` against a plain
double loop over Python ints, ``pyramid`` against the level images cut on the grid, ``plan`` against ``packplan.plan``.  No GPU, no library."""
import numpy as np
import pytest

from qoi_amd import packplan, thumbs, tiles


def loop_tile(S, t, channels, mode):
    """the definition, pixel by pixel"""
    _, x, y, cw, ch, f, flags, _ = tiles.fields(t)
    sch = S.shape[2]
    tw, th = -(-cw // f), -(-ch // f)
    och = channels or sch
    out = np.zeros((th, tw, och), dtype=np.uint8)
    for Y in range(th):
        for X in range(tw):
            px = [[int(v) for v in S[y + yy, x + xx]] + ([255] if sch == 3 else [])
                  for yy in range(Y * f, min(ch, Y * f + f)) for xx in range(X * f, min(cw, X * f + f))]
            cnt = len(px)
            s = [sum(p[c] for p in px) for c in range(4)]
            res = [(s[c] + cnt // 2) // cnt for c in range(4)]
            if mode == tiles.ALPHA_WEIGHTED and sch == 4 and s[3] > 0:
                res[:3] = [(sum(p[c] * p[3] for p in px) + s[3] // 2) // s[3] for c in range(3)]
            dx = tw - 1 - X if flags & tiles.FLIP_X else X
            dy = th - 1 - Y if flags & tiles.FLIP_Y else Y
            out[dy, dx] = res[:och]
    return out


@pytest.mark.parametrize("sch", [3, 4])
def test_tile_against_a_double_loop(sch):
    rng = np.random.default_rng(40 + sch)
    S = rng.integers(0, 256, size=(23, 31, sch), dtype=np.uint8)
    if sch == 4:
        S[:, :, 3] = rng.choice(np.array([0, 3, 255], dtype=np.uint8), size=S.shape[:2])
        S[:6, :6, 3] = 0
    differ = False
    for rect in [(0, 0, 31, 23), (3, 5, 17, 11), (30, 22, 1, 1), (0, 0, 6, 6)]:
        for f in (1, 2, 3, 5, 8, 64):
            for flags in range(4):
                for channels in (0, 3, 4):
                    got = {}
                    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED):
                        t = (0,) + rect + (f, flags)
                        got[mode] = tiles.tile(S, t, channels, mode)
                        assert np.array_equal(got[mode], loop_tile(S, t, channels, mode)), (rect, f, flags, channels, mode)
                        assert got[mode].shape == (-(-rect[3] // f), -(-rect[2] // f), channels or sch)
                    differ |= not np.array_equal(got[tiles.PLAIN], got[tiles.ALPHA_WEIGHTED])
    assert differ == (sch == 4)                                 # with 3 source channels ALPHA_WEIGHTED is PLAIN
    # a tile with factor 1, no flip and och == sch is the rectangle itself; 3 -> 4 sets alpha 255, 4 -> 3 drops alpha after the reduction
    assert np.array_equal(tiles.tile(S, (0, 3, 5, 17, 11, 1)), S[5:16, 3:20])
    other = tiles.tile(S, (0, 3, 5, 17, 11, 2), 7 - sch, tiles.ALPHA_WEIGHTED)
    same = tiles.tile(S, (0, 3, 5, 17, 11, 2), sch, tiles.ALPHA_WEIGHTED)
    assert np.array_equal(other[:, :, :3], same[:, :, :3]) and (sch == 4 or np.all(other[:, :, 3] == 255))


def test_size_and_its_zero_returns():
    assert tiles.size(70, 45, 4, (9, 3, 5, 60, 40, 13, 3, 0), 0) == (5 * 4 * 4, 5, 4)
    assert tiles.size(70, 45, 4, (0, 3, 5, 60, 40, 13), 3) == (5 * 4 * 3, 5, 4)
    assert tiles.size(70, 45, 3, (0, 0, 0, 70, 45, 1), 0) == (70 * 45 * 3, 70, 45)
    for bad in [(0, 0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 11, 0, 60, 1, 1), (0, 0, 6, 1, 40, 1), (0, 0, 0, 1, 1, 0), (0, 0, 0, 1, 1, 65),
                (0, 0, 0, 1, 1, 1, 4), (0, 0, 0, 1, 1, 1, 0, 1), (0, 2 ** 32 - 1, 0, 2, 1, 1)]:
        assert tiles.size(70, 45, 4, bad) == (0, 0, 0), bad
    good = (0, 0, 0, 1, 1, 1)
    for w, h, ch in [(0, 4, 4), (4, 0, 4), (4, 4, 2), (20000, 20000, 4)]:
        assert tiles.size(w, h, ch, good) == (0, 0, 0)
    for channels in (1, 2, 5, -3):
        assert tiles.size(4, 4, 4, good, channels) == (0, 0, 0)
    with pytest.raises(ValueError):
        tiles.tile(np.zeros((4, 4, 4), dtype=np.uint8), (0, 0, 0, 5, 1, 1))


def test_pyramid_covers_every_level_once_and_equals_the_thumbnail_cut_on_the_grid():
    w, h, tw, th, levels = 300, 200, 64, 48, 4
    rng = np.random.default_rng(7)
    S = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    pyr = tiles.pyramid(w, h, tw, th, levels)
    index = tiles.pyramid_index(w, h, tw, th, levels)
    assert len(pyr) == len(index) == sum(-(-(-(-w // (1 << l))) // tw) * -(-(-(-h // (1 << l))) // th) for l in range(levels))
    assert index == sorted(index) and len(set(index)) == len(index)         # level, row, column
    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED):
        level_img = [thumbs.thumbnail(S, 1 << l, mode) for l in range(levels)]
        cover = [np.zeros(level_img[l].shape[:2], dtype=np.int32) for l in range(levels)]
        for t, (l, r, c) in zip(pyr, index):
            image, x, y, cw, ch, f, flags, reserved = t
            assert (image, flags, reserved, f) == (0, 0, 0, 1 << l)
            assert (x, y) == (c * tw * f, r * th * f) and cw == min(tw * f, w - x) and ch == min(th * f, h - y)
            T = tiles.tile(S, t, 0, mode)
            want = level_img[l][r * th:(r + 1) * th, c * tw:(c + 1) * tw]
            assert np.array_equal(T, want), (l, r, c, mode)
            cover[l][r * th:r * th + T.shape[0], c * tw:c * tw + T.shape[1]] += 1
        assert all(np.all(cv == 1) for cv in cover)
    for bad in [(0, 5, 4, 4, 1), (5, 5, 0, 4, 1), (5, 5, 4, (1 << 24) + 1, 1), (5, 5, 4, 4, 0), (5, 5, 4, 4, 8), (20000, 20000, 4, 4, 1)]:
        with pytest.raises(ValueError):
            tiles.pyramid(*bad)
    assert tiles.pyramid(5, 3, 1 << 24, 1 << 24, 7)[6] == (0, 0, 0, 5, 3, 64, 0, 0)


def test_plan_against_packplan():
    descs = [(300, 200, 3), (0, 0, 9), (257, 129, 4)]                    # image 1 is named by no tile
    ts = [(0, 0, 0, 300, 200, 4), (2, 1, 1, 256, 128, 1, 3), (0, 17, 9, 64, 48, 1), (2, 0, 0, 257, 129, 64), (0, 0, 0, 1, 1, 1)]
    for channels in (0, 3, 4):
        raw = []
        for t in ts:
            sch = descs[t[0]][2]
            och = channels or sch
            tw, th = -(-t[3] // t[5]), -(-t[4] // t[5])
            raw.append(packplan.slot(tw * th * och) + packplan.slot(tw * th * (och + 1) + 22))
        for staging in (0, 1, raw[0], raw[0] + raw[1], raw[0] + raw[1] + raw[2] - 1, sum(raw), 1 << 40):
            slots, subs, largest, referenced = tiles.plan(descs, ts, channels, staging)
            assert slots == raw and referenced == 2
            assert subs == packplan.plan(raw, staging if staging else 1 << 30)
            assert largest == max(sum(raw[a:a + n]) for a, n in subs)
            assert sum(n for _, n in subs) == len(ts) and all(n >= 1 for _, n in subs)
        assert len(tiles.plan(descs, ts, channels, 1)[1]) == len(ts)          # raised to one slot: one tile per sub-batch
    with pytest.raises(ValueError):
        tiles.plan(descs, [(1, 0, 0, 1, 1, 1)], 0, 0)
