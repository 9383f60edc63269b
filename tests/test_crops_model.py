"""qoi_amd/crops.py - the normative statement of qoimi_decode_crops - against plain numpy and against qoi_amd/packplan.py; no GPU, no library."""
import numpy as np
import pytest

from qoi_amd import crops, packplan
from qoi_amd.crops import FLIP_X, FLIP_Y


def test_crop_against_slicing():
    rng = np.random.default_rng(1)
    for och in (3, 4):
        D = rng.integers(0, 256, size=(23, 37, och), dtype=np.uint8)
        for (x, y, w, h) in [(0, 0, 37, 23), (0, 0, 1, 1), (36, 0, 1, 1), (0, 22, 1, 1), (36, 22, 1, 1), (5, 0, 1, 23), (0, 7, 37, 1), (3, 5, 11, 9)]:
            plain = D[y:y + h, x:x + w]
            assert np.array_equal(crops.crop(D, (x, y, w, h), 0), plain)
            assert np.array_equal(crops.crop(D, (x, y, w, h), FLIP_X), plain[:, ::-1])
            assert np.array_equal(crops.crop(D, (x, y, w, h), FLIP_Y), plain[::-1])
            assert np.array_equal(crops.crop(D, (x, y, w, h), FLIP_X | FLIP_Y), plain[::-1, ::-1])
            got = crops.crop(D, (x, y, w, h), 3)
            assert got.shape == (h, w, och) and got.flags["C_CONTIGUOUS"]
    assert (FLIP_X, FLIP_Y) == (1, 2)
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (36, 0, 2, 1), (0, 22, 1, 2), (-1, 0, 2, 2)]:
        with pytest.raises(ValueError):
            crops.crop(D, bad, 0)
    with pytest.raises(ValueError):
        crops.crop(D, (0, 0, 1, 1), 4)


def test_size():
    assert crops.size(37, 23, (3, 5, 11, 9), 0, 3) == 11 * 9 * 3
    assert crops.size(37, 23, (3, 5, 11, 9), 3, 4) == 11 * 9 * 4
    assert crops.size(37, 23, (0, 0, 37, 23), 0, 4) == 37 * 23 * 4
    assert crops.size(4294967295, 1, (4294967294, 0, 1, 1), 0, 3) == 3
    for rect, flags, och in [((0, 0, 0, 1), 0, 4), ((0, 0, 1, 0), 0, 4), ((27, 0, 11, 1), 0, 4), ((0, 15, 1, 9), 0, 4), ((0, 0, 1, 1), 4, 4),
                             ((0, 0, 1, 1), 0, 0), ((0, 0, 1, 1), 0, 5), ((4294967295, 0, 2, 1), 0, 4)]:
        assert crops.size(37, 23, rect, flags, och) == 0, (rect, flags, och)


def test_rows_needed():
    descs = [(10, 20), (30, 40), (50, 60), (70, 80)]
    cs = [(2, 0, 5, 1, 1, 0), (0, 0, 0, 10, 3, 0), (2, 1, 17, 2, 2, 3), (0, 4, 10, 1, 10, 1), (2, 0, 0, 50, 7, 0)]
    assert crops.rows_needed(descs, cs) == {0: 20, 2: 19}
    assert list(crops.rows_needed(descs, cs)) == [0, 2]                                 # ascending, whatever the crops' order
    assert crops.rows_needed(descs, [(3, 0, 79, 1, 1, 0)]) == {3: 80}

    class C:                                                                            # a qoimi_crop-like structure
        image, x, y, width, height, flags = 1, 0, 3, 4, 5, 0
    assert crops.rows_needed(descs, [C()]) == {1: 8}
    with pytest.raises(ValueError):
        crops.rows_needed(descs, [(4, 0, 0, 1, 1, 0)])
    with pytest.raises(ValueError):
        crops.rows_needed(descs, [(0, 0, 19, 1, 2, 0)])


def test_plan_against_packplan():
    descs = [(130, 70), (64, 48), (257, 9), (1, 1), (333, 7), (37, 23)]
    cs = [(5, 0, 0, 37, 23, 0), (0, 0, 0, 1, 3, 0), (2, 250, 2, 7, 7, 1), (0, 100, 1, 30, 1, 2), (4, 0, 6, 1, 1, 0)]        # images 1 and 3 unreferenced
    rows = {0: 3, 2: 9, 4: 7, 5: 23}
    raw = [130 * 3 * 4, 257 * 9 * 4, 333 * 7 * 4, 37 * 23 * 4]
    slots = [packplan.slot(b) for b in raw]
    assert crops.rows_needed(descs, cs) == rows
    for staging in (0, 1, slots[0], slots[0] + slots[1], slots[0] + slots[1] + 1, sum(slots) - 1, sum(slots), 1 << 40):
        images, got_slots, subs, largest = crops.plan(descs, cs, staging)
        assert images == [0, 2, 4, 5] and got_slots == slots
        assert subs == packplan.plan(raw, staging if staging else 1 << 30)
        assert sum(count for _, count in subs) == 4 and largest == max(sum(slots[f:f + c]) for f, c in subs)
    assert len(crops.plan(descs, cs, 1)[2]) == 4                                          # a request below one slot: raised to that slot
    assert crops.plan(descs, cs, 1)[3] == max(slots)
    assert crops.plan(descs, cs, 0)[2] == [(0, 4)] and crops.plan(descs, cs, 0)[3] == sum(slots)
    assert crops.plan(descs, cs, slots[0] + slots[1])[2][0] == (0, 2)
    assert crops.plan(descs, cs[1:2], 0) == ([0], [packplan.slot(130 * 3 * 4)], [(0, 1)], 1792)     # rows 0..2 of the 130 x 70 image alone


def test_items_tile_the_output_exactly_once():
    for a in range(16):
        for B in range(1, 41):
            for q in (a, 4096 + a, (1 << 40) + a):
                it = crops.items(q, B)
                assert len(it) == ((q + B + 15) >> 4) - (q >> 4)
                covered = np.zeros(B, dtype=np.int64)
                for k, (b0, b1) in enumerate(it):
                    assert 0 <= b0 < b1 <= B and b1 - b0 <= 16, (q, B, k)
                    assert (q + b0) >> 4 == (q + b1 - 1) >> 4 == (q >> 4) + k                  # inside ONE aligned word, item k's
                    if k > 0:
                        assert (q + b0) % 16 == 0
                    if k + 1 < len(it):
                        assert (q + b1) % 16 == 0
                    covered[b0:b1] += 1
                assert np.all(covered == 1), (q, B)
    with pytest.raises(ValueError):
        crops.items(0, 0)
