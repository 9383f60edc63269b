"""What the tests of QOIMI_FILTER_MODE share (tests/test_mode_model.py, tests/test_mode_core_host.py, tests/test_gpu_mode.py): the label
inputs, an independent brute-force statement of the filter - ``collections.Counter`` over the pixels the centre inequality
``2 * Z * n_src <= (2k + 1) * n_out < 2 * (Z + 1) * n_src`` selects, not ``mode.first`` - and the count of the cases a set of items reaches.
Not a test module."""
import collections

import numpy as np

# Colours whose key order (r, then g, then b, then a) is not the order of any one byte; the last two differ in alpha alone
PALETTE = np.array([[3, 0, 0, 255], [1, 200, 7, 255], [2, 5, 5, 255], [1, 200, 6, 255], [1, 200, 6, 128]], dtype=np.uint8)

# (w, h, channels, classes, seed) of the label images and the items (image, x, y, width, height, out_width, out_height, flags) over them:
# 37 x 29 to 9 x 7 (3 classes), 70 x 45 to 16 x 11 (5 classes), 37 x 29 to 50 x 7 (3 classes: enlarged in x, a vote in y)
IMAGES = [(37, 29, 3, 3, 11), (70, 45, 4, 5, 12)]
SMALL, WIDE = 0, 1
LABEL_ITEMS = [(SMALL, 0, 0, 37, 29, 9, 7, 0), (WIDE, 0, 0, 70, 45, 16, 11, 0), (SMALL, 0, 0, 37, 29, 50, 7, 0)]


def label_map(w, h, channels, classes, seed):
    """uint8[h, w, channels]: every pixel one of the first `classes` colours of PALETTE, drawn independently"""
    idx = np.random.default_rng(seed).integers(0, classes, size=(h, w))
    return np.ascontiguousarray(PALETTE[idx][:, :, :channels])


def images():
    return [label_map(*im) for im in IMAGES]


def axis_cell(Z, n_src, n_out):
    """the source samples whose centre lies in output sample Z's extent; the nearest sample if there is none"""
    ks = [k for k in range(n_src) if 2 * Z * n_src <= (2 * k + 1) * n_out < 2 * (Z + 1) * n_src]
    return ks or [((2 * Z + 1) * n_src) // (2 * n_out)]


def key(px):
    return int(px[0]) << 24 | int(px[1]) << 16 | int(px[2]) << 8 | int(px[3])


def brute(D, rect, out_size, flags=0, reach=None, och=0):
    """The filter by counting: D uint8[h, w, 3 or 4] -> uint8[oh, ow, och] (och 0: D's channels).  reach, a Counter, collects: "a" one winner that is not the
    nearest pixel, "b" a tie the centre decides, "c" a tie the lowest key decides, "d" the item has an empty cell on one axis and a vote
    (more than one pixel) on the other."""
    x, y, cw, rh = rect
    ow, oh = out_size
    sch, och = D.shape[2], och or D.shape[2]
    R = np.full((rh, cw, 4), 255, dtype=np.uint8)
    R[:, :, :sch] = D[y:y + rh, x:x + cw]
    cols = [axis_cell(X, cw, ow) for X in range(ow)]
    rows = [axis_cell(Y, rh, oh) for Y in range(oh)]
    out = np.zeros((oh, ow, 4), dtype=np.uint8)
    for Y in range(oh):
        for X in range(ow):
            votes = collections.Counter(tuple(int(v) for v in R[r, k]) for r in rows[Y] for k in cols[X])
            top = max(votes.values())
            winners = sorted((v for v, n in votes.items() if n == top), key=key)
            centre = tuple(int(v) for v in R[((2 * Y + 1) * rh) // (2 * oh), ((2 * X + 1) * cw) // (2 * ow)])
            if len(winners) == 1:
                out[Y, X] = winners[0]
                if reach is not None and winners[0] != centre:
                    reach["a"] += 1
            elif centre in winners:
                out[Y, X] = centre
                if reach is not None:
                    reach["b"] += 1
            else:
                out[Y, X] = winners[0]
                if reach is not None:
                    reach["c"] += 1
    if reach is not None:
        empty_x, empty_y = cw < ow, rh < oh                                   # (enlarging on an axis: some cell of it is empty)
        if (empty_x and max(len(r) for r in rows) > 1) or (empty_y and max(len(c) for c in cols) > 1):
            assert not empty_x or any(not [k for k in range(cw) if 2 * X * cw <= (2 * k + 1) * ow < 2 * (X + 1) * cw] for X in range(ow))
            reach["d"] += 1
    out = out[:, :, :och]
    if flags & 2:
        out = out[::-1]
    if flags & 1:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def reach_of(decoded, items):
    """the Counter of the cases the items reach; decoded(i) is image i as uint8[h, w, 4]"""
    reach = collections.Counter()
    for it in items:
        brute(decoded(it[0]), it[1:5], it[5:7], 0, reach)
    return reach
