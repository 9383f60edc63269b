"""Label images for the tests of QOIMI_TILE_NEAREST / QOIMI_TILE_MODE (test_tile_labels_model.py, test_tile_select_core_host.py,
test_gpu_tile_labels.py) and the definition of the two reductions as a direct loop over blocks - written from the issue's words, apart from
qoi_amd/tiles.py and qoi_amd/mode.py, so that the model is checked against something that is not itself.  Random bytes alone give
all-distinct pixels, every vote a tie the centre wins: these images hold few classes in regions, noise where regions meet, and planted
blocks for the tie no centre wins."""
import numpy as np

NEAREST, MODE = 4, 5
# r, g, b, a: classes as colour-coded masks; two pairs differ in alpha alone (they vote apart and look alike at och 3)
PALETTE = np.array([[0, 0, 0, 255], [1, 2, 3, 255], [1, 2, 3, 128], [7, 0, 0, 255], [255, 255, 255, 0], [7, 0, 0, 254], [0, 9, 0, 255]], dtype=np.uint8)


def label_image(w, h, ch, seed, cell=5, noise=True):
    """uint8[h, w, ch]: regions of cell x (cell - 2) pixels of one class each, with `noise` a third of the image noise of three classes and a
    band of two-class noise, and - where the image has room - the 3 x 3 block of 4 A, 4 B and a centre C at every (9i, 9j) of a corner region, which
    is a whole block of the full image at f = 3 and f = 9 offsets alike."""
    rng = np.random.default_rng(seed)
    cw, chh = cell, max(cell - 2, 1)
    grid = rng.integers(0, len(PALETTE), size=(-(-h // chh), -(-w // cw)))
    idx = np.repeat(np.repeat(grid, chh, axis=0), cw, axis=1)[:h, :w].copy()
    if noise:
        salt = rng.integers(0, 3, size=(h, w))
        idx[:, w // 3: 2 * w // 3] = salt[:, w // 3: 2 * w // 3]
        idx[h // 2: h // 2 + max(h // 8, 1), :] = 3 + salt[h // 2: h // 2 + max(h // 8, 1), :] % 2
    if w >= 12 and h >= 12:
        for by in range(0, min(h - 2, 18), 9):
            for bx in range(0, min(w // 3 - 2, 18), 9):
                idx[by:by + 3, bx:bx + 3] = np.array([[6, 3, 6], [3, 0, 3], [6, 3, 6]])   # 4 x class 6, 4 x class 3, centre class 0: the lowest key of 3 and 6 wins
    return np.ascontiguousarray(PALETTE[idx][:, :, :ch])


def loop(S, t, channels, mode, census=None):
    """The tile t = (image, x, y, width, height, factor, flags) of S uint8[h, w, sch] in NEAREST or MODE by the definition, block by block.
    census, a dict, counts the blocks of more than one pixel by how they were decided: 'unique', 'centre' (a tie the centre pixel wins),
    'lowest' (a tie in which the centre is no winner)."""
    _, x, y, cw, ch, f, flags = (tuple(t) + (0,))[:7]
    sch = S.shape[2]
    och = channels or sch
    tw, th = -(-cw // f), -(-ch // f)
    out = np.zeros((th, tw, och), dtype=np.uint8)
    for Y in range(th):
        for X in range(tw):
            nx, ny = min((X + 1) * f, cw) - X * f, min((Y + 1) * f, ch) - Y * f
            px = {}
            for r in range(ny):
                for k in range(nx):
                    p = tuple(int(v) for v in S[y + Y * f + r, x + X * f + k]) + ((255,) if sch == 3 else ())
                    px[p] = px.get(p, 0) + 1
                    if (k, r) == (nx // 2, ny // 2):
                        centre = p
            if mode == NEAREST:
                win = centre
            else:
                top = max(px.values())
                winners = sorted(p for p, n in px.items() if n == top)          # (r, g, b, a) ascending: by key
                win = centre if centre in winners else winners[0]
                if census is not None and nx * ny > 1:
                    kind = "unique" if len(winners) == 1 else "centre" if centre in winners else "lowest"
                    census[kind] = census.get(kind, 0) + 1
            dx, dy = (tw - 1 - X if flags & 1 else X), (th - 1 - Y if flags & 2 else Y)
            out[dy, dx] = win[:och]                                              # (4 to 3 drops alpha after the vote; behind 3 it is 255)
    return out
