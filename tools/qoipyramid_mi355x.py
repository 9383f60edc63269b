#!/usr/bin/env python
"""qoipyramid for the MI355X path: one .qoi file as a tiled, multi-resolution pyramid - L levels, level l at 1 / 2^l of the size, each cut
into tiles of T x T pixels (the tiles at the right and lower edge are smaller).

    python tools/qoipyramid_mi355x.py FILE.qoi --tile T --levels L -o DIR [--staging-mb M] [--alpha-weighted] [--filter box|nearest|mode]

Uploads the file, decodes it ONCE with qoimi_decode_images, makes ONE qoimi_encode_tiles call over qoimi_tile_pyramid - every tile of every
level is gathered and box-reduced on the GPU from the full-resolution pixels (one rounding, not a chain of halvings), encoded and appended
to a pack; no tile's pixels and no strided stream ever exist outside the context's staging arena - and writes
DIR/<level>/tile_<row>_<col>.qoi with the file's channel count and colorspace.  --filter nearest / mode is for label maps (segmentation
masks, instance ids, palette indices), whose classes an average would invent: every block gives its centre pixel (QOIMI_TILE_NEAREST) or
the winner of a majority vote (QOIMI_TILE_MODE; a block votes over at most 16 x 16 pixels, so at most five levels - use nearest beyond).  The grid is `pyramid_grid`, a pure function.  Exit status 0,
1 if the file is no QOI stream (size, magic, header rules of qoi.h:497-521), 2 for a bad command line.  Needs torch for device memory, as
tools/qoitile_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qoi_amd import tiles  # noqa: E402
from tools.qoithumb_mi355x import parse_header  # noqa: E402


def pyramid_grid(w: int, h: int, t: int, levels: int) -> List[Tuple[int, int, int, Tuple[int, ...]]]:
    """(level, row, col, tile) of every tile, in the order of ``qoimi_tile_pyramid``: ``tiles.pyramid`` with its index."""
    return [(l, r, c, tl) for (l, r, c), tl in zip(tiles.pyramid_index(w, h, t, t, levels), tiles.pyramid(w, h, t, t, levels))]


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoipyramid_mi355x.py", description="a tile pyramid of a .qoi file through one qoimi_encode_tiles call")
    ap.add_argument("path", metavar="FILE.qoi")
    ap.add_argument("--tile", type=int, required=True, metavar="T")
    ap.add_argument("--levels", type=int, required=True, metavar="L")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for gathered tiles and their streams (0: 1 GiB)")
    ap.add_argument("--alpha-weighted", action="store_true", help="weight the colours of a block by alpha (4-channel files)")
    ap.add_argument("--filter", choices=("box", "nearest", "mode"), default="box", help="label maps: the centre pixel of every block, or its majority vote (at most 5 levels)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    if not 1 <= a.tile <= tiles.MAX_TILE_SIDE:
        out("--tile must be 1..2^24")
        return 2
    if not 1 <= a.levels <= tiles.MAX_LEVELS:
        out("--levels must be 1..7")
        return 2
    if a.staging_mb < 0:
        out("--staging-mb must not be negative")
        return 2
    if a.filter != "box" and a.alpha_weighted:
        out("--alpha-weighted belongs to --filter box")
        return 2
    if a.filter == "mode" and (1 << (a.levels - 1)) > tiles.MODE_MAX_FACTOR:
        out("--filter mode votes over blocks of at most 16 x 16 pixels: --levels must be 1..5 (use --filter nearest for more)")
        return 2
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api

    blob = open(a.path, "rb").read()
    head = parse_header(blob)
    if head is None:
        out(f"{os.path.basename(a.path)}: not a QOI stream")
        return 1
    w, h, ch, cs = head
    grid = pyramid_grid(w, h, a.tile, a.levels)
    desc = api.QoiDesc(w, h, ch, cs)
    src = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).cuda()
    d_px = torch.zeros(w * h * ch, dtype=torch.uint8, device="cuda")
    ctx = api.Context(0)
    try:
        ctx.decode_images(src.data_ptr(), [0], [len(blob)], [desc], 0, d_px.data_ptr(), [0])
        pyr = api.tile_pyramid(w, h, ch, a.tile, a.tile, a.levels)
        assert [tiles.fields(t) for t in pyr] == [g[3] for g in grid]
        n = len(pyr)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        mode = {"box": tiles.ALPHA_WEIGHTED if a.alpha_weighted else tiles.PLAIN, "nearest": tiles.NEAREST, "mode": tiles.MODE}[a.filter]
        # the pack's capacity: the sum of the tiles' encode bounds - every stream fits
        cap = sum(tiles.encode_bound(*tiles.size(w, h, ch, g[3])[1:], ch) for g in grid)
        d_pack = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        off, lens, _ = ctx.encode_tiles(d_px.data_ptr(), [0], [desc], 0, pyr, mode, 1, d_pack.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr(),
                                        a.staging_mb << 20)
        total = int(off[-1])
        staged = ctx.tile_stats()[2]
        torch.cuda.synchronize()
    finally:
        ctx.close()
    pack = d_pack.cpu().numpy()
    for k, (level, row, col, _) in enumerate(grid):
        os.makedirs(os.path.join(a.out, str(level)), exist_ok=True)
        with open(os.path.join(a.out, str(level), f"tile_{row}_{col}.qoi"), "wb") as fh:
            fh.write(pack[int(off[k]):int(off[k]) + int(lens[k])].tobytes())
    out(f"{os.path.basename(a.path)}: {w}x{h}x{ch} -> {n} tiles of {a.tile}x{a.tile} over {a.levels} levels, {total} bytes, {staged} bytes staged")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
