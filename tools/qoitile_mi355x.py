#!/usr/bin/env python
"""qoitile for the MI355X path: one .qoi file cut into tiles of T x T pixels (the tiles at the right and lower edge are smaller).

    python tools/qoitile_mi355x.py FILE.qoi --tile T -o DIR [--staging-mb M]

Uploads the file, makes ONE qoimi_decode_crops call - the stream is decoded on the GPU into a bounded staging arena and every tile is gathered
from there; the full-size image never exists outside that arena - and ONE qoimi_encode_images call over all tiles, and writes
DIR/tile_<row>_<col>.qoi with the file's channel count and colorspace.  The grid is `tile_grid`, a pure function.  Exit status 0, 1 if the file
is no QOI stream (size, magic, header rules of qoi.h:497-521), 2 for a bad command line.  Needs torch for device memory, as
tools/qoithumb_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.qoithumb_mi355x import parse_header  # noqa: E402


def tile_grid(w: int, h: int, t: int) -> List[Tuple[int, int, int, int, int, int]]:
    """(row, col, x, y, width, height) of every tile of a w x h image cut at t, row by row: ceil(h / t) rows of ceil(w / t) tiles, each t x t
    but for the last column (w - col * t wide) and the last row (h - row * t high)."""
    if w < 1 or h < 1 or t < 1:
        raise ValueError("tile_grid: w, h and t must be at least 1")
    return [(row, col, col * t, row * t, min(t, w - col * t), min(t, h - row * t))
            for row in range((h + t - 1) // t) for col in range((w + t - 1) // t)]


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoitile_mi355x.py", description="tiles of a .qoi file through one qoimi_decode_crops call")
    ap.add_argument("path", metavar="FILE.qoi")
    ap.add_argument("--tile", type=int, required=True, metavar="T")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for decoded pixels (0: 1 GiB)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    if a.tile < 1:
        out("--tile must be at least 1")
        return 2
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api

    blob = open(a.path, "rb").read()
    head = parse_header(blob)
    if head is None:
        out(f"{os.path.basename(a.path)}: not a QOI stream")
        return 1
    w, h, ch, cs = head
    grid = tile_grid(w, h, a.tile)
    n = len(grid)
    crops = [(0, x, y, tw, th, 0) for (_, _, x, y, tw, th) in grid]
    px_bytes = [tw * th * ch for (_, _, _, _, tw, th) in grid]
    px_off = [int(v) for v in np.cumsum([0] + px_bytes[:-1])]
    descs = [api.QoiDesc(tw, th, ch, cs) for (_, _, _, _, tw, th) in grid]
    bounds = [api.encode_bound(tw, th, ch) for (_, _, _, _, tw, th) in grid]
    st_off = [int(v) for v in np.cumsum([0] + bounds[:-1])]
    pack = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).cuda()
    d_tiles = torch.zeros(sum(px_bytes), dtype=torch.uint8, device="cuda")
    d_streams = torch.zeros(sum(bounds), dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx = api.Context(0)
    try:
        ctx.decode_crops(pack.data_ptr(), [0], [len(blob)], [api.QoiDesc(w, h, ch, cs)], 0, crops, d_tiles.data_ptr(), px_off, a.staging_mb << 20)
        staged = ctx.crop_stats()[2]
        ctx.encode_images(d_tiles.data_ptr(), px_off, descs, d_streams.data_ptr(), st_off, d_lens.data_ptr())
        ctx.encode_status()
        torch.cuda.synchronize()
    finally:
        ctx.close()
    lens = d_lens.cpu().numpy()
    streams = d_streams.cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    for k, (row, col, _, _, _, _) in enumerate(grid):
        with open(os.path.join(a.out, f"tile_{row}_{col}.qoi"), "wb") as fh:
            fh.write(streams[st_off[k]:st_off[k] + int(lens[k])].tobytes())
    out(f"{os.path.basename(a.path)}: {w}x{h}x{ch} -> {n} tiles of {a.tile}x{a.tile} ({grid[-1][0] + 1} rows, {grid[-1][1] + 1} columns), "
        f"{int(lens.sum())} bytes, {staged} bytes staged")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
