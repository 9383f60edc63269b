#!/usr/bin/env python
"""qoistats for the MI355X path: what is in the pixels of one .qoi file, as a whole or tile by tile.

    python tools/qoistats_mi355x.py FILE.qoi [--tile T] [--staging-mb M]

Uploads the file and makes ONE qoimi_pixel_stats call - the stream is decoded on the GPU into a bounded staging arena and reduced there; the
image never exists outside that arena - over the whole image, or with --tile over the grid of tools/qoitile_mi355x.py: tile_grid.  Prints one
line per region: mean and standard deviation per channel (from `sum` and `sum_sq`, computed here) and the names of the flags; then a summary
line that counts the constant tiles (a tile server need not store them) and the opaque ones (they can be re-encoded with 3 channels).  Exit
status 0, 1 if the file cannot be read or is no QOI stream (size, magic, header rules of qoi.h:497-521), 2 for a bad command line.  Needs torch for device memory,
as tools/qoitile_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.qoithumb_mi355x import parse_header  # noqa: E402
from tools.qoitile_mi355x import tile_grid  # noqa: E402


def line(label: str, f: dict) -> str:
    from qoi_amd import pixelstats
    mean, std = pixelstats.mean_std(f)
    return (f"{label}: {f['pixels']} px  mean " + " ".join(f"{m:.3f}" for m in mean) + "  std " + " ".join(f"{s:.3f}" for s in std) +
            f"  {pixelstats.flag_names(f['flags'])}")


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoistats_mi355x.py", description="pixel statistics of a .qoi file through one qoimi_pixel_stats call")
    ap.add_argument("path", metavar="FILE.qoi")
    ap.add_argument("--tile", type=int, default=None, metavar="T", help="statistics per T x T tile instead of the whole image")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for decoded pixels (0: 1 GiB)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    if a.tile is not None and a.tile < 1:
        out("--tile must be at least 1")
        return 2
    if a.staging_mb < 0:
        out("--staging-mb must not be negative")
        return 2
    try:
        blob = open(a.path, "rb").read()
    except OSError as e:
        out(f"{a.path}: {e.strerror}")
        return 1
    head = parse_header(blob)
    if head is None:
        out(f"{os.path.basename(a.path)}: not a QOI stream")
        return 1
    w, h, ch, cs = head
    grid = tile_grid(w, h, a.tile) if a.tile is not None else [(0, 0, 0, 0, w, h)]
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api, pixelstats

    pack = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).cuda()
    ctx = api.Context(0)
    try:
        got = ctx.pixel_stats(pack.data_ptr(), [0], [len(blob)], [api.QoiDesc(w, h, ch, cs)], [(0, x, y, tw, th, 0) for (_, _, x, y, tw, th) in grid],
                              0, a.staging_mb << 20)
        staged = ctx.pixel_stats_counters()[2]
    finally:
        ctx.close()
    fields = [pixelstats.of_struct(s) for s in got]
    for (row, col, _, _, _, _), f in zip(grid, fields):
        out(line(f"tile_{row}_{col}" if a.tile is not None else "image", f))
    constant = sum(1 for f in fields if f["flags"] & pixelstats.CONSTANT)
    opaque = sum(1 for f in fields if f["flags"] & pixelstats.OPAQUE)
    what = f"{len(grid)} tiles of {a.tile}x{a.tile}" if a.tile is not None else "1 region"
    out(f"{os.path.basename(a.path)}: {w}x{h}x{ch} -> {what}, {constant} constant, {opaque} opaque, {staged} bytes staged")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
