#!/usr/bin/env python
"""qoifromlabels for the MI355X path: an .npy batch of label maps to .qoi files - the sibling of tools/qoifromtensor_mi355x.py.

    python tools/qoifromlabels_mi355x.py FILE.npy -o DIR [--levels L --tile T --mode nearest|vote] [--channels 3|4] [--staging-mb M] [--ids]

FILE.npy holds H x W or N x H x W of uint8, int32 or int64 class indices.  Uploads the array as it is and makes ONE qoimi_encode_tiles call
whose tiles carry QOIMI_TILE_LABELS and the dtype's bits: the saturation to bytes (qoi_amd/tiles.py: labels_to_bytes - below 0 gives 0, above
255 gives 255) and the replication to grey pixels run in the gather kernel, no u8 copy of the batch exists outside the call's staging.
Without --levels it writes DIR/NNNN.qoi, one file a map; with --levels L (1..7) a pyramid a map, DIR/NNNN/LEVEL/tile_ROW_COL.qoi with tiles
of T x T pixels (default 256), reduced by --mode: nearest (the centre element of every block, any level) or vote (the majority of every
block; levels up to 5, a block is at most 16 x 16).  A label map is never averaged.  The library saturates silently, so the tool counts the
elements outside 0..255 with torch before the call and prints the count.  `plan_call` is a pure function.  Exit status 0, 1 if the array
is none of those, 2 for a bad command line.  With --ids the elements are 24-bit ids - instance, panoptic or superpixel maps - and the tiles
carry QOIMI_TILE_LABELS_ID24 too: an id is saturated to 0..2^24 - 1 (qoi_amd/tiles.py: label_ids_to_bytes) and spread over r, g and b, low
byte first, as a COCO panoptic PNG holds it (id = R + 256 * G + 256^2 * B); the count of saturated elements is then taken at 2^24 - 1.  Needs torch for device memory, as tools/qoithumb_mi355x.py does.
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

MODES = {"nearest": tiles.NEAREST, "vote": tiles.MODE}
DTYPES = {np.dtype(np.uint8): tiles.L_U8, np.dtype(np.int32): tiles.L_I32, np.dtype(np.int64): tiles.L_I64}


def plan_call(shape: Tuple[int, ...], dtype, levels: int = 0, tile: int = 256, mode: str = "nearest", ids: bool = False):
    """(n, w, h, flags, plane_bytes, tiles of one map) of the call for an array of this shape and dtype - the tiles as (x, y, width, height,
    factor) with their (level, row, col) - or a string saying what is wrong with it."""
    dt = DTYPES.get(np.dtype(dtype))
    if dt is None:
        return "the array is not uint8, int32 or int64"
    if len(shape) not in (2, 3) or min(shape) < 1:
        return "the array is not H x W or N x H x W"
    n = shape[0] if len(shape) == 3 else 1
    h, w = shape[-2], shape[-1]
    if h >= tiles.PIXEL_CAP // w:
        return "a map of 400 000 000 elements or more"
    if mode not in MODES:
        return "the mode is not nearest or vote"
    if levels and not 1 <= levels <= (5 if mode == "vote" else tiles.MAX_LEVELS):
        return "levels must be 1..7, with --mode vote 1..5 (a block votes over at most 16 x 16 elements)"
    if not 1 <= tile <= tiles.MAX_TILE_SIDE:
        return "the tile side must be 1..2^24"
    flags = tiles.label_flags(dt, ids)
    if not levels:
        grid = [((0, 0, 0), (0, 0, w, h, 1))]
    else:
        grid = [(idx, t[1:6]) for idx, t in zip(tiles.pyramid_index(w, h, tile, tile, levels), tiles.pyramid(w, h, tile, tile, levels))]
    return n, w, h, flags, tiles.label_bytes(w, h, flags), grid


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoifromlabels_mi355x.py", description="an .npy batch of label maps to .qoi files or pyramids through one qoimi_encode_tiles call")
    ap.add_argument("path", metavar="FILE.npy")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--levels", type=int, default=0, metavar="L", help="write a pyramid of L levels a map (0: one file a map)")
    ap.add_argument("--tile", type=int, default=256, metavar="T", help="the side of a pyramid's tiles")
    ap.add_argument("--mode", choices=sorted(MODES), default="nearest", help="how a pyramid's levels are reduced: the centre element or the majority vote")
    ap.add_argument("--channels", type=int, default=3, choices=[3, 4], help="channels of the files: grey, or grey with alpha 255")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for converted pixels and streams (0: 1 GiB)")
    ap.add_argument("--ids", action="store_true", help="the elements are 24-bit ids, spread over r, g and b (QOIMI_TILE_LABELS_ID24)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    try:
        arr = np.load(a.path, allow_pickle=False)
    except (OSError, ValueError) as e:
        out(f"{os.path.basename(a.path)}: {e}")
        return 1
    call = plan_call(arr.shape, arr.dtype, a.levels, a.tile, a.mode, a.ids)
    if isinstance(call, str):
        out(f"{os.path.basename(a.path)}: {call}")
        return 1
    n, w, h, flags, plane_bytes, grid = call
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api

    src = torch.from_numpy(np.ascontiguousarray(arr).reshape(n, h, w)).cuda()
    top = tiles.ID_MAX if a.ids else 255
    outside = int(((src < 0) | (src > top)).sum().item()) if arr.dtype != np.uint8 else 0      # the library does not count them
    descs = [api.QoiDesc(w, h, a.channels, 0)] * n
    ts: List[tuple] = [(i,) + t + (flags,) for i in range(n) for _, t in grid]
    cap = sum(tiles.encode_bound(-(-t[2] // t[4]), -(-t[3] // t[4]), a.channels) for _, t in grid) * n
    pack = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(len(ts) + 1, dtype=torch.int64, device="cuda"), torch.zeros(len(ts), dtype=torch.int32, device="cuda")
    ctx = api.Context(0)
    try:
        off, sizes, _ = ctx.encode_tiles(src.data_ptr(), [i * plane_bytes for i in range(n)], descs, 0, ts, MODES[a.mode], 1, pack.data_ptr(), cap,
                                         d_off.data_ptr(), d_len.data_ptr(), a.staging_mb << 20)
        subs = ctx.tile_stats()[0]
    finally:
        ctx.close()
    host = pack[:int(off[-1])].cpu().numpy()
    k = 0
    for i in range(n):
        for (level, row, col), _ in grid:
            path = os.path.join(a.out, f"{i:04d}", str(level), f"tile_{row}_{col}.qoi") if a.levels else os.path.join(a.out, f"{i:04d}.qoi")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(host[int(off[k]):int(off[k]) + int(sizes[k])].tobytes())
            k += 1
    what = f"{a.levels} levels by {a.mode}, " if a.levels else ""
    out(f"{os.path.basename(a.path)}: {n} x {w}x{h} {arr.dtype.name} -> {what}{len(ts)} files of {a.channels} channels, {int(off[-1])} bytes, "
        f"{subs} sub-batch{'es' if subs != 1 else ''}; {outside} elements outside 0..{top} saturated")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
