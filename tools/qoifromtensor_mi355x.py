#!/usr/bin/env python
"""qoifromtensor for the MI355X path: an .npy batch of tensors to .qoi files - the counterpart of tools/qoitensor_mi355x.py.

    python tools/qoifromtensor_mi355x.py FILE.npy -o DIR [--range unit|symmetric|bytes] [--layout chw|hwc] [--channels 0|3|4] [--staging-mb M]

FILE.npy holds N x C x H x W or N x H x W x C (C = 3 or 4) of uint8, float16 or float32; the layout is taken from the shape (the axis of 3
or 4; --layout decides where both fit).  Uploads the array as it is and makes ONE qoimi_encode_tiles call whose tiles carry QOIMI_TILE_SRC
and the format's bits: the conversion to bytes (qoi_amd/tiles.py: convert - [0, 1], [-1, 1] or 0..255 floats; NaN and everything below 0
give 0, everything above 255 gives 255, ties round to even) runs in the gather kernel, no u8 copy of the batch exists outside the call's
staging.  Writes DIR/NNNN.qoi.  `plan_call` is a pure function.  Exit status 0, 1 if the array is none of those, 2 for a bad command line.
Needs torch for device memory, as tools/qoithumb_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qoi_amd import tiles  # noqa: E402

RANGES = {"unit": tiles.UNIT, "symmetric": tiles.SYMMETRIC, "bytes": tiles.BYTES}
DTYPES = {np.dtype(np.uint8): tiles.U8, np.dtype(np.float16): tiles.F16, np.dtype(np.float32): tiles.F32}


def plan_call(shape: Tuple[int, ...], dtype, range_name: str = "unit", layout: Optional[str] = None):
    """(n, w, h, sch, flags, image_bytes) of the call for an array of this shape and dtype, or a string saying what is wrong with it."""
    dt = DTYPES.get(np.dtype(dtype))
    if dt is None:
        return "the array is not uint8, float16 or float32"
    if len(shape) != 4 or min(shape) < 1:
        return "the array is not N x C x H x W or N x H x W x C"
    fits = [name for name, axis in (("chw", 1), ("hwc", 3)) if shape[axis] in (3, 4)]
    if layout is not None:
        fits = [name for name in fits if name == layout]
    if not fits:
        return "no axis of 3 or 4 channels where the layout wants it"
    chw = fits[0] == "chw"
    n, sch = shape[0], shape[1 if chw else 3]
    h, w = (shape[2], shape[3]) if chw else (shape[1], shape[2])
    if h >= tiles.PIXEL_CAP // w:
        return "an image of 400 000 000 pixels or more"
    rng = tiles.UNIT if dt == tiles.U8 else RANGES[range_name]
    flags = tiles.source_flags(dt, tiles.CHW if chw else tiles.HWC, rng)
    return n, w, h, sch, flags, tiles.source_bytes(w, h, sch, flags)


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoifromtensor_mi355x.py", description="an .npy batch of tensors to .qoi files through one qoimi_encode_tiles call")
    ap.add_argument("path", metavar="FILE.npy")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--range", choices=sorted(RANGES), default="unit", help="what a float element is: [0, 1], [-1, 1] or 0..255 (uint8: ignored)")
    ap.add_argument("--layout", choices=["chw", "hwc"], default=None)
    ap.add_argument("--channels", type=int, default=0, choices=[0, 3, 4], help="channels of the files (0: the tensor's)")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for converted pixels and streams (0: 1 GiB)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    try:
        arr = np.load(a.path, allow_pickle=False)
    except (OSError, ValueError) as e:
        out(f"{os.path.basename(a.path)}: {e}")
        return 1
    call = plan_call(arr.shape, arr.dtype, a.range, a.layout)
    if isinstance(call, str):
        out(f"{os.path.basename(a.path)}: {call}")
        return 1
    n, w, h, sch, flags, image_bytes = call
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api

    och = a.channels or sch
    src = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8)).cuda()
    descs = [api.QoiDesc(w, h, sch, 0)] * n
    ts: List[tuple] = [(i, 0, 0, w, h, 1, flags) for i in range(n)]
    cap = n * tiles.encode_bound(w, h, och)
    pack = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx = api.Context(0)
    try:
        off, sizes, _ = ctx.encode_tiles(src.data_ptr(), [i * image_bytes for i in range(n)], descs, a.channels, ts, tiles.PLAIN, 1, pack.data_ptr(), cap,
                                         d_off.data_ptr(), d_len.data_ptr(), a.staging_mb << 20)
        subs = ctx.tile_stats()[0]
    finally:
        ctx.close()
    host = pack[:int(off[-1])].cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    for i in range(n):
        with open(os.path.join(a.out, f"{i:04d}.qoi"), "wb") as fh:
            fh.write(host[int(off[i]):int(off[i]) + int(sizes[i])].tobytes())
    out(f"{os.path.basename(a.path)}: {n} x {w}x{h}x{sch} {arr.dtype.name} {'chw' if flags & tiles.SRC_CHW else 'hwc'} -> {n} files of {och} channels, "
        f"{int(off[-1])} bytes, {subs} sub-batch{'es' if subs != 1 else ''}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
