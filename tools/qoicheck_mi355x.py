#!/usr/bin/env python
"""qoicheck for the MI355X path: what is in a set of .qoi files, and are they intact?

    python tools/qoicheck_mi355x.py FILE_OR_DIR...

Loads the .qoi files (directories are walked), uploads them as ONE pack and makes ONE qoimi_inspect_streams call - the chunk walk on
the GPU, no decode.  One row per file: size, w x h x channels, bytes per pixel, the six chunk kinds as a share of all chunks, the share
of pixels that come from runs, and the names of the QOIMI_SI_* flags (none: the stream is conforming); then a totals row.
Exit status 1 if any file is flagged, else 0.  Needs torch for device memory, as tools/qoibench_mi355x.py does.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def collect(paths):
    files = []
    for p in paths:
        if os.path.isdir(p):
            for base, _, names in sorted(os.walk(p)):
                files += [os.path.join(base, n) for n in sorted(names) if n.lower().endswith(".qoi")]
        else:
            files.append(p)
    return files


def row(name, size, shape, info, flags):
    chunks = int(sum(int(x) for x in info["ops"]))
    pixels = int(info["pixels"])
    share = " ".join(f"{100.0 * int(x) / chunks:5.1f}" if chunks else "    -" for x in info["ops"])
    run = f"{100.0 * int(info['run_pixels']) / pixels:5.1f}" if pixels else "    -"
    bpp = f"{size / pixels:6.3f}" if pixels else "     -"
    return f"{name:<32} {size:>10} {shape:>16} {bpp}  {share}  {run}  {flags}"


def main(argv, out=print) -> int:
    if not argv or argv[0] in ("-h", "--help"):
        out(__doc__)
        return 2
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api, streaminfo as si

    files = collect(argv)
    if not files:
        out("no .qoi files")
        return 2
    blobs = [open(f, "rb").read() for f in files]
    offsets = [int(x) for x in np.cumsum([0] + [len(b) for b in blobs[:-1]])]
    sizes = [len(b) for b in blobs]
    pack = torch.from_numpy(np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8).copy()).cuda()
    ctx = api.Context(0)
    try:
        infos, first = ctx.inspect_streams(pack.data_ptr(), offsets, sizes)
    finally:
        ctx.close()
    out(f"{'file':<32} {'bytes':>10} {'w x h x ch':>16} {'B/px':>6}  " + " ".join(f"{n:>5}" for n in si.OP_NAMES) + "   run%  flags")
    total = np.zeros((), dtype=si.INFO_DTYPE)
    for f, b, info in zip(files, blobs, infos):
        shape = f"{int.from_bytes(b[4:8], 'big')}x{int.from_bytes(b[8:12], 'big')}x{b[12]}" if len(b) >= 14 else "-"
        out(row(os.path.basename(f)[-32:], len(b), shape, info, " ".join(si.flag_names(int(info["flags"]))) or "-"))
        for k in ("pixels", "run_pixels", "repeat_index"):
            total[k] += info[k]
        total["ops"] += info["ops"]
    flagged = int(np.count_nonzero(infos["flags"]))
    out(row(f"total: {len(files)} files", sum(sizes), "", total, f"{flagged} flagged" if flagged else "-"))
    return 1 if first is not None else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
