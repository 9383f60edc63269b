#!/usr/bin/env python
"""qoithumb for the MI355X path: previews of a set of .qoi files, none longer than --max-side on its longer side.

    python tools/qoithumb_mi355x.py FILE_OR_DIR... --max-side N -o DIR [--mode plain|weighted] [--staging-mb M]

Loads the .qoi files (directories are walked), uploads them as ONE pack and makes ONE qoimi_decode_thumbnails call: every stream is decoded
on the GPU into a bounded staging arena and reduced there by the exact box filter qoi_amd/thumbs.py states; the full-size images never
exist outside that arena.  Each image gets the smallest factor 1..64 that brings its longer side to N or below (thumbs.factor_for; an image
larger than 64 x N comes out at 1/64).  Thumbnails hold 4 channels if any file does, else 3, and are written as DIR/<name>.png through
tools/png_io.py.  One row per file: w x h x channels, factor, thumbnail size.  A file that is no QOI stream (size, magic, header rules of
qoi.h:497-521) is reported and left out; exit status 1 if there was one, else 0.  Needs torch for device memory, as tools/qoicheck_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.qoicheck_mi355x import collect  # noqa: E402


def parse_header(blob: bytes):
    """(w, h, channels, colorspace) by the rules of qoi.h:497-521, or None"""
    if len(blob) < 22 or blob[:4] != b"qoif":
        return None
    w, h, ch, cs = int.from_bytes(blob[4:8], "big"), int.from_bytes(blob[8:12], "big"), blob[12], blob[13]
    if w == 0 or h == 0 or ch not in (3, 4) or cs > 1 or h >= 400000000 // w:
        return None
    return w, h, ch, cs


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoithumb_mi355x.py", description="thumbnails of .qoi files through one qoimi_decode_thumbnails call")
    ap.add_argument("paths", nargs="+", metavar="FILE_OR_DIR")
    ap.add_argument("--max-side", type=int, required=True, metavar="N")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--mode", choices=("plain", "weighted"), default="plain")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for decoded pixels (0: 1 GiB)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    if a.max_side < 1:
        out("--max-side must be at least 1")
        return 2
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api, thumbs
    from tools import png_io

    files = collect(a.paths)
    if not files:
        out("no .qoi files")
        return 2
    blobs = [open(f, "rb").read() for f in files]
    heads = [parse_header(b) for b in blobs]
    good = [i for i, hd in enumerate(heads) if hd is not None]
    for i, hd in enumerate(heads):
        if hd is None:
            out(f"{os.path.basename(files[i])}: not a QOI stream, left out")
    if not good:
        return 1
    och = 4 if any(heads[i][2] == 4 for i in good) else 3
    offsets, sizes, descs, factors, t_off, shapes = [], [], [], [], [], []
    pos = t_pos = 0
    for i in good:
        w, h, ch, cs = heads[i]
        f = thumbs.factor_for(w, h, a.max_side)
        nbytes, tw, th = api.thumbnail_size(w, h, ch, f, och)
        offsets.append(pos); sizes.append(len(blobs[i])); descs.append(api.QoiDesc(w, h, ch, cs)); factors.append(f)
        t_off.append(t_pos); shapes.append((th, tw))
        pos += len(blobs[i]); t_pos += nbytes
    pack = torch.from_numpy(np.frombuffer(b"".join(blobs[i] for i in good) + b"\0", dtype=np.uint8).copy()).cuda()
    d_thumbs = torch.zeros(t_pos, dtype=torch.uint8, device="cuda")
    ctx = api.Context(0)
    try:
        ctx.decode_thumbnails(pack.data_ptr(), offsets, sizes, descs, och, factors, thumbs.ALPHA_WEIGHTED if a.mode == "weighted" else thumbs.PLAIN,
                              d_thumbs.data_ptr(), t_off, a.staging_mb << 20)
        subs = ctx.thumbnail_stats()[0]
    finally:
        ctx.close()
    res = d_thumbs.cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    used = set()
    out(f"{'file':<32} {'w x h x ch':>16} {'f':>3} {'thumbnail':>12}")
    for k, i in enumerate(good):
        th, tw = shapes[k]
        stem = os.path.splitext(os.path.basename(files[i]))[0]
        name, j = stem, 1
        while name in used:                                        # the same file name in two directories
            name, j = f"{stem}_{j}", j + 1
        used.add(name)
        px = res[t_off[k]:t_off[k] + th * tw * och].reshape(th, tw, och)
        with open(os.path.join(a.out, name + ".png"), "wb") as fh:
            fh.write(png_io.write_png(px))
        d = descs[k]
        out(f"{os.path.basename(files[i])[-32:]:<32} {f'{d.width}x{d.height}x{d.channels}':>16} {factors[k]:>3} {f'{tw}x{th}x{och}':>12}")
    out(f"total: {len(good)} thumbnails, {t_pos} bytes, {subs} sub-batch{'es' if subs != 1 else ''}")
    return 0 if len(good) == len(files) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
