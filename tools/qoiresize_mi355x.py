#!/usr/bin/env python
"""qoiresize for the MI355X path: a set of .qoi files as PNGs of one fixed size.

    python tools/qoiresize_mi355x.py FILE_OR_DIR... --size WxH -o DIR [--fit whole|crop] [--mode plain|weighted] [--flip x|y|xy] [--filter area|bilinear|bicubic|lanczos|nearest|mode]
                                     [--staging-mb M]

Loads the .qoi files (directories are walked), uploads them as ONE pack and makes ONE qoimi_decode_resized call: every stream is decoded on
the GPU into a bounded staging arena - only down to the last row its rectangle needs - and resampled there by the exact area filter
qoi_amd/resize.py states; neither the full-size images nor the unscaled rectangles exist outside that arena.  --fit whole (the default) resamples
the whole image to W x H, whatever its aspect; --fit crop takes the largest centred rectangle of the target's aspect (fit_rect).  Outputs hold
4 channels if any file does, else 3, and are written as DIR/<name>.png through tools/png_io.py.  One row per file: w x h x channels, the
rectangle, the output size.  --filter bilinear makes the call qoimi_decode_bilinear instead: the antialiased triangle filter qoi_amd/bilinear.py
states, the one to enlarge with; its rectangles are at most 32 times the target in an axis and max(width, W) * max(height, H) stays below 2**30.
--filter bicubic is the antialiased bicubic filter qoi_amd/bicubic.py states, through qoimi_decode_tensors as u8 HWC (it has no call of its own): at
most 16 times the target in an axis, no side above 16384.  --filter lanczos is the Lanczos filter with three lobes qoi_amd/lanczos.py states, by
the same call and with the same limits.  --filter nearest is the selection qoi_amd/nearest.py states, for label maps - one pixel of the source per
output pixel, nothing averaged -, by the same call: no side above 16384, no ratio limit.  --filter mode is the majority vote qoi_amd/mode.py
states, for REDUCING label maps - the most frequent pixel of each output pixel's cell -, by the same call: at most 16 times the target in an
axis, no side above 16384.
A file that is no QOI stream (size, magic, header rules of qoi.h:497-521) or whose rectangle is more than 64 (32, 16)
times the target in an axis is reported and left out; exit status 1 if there was one, else 0.  Needs torch for device memory, as
tools/qoicheck_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.qoicheck_mi355x import collect  # noqa: E402
from tools.qoithumb_mi355x import parse_header  # noqa: E402


def parse_size(text: str):
    """'224x160' -> (224, 160); None if it is no such size"""
    m = re.fullmatch(r"(\d+)[xX](\d+)", text.strip())
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1 or int(m.group(1)) >= 2 ** 32 or int(m.group(2)) >= 2 ** 32:
        return None
    return int(m.group(1)), int(m.group(2))


def fit_rect(w: int, h: int, ow: int, oh: int, fit: str):
    """(x, y, width, height) of the source rectangle of a w x h image for a target of ow x oh: the whole image, or - 'crop' - the largest
    centred rectangle with the target's aspect (one side is the image's, the other is floor(side * aspect), at least 1)."""
    if min(w, h, ow, oh) < 1 or fit not in ("whole", "crop"):
        raise ValueError("fit_rect: sizes >= 1, fit 'whole' or 'crop'")
    if fit == "whole":
        return 0, 0, w, h
    if w * oh > h * ow:                                            # the image is wider than the target: full height
        cw, rh = max(1, h * ow // oh), h
    else:
        cw, rh = w, max(1, w * oh // ow)
    return (w - cw) // 2, (h - rh) // 2, cw, rh


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoiresize_mi355x.py", description=".qoi files as PNGs of one fixed size through one qoimi_decode_resized call")
    ap.add_argument("paths", nargs="+", metavar="FILE_OR_DIR")
    ap.add_argument("--size", required=True, metavar="WxH")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--fit", choices=("whole", "crop"), default="whole")
    ap.add_argument("--mode", choices=("plain", "weighted"), default="plain")
    ap.add_argument("--flip", choices=("none", "x", "y", "xy"), default="none")
    ap.add_argument("--filter", choices=("area", "bilinear", "bicubic", "lanczos", "nearest", "mode"), default="area")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for decoded pixels (0: 1 GiB)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    size = parse_size(a.size)
    if size is None:
        out("--size must be WxH, both at least 1")
        return 2
    if a.staging_mb < 0:
        out("--staging-mb must not be negative")
        return 2
    ow, oh = size
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api, bicubic, bilinear, lanczos, nearest, resize, tensors
    from qoi_amd import mode as mode_filter
    from tools import png_io

    files = collect(a.paths)
    if not files:
        out("no .qoi files")
        return 2
    flags = (resize.FLIP_X if "x" in a.flip and a.flip != "none" else 0) | (resize.FLIP_Y if "y" in a.flip else 0)
    blobs = [open(f, "rb").read() for f in files]
    heads = [parse_header(b) for b in blobs]
    good = []
    for i, hd in enumerate(heads):
        if hd is None:
            out(f"{os.path.basename(files[i])}: not a QOI stream, left out")
            continue
        x, y, cw, rh = fit_rect(hd[0], hd[1], ow, oh, a.fit)
        cap = {"area": resize.MAX_RATIO, "bilinear": bilinear.MAX_RATIO, "bicubic": bicubic.MAX_RATIO, "lanczos": lanczos.MAX_RATIO, "nearest": None, "mode": mode_filter.MAX_RATIO}[a.filter]
        if cap is not None and (cw > cap * ow or rh > cap * oh):
            out(f"{os.path.basename(files[i])}: {cw}x{rh} is more than {cap} times {ow}x{oh} in an axis, left out")
            continue
        if a.filter == "bilinear" and max(cw, ow) * max(rh, oh) >= bilinear.MAX_AREA:
            out(f"{os.path.basename(files[i])}: {cw}x{rh} to {ow}x{oh} is beyond the bilinear filter's size limit, left out")
            continue
        if a.filter in ("bicubic", "lanczos", "nearest", "mode") and max(cw, ow, rh, oh) > {"nearest": nearest.MAX_SIZE, "mode": mode_filter.MAX_SIZE}.get(a.filter, bicubic.MAX_SIZE):
            out(f"{os.path.basename(files[i])}: {cw}x{rh} to {ow}x{oh} is beyond the {a.filter} filter's size limit, left out")
            continue
        good.append(i)
    if not good:
        return 1
    och = 4 if any(heads[i][2] == 4 for i in good) else 3
    offsets, sizes, descs, items, o_off = [], [], [], [], []
    pos = 0
    for k, i in enumerate(good):
        w, h, ch, cs = heads[i]
        offsets.append(pos); sizes.append(len(blobs[i])); descs.append(api.QoiDesc(w, h, ch, cs))
        items.append((k,) + fit_rect(w, h, ow, oh, a.fit) + (ow, oh, flags))
        o_off.append(k * ow * oh * och)
        pos += len(blobs[i])
    pack = torch.from_numpy(np.frombuffer(b"".join(blobs[i] for i in good) + b"\0", dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(len(good) * ow * oh * och, dtype=torch.uint8, device="cuda")
    ctx = api.Context(0)
    try:
        mode = resize.ALPHA_WEIGHTED if a.mode == "weighted" else resize.PLAIN
        if a.filter in ("bicubic", "lanczos", "nearest", "mode"):
            filt = {"bicubic": tensors.FILTER_BICUBIC, "lanczos": tensors.FILTER_LANCZOS, "nearest": tensors.FILTER_NEAREST, "mode": tensors.FILTER_MODE}[a.filter]
            ctx.decode_tensors(pack.data_ptr(), offsets, sizes, descs, och, items, filt, mode, tensors.fmt(), d_out.data_ptr(), o_off,
                               a.staging_mb << 20)
            stats = ctx.tensor_stats
        else:
            decode, stats = (ctx.decode_bilinear, ctx.bilinear_stats) if a.filter == "bilinear" else (ctx.decode_resized, ctx.resize_stats)
            decode(pack.data_ptr(), offsets, sizes, descs, och, items, mode, d_out.data_ptr(), o_off, a.staging_mb << 20)
        subs = stats()[0]
    finally:
        ctx.close()
    res = d_out.cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    used = set()
    out(f"{'file':<32} {'w x h x ch':>16} {'rectangle':>24} {'output':>12}")
    for k, i in enumerate(good):
        stem = os.path.splitext(os.path.basename(files[i]))[0]
        name, j = stem, 1
        while name in used:                                        # the same file name in two directories
            name, j = f"{stem}_{j}", j + 1
        used.add(name)
        px = res[o_off[k]:o_off[k] + ow * oh * och].reshape(oh, ow, och)
        with open(os.path.join(a.out, name + ".png"), "wb") as fh:
            fh.write(png_io.write_png(px))
        d = descs[k]
        _, x, y, cw, rh, _, _, _ = items[k]
        out(f"{os.path.basename(files[i])[-32:]:<32} {f'{d.width}x{d.height}x{d.channels}':>16} {f'{cw}x{rh}+{x}+{y}':>24} {f'{ow}x{oh}x{och}':>12}")
    out(f"total: {len(good)} images at {ow}x{oh}, {len(good) * ow * oh * och} bytes, {subs} sub-batch{'es' if subs != 1 else ''}")
    return 0 if len(good) == len(files) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
