#!/usr/bin/env python
"""qoiwarp for the MI355X path: a set of .qoi files as PNGs, re-oriented, turned about their centre or seen in perspective.

    python tools/qoiwarp_mi355x.py FILE_OR_DIR... -o DIR (--orient N | --rotate DEG [--scale S]) [--size WxH] [--border fill|replicate|reflect|reflect101|wrap]
                                   (or --perspective x0,y0,x1,y1,x2,y2,x3,y3 in the place of --orient / --rotate)
                                   [--sample bilinear|nearest|bicubic|vote2|vote4] [--supersample 1|2|4]
                                   [--fill RRGGBBAA] [--mode plain|weighted] [--staging-mb M]

Loads the .qoi files (directories are walked), uploads them as ONE pack and makes ONE qoimi_decode_warped call: every stream is decoded on the
GPU into a bounded staging arena and sampled there through the affine map with the bilinear weights qoi_amd/warp.py states; the unturned
images do not exist outside that arena.  --orient N shows every image in the EXIF orientation N (1..8; the output is w x h, h x w for 5..8,
every output pixel one source pixel: qoimi_warp_orient).  --rotate DEG turns the image counter-clockwise about its centre, enlarged by
--scale (default 1), into an output of --size (default: the image's own size); the matrix is quantised to 2**-16 here on the host
(rotation_matrix).  Samples outside the image take --fill (default 00000000) or, with --border replicate, the nearest pixel; --border reflect
mirrors the image about its edges ("dcba|abcd|dcba", warp.REFLECT), --border reflect101 about its edge pixels ("dcb|abcd|cba", warp.REFLECT_101: the
border cv2.warpAffine pipelines default to) and --border wrap repeats it (warp.WRAP) - --fill is then not used.  --sample nearest takes
one source pixel per output pixel instead of the 2 x 2 bilinear taps (warp.NEAREST): for label maps, whose values must not be averaged; --sample bicubic takes 4 x 4 under Keys' cubic with a = -1/2 (warp.BICUBIC): sharper photographs under a turn; --sample vote2 or vote4 takes the majority vote of 2 x 2 or 4 x 4 nearest sub-samples per output pixel (warp.VOTE2, warp.VOTE4): label maps under a scale down to about 1/4, where nearest skips pixels.  There is no
adaptive antialiasing: --supersample 2 or 4 (warp.SUPER2, warp.SUPER4; default 1; with --sample bilinear only) averages 2 x 2 or 4 x 4 bilinear
sub-samples per output pixel with one rounding, which serves scales down to about 1/4; a scale well below that wants
tools/qoiresize_mi355x.py first.  --perspective x0,y0,x1,y1,x2,y2,x3,y3 names the source points - in pixel-centre coordinates of each
image - that the output's top-left, top-right, bottom-right and bottom-left corner pixels show (warp.perspective, warp.PROJECTIVE): the
output, of --size or the image's own size, is that quadrilateral rectified.  It goes with every --border and with --sample bilinear, nearest
or bicubic, not with --supersample 2 or 4 or a vote.  The homography is quantised on the host; the row of a file ends with the largest
displacement that costs at the output's corners, in source pixels.  Outputs hold 4 channels if any file does, else 3, and are
written as DIR/<name>.png through tools/png_io.py.  One row per file: w x h x channels, the map, the output size.  A file that is no QOI
stream (size, magic, header rules of qoi.h:497-521) is reported and left out; exit status 1 if there was one, else 0.  Needs torch for device
memory, as tools/qoicheck_mi355x.py does.
"""
from __future__ import annotations

import argparse
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.qoicheck_mi355x import collect  # noqa: E402
from tools.qoiresize_mi355x import parse_size  # noqa: E402
from tools.qoithumb_mi355x import parse_header  # noqa: E402

ONE = 1 << 16
BORDERS = {"fill": 0, "replicate": 1, "reflect": 64, "reflect101": 128, "wrap": 256}          # --border -> warp.REPLICATE, REFLECT, REFLECT_101, WRAP
SAMPLES = {"bilinear": 0, "nearest": 4, "bicubic": 16}                                        # --sample -> warp.NEAREST, BICUBIC
SUPERSAMPLES = {1: 0, 2: 1024, 4: 2048}                                                       # --supersample -> warp.SUPER2, SUPER4
VOTE_SAMPLES = {"vote2": 8192, "vote4": 16384}                                                # --sample, beside SAMPLES -> warp.VOTE2, VOTE4


def parse_fill(text: str):
    """'ff8000c0' -> r | g << 8 | b << 16 | a << 24; None if it is no RRGGBBAA"""
    if not re.fullmatch(r"[0-9a-fA-F]{8}", text.strip()):
        return None
    r, g, b, a = (int(text.strip()[k:k + 2], 16) for k in (0, 2, 4, 6))
    return r | g << 8 | b << 16 | a << 24


def rotation_matrix(w: int, h: int, ow: int, oh: int, degrees: float, scale: float):
    """(a, b, c, d, e, f) of qoimi_warp, quantised to 2**-16: the output shows the w x h image turned by `degrees` counter-clockwise about
    its centre and enlarged by `scale`, the image's centre at the output's centre; None where an offset leaves the limit of 2**56."""
    if min(w, h, ow, oh) < 1 or not scale > 0 or not math.isfinite(scale) or not math.isfinite(degrees):
        raise ValueError("rotation_matrix: sizes >= 1, a positive scale, a finite angle")
    t = math.radians(degrees)
    vals = [math.cos(t) / scale, -math.sin(t) / scale, math.sin(t) / scale, math.cos(t) / scale]
    if any(abs(v) * ONE >= 2 ** 31 for v in vals):
        return None
    a, b, d, e = (int(round(v * ONE)) for v in vals)
    c, f = w * ONE - a * ow - b * oh, h * ONE - d * ow - e * oh           # the output's centre (ow, oh) goes to the image's centre (w, h) << 16
    if abs(c) >= 2 ** 56 or abs(f) >= 2 ** 56:
        return None
    return a, b, c, d, e, f


def parse_perspective(text: str):
    """'x0,y0,x1,y1,x2,y2,x3,y3' -> [(x0, y0), ..., (x3, y3)] as floats; None if it is not eight finite numbers"""
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        return None
    if len(v) != 8 or not all(math.isfinite(t) for t in v):
        return None
    return [(v[0], v[1]), (v[2], v[3]), (v[4], v[5]), (v[6], v[7])]


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoiwarp_mi355x.py", description=".qoi files as re-oriented or turned PNGs through one qoimi_decode_warped call")
    ap.add_argument("paths", nargs="+", metavar="FILE_OR_DIR")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--orient", type=int, default=None, metavar="N")
    ap.add_argument("--rotate", type=float, default=None, metavar="DEG")
    ap.add_argument("--scale", type=float, default=1.0, metavar="S")
    ap.add_argument("--perspective", default=None, metavar="x0,y0,x1,y1,x2,y2,x3,y3")
    ap.add_argument("--size", default=None, metavar="WxH")
    ap.add_argument("--border", choices=tuple(BORDERS), default="fill")
    ap.add_argument("--sample", choices=tuple(SAMPLES) + tuple(VOTE_SAMPLES), default="bilinear")
    ap.add_argument("--supersample", type=int, choices=tuple(SUPERSAMPLES), default=1)
    ap.add_argument("--fill", default="00000000", metavar="RRGGBBAA")
    ap.add_argument("--mode", choices=("plain", "weighted"), default="plain")
    ap.add_argument("--staging-mb", type=int, default=0, metavar="M", help="device memory for decoded pixels (0: 1 GiB)")
    try:
        a = ap.parse_args(argv)
    except SystemExit:
        return 2
    corners = None
    if a.perspective is not None:
        if a.orient is not None or a.rotate is not None or a.scale != 1.0:
            out("--perspective takes the place of --orient and --rotate and takes no --scale")
            return 2
        corners = parse_perspective(a.perspective)
        if corners is None:
            out("--perspective must be x0,y0,x1,y1,x2,y2,x3,y3: eight finite numbers")
            return 2
        if a.supersample != 1 or a.sample in VOTE_SAMPLES:
            out("--perspective goes with --sample bilinear, nearest or bicubic and --supersample 1 only")
            return 2
    elif (a.orient is None) == (a.rotate is None):
        out("one of --orient N and --rotate DEG")
        return 2
    if a.orient is not None and (a.orient < 1 or a.orient > 8 or a.size is not None or a.scale != 1.0):
        out("--orient takes 1..8 and neither --size nor --scale")
        return 2
    size = None
    if a.size is not None:
        size = parse_size(a.size)
        if size is None or max(size) >= 1 << 20 or size[0] * size[1] >= 400_000_000:
            out("--size must be WxH, both at least 1 and below 2**20, fewer than 400 000 000 pixels")
            return 2
    if a.supersample != 1 and a.sample != "bilinear":
        out("--supersample 2 or 4 goes with --sample bilinear only")
        return 2
    fill = parse_fill(a.fill)
    if fill is None:
        out("--fill must be RRGGBBAA in hexadecimal")
        return 2
    if a.rotate is not None and (not math.isfinite(a.rotate) or not math.isfinite(a.scale) or not a.scale > 0):
        out("--rotate takes a finite angle, --scale a positive factor")
        return 2
    if a.staging_mb < 0:
        out("--staging-mb must not be negative")
        return 2
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api, warp
    from tools import png_io

    files = collect(a.paths)
    if not files:
        out("no .qoi files")
        return 2
    flags = BORDERS[a.border] | {**SAMPLES, **VOTE_SAMPLES}[a.sample] | SUPERSAMPLES[a.supersample]
    blobs = [open(f, "rb").read() for f in files]
    heads = [parse_header(b) for b in blobs]
    good, items, moved = [], [], []
    for i, hd in enumerate(heads):
        if hd is None:
            out(f"{os.path.basename(files[i])}: not a QOI stream, left out")
            continue
        w, h = hd[0], hd[1]
        k = len(good)
        if corners is not None:
            ow, oh = size if size is not None else (w, h)
            try:
                m, proj, displaced = warp.perspective((w, h), (ow, oh), corners)
            except ValueError as err:
                out(f"{os.path.basename(files[i])}: {err}, left out")
                continue
            it = warp.item(k, (0, 0, w, h), (ow, oh), m, flags, fill, proj=proj)
            wrong = warp._wrong(w, h, (0, 0, w, h), (ow, oh), m, it[7], it[13])
            if wrong:
                out(f"{os.path.basename(files[i])}: {wrong}, left out")
                continue
            moved.append(displaced)
        elif a.orient is not None:
            it = warp.orient(w, h, (0, 0, w, h), a.orient)
            it = (k,) + it[1:7] + (flags,) + it[8:12] + (fill,) + it[13:]
        else:
            ow, oh = size if size is not None else (w, h)
            m = rotation_matrix(w, h, ow, oh, a.rotate, a.scale)
            if m is None or ow >= 1 << 20 or oh >= 1 << 20:
                out(f"{os.path.basename(files[i])}: the map leaves the limits of qoimi_decode_warped, left out")
                continue
            it = warp.item(k, (0, 0, w, h), (ow, oh), m, flags, fill)
        good.append(i); items.append(it)
    if not good:
        return 1
    och = 4 if any(heads[i][2] == 4 for i in good) else 3
    offsets, sizes, descs, o_off = [], [], [], []
    pos = opos = 0
    for k, i in enumerate(good):
        w, h, ch, cs = heads[i]
        offsets.append(pos); sizes.append(len(blobs[i])); descs.append(api.QoiDesc(w, h, ch, cs))
        o_off.append(opos)
        pos += len(blobs[i]); opos += items[k][5] * items[k][6] * och
    pack = torch.from_numpy(np.frombuffer(b"".join(blobs[i] for i in good) + b"\0", dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(opos, dtype=torch.uint8, device="cuda")
    ctx = api.Context(0)
    try:
        ctx.decode_warped(pack.data_ptr(), offsets, sizes, descs, och, items, warp.ALPHA_WEIGHTED if a.mode == "weighted" else warp.PLAIN,
                          d_out.data_ptr(), o_off, a.staging_mb << 20)
        subs = ctx.warp_stats()[0]
    finally:
        ctx.close()
    res = d_out.cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    used = set()
    out(f"{'file':<32} {'w x h x ch':>16} {'a b / d e (2^-16)':>32} {'output':>14}")
    for k, i in enumerate(good):
        stem = os.path.splitext(os.path.basename(files[i]))[0]
        name, j = stem, 1
        while name in used:                                        # the same file name in two directories
            name, j = f"{stem}_{j}", j + 1
        used.add(name)
        ow, oh = items[k][5], items[k][6]
        px = res[o_off[k]:o_off[k] + ow * oh * och].reshape(oh, ow, och)
        with open(os.path.join(a.out, name + ".png"), "wb") as fh:
            fh.write(png_io.write_png(px))
        d = descs[k]
        m = items[k]
        out(f"{os.path.basename(files[i])[-32:]:<32} {f'{d.width}x{d.height}x{d.channels}':>16} {f'{m[8]} {m[9]} / {m[10]} {m[11]}':>32} {f'{ow}x{oh}x{och}':>14}"
            + (f"  g h {' '.join(str(v) for v in warp.proj_of(m[13]))}, corners displaced by at most {moved[k]:.6f} source pixels" if corners is not None else ""))
    out(f"total: {len(good)} images, {opos} bytes, {subs} sub-batch{'es' if subs != 1 else ''}")
    return 0 if len(good) == len(files) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
