#!/usr/bin/env python
"""qoitensor for the MI355X path: a set of .qoi files as ONE .npy tensor, N x C x H x W or N x H x W x C, normalised.

    python tools/qoitensor_mi355x.py FILE_OR_DIR... --size WxH -o OUT.npy [--filter area|bilinear|bicubic|lanczos|nearest|mode] [--dtype u8|f16|bf16|f32|i32|i64]
                                     [--layout chw|hwc|hw|id24]
                                     [--mean M[,M,M[,M]]] [--std S[,S,S[,S]]] [--fit whole|crop] [--channels 3|4] [--staging-mb M]

Loads the .qoi files (directories are walked), uploads them as ONE pack and makes ONE qoimi_decode_tensors call: every stream is decoded on the
GPU into a bounded staging arena, resampled there to W x H (tools/qoiresize_mi355x.py: fit_rect chooses the rectangle) and written as elements
of the tensor straight from the filter's registers - 8-bit interleaved pixels never exist.  Element = (p / 255 - mean) / std per channel:
scale = 1 / (255 * std) and bias = -mean / std are computed in float64 and rounded once to float32 (scale_bias); the library then computes
float32(p) * scale + bias with two roundings and narrows once (qoi_amd/tensors.py states it).  Without --mean / --std the elements are
p / 255; --dtype u8, i32 and i64 take neither and store p.  --filter nearest --dtype i64 --layout hw makes N x H x W class indices of label maps:
one pixel of the source per element, nothing averaged, the first channel alone; --filter mode instead takes the most frequent pixel of each
element's cell (qoi_amd/mode.py: a majority vote, for REDUCING label maps).  --layout id24 (with --dtype i32 or i64 only) makes N x H x W of
24-bit ids, r | g << 8 | b << 16 of each pixel - instance and panoptic maps, what tools/qoifromlabels_mi355x.py --ids writes; it means something only with --filter nearest or mode.  One value of --mean / --std serves every channel; a fourth (alpha) defaults to mean 0, std 1.
--channels defaults to 3.  bf16 is stored as the uint16 of its bits (NumPy has no bfloat16).  A file that is no QOI stream or whose
rectangle the filter cannot reduce to the target (64 times in an axis, 32 for bilinear, 16 for bicubic and lanczos, no limit but a side of 16384 for nearest, 16 and a side of 16384 for mode) is reported and left out; exit status 1 if there was
one, else 0.  Needs torch for device memory, as tools/qoicheck_mi355x.py does.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.qoicheck_mi355x import collect  # noqa: E402
from tools.qoiresize_mi355x import fit_rect, parse_size  # noqa: E402
from tools.qoithumb_mi355x import parse_header  # noqa: E402


def parse_floats(text: str, och: int, rest: float):
    """'0.485,0.456,0.406' -> four float64: one value serves the och channels, och values are taken as they are, the channels beyond those
    given get `rest`; None if it is no such list"""
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        return None
    if len(v) == 1:
        v = v * och
    if len(v) not in (3, 4) or len(v) < och or not all(np.isfinite(v)):
        return None
    return np.array((v + [rest] * 4)[:4], np.float64)


def scale_bias(mean, std):
    """(scale, bias) as float32[4] for (p / 255 - mean) / std: 1 / (255 * std) and -mean / std in float64, each rounded once; None for a std
    of 0 or a result that is not finite in float32"""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    if mean.shape != (4,) or std.shape != (4,) or np.any(std == 0.0):
        return None
    with np.errstate(over="ignore"):
        scale, bias = (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)
    if not (np.isfinite(scale).all() and np.isfinite(bias).all()):
        return None
    return scale, bias


def main(argv, out=print) -> int:
    ap = argparse.ArgumentParser(prog="qoitensor_mi355x.py", description=".qoi files as one normalised .npy tensor through one qoimi_decode_tensors call")
    ap.add_argument("paths", nargs="+", metavar="FILE_OR_DIR")
    ap.add_argument("--size", required=True, metavar="WxH")
    ap.add_argument("-o", "--out", required=True, metavar="OUT.npy")
    ap.add_argument("--filter", choices=("area", "bilinear", "bicubic", "lanczos", "nearest", "mode"), default="bilinear")
    ap.add_argument("--dtype", choices=("u8", "f16", "bf16", "f32", "i32", "i64"), default="f32")
    ap.add_argument("--layout", choices=("chw", "hwc", "hw", "id24"), default="chw")
    ap.add_argument("--mean", default=None, metavar="M[,M,M[,M]]")
    ap.add_argument("--std", default=None, metavar="S[,S,S[,S]]")
    ap.add_argument("--fit", choices=("whole", "crop"), default="whole")
    ap.add_argument("--channels", type=int, choices=(3, 4), default=3)
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
    och = a.channels
    if a.layout == "id24" and a.dtype not in ("i32", "i64"):
        out("--layout id24 goes with --dtype i32 or i64 only")
        return 2
    if a.dtype in ("u8", "i32", "i64"):
        if a.mean is not None or a.std is not None:
            out(f"--dtype {a.dtype} stores the pixel values: it takes no --mean / --std")
            return 2
        sb = (np.ones(4, np.float32), np.zeros(4, np.float32))
    else:
        mean = parse_floats(a.mean, och, 0.0) if a.mean is not None else np.zeros(4)
        std = parse_floats(a.std, och, 1.0) if a.std is not None else np.ones(4)
        sb = scale_bias(mean, std) if mean is not None and std is not None else None
        if sb is None:
            out("--mean / --std: one finite value or one per channel, no std of 0")
            return 2
    ow, oh = size
    import torch  # first: the library then binds to the HIP runtime torch already loaded
    from qoi_amd import api, bicubic, bilinear, lanczos, nearest, resize, tensors
    from qoi_amd import mode as mode_filter

    files = collect(a.paths)
    if not files:
        out("no .qoi files")
        return 2
    model, filt = {"area": (resize, tensors.FILTER_AREA), "bilinear": (bilinear, tensors.FILTER_BILINEAR), "bicubic": (bicubic, tensors.FILTER_BICUBIC),
                   "lanczos": (lanczos, tensors.FILTER_LANCZOS), "nearest": (nearest, tensors.FILTER_NEAREST), "mode": (mode_filter, tensors.FILTER_MODE)}[a.filter]
    blobs = [open(f, "rb").read() for f in files]
    heads = [parse_header(b) for b in blobs]
    good = []
    for i, hd in enumerate(heads):
        if hd is None:
            out(f"{os.path.basename(files[i])}: not a QOI stream, left out")
            continue
        rect = fit_rect(hd[0], hd[1], ow, oh, a.fit)
        if model.size(hd[0], hd[1], rect, (ow, oh), 0, och) == 0:
            out(f"{os.path.basename(files[i])}: {rect[2]}x{rect[3]} to {ow}x{oh} is beyond the {a.filter} filter's limits, left out")
            continue
        good.append(i)
    if not good:
        return 1
    f = (tensors.DTYPE_NAMES[a.dtype], {**tensors.LAYOUT_NAMES, **tensors.ID_LAYOUT_NAMES}[a.layout], sb[0], sb[1])
    one = ow * oh * (1 if a.layout in ("hw", "id24") else och) * tensors.elem(f[0])
    offsets, sizes, descs, items = [], [], [], []
    pos = 0
    for k, i in enumerate(good):
        w, h, ch, cs = heads[i]
        offsets.append(pos); sizes.append(len(blobs[i])); descs.append(api.QoiDesc(w, h, ch, cs))
        items.append((k,) + fit_rect(w, h, ow, oh, a.fit) + (ow, oh, 0))
        pos += len(blobs[i])
    pack = torch.from_numpy(np.frombuffer(b"".join(blobs[i] for i in good) + b"\0", dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(len(good) * one, dtype=torch.uint8, device="cuda")
    ctx = api.Context(0)
    try:
        ctx.decode_tensors(pack.data_ptr(), offsets, sizes, descs, och, items, filt, tensors.PLAIN, f,
                           d_out.data_ptr(), [k * one for k in range(len(good))], a.staging_mb << 20)
        subs = ctx.tensor_stats()[0]
    finally:
        ctx.close()
    shape = {"chw": (len(good), och, oh, ow), "hwc": (len(good), oh, ow, och), "hw": (len(good), oh, ow), "id24": (len(good), oh, ow)}[a.layout]
    res = d_out.cpu().numpy().view(tensors.numpy_dtype(f[0])).reshape(shape)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.save(a.out, res)
    for k, i in enumerate(good):
        d = descs[k]
        _, x, y, cw, rh, _, _, _ = items[k]
        out(f"{k:>5} {os.path.basename(files[i])[-32:]:<32} {f'{d.width}x{d.height}x{d.channels}':>16} {f'{cw}x{rh}+{x}+{y}':>24}")
    out(f"total: {len(good)} images as {a.dtype} {'x'.join(str(s) for s in shape)}, scale {[float(v) for v in sb[0][:och]]}, bias {[float(v) for v in sb[1][:och]]}, "
        f"{subs} sub-batch{'es' if subs != 1 else ''}")
    return 0 if len(good) == len(files) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
