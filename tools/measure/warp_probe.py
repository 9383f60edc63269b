"""decode_warped, measured: python tools/measure/warp_probe.py [--frames N] [--reps R] [--out FILE]

For N photographs (default 64, 1024 x 768 RGBA) with ONE random rectangle each (between a quarter and the whole of each side) prints as JSON lines
  * the time of qoimi_decode_warped of the rectangles to 224 x 224 x 3 under three maps - the rectangle scaled to the output and turned about
    its centre by 0, 90 and 30 degrees (REPLICATE) -, of qoimi_decode_bilinear of THE SAME rectangles to 224 x 224 x 3, and of
    qoimi_decode_crops of the same rectangles at 3 channels - what a caller had before, still to be warped by a kernel of the caller's own.
    Device events around calls that end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median of R
    and the best beside it.
  * the result is compared first: a few outputs of every map against qoi_amd/warp.py: warp of the whole-image decode.
All calls decode the same images down to the same rows, so the difference of two medians is what one kernel costs over the other (with the
noise of both medians).  90 against 0 degrees is what the 16 x 16 output tile is there for: the same samples, the staged rows walked along
the output's columns.  Needs a GPU; a run without one fails."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, OW, OH = 1024, 768, 224, 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, resize, synth, warp
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.current_stream().cuda_stream
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    n = args.frames
    descs = [api.QoiDesc(W, H, 4, 0)] * n
    image = W * H * 4
    po = [i * image for i in range(n)]
    pixels = u8(n * image)
    ctx = api.Context(0)
    for i in range(n):
        ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, i, 1, W, H, pixels.data_ptr() + po[i], image, st)
    torch.cuda.synchronize()
    cap = n * api.encode_bound(W, H, 4)
    packed = u8(cap + 256)
    off, lens = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_images_packed(pixels.data_ptr(), po, descs, 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
    so, sizes = [int(x) for x in so[:n]], [int(x) for x in sizes]
    rng = np.random.default_rng(7)
    rects = []
    for i in range(n):
        cw, rh = int(rng.integers(W // 4, W + 1)), int(rng.integers(H // 4, H + 1))
        rects.append((int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - rh + 1)), cw, rh))

    def matrix(cw, rh, degrees):
        """the rectangle scaled to the output (cw / OW in x, rh / OH in y), turned by `degrees` about its centre, quantised to 2**-16"""
        t = math.radians(degrees)
        a, b = (int(round(v * warp.ONE)) for v in (cw / OW * math.cos(t), -cw / OW * math.sin(t)))
        d, e = (int(round(v * warp.ONE)) for v in (rh / OH * math.sin(t), rh / OH * math.cos(t)))
        return (a, b, cw * warp.ONE - a * OW - b * OH, d, e, rh * warp.ONE - d * OW - e * OH)

    warped = {deg: [warp.item(i, r, (OW, OH), matrix(r[2], r[3], deg), warp.REPLICATE) for i, r in enumerate(rects)] for deg in (0, 90, 30)}
    items = [(i,) + r + (OW, OH, 0) for i, r in enumerate(rects)]
    cs = [(i,) + r + (0,) for i, r in enumerate(rects)]
    r_off = [i * OW * OH * 3 for i in range(n)]
    c_off = [int(x) for x in np.cumsum([0] + [r[2] * r[3] * 3 for r in rects[:-1]])]
    out_r = u8(n * OW * OH * 3)
    out_c = u8(sum(r[2] * r[3] * 3 for r in rects))

    # the result first
    ctx.decode_images(packed.data_ptr(), so, sizes, descs, 3, pixels.data_ptr(), [i * W * H * 3 for i in range(n)], st)
    whole = pixels[:n * W * H * 3].view(n, H, W, 3).cpu().numpy()
    for deg, its in warped.items():
        ctx.decode_warped(packed.data_ptr(), so, sizes, descs, 3, its, warp.PLAIN, out_r.data_ptr(), r_off, 0, st)
        got = out_r.view(n, OH, OW, 3).cpu().numpy()
        for i in range(min(n, 2)):
            f = its[i]
            assert np.array_equal(got[i], warp.warp(whole[i], rects[i], (OW, OH), (f[8], f[9], f[14], f[10], f[11], f[15]), warp.REPLICATE, 0, warp.PLAIN)), (deg, i)
    stats = ctx.warp_stats()
    emit({"leg": "decode_warped", "staging_planned_bytes": stats[2], "sub_batches": stats[0], "images": stats[3], "source_pixels": sum(r[2] * r[3] for r in rects),
          "output_pixels": n * OW * OH})

    legs = {"decode_crops same rectangles x3": lambda: ctx.decode_crops(packed.data_ptr(), so, sizes, descs, 3, cs, out_c.data_ptr(), c_off, 0, st),
            "decode_bilinear 224x224x3": lambda: ctx.decode_bilinear(packed.data_ptr(), so, sizes, descs, 3, items, resize.PLAIN, out_r.data_ptr(), r_off, 0, st)}
    for deg, its in warped.items():
        legs["decode_warped %d degrees 224x224x3" % deg] = (lambda its_: lambda: ctx.decode_warped(packed.data_ptr(), so, sizes, descs, 3, its_, warp.PLAIN, out_r.data_ptr(), r_off, 0, st))(its)
    times = {k: [] for k in legs}
    for _ in range(2):                                          # warm-up of every leg
        for fn in legs.values():
            fn(); torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        emit({"leg": k, "images": n, "reps": args.reps, "median_ms": round(med[k], 3), "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3)})
    crops_ms = med["decode_crops same rectangles x3"]
    for deg in warped:
        w = med["decode_warped %d degrees 224x224x3" % deg]
        emit({"leg": "warp %d degrees over gather" % deg, "warped_minus_crops_ms": round(w - crops_ms, 3), "ratio": round(w / crops_ms, 3)})
    w0, w90 = med["decode_warped 0 degrees 224x224x3"], med["decode_warped 90 degrees 224x224x3"]
    emit({"leg": "90 degrees against 0 degrees", "minus_ms": round(w90 - w0, 3), "ratio": round(w90 / w0, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
