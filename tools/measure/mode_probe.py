"""Label maps reduced by a majority vote, measured: python tools/measure/mode_probe.py [--frames N] [--reps R] [--out FILE]

For N label images (default 64, 1024 x 768 with 3 channels: regions of 21 classes with curved borders and one speckle pixel in 200) with ONE
random rectangle each (between a quarter and the whole of each side; the rectangles of tools/measure/label_probe.py), reduced to 224 x 224 as
QOIMI_TENSOR_I64 with QOIMI_TENSOR_HW, prints as JSON lines the time of qoimi_decode_tensors with
  (a) QOIMI_FILTER_MODE - the vote over each output pixel's cell;
  (b) QOIMI_FILTER_NEAREST - one pixel of each cell;
  (c) QOIMI_FILTER_AREA - the average, which is no label, for scale.
Device events around calls that end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median of R
and the best and worst beside it.  The results are compared first, bit for bit: (a) and (b) against qoi_amd/tensors.py: tensors of the
pixels for the first two items; how many elements of (a) and (b) differ and the lane counts the items take are printed.  All legs decode
the same images down to the same rows - the decode is most of every leg -, so the difference of two medians is what the kernels differ by
(with the noise of both medians).  The kernel's own time, its occupancy and its counters, and other ratios are not measured here.  Needs a
GPU; a run without one fails."""
import argparse
import collections
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, OW, OH = 1024, 768, 224, 224
CLASSES = 21


def label_image(rng):
    """uint8[H, W, 3]: a coarse random class map read through a smoothly bent grid, with speckle; the class is the first byte"""
    coarse = rng.integers(0, CLASSES, size=(13, 17))
    yy, xx = np.mgrid[0:H, 0:W]
    bx = xx + 40.0 * np.sin(yy / rng.uniform(40, 90)) + rng.uniform(0, 64)
    by = yy + 40.0 * np.sin(xx / rng.uniform(40, 90)) + rng.uniform(0, 64)
    cls = coarse[(by / 80).astype(int) % 13, (bx / 80).astype(int) % 17]
    speck = rng.random((H, W)) < 0.005
    cls = np.where(speck, rng.integers(0, CLASSES, size=(H, W)), cls).astype(np.int64)
    return np.ascontiguousarray(np.stack([cls, cls * 7, 255 - cls * 11], axis=2).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, mode, resize, tensors
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.current_stream().cuda_stream
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    n = args.frames
    rng = np.random.default_rng(7)
    D = [label_image(rng) for _ in range(n)]
    descs = [api.QoiDesc(W, H, 3, 0)] * n
    image = W * H * 3
    po = [i * image for i in range(n)]
    pixels = torch.from_numpy(np.concatenate([d.reshape(-1) for d in D])).cuda()
    ctx = api.Context(0)
    cap = n * api.encode_bound(W, H, 3)
    packed = torch.empty(cap + 256, dtype=torch.uint8, device="cuda")
    off, lens = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_images_packed(pixels.data_ptr(), po, descs, 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
    so, sizes = [int(x) for x in so[:n]], [int(x) for x in sizes]
    items = []
    for i in range(n):
        cw, rh = int(rng.integers(W // 4, W + 1)), int(rng.integers(H // 4, H + 1))
        x, y = int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - rh + 1))
        items.append((i, x, y, cw, rh, OW, OH, 0))
    f = tensors.fmt(tensors.I64, tensors.HW)
    filters = {"a": tensors.FILTER_MODE, "b": tensors.FILTER_NEAREST, "c": tensors.FILTER_AREA}
    outs = {k: torch.empty((n, OH, OW), dtype=torch.int64, device="cuda") for k in filters}
    offs = [i * OW * OH * 8 for i in range(n)]

    def leg(k):
        return lambda: ctx.decode_tensors(packed.data_ptr(), so, sizes, descs, 3, items, filters[k], resize.PLAIN, f, outs[k].data_ptr(), offs, 0, st)

    # the results first
    leg("a")(); stats = ctx.tensor_stats(); leg("b")(); torch.cuda.synchronize()
    got_a, got_b = outs["a"].cpu().numpy(), outs["b"].cpu().numpy()
    for i in range(min(n, 2)):
        for k, got in (("a", got_a), ("b", got_b)):
            want = tensors.tensors(D[i], items[i][1:5], (OW, OH), 0, filters[k], resize.PLAIN, f)
            assert want.dtype == np.int64 and np.array_equal(got[i], want), (k, i)
    lanes = collections.Counter(1 << mode.split(it[3], it[4], OW, OH)[0] for it in items)
    emit({"leg": "decode_tensors mode", "staging_planned_bytes": stats[2], "sub_batches": stats[0], "images": stats[3], "source_pixels": sum(it[3] * it[4] for it in items),
          "output_pixels": n * OW * OH, "bit_equal_to_the_models": True, "elements_where_mode_and_nearest_differ": int((got_a != got_b).sum()),
          "items_by_lanes_per_pixel": {str(k): v for k, v in sorted(lanes.items())}})

    legs = {"(a) decode_tensors mode i64 HW 224x224": leg("a"), "(b) decode_tensors nearest i64 HW 224x224": leg("b"), "(c) decode_tensors area i64 HW 224x224": leg("c")}
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
    a, b, c = (med[k] for k in legs)
    emit({"leg": "mode filter against the nearest and the area filter", "a_minus_b_ms": round(a - b, 3), "a_over_b": round(a / b, 3), "a_over_c": round(a / c, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
