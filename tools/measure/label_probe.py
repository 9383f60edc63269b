"""Label maps to N x H x W int64, measured: python tools/measure/label_probe.py [--frames N] [--reps R] [--out FILE]

For N images (default 64, 1024 x 768 RGBA) with ONE random rectangle each (between a quarter and the whole of each side; the rectangles of
tools/measure/tensor_probe.py), sampled to 224 x 224, prints as JSON lines the time of
  (a) the route without the nearest filter: qoimi_decode_warped_tensors with a scale map (a = floor(65536 * cw / ow), e likewise) and
      QOIMI_WARP_NEAREST | QOIMI_WARP_REPLICATE to f32 CHW with 3 channels, then torch's [:, 0].long() - a second pass of the caller's;
  (b) qoimi_decode_tensors with QOIMI_FILTER_NEAREST to QOIMI_TENSOR_I64 with QOIMI_TENSOR_HW - the same N x H x W int64 in one call;
  (c) qoimi_decode_tensors with QOIMI_FILTER_BILINEAR to normalised f16 CHW, for scale.
Device events around calls that end synchronised ((a) includes its torch pass); the legs are INTERLEAVED in every repetition after a warm-up
of every leg; median of R and the best and worst beside it.  The results are compared first, bit for bit: (b) against qoi_amd/tensors.py:
tensors of the decoded pixels and (a) against qoi_amd/warp.py: warp of them, for the first four items; how many elements of (a) and (b)
differ (the map of (a) has 16 fractional bits and is exact only for some ratios) is printed.  All legs decode the same images down to the
same rows - the decode is most of every leg -, so the difference of two medians is what the kernels and the second pass differ by (with the
noise of both medians).  The kernels' own times, their occupancy and their counters are not measured here.  Needs a GPU; a run without one
fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, OW, OH = 1024, 768, 224, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, resize, synth, tensors, warp
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
    items, warps = [], []
    for i in range(n):
        cw, rh = int(rng.integers(W // 4, W + 1)), int(rng.integers(H // 4, H + 1))
        x, y = int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - rh + 1))
        items.append((i, x, y, cw, rh, OW, OH, 0))
        warps.append(warp.item(i, (x, y, cw, rh), (OW, OH), (65536 * cw // OW, 0, 0, 0, 65536 * rh // OH, 0), warp.NEAREST | warp.REPLICATE, 0))
    f_a = tensors.fmt(tensors.F32, tensors.CHW)
    f_b = tensors.fmt(tensors.I64, tensors.HW)
    f_c = (tensors.F16, tensors.CHW, *tensors.normalise(MEAN, STD))
    out_a = torch.empty((n, 3, OH, OW), dtype=torch.float32, device="cuda")
    out_b = torch.empty((n, OH, OW), dtype=torch.int64, device="cuda")
    out_c = torch.empty((n, 3, OH, OW), dtype=torch.float16, device="cuda")
    off_a, off_b, off_c = ([i * OW * OH * k for i in range(n)] for k in (12, 8, 6))
    labels = {}

    def leg_a():
        ctx.decode_warped_tensors(packed.data_ptr(), so, sizes, descs, 3, warps, resize.PLAIN, f_a, out_a.data_ptr(), off_a, 0, st)
        labels["a"] = out_a[:, 0].long()

    def leg_b():
        ctx.decode_tensors(packed.data_ptr(), so, sizes, descs, 3, items, tensors.FILTER_NEAREST, resize.PLAIN, f_b, out_b.data_ptr(), off_b, 0, st)

    def leg_c():
        ctx.decode_tensors(packed.data_ptr(), so, sizes, descs, 3, items, tensors.FILTER_BILINEAR, resize.PLAIN, f_c, out_c.data_ptr(), off_c, 0, st)

    # the results first
    leg_a(); leg_b(); torch.cuda.synchronize()
    got_a, got_b = labels["a"].cpu().numpy(), out_b.cpu().numpy()
    D = pixels.view(n, H, W, 4).cpu().numpy()
    for i in range(min(n, 4)):
        rgb = np.ascontiguousarray(D[i][:, :, :3])
        want = tensors.tensors(rgb, items[i][1:5], (OW, OH), 0, tensors.FILTER_NEAREST, resize.PLAIN, f_b)
        assert want.dtype == np.int64 and np.array_equal(got_b[i], want), ("b", i)
        wa = warps[i]
        want = warp.warp(rgb, wa[1:5], (OW, OH), (wa[8], wa[9], wa[14], wa[10], wa[11], wa[15]), wa[7], wa[12], resize.PLAIN)[:, :, 0].astype(np.int64)
        assert np.array_equal(got_a[i], want), ("a", i)
    stats = ctx.tensor_stats()
    emit({"leg": "decode_tensors nearest", "staging_planned_bytes": stats[2], "sub_batches": stats[0], "images": stats[3], "source_pixels": sum(it[3] * it[4] for it in items),
          "output_pixels": n * OW * OH, "bit_equal_to_the_models": True, "elements_where_a_and_b_differ": int((got_a != got_b).sum())})

    legs = {"(a) decode_warped_tensors scale map NEAREST f32 CHW 224x224x3, then [:, 0].long()": leg_a, "(b) decode_tensors nearest i64 HW 224x224": leg_b,
            "(c) decode_tensors bilinear f16 CHW 224x224x3": leg_c}
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
    emit({"leg": "nearest filter against the warp route", "difference_ms": round(b - a, 3), "b_over_a": round(b / a, 3), "b_over_c": round(b / c, 3),
          "bytes_stored_a": n * OW * OH * (12 + 8), "bytes_stored_b": n * OW * OH * 8})
    ctx.close()


if __name__ == "__main__":
    main()
