"""decode_tensors with the Lanczos filter, measured: python tools/measure/lanczos_probe.py [--frames N] [--reps R] [--out FILE]

For N photographs (default 64, 1024 x 768 RGBA) with ONE random rectangle each (between a quarter and the whole of each side; the rectangles of
tools/measure/tensor_probe.py), resampled to 224 x 224 x 3 as normalised f16 CHW, prints as JSON lines the time of
  (a) qoimi_decode_tensors with QOIMI_FILTER_BILINEAR;
  (b) qoimi_decode_tensors with QOIMI_FILTER_BICUBIC;
  (c) qoimi_decode_tensors with QOIMI_FILTER_LANCZOS.
Device events around calls that end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median of R and
the best beside it.  The result is compared first: (c) against qoi_amd/tensors.py: tensors of the decoded pixels for the first four items, bit
for bit.  All legs decode the same images down to the same rows, so the difference of two medians is what the filter kernels differ by (with
the noise of both medians); the ratio to compare (c) / (b) with is arithmetic, 1.5 times the taps per axis.  The kernel's own time, its
occupancy and its counters are not measured here.  Needs a GPU; a run without one fails."""
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
    from qoi_amd import api, resize, synth, tensors
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
    items = []
    for i in range(n):
        cw, rh = int(rng.integers(W // 4, W + 1)), int(rng.integers(H // 4, H + 1))
        items.append((i, int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - rh + 1)), cw, rh, OW, OH, 0))
    fmt = (tensors.F16, tensors.CHW, *tensors.normalise(MEAN, STD))
    out_t = torch.empty((n, 3, OH, OW), dtype=torch.float16, device="cuda")
    t_off = [i * OW * OH * 3 * 2 for i in range(n)]

    def leg_a():
        ctx.decode_tensors(packed.data_ptr(), so, sizes, descs, 3, items, tensors.FILTER_BILINEAR, resize.PLAIN, fmt, out_t.data_ptr(), t_off, 0, st)

    def leg_b():
        ctx.decode_tensors(packed.data_ptr(), so, sizes, descs, 3, items, tensors.FILTER_BICUBIC, resize.PLAIN, fmt, out_t.data_ptr(), t_off, 0, st)

    def leg_c():
        ctx.decode_tensors(packed.data_ptr(), so, sizes, descs, 3, items, tensors.FILTER_LANCZOS, resize.PLAIN, fmt, out_t.data_ptr(), t_off, 0, st)

    # the result first
    leg_c(); torch.cuda.synchronize()
    got = out_t.cpu().numpy()
    D = pixels.view(n, H, W, 4).cpu().numpy()
    for i in range(min(n, 4)):
        want = tensors.tensors(np.ascontiguousarray(D[i][:, :, :3]), items[i][1:5], (OW, OH), 0, tensors.FILTER_LANCZOS, resize.PLAIN, fmt)
        assert np.array_equal(got[i].view(np.uint16), want.view(np.uint16)), i
    stats = ctx.tensor_stats()
    emit({"leg": "decode_tensors lanczos", "staging_planned_bytes": stats[2], "sub_batches": stats[0], "images": stats[3], "source_pixels": sum(it[3] * it[4] for it in items),
          "output_pixels": n * OW * OH, "bit_equal_to_the_model": True})

    legs = {"(a) decode_tensors bilinear f16 CHW 224x224x3": leg_a, "(b) decode_tensors bicubic f16 CHW 224x224x3": leg_b,
            "(c) decode_tensors lanczos f16 CHW 224x224x3": leg_c}
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
    emit({"leg": "lanczos against bicubic", "difference_ms": round(c - b, 3), "c_over_b": round(c / b, 3), "c_over_a": round(c / a, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
