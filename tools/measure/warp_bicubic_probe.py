"""The warp with QOIMI_WARP_BICUBIC against the bilinear and the nearest warp, measured: python tools/measure/warp_bicubic_probe.py [--frames N] [--reps R] [--out FILE]

For N images (default 256, 512 x 512 RGBA) with ONE item each - a turn by 30 degrees of the whole image, reduced into 224 x 224 x 3 as f16
CHW, REPLICATE - prints as JSON lines the time of qoimi_decode_warped_tensors
  (a) with QOIMI_WARP_BICUBIC (4 x 4 samples, the kernel warp_bicubic_tensor);
  (b) without a flag (2 x 2 bilinear taps, tensor_warp);
  (c) with QOIMI_WARP_NEAREST (one sample, tensor_warp).
Device events around calls that end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median of R
(default 20) with the best and the worst beside it.  The result is compared first: (a) against qoi_amd/tensors.py: warped_tensors of the
pixels for the first two items, bit for bit.  A call's time is mostly its decode (all legs decode the same N images into the staging arena):
the difference of the medians is what the kernels differ by, with the noise of both medians.  The kernel's own time, its occupancy and its
counters are not measured here.  Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, OW, OH = 512, 512, 224, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
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
        ctx.synth_frames(synth.KIND_ID["sprite_alpha"], synth.DEFAULT_SEED, i, 1, W, H, pixels.data_ptr() + po[i], image, st)
    torch.cuda.synchronize()
    cap = n * api.encode_bound(W, H, 4)
    packed = u8(cap + 256)
    off, lens = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_images_packed(pixels.data_ptr(), po, descs, 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
    so, sizes = [int(x) for x in so[:n]], [int(x) for x in sizes]
    turn = warp.rotation((W, H), (OW, OH), 30.0, OW / W)
    warped = {flag: [warp.item(i, (0, 0, W, H), (OW, OH), turn, flag | warp.REPLICATE) for i in range(n)] for flag in (warp.BICUBIC, 0, warp.NEAREST)}
    fmt = (tensors.F16, tensors.CHW, *tensors.normalise(MEAN, STD))
    out_t = torch.empty((n, 3, OH, OW), dtype=torch.float16, device="cuda")
    t_off = [i * OW * OH * 3 * 2 for i in range(n)]

    def turned(flag):
        ctx.decode_warped_tensors(packed.data_ptr(), so, sizes, descs, 3, warped[flag], resize.PLAIN, fmt, out_t.data_ptr(), t_off, 0, st)

    # the results first
    D = pixels.view(n, H, W, 4).cpu().numpy()
    turned(warp.BICUBIC); torch.cuda.synchronize()
    got = out_t.cpu().numpy()
    for i in range(min(n, 2)):
        want = tensors.warped_tensors(np.ascontiguousarray(D[i][:, :, :3]), (0, 0, W, H), (OW, OH), turn, warp.BICUBIC | warp.REPLICATE, 0, resize.PLAIN, fmt)
        assert np.array_equal(got[i].view(np.uint16), want.view(np.uint16)), i
    stats = ctx.tensor_stats()
    emit({"leg": "decode_warped_tensors bicubic", "staging_planned_bytes": stats[2], "sub_batches": stats[0], "images": stats[3], "source_pixels": n * W * H,
          "output_pixels": n * OW * OH, "bit_equal_to_the_model": True})

    legs = {"(a) decode_warped_tensors 30 degrees bicubic -> f16 CHW 224x224x3": lambda: turned(warp.BICUBIC),
            "(b) decode_warped_tensors 30 degrees bilinear -> f16 CHW 224x224x3": lambda: turned(0),
            "(c) decode_warped_tensors 30 degrees nearest -> f16 CHW 224x224x3": lambda: turned(warp.NEAREST)}
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
    emit({"leg": "bicubic against bilinear", "difference_ms": round(a - b, 3), "a_over_b": round(a / b, 3)})
    emit({"leg": "bicubic against nearest", "difference_ms": round(a - c, 3), "a_over_c": round(a / c, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
