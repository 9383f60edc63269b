"""The warp with QOIMI_WARP_PROJECTIVE against the same call without the flag, measured:
python tools/measure/warp_proj_probe.py [--frames N] [--reps R] [--out FILE]

The workload of tools/measure/warp_border_probe.py: N images (default 256, 512 x 512 RGBA) with ONE item each - a turn by 30 degrees of the
whole image, reduced into 224 x 224 x 3 as f16 CHW under REPLICATE.  Three legs of qoimi_decode_warped_tensors: the projective item (the turn
with a moderate perspective: g and h use 0.35 and 0.25 of what the limit on the denominator leaves), the same item with g = h = 0 and the
flag (the kernel warp_proj_tensor dividing by W = 2**F), and the same affine item without the flag (the kernel tensor_warp: the call as it
was before the flag existed - the yardstick).  Device events around calls that end synchronised; the legs are INTERLEAVED in every
repetition after a warm-up of every leg; median of R (default 20) with the best and the worst beside it.  The results are compared first:
the projective leg against qoi_amd/warp.py: warp and qoi_amd/tensors.py: convert for the first item, bit for bit, and the g = h = 0 leg
against the unflagged leg on the device over all N outputs.  A call's time is mostly its decode (all legs decode the same N images into the
staging arena): the difference of two medians is what the kernels differ by, with the noise of both medians.  The kernel's own time, its
occupancy and its counters, other angles, samplings and sizes are not measured here.  Needs a GPU; a run without one fails."""
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
    room = 7 * 2 ** (warp.proj_bits(OW, OH) - 3)
    gh = (int(0.35 * room / (OW - 1)), -int(0.25 * room / (OH - 1)))
    kinds = {"projective": dict(proj=gh), "projective g=h=0": dict(proj=(0, 0)), "unflagged": dict()}
    warped = {k: [warp.item(i, (0, 0, W, H), (OW, OH), turn, warp.REPLICATE, **kw) for i in range(n)] for k, kw in kinds.items()}
    fmt = (tensors.F16, tensors.CHW, *tensors.normalise(MEAN, STD))
    out_t = torch.empty((n, 3, OH, OW), dtype=torch.float16, device="cuda")
    t_off = [i * OW * OH * 3 * 2 for i in range(n)]

    def turned(key):
        ctx.decode_warped_tensors(packed.data_ptr(), so, sizes, descs, 3, warped[key], resize.PLAIN, fmt, out_t.data_ptr(), t_off, 0, st)

    # the results first
    D = np.ascontiguousarray(pixels.view(n, H, W, 4)[0].cpu().numpy()[:, :, :3])
    turned("projective"); torch.cuda.synchronize()
    it = warped["projective"][0]
    want = tensors.convert(warp.warp(D, (0, 0, W, H), (OW, OH), turn, it[7], 0, resize.PLAIN, reserved=it[13]), fmt)
    assert np.array_equal(out_t[0].cpu().numpy().view(np.uint16).reshape(-1), want.view(np.uint16).reshape(-1)), "projective"
    turned("unflagged"); torch.cuda.synchronize()
    plain = out_t.clone()
    turned("projective g=h=0"); torch.cuda.synchronize()
    assert torch.equal(out_t.view(torch.int16), plain.view(torch.int16)), "g = h = 0 against the unflagged call"
    stats = ctx.tensor_stats()
    emit({"leg": "decode_warped_tensors with QOIMI_WARP_PROJECTIVE", "g": gh[0], "h": gh[1], "F": warp.proj_bits(OW, OH), "staging_planned_bytes": stats[2],
          "sub_batches": stats[0], "images": stats[3], "source_pixels": n * W * H, "output_pixels": n * OW * OH, "bit_equal_to_the_model": True,
          "zero_coefficients_equal_the_unflagged_call": True})

    legs = {k: (lambda k=k: turned(k)) for k in warped}
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
        emit({"leg": "decode_warped_tensors 30 degrees bilinear replicate %s -> f16 CHW 224x224x3" % k, "images": n, "reps": args.reps, "median_ms": round(med[k], 3),
              "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3)})
    for k in ("projective", "projective g=h=0"):
        emit({"leg": k, "over_unflagged_ms": round(med[k] - med["unflagged"], 3)})
    ctx.close()


if __name__ == "__main__":
    main()
