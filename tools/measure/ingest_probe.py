"""Float tensors into a pack, measured: python tools/measure/ingest_probe.py [--images N] [--reps R] [--out FILE]

N (default 64) images of 1024 x 768 x 3 as float16 C x H x W in [0, 1] (a smooth synthetic photo with noise) in one device buffer, into one
pack, align 1, default staging.  Prints as JSON lines the time of the two routes a caller has:
  (a) today's route: torch float / mul / round / clamp / to(uint8) / permute / contiguous over the whole batch - a full-size u8 HWC copy the caller
      owns; the product is taken in float32 as the header's conversion takes it, so both routes give the same bytes - then ONE
      qoimi_encode_images_packed call;
  (b) the new route: ONE qoimi_encode_tiles call whose tiles carry QOIMI_TILE_SRC | _CHW | _F16 (UNIT): the conversion runs in the gather.
Device events around whole routes, which end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of both; median of R
and the best and worst beside it.  The results are compared first, bit for bit: both packs, every stream, against each other, and a sample
of images decoded back with qoimi_decode_images against qoi_amd/tiles.py: convert.  Both legs run the same encoder over the same bytes, so
the difference of the medians is the conversion passes against the gather kernel plus one staging copy of the pixels inside (b).  The
kernel's own time, its counters, other dtypes, layouts and sizes are not measured here.  Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, CH = 1024, 768, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, tiles
    assert torch.cuda.is_available(), "needs a GPU"
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    n = args.images
    g = torch.Generator(device="cuda").manual_seed(7)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    phase = torch.arange(n * CH, device="cuda", dtype=torch.float32).reshape(n, CH, 1, 1)
    x = 0.5 + 0.45 * torch.sin(xx / 97.0 + phase) * torch.cos(yy / 61.0 + 0.3 * phase) + 0.02 * torch.randn((n, CH, H, W), device="cuda", generator=g)
    src = x.clamp(0.0, 1.0).to(torch.float16).contiguous()                   # N x C x H x W in [0, 1]
    del x
    image_bytes = W * H * CH * 2
    descs = [api.QoiDesc(W, H, CH, 0)] * n
    flags = tiles.source_flags(tiles.F16, tiles.CHW, tiles.UNIT)
    ts = [(i, 0, 0, W, H, 1, flags) for i in range(n)]
    cap = n * tiles.encode_bound(W, H, CH)
    packs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_off, d_len = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx = api.Context(0)

    def today():
        u8 = src.float().mul(255.0).round().clamp(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return ctx.encode_images_packed(u8.data_ptr(), [i * W * H * CH for i in range(n)], descs, 1, packs[0].data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())

    def new():
        return ctx.encode_tiles(src.data_ptr(), [i * image_bytes for i in range(n)], descs, 0, ts, tiles.PLAIN, 1, packs[1].data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())[:2]

    # the results first
    off_a, len_a = today()
    off_b, len_b = new()
    stats = ctx.tile_stats()
    torch.cuda.synchronize()
    total = int(off_a[-1])
    assert np.array_equal(off_a, off_b) and len_a.tolist() == len_b.tolist() and bool(torch.equal(packs[0][:total], packs[1][:total]))
    sample = sorted({0, 1, n // 2, n - 1})
    out = torch.empty(len(sample) * W * H * CH, dtype=torch.uint8, device="cuda")
    ctx.decode_images(packs[1].data_ptr(), [int(off_b[k]) for k in sample], [int(len_b[k]) for k in sample], [descs[k] for k in sample], 0, out.data_ptr(),
                      [j * W * H * CH for j in range(len(sample))])
    got = out.cpu().numpy().reshape(len(sample), H, W, CH)
    for j, k in enumerate(sample):
        assert np.array_equal(got[j], tiles.convert(src[k].cpu().numpy(), flags)), k
    emit({"leg": "f16 CHW [0, 1] into a pack", "images": n, "width": W, "height": H, "channels": CH, "source_bytes": n * image_bytes, "pack_bytes": total,
          "sub_batches": stats[0], "ingest_launches": stats[1], "staging_planned_bytes": stats[2], "packs_bit_equal": True,
          "images_compared_with_the_model": len(sample), "work_item_tiles": n * tiles.ingest_tiles(W, H)})

    legs = {"(a) torch float/mul/round/clamp/to(uint8)/permute/contiguous + encode_images_packed": today, "(b) encode_tiles with QOIMI_TILE_SRC_CHW | _F16": new}
    times = {k: [] for k in legs}
    for _ in range(2):                                          # warm-up of both legs
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
    a, b = (med[k] for k in legs)
    emit({"leg": "the new route against today's", "b_over_a": round(b / a, 3), "a_minus_b_ms": round(a - b, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
