"""Label tensors into a pack, measured: python tools/measure/label_ingest_probe.py [--images N] [--reps R] [--out FILE]

N (default 64) int64 planes of 1024 x 1024 class indices (regions of a few classes with noise where they meet, some elements outside 0..255)
in one device buffer, into one pack, align 1, default staging, och 4.  Two workloads: every plane whole at factor 1, and a 5-level vote
pyramid (QOIMI_TILE_MODE, f = 1 .. 16) of 256 x 256 tiles a plane.  Prints as JSON lines the time of the two routes a caller has for each:
  (a) the route without label sources: torch clamp / to(uint8) / expand to H x W x 4 with alpha 255 / contiguous over the whole batch - a u8
      HWC copy the caller owns - then ONE qoimi_encode_tiles byte call with the same tiles and mode;
  (b) ONE qoimi_encode_tiles call whose tiles carry QOIMI_TILE_LABELS | _I64: saturation and replication run in the gather kernel.
Device events around whole routes, which end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of both; median of
R (at least 20) with the best, the worst and the interquartile spread beside it.  The results are compared first, bit for bit: both packs and
both tables against each other.  The expectation looked at: the median of (b) is no worse than the median of (a) plus (a)'s own spread.  If
it fails, the per-kernel times of the encoder (qoimi_set_profiling) and a device-event time of the label kernel's launch belong beside the
numbers; this probe does not take them.  Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W = H = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions a leg"
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
    coarse = torch.randint(0, 21, (n, H // 32, W // 32), device="cuda", generator=g)
    src = coarse.repeat_interleave(32, dim=1).repeat_interleave(32, dim=2).to(torch.int64)
    noise = torch.rand((n, H, W), device="cuda", generator=g)
    src = torch.where(noise < 0.05, torch.randint(0, 21, (n, H, W), device="cuda", generator=g), src)
    src = torch.where(noise > 0.999, torch.full_like(src, -100), src)
    src = torch.where((noise > 0.998) & (noise <= 0.999), torch.full_like(src, 2 ** 32 + 5), src).contiguous()
    del coarse, noise
    flags = tiles.label_flags(tiles.L_I64)
    descs = [api.QoiDesc(W, H, 4, 0)] * n
    pyr = tiles.pyramid(W, H, 256, 256, 5)
    works = {"factor 1": ([(i, 0, 0, W, H, 1, 0) for i in range(n)], tiles.NEAREST),
             "5-level vote pyramid": ([(i,) + t[1:6] + (0,) for i in range(n) for t in pyr], tiles.MODE)}
    ctx = api.Context(0)
    for name, (ts, mode) in works.items():
        m = len(ts)
        cap = sum(tiles.encode_bound(-(-t[3] // t[5]), -(-t[4] // t[5]), 4) for t in ts)
        packs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_off, d_len = torch.zeros(m + 1, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
        lab = [t[:6] + (flags,) for t in ts]

        def baseline():
            b = src.clamp(0, 255).to(torch.uint8)
            u8 = torch.cat([b.unsqueeze(-1).expand(n, H, W, 3), torch.full((n, H, W, 1), 255, dtype=torch.uint8, device="cuda")], dim=3).contiguous()
            return ctx.encode_tiles(u8.data_ptr(), [i * W * H * 4 for i in range(n)], descs, 0, ts, mode, 1, packs[0].data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())[:2]

        def labels():
            return ctx.encode_tiles(src.data_ptr(), [i * W * H * 8 for i in range(n)], descs, 0, lab, mode, 1, packs[1].data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())[:2]

        off_a, len_a = baseline()
        off_b, len_b = labels()
        stats = ctx.tile_stats()
        torch.cuda.synchronize()
        total = int(off_a[-1])
        assert np.array_equal(off_a, off_b) and len_a.tolist() == len_b.tolist() and bool(torch.equal(packs[0][:total], packs[1][:total])), name
        emit({"workload": name, "planes": n, "width": W, "height": H, "tiles": m, "source_bytes": n * W * H * 8, "pack_bytes": total, "sub_batches": stats[0],
              "label_launches": stats[1], "packs_bit_equal": True})
        legs = {"(a) torch clamp/to(uint8)/expand x 4/contiguous + encode_tiles as a byte call": baseline, "(b) encode_tiles with QOIMI_TILE_LABELS | _I64": labels}
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
        med, spread = {}, {}
        for k, v in times.items():
            q = statistics.quantiles(v, n=4)
            med[k], spread[k] = statistics.median(v), q[2] - q[0]
            emit({"workload": name, "leg": k, "reps": args.reps, "median_ms": round(med[k], 3), "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3),
                  "interquartile_ms": round(spread[k], 3)})
        a, b = legs.keys()
        emit({"workload": name, "b_over_a": round(med[b] / med[a], 3), "a_minus_b_ms": round(med[a] - med[b], 3),
              "b_no_worse_than_a_plus_its_spread": bool(med[b] <= med[a] + spread[a])})
        del packs
    ctx.close()


if __name__ == "__main__":
    main()
