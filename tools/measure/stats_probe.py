"""pixel_stats, measured: python tools/measure/stats_probe.py [--frames N] [--reps R] [--out FILE]

For N 4K photographs (default 64, 3840 x 2160 RGBA) and ONE region each - the whole image - prints as JSON lines the time of
qoimi_pixel_stats without a histogram, with one, and of qoimi_decode_crops of the same rectangles at 4 channels (the gather reads the same
staged bytes and writes them out again; the reduction writes almost nothing), all in ONE sub-batch (staging_bytes is set to what the plan
needs).  Device events around calls that end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median
of R and the best beside it.  The three calls share the decode, so the difference of two medians is the difference of their kernels - with the
noise of both; the kernels' own times are the stats_reduce and crop_gather rows of a kernel trace of this probe, taken in a run of its own.
The result is compared first: sums and histograms against torch reductions of the whole-image decode.
Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H = 3840, 2160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, pixelstats, synth
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
    regions = [(i, 0, 0, W, H, 0) for i in range(n)]
    staging = pixelstats.plan(descs, regions, 1 << 62)[3]
    hist = torch.empty(n * 1024, dtype=torch.int32, device="cuda")

    # the result first
    got = [pixelstats.of_struct(s) for s in ctx.pixel_stats(packed.data_ptr(), so, sizes, descs, regions, hist.data_ptr(), staging, st)]
    assert ctx.pixel_stats_counters()[:2] == (1, 1)
    ctx.decode_images(packed.data_ptr(), so, sizes, descs, 4, pixels.data_ptr(), po, st)
    torch.cuda.synchronize()
    whole = pixels.view(n, H * W, 4)
    for i in (0, n // 2, n - 1):
        px = whole[i].to(torch.int64)
        assert got[i]["sum"] == tuple(int(v) for v in px.sum(dim=0)) and got[i]["sum_sq"] == tuple(int(v) for v in (px * px).sum(dim=0)), i
        for c in range(4):
            assert torch.equal(hist.view(n, 4, 256)[i, c].to(torch.int64), torch.bincount(px[:, c], minlength=256)), (i, c)
    emit({"leg": "result", "images": n, "staging_planned_bytes": ctx.pixel_stats_counters()[2], "sub_batches": 1, "tile_px": pixelstats.TILE_PX})

    legs = {"pixel_stats": lambda: ctx.pixel_stats(packed.data_ptr(), so, sizes, descs, regions, 0, staging, st),
            "pixel_stats with histogram": lambda: ctx.pixel_stats(packed.data_ptr(), so, sizes, descs, regions, hist.data_ptr(), staging, st),
            "decode_crops": lambda: ctx.decode_crops(packed.data_ptr(), so, sizes, descs, 4, regions, pixels.data_ptr(), po, staging, st)}
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
    emit({"leg": "difference of medians", "pixel_stats_minus_decode_crops_ms": round(med["pixel_stats"] - med["decode_crops"], 3),
          "with_histogram_minus_decode_crops_ms": round(med["pixel_stats with histogram"] - med["decode_crops"], 3)})
    ctx.close()


if __name__ == "__main__":
    main()
