"""The row seek index, measured: python tools/measure/seek_probe.py [--size N] [--band R] [--reps R] [--out FILE]

For ONE N x N photograph (default 4096 x 4096 RGBA) and one band of R rows (default 256) at its bottom prints as JSON lines
  * the one-off time of qoimi_build_seek_index at an interval of R rows (host clock around the synchronous call, a warm-up call first),
  * the time of qoimi_decode_crops for the band - the whole image is decoded - and of qoimi_decode_crops_indexed for the same crop in the same
    process: device events around calls that end synchronised, the two legs INTERLEAVED in every repetition after a warm-up of both; median of
    the repetitions and the best beside it,
  * the staging each call planned (qoimi_crop_stats [2]) and the band arena and stream bytes of the indexed call (qoimi_seek_stats).
The result is compared first: both outputs equal the rectangle of the whole-image decode.  Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--band", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.current_stream().cuda_stream
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    N, R = args.size, args.band
    desc = api.QoiDesc(N, N, 4, 0)
    image = N * N * 4
    pixels = u8(image)
    ctx = api.Context(0)
    ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 0, 1, N, N, pixels.data_ptr(), image, st)
    torch.cuda.synchronize()
    cap = api.encode_bound(N, N, 4)
    packed = u8(cap + 256)
    off, lens = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_images_packed(pixels.data_ptr(), [0], [desc], 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
    so, sizes = [int(so[0])], [int(sizes[0])]

    ctx.build_seek_index(packed.data_ptr(), so, sizes, [desc], [R], 0, st)          # warm-up: the arenas are allocated
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    points, firsts = ctx.build_seek_index(packed.data_ptr(), so, sizes, [desc], [R], 0, st)
    build_ms = (time.perf_counter() - t0) * 1e3
    emit({"leg": "build_seek_index", "image": [N, N], "interval_rows": R, "points": int(points.size), "stream_bytes": sizes[0], "ms": round(build_ms, 3),
          "index_bytes": int(points.nbytes)})

    crop = [(0, 0, N - R, N, R, 0)]
    out_plain, out_indexed = u8(N * R * 4), u8(N * R * 4)
    plain = lambda: ctx.decode_crops(packed.data_ptr(), so, sizes, [desc], 4, crop, out_plain.data_ptr(), [0], 0, st)
    indexed = lambda: ctx.decode_crops_indexed(packed.data_ptr(), so, sizes, [desc], 4, crop, out_indexed.data_ptr(), [0], [R], points, firsts, 0, st)
    plain()
    staging_plain = ctx.crop_stats()[2]
    indexed()
    staging_indexed, seek = ctx.crop_stats()[2], ctx.seek_stats()
    torch.cuda.synchronize()
    want = pixels.view(N, N, 4)[N - R:].reshape(-1)
    assert bool(torch.equal(out_plain, want)) and bool(torch.equal(out_indexed, want)), "the band differs from the pixels it was encoded from"
    legs = {"decode_crops": plain, "decode_crops_indexed": indexed}
    times = {k: [] for k in legs}
    for _ in range(2):
        for fn in legs.values():
            fn(); torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    for k, v in times.items():
        emit({"leg": k, "band_rows": [N - R, N], "reps": args.reps, "median_ms": round(statistics.median(v), 3), "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3),
              "staging_planned_bytes": staging_plain if k == "decode_crops" else staging_indexed})
    emit({"leg": "indexed call", "band_arena_bytes": seek[2], "stream_bytes_copied": seek[3],
          "ratio_to_decode_crops": round(statistics.median(times["decode_crops_indexed"]) / statistics.median(times["decode_crops"]), 4)})
    ctx.close()


if __name__ == "__main__":
    main()
