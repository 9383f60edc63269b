"""Building the row seek index, measured: python tools/measure/seek_pixels_probe.py [--size N] [--interval R] [--reps R] [--out FILE]

For ONE N x N photograph (default 4096 x 4096 RGBA, the image of tools/measure/seek_probe.py) and an interval of R rows (default 256) prints as
JSON lines the time of qoimi_build_seek_index - one inspect plus one full decode through the staging arena - and of
qoimi_seek_index_from_pixels - the same inspect and two kernels over the pixels the pack was encoded from - in the same process: host clock
around the synchronous calls on an idle device, the two legs INTERLEAVED in every repetition after a warm-up of both (the arenas are
allocated); median of the repetitions, the best and the worst beside it.  A third leg takes the pixels from an odd byte offset (every lane's
dwords are turned).  The results are compared first: the three indexes are equal byte for byte.  The decode workspace either build leaves
behind on a fresh context is printed too.  Needs a GPU; a run without one fails."""
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
    ap.add_argument("--interval", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
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

    N, R = args.size, args.interval
    desc = api.QoiDesc(N, N, 4, 0)
    image = N * N * 4
    pixels = u8(image)
    ctx = api.Context(0)
    ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 0, 1, N, N, pixels.data_ptr(), image, st)
    torch.cuda.synchronize()
    shifted = u8(image + 8)
    shifted[3:3 + image] = pixels
    cap = api.encode_bound(N, N, 4)
    packed = u8(cap + 256)
    off, lens = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_images_packed(pixels.data_ptr(), [0], [desc], 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
    so, sizes = [int(so[0])], [int(sizes[0])]

    legs = {"build_seek_index": lambda c: c.build_seek_index(packed.data_ptr(), so, sizes, [desc], [R], 0, st),
            "seek_index_from_pixels": lambda c: c.seek_index_from_pixels(pixels.data_ptr(), [0], packed.data_ptr(), so, sizes, [desc], [R], st),
            "seek_index_from_pixels, pixels at byte offset 3": lambda c: c.seek_index_from_pixels(shifted.data_ptr(), [3], packed.data_ptr(), so, sizes, [desc], [R], st)}
    results = {k: fn(ctx)[0] for k, fn in legs.items()}
    first = results["build_seek_index"]
    assert all(v.tobytes() == first.tobytes() for v in results.values()), "the indexes differ"
    times = {k: [] for k in legs}
    for _ in range(2):
        for fn in legs.values():
            fn(ctx)
    for _ in range(args.reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(ctx)
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in times.items():
        emit({"leg": k, "image": [N, N], "interval_rows": R, "points": int(first.size), "stream_bytes": sizes[0], "reps": args.reps,
              "median_ms": round(statistics.median(v), 3), "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3)})
    emit({"leg": "ratio", "from_pixels_to_build": round(statistics.median(times["seek_index_from_pixels"]) / statistics.median(times["build_seek_index"]), 4)})
    ctx.close()
    for k in ("build_seek_index", "seek_index_from_pixels"):
        fresh = api.Context(0)
        legs[k](fresh)
        emit({"leg": k + ", fresh context", "decode_workspace_bytes": fresh.workspace_bytes()["decode"]})
        fresh.close()


if __name__ == "__main__":
    main()
