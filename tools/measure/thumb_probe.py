"""decode_thumbnails, measured: python tools/measure/thumb_probe.py [--frames N] [--reps R] [--out FILE]

For N 4K photographs (default 64) and for the mixed directory of bench.py (288 images, 64 shapes, all content classes) prints as JSON lines,
per factor f = 2, 4, 8, 64 and mode (plain, alpha weighted):
  * the time of qoimi_decode_thumbnails of the pack (4 output channels, staging: everything in one sub-batch - the decode is then the same
    one call in both legs) and the time of qoimi_decode_images of the same pack into full-size images.  Host clock around calls that end
    synchronised; every leg INTERLEAVED in every repetition, best of R (and the median beside it).  The decoder is the same code in both
    legs, so the second time is also what a caller paid before this call existed - without the shrinking it then had to do itself.
  * their ratio, and the reduction pass read as a bandwidth: width * height * 4 bytes per image (the staging it reads once) over the
    DIFFERENCE of the two best times, against 6.3 TB/s, the achievable HBM rate of the MI355X.  The difference of two wall-clock times
    carries the noise of both: it is a figure to read against the expectation "the call costs the decode plus one read of the staging",
    not a kernel time.
  * the result is compared first: the thumbnails of a second context with staging_bytes of 1/4 of the slots are byte-identical.
Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, synth, thumbs
    from qoi_amd.packplan import plan, slot
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.current_stream().cuda_stream
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    def workload(name, shapes, kinds, frame0):
        n = len(shapes)
        descs = [api.QoiDesc(w, h, 4, 0) for (w, h) in shapes]
        px_bytes = [w * h * 4 for (w, h) in shapes]
        slots = [slot(b) for b in px_bytes]
        po = [int(x) for x in np.cumsum([0] + slots[:-1])]
        pixels = u8(po[-1] + slots[-1])
        ctx = api.Context(0)
        for i, ((w, h), kind) in enumerate(zip(shapes, kinds)):
            ctx.synth_frames(synth.KIND_ID[kind], synth.DEFAULT_SEED, frame0 + i, 1, w, h, pixels.data_ptr() + po[i], w * h * 4, st)
        torch.cuda.synchronize()
        cap = sum(api.encode_bound(w, h, 4) for (w, h) in shapes)
        packed = u8(cap + 256)
        off, lens = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        so, sizes = ctx.encode_images_packed(pixels.data_ptr(), po, descs, 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
        so, sizes = [int(x) for x in so[:n]], [int(x) for x in sizes]
        all_slots = sum(slots)
        other = api.Context(0)                                   # the same call through four or more sub-batches: the result must not change

        def full_decode():
            ctx.decode_images(packed.data_ptr(), so, sizes, descs, 4, pixels.data_ptr(), po, st)

        configs = [(f, mode) for f in (2, 4, 8, 64) for mode in (thumbs.PLAIN, thumbs.ALPHA_WEIGHTED)]
        t_off, t_bytes, t_total = {}, {}, 0
        for f in (2, 4, 8, 64):
            nb = [api.thumbnail_size(w, h, 4, f, 4)[0] for (w, h) in shapes]
            t_off[f] = [int(x) for x in np.cumsum([0] + nb[:-1])]
            t_bytes[f] = sum(nb)
            t_total = max(t_total, sum(nb))
        out_a, out_b = u8(t_total + 64), u8(t_total + 64)

        def thumb_call(c, f, mode, dst, staging):
            c.decode_thumbnails(packed.data_ptr(), so, sizes, descs, 4, f, mode, dst.data_ptr(), t_off[f], staging, st)

        legs = {"decode_images": full_decode}
        for f, mode in configs:
            thumb_call(ctx, f, mode, out_a, all_slots)
            assert ctx.thumbnail_stats()[:2] == (1, 1)
            thumb_call(other, f, mode, out_b, all_slots // 4)
            assert other.thumbnail_stats()[0] == len(plan(px_bytes, all_slots // 4)) >= 4
            used = t_bytes[f]
            assert bool(torch.equal(out_a[:used], out_b[:used])), (f, mode)
            legs[(f, mode)] = (lambda f_, m_: lambda: thumb_call(ctx, f_, m_, out_a, all_slots))(f, mode)
        other.close()
        times = {k: [] for k in legs}
        for fn in legs.values():                                # warm-up of every leg
            fn(); torch.cuda.synchronize()
        for _ in range(args.reps):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
        dec_best, dec_med = min(times["decode_images"]), statistics.median(times["decode_images"])
        emit({"workload": name, "leg": "decode_images", "images": n, "decoded_bytes": sum(px_bytes), "best_ms": round(dec_best, 3), "median_ms": round(dec_med, 3)})
        for f, mode in configs:
            best, med = min(times[(f, mode)]), statistics.median(times[(f, mode)])
            extra = best - dec_best
            emit({"workload": name, "leg": "decode_thumbnails", "factor": f, "mode": "weighted" if mode else "plain", "best_ms": round(best, 3),
                  "median_ms": round(med, 3), "ratio_to_decode_images": round(best / dec_best, 3), "reduction_ms": round(extra, 3),
                  "reduction_TBps": round(sum(px_bytes) / (extra * 1e-3) / 1e12, 3) if extra > 0 else None,
                  "share_of_6.3TBps": round(sum(px_bytes) / (extra * 1e-3) / HBM_ACHIEVABLE, 3) if extra > 0 else None,
                  "thumbnail_bytes": t_bytes[f], "staging_bytes": ctx.thumbnail_stats()[2]})
        ctx.close()

    workload(f"{args.frames} x 3840x2160 photo", [(3840, 2160)] * args.frames, ["photo"] * args.frames, 0)
    rng = np.random.default_rng(2026)                           # the item list of bench.py's mixed_directory leg
    kinds = ["photo", "noise", "uiflat", "constant", "photo_hard", "sprite_alpha"]
    shapes = set()
    while len(shapes) < 64:
        shapes.add((int(rng.integers(48, 2049)), int(rng.integers(48, 1537))))
    shapes = sorted(shapes)
    workload("mixed directory, 288 images", [shapes[(i * 7) % len(shapes)] for i in range(288)], [kinds[i % len(kinds)] for i in range(288)], 40000)


if __name__ == "__main__":
    main()
