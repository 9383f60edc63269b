"""Packed streams, measured: python tools/measure/packed_probe.py [--frames N] [--reps R] [--package-root DIR]

For a headline-like batch (N 4K photographs) and for the mixed directory of bench.py (288 images, 48x48 .. 2048x1536), prints as JSON lines
  * decode_batch on strided streams, decode_images on the same i*stride offsets, decode_images on a pack (align 1) into tight images
  * pack_streams against what a caller did before it (lengths to the host + one device-to-device copy per stream) and against ONE
    contiguous device copy of the same byte count (the ceiling), with the pack's fraction of it
  * stream bytes held, strided against packed
--package-root: import qoi_amd from another tree (an A/B against another build; a build without the packed entry points gives the
decode_batch figures only).  Times: milliseconds, median of R repetitions, host clock around a synchronised stream."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch
    from qoi_amd import api, synth
    ctx = api.Context(0)
    packed_api = hasattr(ctx, "pack_streams")
    st = torch.cuda.current_stream().cuda_stream
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 4)

    def workload(name, shapes, kinds, frame0):
        n = len(shapes)
        descs = [api.QoiDesc(w, h, 4, 0) for (w, h) in shapes]
        px_bytes = [w * h * 4 for (w, h) in shapes]
        po = [int(x) for x in np.cumsum([0] + [(b + 255) // 256 * 256 for b in px_bytes[:-1]])]
        ss = (max(api.encode_bound(w, h, 4) for (w, h) in shapes) + 255) // 256 * 256
        ps = (max(px_bytes) + 255) // 256 * 256
        pixels, streams, decoded = u8(po[-1] + ps), u8(n * ss), u8(n * ps)
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        for i, ((w, h), kind) in enumerate(zip(shapes, kinds)):
            ctx.synth_frames(synth.KIND_ID[kind], synth.DEFAULT_SEED, frame0 + i, 1, w, h, pixels.data_ptr() + po[i], w * h * 4, st)
        ctx.encode_images(pixels.data_ptr(), po, descs, streams.data_ptr(), [i * ss for i in range(n)], lens.data_ptr(), st)
        ctx.encode_status(st)
        sizes = [int(x) for x in lens.cpu().numpy()]
        total = sum(sizes)
        out = {"workload": name, "images": n, "stream_bytes_strided": n * ss, "stream_bytes_packed": total, "packed_api": packed_api}
        out["decode_batch_strided_ms"] = timed(lambda: ctx.decode_batch(streams.data_ptr(), ss, sizes, descs, 4, decoded.data_ptr(), ps, st))
        if packed_api:
            s_off, p_off = [i * ss for i in range(n)], [i * ps for i in range(n)]
            out["decode_images_strided_ms"] = timed(lambda: ctx.decode_images(streams.data_ptr(), s_off, sizes, descs, 4, decoded.data_ptr(), p_off, st))
            packed, off = u8(total + 256), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            out["pack_streams_ms"] = timed(lambda: ctx.pack_streams(streams.data_ptr(), ss, lens.data_ptr(), n, 1, packed.data_ptr(), total, off.data_ptr(), st))

            def by_memcpy():                                   # what a caller did before: lengths to the host, a copy per stream
                at = 0
                for i, ln in enumerate(lens.cpu().tolist()):
                    packed[at:at + ln].copy_(streams[i * ss:i * ss + ln], non_blocking=True)
                    at += ln
            out["memcpy_per_stream_ms"] = timed(by_memcpy)
            src, dst = u8(total), u8(total)
            out["one_copy_ms"] = timed(lambda: dst.copy_(src))
            del src, dst
            out["pack_fraction_of_one_copy"] = round(out["one_copy_ms"] / out["pack_streams_ms"], 3)
            out["pack_GBps_read_plus_write"] = round(2 * total / out["pack_streams_ms"] / 1e6, 1)
            offs = [int(x) for x in off.cpu().numpy()]
            assert offs[n] == total
            tight = [int(x) for x in np.cumsum([0] + px_bytes[:-1])]
            out["decode_images_packed_tight_ms"] = timed(lambda: ctx.decode_images(packed.data_ptr(), offs[:n], sizes, descs, 4, decoded.data_ptr(), tight, st))
            ok = all(bool(torch.equal(decoded[tight[i]:tight[i] + px_bytes[i]], pixels[po[i]:po[i] + px_bytes[i]])) for i in range(n))
            out["round_trip_exact"] = ok
        print(json.dumps(out), flush=True)

    workload(f"{args.frames} x 3840x2160 photo", [(3840, 2160)] * args.frames, ["photo"] * args.frames, 0)
    rng = np.random.default_rng(2026)                           # the item list of bench.py's mixed_directory leg
    kinds = ["photo", "noise", "uiflat", "constant", "photo_hard", "sprite_alpha"]
    shapes = set()
    while len(shapes) < 64:
        shapes.add((int(rng.integers(48, 2049)), int(rng.integers(48, 1537))))
    shapes = sorted(shapes)
    workload("mixed directory, 288 images", [shapes[(i * 7) % len(shapes)] for i in range(288)], [kinds[i % len(kinds)] for i in range(288)], 40000)
    ctx.close()


if __name__ == "__main__":
    main()
