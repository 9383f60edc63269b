"""qoimi_inspect_streams, measured: python tools/measure/inspect_probe.py [--frames N] [--reps R]

N (default 256) synthetic 4K frames - once `photo`, once `uiflat` - are encoded and packed on the device (align 1); on that pack, in one
process, prints as JSON lines
  * inspect_streams: milliseconds (HIP events around the call, median of R after 3 warm-ups) and GB/s of stream bytes
  * hash_streams on the strided streams: an existing kernel that reads the same bytes once - the yardstick for "one read"
  * decode_images of the same pack: what a caller pays to learn the same thing by decoding
  * the per-kernel times of one inspect_streams call from qoimi_get_profile, and the context's workspace"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from qoi_amd import api, synth
    n, w, h = args.frames, 3840, 2160
    st = torch.cuda.current_stream().cuda_stream
    u8 = lambda k: torch.empty(int(k), dtype=torch.uint8, device="cuda")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b))
        return round(statistics.median(ts), 4)

    for kind in ("photo", "uiflat"):
        ctx = api.Context(0)
        desc = api.QoiDesc(w, h, 4, 0)
        ps = w * h * 4
        ss = (api.encode_bound(w, h, 4) + 255) // 256 * 256
        pixels, streams = u8(n * ps), u8(n * ss)
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx.synth_frames(synth.KIND_ID[kind], synth.DEFAULT_SEED, 0, n, w, h, pixels.data_ptr(), ps, st)
        ctx.encode_batch(pixels.data_ptr(), ps, desc, n, streams.data_ptr(), ss, lens.data_ptr(), st)
        ctx.encode_status(st)
        sizes = [int(x) for x in lens.cpu().numpy()]
        total = sum(sizes)
        packed, off = u8(total + 256), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        ctx.pack_streams(streams.data_ptr(), ss, lens.data_ptr(), n, 1, packed.data_ptr(), total, off.data_ptr(), st)
        ctx.encode_status(st)
        offs = [int(x) for x in off.cpu().numpy()[:n]]
        hashes = torch.zeros(n, dtype=torch.int64, device="cuda")
        out = {"workload": f"{n} x {w}x{h} {kind}", "stream_bytes": total}
        infos, first = ctx.inspect_streams(packed.data_ptr(), offs, sizes, st)
        out["all_conforming"] = first is None and all(int(x) == w * h for x in infos["pixels"])
        chunks = infos["ops"].sum(axis=0).astype(float)
        out["op_share"] = {k: round(float(v / chunks.sum()), 4) for k, v in zip(("index", "diff", "luma", "run", "rgb", "rgba"), chunks)}
        out["run_pixel_share"] = round(float(infos["run_pixels"].sum()) / float(infos["pixels"].sum()), 4)
        out["inspect_ms"] = timed(lambda: ctx.inspect_streams(packed.data_ptr(), offs, sizes, st))
        out["inspect_GBps"] = round(total / out["inspect_ms"] / 1e6, 1)
        out["hash_streams_ms"] = timed(lambda: ctx.hash_streams(streams.data_ptr(), ss, lens.data_ptr(), n, hashes.data_ptr(), st))
        out["hash_GBps"] = round(total / out["hash_streams_ms"] / 1e6, 1)
        out["inspect_over_hash"] = round(out["inspect_ms"] / out["hash_streams_ms"], 2)
        ctx.set_profiling(True)
        ctx.inspect_streams(packed.data_ptr(), offs, sizes, st)
        prof = ctx.get_profile(st)
        ctx.set_profiling(False)
        out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.items() if k.startswith("inspect_")}
        out["workspace_bytes"] = ctx.workspace_bytes()
        del pixels
        descs = [desc] * n
        decoded = u8(n * ps)
        tight = [i * ps for i in range(n)]
        out["decode_images_ms"] = timed(lambda: ctx.decode_images(packed.data_ptr(), offs, sizes, descs, 4, decoded.data_ptr(), tight, st))
        out["inspect_over_decode"] = round(out["inspect_ms"] / out["decode_images_ms"], 3)
        print(json.dumps(out), flush=True)
        ctx.close()
        del decoded, streams, packed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
