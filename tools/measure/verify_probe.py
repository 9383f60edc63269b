"""verify_images, measured: python tools/measure/verify_probe.py [--frames N] [--reps R] [--out FILE]

For a pack of N 4K photographs (qoimi_encode_packed) prints as JSON lines, and appends to FILE (default profiles/verify_probe.txt):
  * qoimi_verify_images at three staging sizes (256 MiB, 1 GiB, everything in one sub-batch) and a plain qoimi_decode_images of the same
    pack into a full-size buffer ON THE SAME CONTEXT, all legs INTERLEAVED in every repetition after a warm-up of every leg, median and
    minimum of R, host clock around calls that return synchronised; every verify leg's ratio to the plain decode
  * cmp_pixels alone from the kernel timer (a separate, profiled call per staging size): milliseconds, launches, and its bytes per second
    over the 8 bytes per pixel the comparison reads, against the 6.3 TB/s a streaming kernel achieves on an MI355X
  * device bytes the context holds for the decode workspace, the tables and the staging
The result first: every verify call must report a clean pack, and a planted difference must be found where it was planted."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ACHIEVABLE_COPY_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_probe.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, synth
    from qoi_amd.packplan import plan, slot
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.current_stream().cuda_stream
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n"); sink.flush()

    n, w, h = args.frames, 3840, 2160
    npx, ps = w * h, w * h * 4
    desc = api.QoiDesc(w, h, 4, 0)
    descs = [desc] * n
    po = [i * ps for i in range(n)]
    pixels = u8(n * ps)
    c = api.Context(0)
    for lo in range(0, n, 64):
        c.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, lo, min(64, n - lo), w, h, pixels.data_ptr() + lo * ps, ps, st)
    off, lens = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    so, sizes = c.encode_packed(pixels.data_ptr(), ps, desc, n, 1, 0, 0, off.data_ptr(), lens.data_ptr(), 1 << 30, st)
    total = int(so[-1])
    packed = u8(total + 256)
    so, sizes = c.encode_packed(pixels.data_ptr(), ps, desc, n, 1, packed.data_ptr(), total, off.data_ptr(), lens.data_ptr(), 1 << 30, st)
    so, sizes = [int(x) for x in so[:n]], [int(x) for x in sizes]
    out = u8(n * ps)
    one = slot(ps)
    settings = [("256MiB", 256 << 20), ("1GiB", 1 << 30), ("one sub-batch", n * one)]
    legs = {"decode_images": lambda: c.decode_images(packed.data_ptr(), so, sizes, descs, 4, out.data_ptr(), po, st)}
    for label, staging in settings:
        legs[label] = (lambda s: lambda: c.verify_images(pixels.data_ptr(), po, descs, packed.data_ptr(), so, sizes, s, st))(staging)
    # the result first
    for label, _ in settings:
        diffs, first = legs[label]()
        assert first == -1 and not diffs["flags"].any(), label
    victim, where = n // 2, npx - 5
    pixels[victim * ps + where * 4 + 1] ^= 0x20
    diffs, first = legs["256MiB"]()
    assert first == victim and int(diffs["mismatched"][victim]) == 1 and int(diffs["first"][victim]) == where and int(diffs["flags"].astype(bool).sum()) == 1
    pixels[victim * ps + where * 4 + 1] ^= 0x20
    legs["decode_images"]()
    assert bool(torch.equal(out, pixels)), "the plain decode does not give the pixels back"
    times = {k: [] for k in legs}
    for fn in legs.values():                                   # warm-up of every leg (the arenas reach their final size here)
        fn(); torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    emit({"workload": f"{n} x {w}x{h} photo", "leg": "decode_images", "ms": round(med["decode_images"], 3), "min_ms": round(min(times["decode_images"]), 3),
          "reps": args.reps, "stream_bytes": total, "pixel_bytes": n * ps})
    for label, staging in settings:
        c.set_profiling(True)
        legs[label]()
        prof = c.get_profile(st)
        c.set_profiling(False)
        cmp_ms, cmp_calls = prof["cmp_pixels"]
        rate = 8.0 * npx * n / (cmp_ms * 1e-3) if cmp_ms > 0 else 0.0
        emit({"workload": f"{n} x {w}x{h} photo", "leg": "verify_images", "staging": label, "staging_bytes": staging,
              "sub_batches": len(plan([ps] * n, staging)), "ms": round(med[label], 3), "min_ms": round(min(times[label]), 3),
              "ratio_to_decode_images": round(med[label] / med["decode_images"], 3),
              "cmp_pixels_ms": round(cmp_ms, 3), "cmp_pixels_launches": int(cmp_calls), "cmp_first_ms": round(prof["cmp_first"][0], 3),
              "cmp_pixels_bytes_per_s": round(rate, 0), "cmp_pixels_share_of_achievable_copy": round(rate / ACHIEVABLE_COPY_BYTES_PER_S, 3),
              "kernel_ms": {k: round(v[0], 3) for k, v in prof.items() if v[1] and v[0] > 0.005}})
    emit({"workload": f"{n} x {w}x{h} photo", "leg": "memory", "decode_arenas": c.workspace_bytes()["decode"], "full_size_buffer_avoided": n * ps})
    c.close()


if __name__ == "__main__":
    main()
