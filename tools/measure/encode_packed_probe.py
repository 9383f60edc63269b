"""encode_packed, measured: python tools/measure/encode_packed_probe.py [--frames N] [--reps R] [--out FILE] [--other-lib PATH]

For N 4K photographs (equal shapes, qoimi_encode_packed) and for the mixed directory of bench.py (288 images, qoimi_encode_images_packed)
prints as JSON lines, per staging_bytes setting (64 MiB, 256 MiB, 1 GiB, 4 GiB, everything in one sub-batch):
  * the call's time and its ratio to the two-call path (encode_batch / encode_images into worst-case strides + encode_status + pack_streams
    + the two tables copied to the host) - all settings and the two-call path INTERLEAVED in every repetition, median of R, host clock
    around calls that end synchronised
  * sub-batches, per-kernel milliseconds of one call from the kernel timer (a separate, profiled call)
  * device bytes held for streams: the context's encode arenas (workspace + staging) + the pack, against workspace + n strides + the pack
--other-lib: a second build of the library (e.g. the parent commit's); its two-call path and its pack_streams are timed in the same
repetitions, for an A/B of the calls this feature shares code with."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--other-lib", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, synth
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

    def other_context():
        """a context of the other build: the prototypes of the symbols it has are taken from this build's binding"""
        import ctypes
        main, lib = api.load_library(), ctypes.CDLL(os.path.abspath(args.other_lib))
        for name in api.EXPORTS:
            try:
                f = getattr(lib, name)
            except AttributeError:
                continue
            f.restype, f.argtypes = getattr(main, name).restype, getattr(main, name).argtypes
        c = api.Context.__new__(api.Context)
        c._lib, c._h, c.device = lib, ctypes.c_void_p(), 0
        assert lib.qoimi_ctx_create(0, ctypes.byref(c._h)) == 0
        return c

    def workload(name, shapes, kinds, frame0, equal):
        n = len(shapes)
        descs = [api.QoiDesc(w, h, 4, 0) for (w, h) in shapes]
        bounds = [api.encode_bound(w, h, 4) for (w, h) in shapes]
        px_bytes = [w * h * 4 for (w, h) in shapes]
        ps = (max(px_bytes) + 255) // 256 * 256
        po = [i * ps for i in range(n)] if equal else [int(x) for x in np.cumsum([0] + [(b + 255) // 256 * 256 for b in px_bytes[:-1]])]
        ss = slot(max(bounds))
        pixels = u8(po[-1] + ps)
        gen = api.Context(0)
        for i, ((w, h), kind) in enumerate(zip(shapes, kinds)):
            gen.synth_frames(synth.KIND_ID[kind], synth.DEFAULT_SEED, frame0 + i, 1, w, h, pixels.data_ptr() + po[i], w * h * 4, st)
        torch.cuda.synchronize()
        gen.close()
        streams = u8(n * ss)
        lens, off = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        lens2, off2 = torch.zeros_like(lens), torch.zeros_like(off)

        def two_calls(c, packed, cap):
            if equal:
                c.encode_batch(pixels.data_ptr(), ps, descs[0], n, streams.data_ptr(), ss, lens.data_ptr(), st)
            else:
                c.encode_images(pixels.data_ptr(), po, descs, streams.data_ptr(), [i * ss for i in range(n)], lens.data_ptr(), st)
            c.encode_status(st)
            c.pack_streams(streams.data_ptr(), ss, lens.data_ptr(), n, 1, packed, cap, off.data_ptr(), st)
            return off.cpu().numpy(), lens.cpu().numpy()

        def one_call(c, staging, packed, cap):
            if equal:
                return c.encode_packed(pixels.data_ptr(), ps, descs[0], n, 1, packed, cap, off2.data_ptr(), lens2.data_ptr(), staging, st)
            return c.encode_images_packed(pixels.data_ptr(), po, descs, 1, packed, cap, off2.data_ptr(), lens2.data_ptr(), staging, st)

        ref_ctx = api.Context(0)
        want_off, want_len = two_calls(ref_ctx, 0, 0)
        total = int(want_off[-1])
        packed_a, packed_b = u8(total + 256), u8(total + 256)
        two_calls(ref_ctx, packed_a.data_ptr(), total)
        settings = [("64MiB", 64 << 20), ("256MiB", 256 << 20), ("1GiB", 1 << 30), ("4GiB", 4 << 30), ("one sub-batch", sum(slot(b) for b in bounds))]
        ctxs = {label: api.Context(0) for label, _ in settings}
        legs = {"two_calls": lambda: two_calls(ref_ctx, packed_a.data_ptr(), total)}
        for label, staging in settings:
            legs[label] = (lambda c, s: lambda: one_call(c, s, packed_b.data_ptr(), total))(ctxs[label], staging)
        other = other_context() if args.other_lib else None
        if other:
            legs["other_lib_two_calls"] = lambda: two_calls(other, packed_a.data_ptr(), total)
            legs["pack_streams"] = lambda: ref_ctx.pack_streams(streams.data_ptr(), ss, lens.data_ptr(), n, 1, packed_a.data_ptr(), total, off.data_ptr(), st)
            legs["other_lib_pack_streams"] = lambda: other.pack_streams(streams.data_ptr(), ss, lens.data_ptr(), n, 1, packed_a.data_ptr(), total, off.data_ptr(), st)
        for label, staging in settings:                        # the result first: the same pack, the same tables
            packed_b.fill_(0)
            got_off, got_len = one_call(ctxs[label], staging, packed_b.data_ptr(), total)
            assert np.array_equal(got_off, want_off.astype(np.uint64)) and np.array_equal(got_len, want_len), label
            assert bool(torch.equal(packed_a[:total], packed_b[:total])), label
        times = {k: [] for k in legs}
        for k, fn in legs.items():                             # warm-up of every leg
            fn(); torch.cuda.synchronize()
        for _ in range(args.reps):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        base_ws = ref_ctx.workspace_bytes()["encode"]
        emit({"workload": name, "leg": "two_calls", "ms": round(med["two_calls"], 3), "min_ms": round(min(times["two_calls"]), 3),
              "stream_bytes_held": base_ws + n * ss + total, "strided_bytes": n * ss, "pack_bytes": total, "encode_workspace": base_ws})
        for k in ("other_lib_two_calls", "pack_streams", "other_lib_pack_streams"):
            if k in med:
                emit({"workload": name, "leg": k, "ms": round(med[k], 4), "min_ms": round(min(times[k]), 4)})
        for label, staging in settings:
            c = ctxs[label]
            c.set_profiling(True)
            legs[label]()
            prof = {k: round(v[0], 3) for k, v in c.get_profile(st).items() if v[1] and v[0] > 0.005}
            c.set_profiling(False)
            held = c.workspace_bytes()["encode"]
            emit({"workload": name, "leg": "encode_packed", "staging": label, "staging_bytes": staging, "sub_batches": len(plan(bounds, staging)),
                  "ms": round(med[label], 3), "min_ms": round(min(times[label]), 3), "ratio_to_two_calls": round(med[label] / med["two_calls"], 3),
                  "stream_bytes_held": held + total, "encode_arenas": held, "kernel_ms": prof})
        for c in list(ctxs.values()) + [ref_ctx] + ([other] if other else []):
            c.close()

    workload(f"{args.frames} x 3840x2160 photo", [(3840, 2160)] * args.frames, ["photo"] * args.frames, 0, True)
    rng = np.random.default_rng(2026)                           # the item list of bench.py's mixed_directory leg
    kinds = ["photo", "noise", "uiflat", "constant", "photo_hard", "sprite_alpha"]
    shapes = set()
    while len(shapes) < 64:
        shapes.add((int(rng.integers(48, 2049)), int(rng.integers(48, 1537))))
    shapes = sorted(shapes)
    workload("mixed directory, 288 images", [shapes[(i * 7) % len(shapes)] for i in range(288)], [kinds[i % len(kinds)] for i in range(288)], 40000, False)


if __name__ == "__main__":
    main()
