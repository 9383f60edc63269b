"""decode_crops, measured: python tools/measure/crop_probe.py [--frames N] [--reps R] [--out FILE] [--only-crops]

For N 4K photographs (default 64, 3840 x 2160 RGBA) with ONE 256 x 256 crop each prints as JSON lines
  * the time of qoimi_decode_crops with every crop in the top 256 rows (a), with every crop in the bottom 256 rows (b), and of what a caller had
    before this call existed: qoimi_decode_images of the N whole images into memory the caller owns, with no cutting at all.  Device events
    around calls that end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median of R and the best
    beside it.
  * the gather step: the decode sub-call of (a) and of (b) - qoimi_decode_images at 4 channels with the shortened descriptors, into a buffer of
    the probe - is timed as a leg of its own; the call's median minus that leg's median is what the table copy and the launch of crop_gather
    add.  A difference of two medians carries the noise of both; the kernel's own time is what a kernel trace of a --only-crops run shows.
  * qoimi_workspace_bytes [1] of a fresh context after (a) and of another after (b), against the N x 33 MB the caller of the whole-image
    decode owns, and the staging each call planned (qoimi_crop_stats [2]).
  * the result is compared first: every crop equals the rectangle of the whole-image decode.
Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, T = 3840, 2160, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-crops", action="store_true", help="time the two decode_crops legs alone (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, crops, synth
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
    rng = np.random.default_rng(7)
    xs = [int(x) for x in rng.integers(0, W - T + 1, size=n)]
    top = [(i, xs[i], 0, T, T, i & 1) for i in range(n)]
    bottom = [(i, xs[i], H - T, T, T, i & 1) for i in range(n)]
    oo = [i * T * T * 4 for i in range(n)]
    out_top, out_bottom = u8(n * T * T * 4), u8(n * T * T * 4)

    def full_decode():
        ctx.decode_images(packed.data_ptr(), so, sizes, descs, 4, pixels.data_ptr(), po, st)

    # the result first, and the arenas of a fresh context per leg
    full_decode()
    torch.cuda.synchronize()
    whole = pixels.view(n, H, W, 4)
    for name, cs, dst in (("top", top, out_top), ("bottom", bottom, out_bottom)):
        fresh = api.Context(0)
        fresh.decode_crops(packed.data_ptr(), so, sizes, descs, 4, cs, dst.data_ptr(), oo, 0, st)
        got = dst.view(n, T, T, 4)
        for (i, x, y, _, _, flags) in cs:
            want = whole[i, y:y + T, x:x + T]
            assert bool(torch.equal(got[i], want.flip(1) if flags & crops.FLIP_X else want)), (name, i)
        stats = fresh.crop_stats()
        emit({"leg": "decode_crops " + name, "workspace_decode_bytes": fresh.workspace_bytes()["decode"], "staging_planned_bytes": stats[2],
              "sub_batches": stats[0], "caller_owned_bytes_of_the_whole_decode": n * image})
        fresh.close()

    def short_descs(cs):
        rows = crops.rows_needed(descs, cs)
        ds = [api.QoiDesc(W, rows[i], 4, 0) for i in range(n)]
        return ds, [i * W * rows[0] * 4 for i in range(n)]

    ds_top, po_top = short_descs(top)
    ds_bottom, po_bottom = short_descs(bottom)
    legs = {"decode_crops top": lambda: ctx.decode_crops(packed.data_ptr(), so, sizes, descs, 4, top, out_top.data_ptr(), oo, 0, st),
            "decode_crops bottom": lambda: ctx.decode_crops(packed.data_ptr(), so, sizes, descs, 4, bottom, out_bottom.data_ptr(), oo, 0, st)}
    if not args.only_crops:
        legs["decode_images whole"] = full_decode
        legs["decode sub-call top"] = lambda: ctx.decode_images(packed.data_ptr(), so, sizes, ds_top, 4, pixels.data_ptr(), po_top, st)
        legs["decode sub-call bottom"] = lambda: ctx.decode_images(packed.data_ptr(), so, sizes, ds_bottom, 4, pixels.data_ptr(), po_bottom, st)
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
    if not args.only_crops:
        for name in ("top", "bottom"):
            call, sub = med["decode_crops " + name], med["decode sub-call " + name]
            emit({"leg": "gather step " + name, "call_minus_decode_sub_call_ms": round(call - sub, 3), "share_of_call": round((call - sub) / call, 4),
                  "ratio_to_whole_decode": round(call / med["decode_images whole"], 3)})
    ctx.close()


if __name__ == "__main__":
    main()
