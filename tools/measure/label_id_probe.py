"""24-bit label ids into a pack and back, measured: python tools/measure/label_id_probe.py [--images N] [--reps R] [--out FILE]

N (default 64) int32 instance maps of 1024 x 768 (regions of ids up to 2^24 - 1 with noise where they meet) in one device buffer, into one
pack (align 1, default staging, och 4) and back as N x 224 x 224 int64.  Prints as JSON lines the time of the two routes a caller has:
  (A) ONE qoimi_encode_tiles call whose tiles carry QOIMI_TILE_LABELS | _I32 | _ID24, then ONE qoimi_decode_tensors call with
      QOIMI_FILTER_NEAREST, QOIMI_TENSOR_I64 and QOIMI_TENSOR_HW_ID24;
  (B) the route without them: torch mask / shift / stack to an RGBA copy the caller owns, qoimi_encode_images_packed; then
      qoimi_decode_tensors with QOIMI_FILTER_NEAREST as QOIMI_TENSOR_U8 in QOIMI_TENSOR_HWC and the torch recombination of r, g and b.
The packs (streams, offsets, lengths) and the two results are compared first, bit for bit.  Whole calls are timed with device events, each
leg ending synchronised; the legs are INTERLEAVED in every repetition after a warm-up of all; median of R (default 9) with the best and the
worst beside it.  The comparison base is route (B) on the same build; no threshold is set.  Not measured: the kernels' own time, other
sizes.  Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, OUT = 1024, 768, 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, tensors, tiles
    assert torch.cuda.is_available(), "needs a GPU"
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    n = args.images
    g = torch.Generator(device="cuda").manual_seed(24)
    coarse = torch.randint(0, 1 << 24, (n, H // 32, W // 32), device="cuda", generator=g)
    src = coarse.repeat_interleave(32, dim=1).repeat_interleave(32, dim=2)
    noise = torch.rand((n, H, W), device="cuda", generator=g)
    src = torch.where(noise < 0.02, torch.randint(0, 1 << 24, (n, H, W), device="cuda", generator=g), src).to(torch.int32).contiguous()
    del coarse, noise
    flags = tiles.label_flags(tiles.L_I32, ids=True)
    descs = [api.QoiDesc(W, H, 4, 0)] * n
    ts = [(i, 0, 0, W, H, 1, flags) for i in range(n)]
    items = [(i, 0, 0, W, H, OUT, OUT, 0) for i in range(n)]
    cap = n * tiles.encode_bound(W, H, 4)
    packs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_off = [torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(2)]
    d_len = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    out_a = torch.empty((n, OUT, OUT), dtype=torch.int64, device="cuda")
    out_u8 = torch.empty((n, OUT, OUT, 4), dtype=torch.uint8, device="cuda")
    ctx = api.Context(0)
    state = {}

    def encode_a():
        off, sizes, dd = ctx.encode_tiles(src.data_ptr(), [i * W * H * 4 for i in range(n)], descs, 0, ts, tiles.NEAREST, 1, packs[0].data_ptr(), cap,
                                          d_off[0].data_ptr(), d_len[0].data_ptr())
        state["a"] = ([int(o) for o in off[:n]], [int(s) for s in sizes], dd, int(off[-1]))

    def encode_b():
        rgba = torch.stack([src & 255, (src >> 8) & 255, (src >> 16) & 255, torch.full_like(src, 255)], dim=3).to(torch.uint8).contiguous()
        so, sizes = ctx.encode_images_packed(rgba.data_ptr(), [i * W * H * 4 for i in range(n)], descs, 1, packs[1].data_ptr(), cap, d_off[1].data_ptr(), d_len[1].data_ptr())
        state["b"] = ([int(o) for o in so[:n]], [int(s) for s in sizes], descs, int(so[n]))

    def decode_a():
        so, sizes, dd, _ = state["a"]
        ctx.decode_tensors(packs[0].data_ptr(), so, sizes, dd, 4, items, tensors.FILTER_NEAREST, tensors.PLAIN, tensors.fmt(tensors.I64, tensors.HW_ID24), out_a.data_ptr(),
                           [i * OUT * OUT * 8 for i in range(n)])

    def decode_b():
        so, sizes, dd, _ = state["b"]
        ctx.decode_tensors(packs[1].data_ptr(), so, sizes, dd, 4, items, tensors.FILTER_NEAREST, tensors.PLAIN, tensors.fmt(tensors.U8, tensors.HWC), out_u8.data_ptr(),
                           [i * OUT * OUT * 4 for i in range(n)])
        p = out_u8.to(torch.int64)
        state["out_b"] = p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)

    encode_a(); encode_b(); decode_a(); decode_b()
    torch.cuda.synchronize()
    (so_a, len_a, _, end_a), (so_b, len_b, _, end_b) = state["a"], state["b"]
    assert so_a == so_b and len_a == len_b and end_a == end_b and bool(torch.equal(packs[0][:end_a], packs[1][:end_b])), "the two packs differ"
    assert bool(torch.equal(d_off[0], d_off[1])) and bool(torch.equal(d_len[0], d_len[1])), "the two tables differ"
    assert bool(torch.equal(out_a, state["out_b"])), "the two results differ"
    yy = ((2 * torch.arange(OUT, device="cuda") + 1) * H) // (2 * OUT)
    xx = ((2 * torch.arange(OUT, device="cuda") + 1) * W) // (2 * OUT)
    assert bool(torch.equal(out_a, src[:, yy][:, :, xx].to(torch.int64))), "the result is not the nearest element of the source"
    emit({"maps": n, "width": W, "height": H, "dtype": "int32", "out": [OUT, OUT], "source_bytes": n * W * H * 4, "pack_bytes": end_a, "packs_bit_equal": True,
          "results_bit_equal": True})
    legs = {"encode (A) encode_tiles with QOIMI_TILE_LABELS | _I32 | _ID24": encode_a,
            "encode (B) torch mask/shift/stack to RGBA + encode_images_packed": encode_b,
            "decode (A) decode_tensors NEAREST as I64 HW_ID24": decode_a,
            "decode (B) decode_tensors NEAREST as U8 HWC + torch recombination": decode_b}
    times = {k: [] for k in legs}
    for _ in range(2):                                              # warm-up of every leg
        for fn in legs.values():
            fn(); torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        emit({"leg": k, "reps": args.reps, "median_ms": round(med[k], 3), "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3)})
    ea, eb, da, db = legs.keys()
    emit({"encode_a_over_b": round(med[ea] / med[eb], 3), "decode_a_over_b": round(med[da] / med[db], 3),
          "route_a_ms": round(med[ea] + med[da], 3), "route_b_ms": round(med[eb] + med[db], 3), "route_a_over_b": round((med[ea] + med[da]) / (med[eb] + med[db]), 3)})
    ctx.close()


if __name__ == "__main__":
    main()
