"""A label pyramid through qoimi_encode_tiles, measured: python tools/measure/tile_label_probe.py [--side N] [--reps R] [--out FILE]

One label image of N x N x 4 (default 4096: regions of 21 classes with curved borders and one speckle pixel in 200, the image of
tools/measure/mode_probe.py at 4 channels) in device memory, a five-level pyramid of 256 x 256 tiles over it (qoimi_tile_pyramid: 256 + 64 +
16 + 4 + 1 tiles at the default size), align 1, default staging.  Prints as JSON lines the time of ONE qoimi_encode_tiles call in
  (a) QOIMI_THUMB_PLAIN  - the box average, which invents classes: the baseline the other two are read against;
  (b) QOIMI_TILE_NEAREST - the centre pixel of every block;
  (c) QOIMI_TILE_MODE    - the majority vote over every block.
Device events around whole calls, which end synchronised; the legs are INTERLEAVED in every repetition after a warm-up of every leg; median
of R and the best and worst beside it.  The results are compared first, bit for bit: a sample of tiles of every level of every leg, decoded
back with qoimi_decode_images, against qoi_amd/tiles.py: tile.  The legs differ in the gather kernel and in the streams the encoder then
writes (other pixels compress differently), so the difference of two medians is not the kernels' alone.  The kernel's own time, its
occupancy and counters, other sizes, 3-channel and misaligned sources are not measured here.  Needs a GPU; a run without one fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CLASSES = 21
TILE, LEVELS = 256, 5


def label_image(rng, side):
    """uint8[side, side, 4]: a coarse random class map read through a smoothly bent grid, with speckle; the class is the first byte"""
    coarse = rng.integers(0, CLASSES, size=(13, 17))
    yy, xx = np.mgrid[0:side, 0:side]
    bx = xx + 40.0 * np.sin(yy / rng.uniform(40, 90)) + rng.uniform(0, 64)
    by = yy + 40.0 * np.sin(xx / rng.uniform(40, 90)) + rng.uniform(0, 64)
    cls = coarse[(by / 80).astype(int) % 13, (bx / 80).astype(int) % 17]
    speck = rng.random((side, side)) < 0.005
    cls = np.where(speck, rng.integers(0, CLASSES, size=(side, side)), cls).astype(np.int64)
    return np.ascontiguousarray(np.stack([cls, cls * 7, 255 - cls * 11, np.full_like(cls, 255)], axis=2).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, tiles
    assert torch.cuda.is_available(), "needs a GPU"
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    side = args.side
    S = label_image(np.random.default_rng(7), side)
    desc = api.QoiDesc(side, side, 4, 0)
    src = torch.from_numpy(S.reshape(-1)).cuda()
    pyr = api.tile_pyramid(side, side, 4, TILE, TILE, LEVELS)
    ts = [tiles.fields(t) for t in pyr]
    n = len(ts)
    cap = sum(tiles.encode_bound(*tiles.size(side, side, 4, t)[1:], 4) for t in ts)
    pack = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx = api.Context(0)
    modes = {"(a) encode_tiles QOIMI_THUMB_PLAIN": tiles.PLAIN, "(b) encode_tiles QOIMI_TILE_NEAREST": tiles.NEAREST, "(c) encode_tiles QOIMI_TILE_MODE": tiles.MODE}

    def leg(mode):
        return lambda: ctx.encode_tiles(src.data_ptr(), [0], [desc], 0, pyr, mode, 1, pack.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())

    # the results first: tiles of every level, decoded back, against the model
    first = [0] + [int(np.searchsorted([t[5] for t in ts], 1 << l)) for l in range(1, LEVELS)]
    sample = sorted({k + d for k in first for d in (0, 1, 5) if k + d < n} | {n - 1})
    pack_bytes = {}
    for name, mode in modes.items():
        off, sizes, descs = leg(mode)()
        stats = ctx.tile_stats()
        pack_bytes[name] = int(off[-1])
        nbytes = [descs[k].width * descs[k].height * 4 for k in sample]
        out_off = [int(v) for v in np.cumsum([0] + nbytes[:-1])]
        out = torch.empty(sum(nbytes), dtype=torch.uint8, device="cuda")
        ctx.decode_images(pack.data_ptr(), [int(off[k]) for k in sample], [int(sizes[k]) for k in sample], [descs[k] for k in sample], 0, out.data_ptr(), out_off)
        got = out.cpu().numpy()
        for k, o, b in zip(sample, out_off, nbytes):
            want = tiles.tile(S, ts[k], 0, mode)
            assert np.array_equal(got[o:o + b].reshape(want.shape), want), (name, k, ts[k])
    emit({"leg": "encode_tiles label pyramid", "side": side, "tile": TILE, "levels": LEVELS, "tiles": n, "sub_batches": stats[0], "staging_planned_bytes": stats[2],
          "tiles_compared_with_the_model_per_leg": len(sample), "bit_equal_to_the_model": True, "pack_bytes": pack_bytes,
          "work_item_tiles": {"nearest": sum(tiles.select_tiles(t[3], t[4], t[5], 4, tiles.NEAREST) for t in ts),
                              "mode": sum(tiles.select_tiles(t[3], t[4], t[5], 4, tiles.MODE) for t in ts)}})

    legs = {name: leg(mode) for name, mode in modes.items()}
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
        emit({"leg": k, "tiles": n, "reps": args.reps, "median_ms": round(med[k], 3), "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3)})
    a, b, c = (med[k] for k in legs)
    emit({"leg": "the label modes against the box average", "b_over_a": round(b / a, 3), "c_over_a": round(c / a, 3), "c_minus_b_ms": round(c - b, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
