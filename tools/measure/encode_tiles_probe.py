#!/usr/bin/env python
"""qoimi_encode_tiles against the route without it, on one 16384 x 16384 RGBA photo frame cut into 256 x 256 tiles over 4 levels.

    python tools/measure/encode_tiles_probe.py [--side 16384] [--tile 256] [--levels 4] [--reps 5] [--once]

(a) one qoimi_encode_tiles call over qoimi_tile_pyramid; (b) the caller's own torch code - every tile sliced into a tight buffer, levels
made by its own 2 x 2 reductions (a chain of halvings, so its pixels are NOT those of (a) beyond level 1: the times are compared, not the
bytes) - then one qoimi_encode_images_packed call.  Legs interleaved, median of --reps, wall clock around calls that end synchronised.
Prints one JSON line: times, the bytes the gather moves, peak caller-owned device bytes.  --once: leg (a) only, one call (for a kernel trace).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from qoi_amd import api, synth, tiles

    w = h = a.side
    ctx = api.Context(0)
    src = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
    ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 0, 1, w, h, src.data_ptr(), w * h * 4)
    torch.cuda.synchronize()
    desc = api.QoiDesc(w, h, 4, 0)
    pyr = api.tile_pyramid(w, h, 4, a.tile, a.tile, a.levels)
    n = len(pyr)
    sizes = [tiles.size(w, h, 4, t) for t in pyr]
    tile_bytes = sum(s[0] for s in sizes)
    cap = sum(tiles.encode_bound(s[1], s[2], 4) for s in sizes)
    pack = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    # bytes tile_gather reads and writes: level l reads the whole image once and writes 1 / 4^l of it
    moved = a.levels * w * h * 4 + tile_bytes

    def leg_tiles():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        off, lens, _ = ctx.encode_tiles(src.data_ptr(), [0], [desc], 0, pyr, tiles.PLAIN, 1, pack.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())
        return (time.perf_counter() - t0) * 1e3, int(off[-1])

    if a.once:
        ms, total = leg_tiles()
        print(json.dumps({"leg": "encode_tiles once", "ms": round(ms, 3), "pack_bytes": total, "tiles": n, "gather_bytes_moved": moved}))
        ctx.close()
        return 0

    def leg_torch():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        tight = torch.empty(tile_bytes, dtype=torch.uint8, device="cuda")
        level = src.view(h, w, 4)
        at, offs, descs = 0, [], []
        for l in range(a.levels):
            if l:
                lh, lw = level.shape[0] // 2, level.shape[1] // 2                 # (side a power of two: no edge blocks in this probe)
                level = ((level.view(lh, 2, lw, 2, 4).to(torch.int32).sum(dim=(1, 3)) + 2) // 4).to(torch.uint8)
            lh, lw = level.shape[0], level.shape[1]
            for y in range(0, lh, a.tile):
                for x in range(0, lw, a.tile):
                    th, tw = min(a.tile, lh - y), min(a.tile, lw - x)
                    tight[at:at + th * tw * 4].view(th, tw, 4).copy_(level[y:y + th, x:x + tw])
                    offs.append(at); descs.append(api.QoiDesc(tw, th, 4, 0)); at += th * tw * 4
        off, lens = ctx.encode_images_packed(tight.data_ptr(), offs, descs, 1, pack.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr())
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(off[-1]), torch.cuda.max_memory_allocated() - base

    leg_tiles(); leg_torch()                                                       # warm both (arenas, allocator)
    ta, tb, peak_b, pa, pb = [], [], 0, 0, 0
    for _ in range(a.reps):
        ms, pa = leg_tiles(); ta.append(ms)
        ms, pb, peak = leg_torch(); tb.append(ms); peak_b = max(peak_b, peak)
    ws = ctx.workspace_bytes()
    print(json.dumps({
        "image": f"{w}x{h}x4 photo", "tile": a.tile, "levels": a.levels, "tiles": n, "reps": a.reps,
        "encode_tiles_ms": {"median": round(statistics.median(ta), 3), "min": round(min(ta), 3), "max": round(max(ta), 3)},
        "torch_slices_then_encode_images_packed_ms": {"median": round(statistics.median(tb), 3), "min": round(min(tb), 3), "max": round(max(tb), 3)},
        "pack_bytes": {"encode_tiles": pa, "torch_route": pb},
        "gather_bytes_moved": moved,
        "caller_owned_peak_bytes_beyond_source_and_pack": {"encode_tiles": 0, "torch_route": int(peak_b)},
        "context_workspace_bytes": {k: int(v) for k, v in ws.items()},
        "tile_stats": list(ctx.tile_stats()),
    }))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
