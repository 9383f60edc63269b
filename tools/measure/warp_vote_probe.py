"""The warp with QOIMI_WARP_VOTE2 and QOIMI_WARP_VOTE4 against QOIMI_WARP_NEAREST, measured:
python tools/measure/warp_vote_probe.py [--frames N] [--reps R] [--out FILE]

The workload of tools/measure/warp_super_probe.py for label maps: N label images (default 256, 512 x 512 RGBA: a few classes in regions with
noise where they meet, eight different ones in turn) with ONE item each - a turn by 30 degrees of the whole image into 224 x 224 as I64 HW
(the N x H x W a loss function takes) with REPLICATE; that map reduces by 512 / 224 = 2.29.  A second set of legs has the linear part of
that map scaled by 2.3 about the centre (it reduces by 5.26, and most of the output lies beyond the image, where REPLICATE clamps).  Prints as
JSON lines the time of qoimi_decode_warped_tensors for each map with NEAREST (tensor_warp, as before the flags existed), with VOTE2 and with
VOTE4 (warp_vote_tensor).  Device events around calls that end synchronised; the six legs are INTERLEAVED in every repetition after a
warm-up of every leg; median of R (default 20) with the best and the worst beside it.  The results are compared first: every leg against
qoi_amd/tensors.py: warped_tensors of the pixels for the first item, bit for bit.  A call's time is mostly its decode (all legs decode the
same N images into the staging arena): the difference of two medians is what the kernels differ by, with the noise of both medians.  The
kernel's own time, its occupancy and its counters, other angles and other sizes are not measured here.  Needs a GPU; a run without one
fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, OW, OH = 512, 512, 224, 224
FURTHER = 2.3
CLASSES = 7
DIFFERENT = 8


def label_image(seed):
    """uint8[H, W, 4]: regions of 23 x 17 pixels of one class each (the class in r, alpha 255), a band of two-class noise, noise of three
    classes in every ninth column"""
    rng = np.random.default_rng(seed)
    grid = rng.integers(0, CLASSES, size=(-(-H // 17), -(-W // 23)))
    idx = np.repeat(np.repeat(grid, 17, axis=0), 23, axis=1)[:H, :W].copy()
    salt = rng.integers(0, 3, size=(H, W))
    idx[:, ::9] = salt[:, ::9]
    idx[H // 2:H // 2 + 40] = 3 + salt[H // 2:H // 2 + 40] % 2
    D = np.zeros((H, W, 4), dtype=np.uint8)
    D[:, :, 0] = idx
    D[:, :, 3] = 255
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from qoi_amd import api, resize, tensors, warp
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
    kinds = [label_image(50 + k) for k in range(min(DIFFERENT, n))]
    pixels = torch.from_numpy(np.stack([kinds[i % len(kinds)] for i in range(n)]).reshape(-1)).cuda()
    ctx = api.Context(0)
    cap = n * api.encode_bound(W, H, 4)
    packed = u8(cap + 256)
    off, lens = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_images_packed(pixels.data_ptr(), po, descs, 1, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 0, st)
    so, sizes = [int(x) for x in so[:n]], [int(x) for x in sizes]
    maps = {"reduces 2.29": warp.rotation((W, H), (OW, OH), 30.0, OW / W), "reduces 5.26": warp.rotation((W, H), (OW, OH), 30.0, OW / W / FURTHER)}
    samplings = {"nearest": warp.NEAREST, "vote2": warp.VOTE2, "vote4": warp.VOTE4}
    warped = {(m, s): [warp.item(i, (0, 0, W, H), (OW, OH), maps[m], warp.REPLICATE | samplings[s]) for i in range(n)] for m in maps for s in samplings}
    fmt = tensors.fmt(tensors.I64, tensors.HW)
    out_t = torch.empty((n, OH, OW), dtype=torch.int64, device="cuda")
    t_off = [i * OW * OH * 8 for i in range(n)]

    def turned(key):
        ctx.decode_warped_tensors(packed.data_ptr(), so, sizes, descs, 4, warped[key], resize.PLAIN, fmt, out_t.data_ptr(), t_off, 0, st)

    # the results first
    changed = {}
    for m in maps:
        for s in samplings:
            turned((m, s)); torch.cuda.synchronize()
            got = out_t[0].cpu().numpy()
            want = tensors.warped_tensors(kinds[0], (0, 0, W, H), (OW, OH), maps[m], warp.REPLICATE | samplings[s], 0, resize.PLAIN, fmt)
            assert np.array_equal(got.reshape(-1), np.asarray(want).view(np.int64).reshape(-1)), (m, s)
            changed[(m, s)] = got.copy()
    stats = ctx.tensor_stats()
    emit({"leg": "decode_warped_tensors with NEAREST, VOTE2, VOTE4", "staging_planned_bytes": stats[2], "sub_batches": stats[0], "images": stats[3],
          "source_pixels": n * W * H, "output_pixels": n * OW * OH, "bit_equal_to_the_model": True})
    for m in maps:
        for s in ("vote2", "vote4"):
            emit({"leg": "%s, %s" % (m, s), "labels_of_item_0_that_differ_from_nearest": int((changed[(m, s)] != changed[(m, "nearest")]).sum()), "of": OW * OH})

    legs = {"%s, %s" % key: (lambda key=key: turned(key)) for key in warped}
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
        emit({"leg": "decode_warped_tensors 30 degrees replicate, %s -> i64 HW 224x224" % k, "images": n, "reps": args.reps, "median_ms": round(med[k], 3),
              "best_ms": round(min(v), 3), "worst_ms": round(max(v), 3)})
    for m in maps:
        for s in ("vote2", "vote4"):
            emit({"leg": "%s, %s" % (m, s), "over_nearest_ms": round(med["%s, %s" % (m, s)] - med[m + ", nearest"], 3),
                  "times_nearest": round(med["%s, %s" % (m, s)] / med[m + ", nearest"], 3)})
    ctx.close()


if __name__ == "__main__":
    main()
