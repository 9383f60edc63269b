"""qoimi_pixel_stats on the GPU (-m gpu) where a workgroup's share of one region passes 2^32: one all-white 4-channel square, encoded by the
oracle into a few MB of run chunks and staged whole.

The arithmetic.  255^2 * n passes 2^32 at n = 66 052.  run_staged launches min(tiles, 8 * compute units) workgroups, each takes
ceil(tiles / workgroups) tiles of TILE_PX pixels; the side is the smallest for which that share exceeds 66 052 pixels.  With 256 compute units
and TILE_PX 1024: 2048 workgroups, a share of 65 tiles = 66 560 pixels needs more than 64 * 2048 tiles = 134 217 728 pixels: a side of 11 586,
537 MB of staging.  A reduction that carried anything above the lane in 32 bits would lose the high half of that workgroup's square sums."""
import numpy as np
import pytest

from qoi_amd import pixelstats as ps
from gpu_pack import GUARD, dev, filled

pytestmark = pytest.mark.gpu
T = ps.TILE_PX
EDGE = 66052


def share(side, cus):
    tiles = ps.tiles(side, side)
    return -(-tiles // min(tiles, 8 * cus)) * T


def test_a_workgroups_share_passes_32_bits(ref, port):
    import torch
    from qoi_amd import api
    oracle = ref or port
    assert 65025 * EDGE > 2 ** 32 > 65025 * (EDGE - 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    side = next(s for s in range(1, 16385) if share(s, cus) > EDGE)
    assert share(side - 1, cus) <= EDGE < share(side, cus) and side * side < 400000000
    n = side * side
    print("compute units", cus, "side", side, "tiles", ps.tiles(side, side), "pixels per workgroup", share(side, cus))
    white = np.full(n * 4, 255, dtype=np.uint8)
    stream = oracle.encode(white, side, side, 4)
    assert len(stream) < 8 << 20
    decoded, _ = oracle.decode(stream, 4)
    assert decoded.size == n * 4 and int(decoded.min()) == 255          # the oracle's decode: all white
    del white, decoded
    packed = dev(np.frombuffer(stream, dtype=np.uint8).copy())
    ctx = api.Context(0)
    try:
        descs, half = [api.QoiDesc(side, side, 4, 0)], side // 2
        whole = [(0, 0, 0, side, side, 0)]
        quads = [(0, 0, 0, half, half, 1), (0, half, 0, side - half, half, 2), (0, 0, half, half, side - half, 3), (0, half, half, side - half, side - half, 0)]
        results = []
        for regions in (whole, quads):
            buf = filled(64 + len(regions) * 4096 + 64, GUARD)
            got = [ps.of_struct(s) for s in ctx.pixel_stats(packed.data_ptr(), [0], [len(stream)], descs, regions, buf.data_ptr() + 64)]
            assert ctx.pixel_stats_counters() == (1, 1, (n * 4 + 255) // 256 * 256, 1)
            host = buf.cpu().numpy()
            assert np.all(host[:64] == GUARD) and np.all(host[-64:] == GUARD)
            results.append((got, host[64:-64].view(np.uint32).reshape(len(regions), 4, 256)))
        (w,), hw = results[0]
        assert w["pixels"] == n and w["sum"] == (255 * n,) * 4 and w["sum_sq"] == (65025 * n,) * 4
        assert w["opaque_pixels"] == n and w["grey_pixels"] == n and w["transparent_pixels"] == 0
        assert w["min"] == w["max"] == (255,) * 4 and w["first"] == 0xFFFFFFFF and w["flags"] == ps.CONSTANT | ps.OPAQUE | ps.GREY
        assert np.all(hw[0, :, 255] == n) and int(hw.astype(np.uint64).sum()) == 4 * n
        q, hq = results[1]
        assert sum(g["pixels"] for g in q) == n and all(g["flags"] == w["flags"] and g["first"] == 0xFFFFFFFF for g in q)
        for key in ("sum", "sum_sq"):
            assert tuple(sum(g[key][c] for g in q) for c in range(4)) == w[key]
        assert sum(g["opaque_pixels"] for g in q) == n and all(g["sum_sq"][0] == 65025 * g["pixels"] for g in q)
        assert np.array_equal(hq.astype(np.uint64).sum(axis=0), hw[0].astype(np.uint64))
    finally:
        ctx.close()
