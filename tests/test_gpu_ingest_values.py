"""The conversion of tensor sources as the DEVICE compiles it (-m gpu): qoi_ingest_core.h has a body of its own under __HIP_DEVICE_COMPILE__
for ingest_widen (a _Float16 cast), another way of keeping the multiply and the add of SYMMETRIC apart (a pragma), and v_rndne_f32 for the
rounding; tests/test_ingest_core_host.py holds the host build to every binary16 and bfloat16 pattern and a binary32 set, and this file
holds the kernel tensor_ingest to the same: all 65536 patterns of f16 and of bf16 as a 128 x 128 x 4 image, and the binary32 set of
tests/ingest_cases.py - ties, clamps, specials, random patterns, and the witnesses whose byte differs between two roundings and a fused
multiply-add - as an 80-wide image, in every range, HWC and CHW, each once at a 256-aligned address (the 8- and 16-byte loads of
ingest_load_run, for a CHW run and for a four-element HWC pixel) and once one element behind a 16-byte boundary (the element loads).
Tiles: the whole image unflipped and flipped in x, rectangles at x = 1 three pixels narrower whose items cross rows and whose last item
holds 3, 2 and 1 pixels; output channels 4 and 3.  Every expectation is qoi_amd/tiles.py: convert and tile, then the reference encoder's
stream, byte for byte (tests/test_gpu_encode_tiles.py: run).  What the expectation must contain for the comparison to mean something is
asserted before any GPU work (`conditions`); tests/test_ingest_paths.py asserts the same without a GPU."""
import numpy as np
import pytest

import ingest_cases
from qoi_amd import tiles
from gpu_calls import Tensors, conditions, ingest_model as model, run_tiles as run
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=ingest_cases.FLOATS, ids=["f16", "bf16", "f32"])
def values(request, api):
    dtype = request.param
    specs, hows = ingest_cases.value_specs(dtype)
    ts = ingest_cases.value_tiles(specs)
    src = Tensors(api, specs, seed=11, how=hows)
    assert [o % 256 == 0 for o in src.off] == [h == ingest_cases.ALIGNED for h in hows]
    assert all(o % 16 == tiles.ELEM[dtype] for o, h in zip(src.off, hows) if h == ingest_cases.ONE)
    conditions(dtype, specs, ts, src.bytes)
    return src, ts


@pytest.mark.parametrize("channels", ingest_cases.VALUE_CHANNELS)
def test_every_pattern_on_the_device(ctx, oracle, values, channels):
    src, ts = values
    before = src.host.copy()
    px, streams = model(oracle, src, ts, channels)
    run(ctx, src, ts, channels, tiles.PLAIN, 1, streams, shift=channels)
    assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == len(src.descs)
    assert np.array_equal(src.d.cpu().numpy(), before)                 # the source is only read
