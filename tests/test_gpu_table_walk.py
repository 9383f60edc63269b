"""The tile walk of tensor_cubic and tensor_lanczos on the GPU (-m gpu): one call of qoimi_decode_tensors whose tiles outnumber the launch's
workgroups (eight per compute unit) by more than two to one, so that every workgroup runs three tiles one behind the other over the same two
LDS tables (qoi_table_tiles.h: table_tile_run - the barrier in front of the normalisation is there for the tile before) - tiles of different
items, lane counts and table strides (tests/table_tiles.py: items; tests/test_table_walk.py shows from the models that the tables of two
tiles a workgroup runs back to back always differ, that a workgroup begins inside an item and that workgroups step from item to item).  Every
output is compared bit for bit, over its whole length, with the definition - the oracle decodes the stream at the call's output channel count,
qoi_amd/bicubic.py or lanczos.py resamples that, qoi_amd/tensors.py: convert makes the tensor; each of the few distinct items is computed
once - and every guard byte between and around the outputs is checked (gpu_calls.py: tensor_layout, run_tensors)."""
import numpy as np
import pytest

import table_tiles as tt
from qoi_amd import tensors
from qoi_amd.tensors import ALPHA_WEIGHTED, CHW, F16, FILTER_BICUBIC, FILTER_LANCZOS, HWC, PLAIN, U8
from gpu_calls import run_tensors as run
from gpu_pack import IMAGENET, Pack, batch_of
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    return Pack(ctx, oracle, batch_of(api, oracle, tt.SHAPES, tt.pixels()))


_WANT = {}


def want(p, filt, it, och, mode, f, name):
    """the bytes of one item's tensor: the model and its conversion computed once per distinct item, never changed"""
    key = (filt, it, och, mode, name)
    if key not in _WANT:
        i, x, y, cw, rh, ow, oh, flags = it
        resample = tt.MODELS[filt].bicubic if filt == FILTER_BICUBIC else tt.MODELS[filt].lanczos
        w = tensors.convert(resample(p.decoded(i, och), (x, y, cw, rh), (ow, oh), flags, mode), f).view(np.uint8).reshape(-1)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


@pytest.mark.parametrize("filt", [FILTER_BICUBIC, FILTER_LANCZOS])
def test_a_workgroup_runs_three_tiles(ctx, pack, filt):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    call = tt.items(filt, cus)
    tiles, grid, per_wg, _ = tt.walk(filt, call, cus)
    assert 8 * cus < tiles and grid == 8 * cus and per_wg == 3
    for channels, mode in ((4, ALPHA_WEIGHTED), (3, PLAIN)):
        for name, f in (("f16 chw", (F16, CHW, *IMAGENET)), ("u8 hwc", tensors.fmt(U8, HWC))):
            got = run(ctx, pack, filt, channels, call, mode, f)
            assert ctx.tensor_stats()[:2] == (1, 1) and ctx.tensor_stats()[3] == 2          # one sub-batch, one launch: the walk is one launch
            for j, it in enumerate(call):
                w = want(pack, filt, it, channels, mode, f, name)
                assert got[j].size == w.size and np.array_equal(got[j], w), (name, channels, mode, j, it, int(np.argmax(got[j] != w)) // tensors.ELEM[f[0]])
