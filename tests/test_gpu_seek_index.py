"""qoimi_build_seek_index on the GPU (-m gpu): the points of every stream of tests/seek_cases.py equal qoi_amd/seekindex.py: points over the
oracle's decode, field for field - points in different 16 KiB blocks, 4 KiB tiles and 64-byte pieces, inside runs (skip 1, 61, at a block
edge), in a body of 0xFF bytes, behind the end of a cut stream, colours last seen many intervals back, slots never written, widths 1 and 63 to
65, 3- and 4-channel streams in one call, an image without a point.  Sub-batches are forced through staging_bytes."""
import ctypes

import numpy as np
import pytest

from qoi_amd import packplan
from qoi_amd import seekindex as si
from seek_cases import DevicePack, cases
from gpu_pack import E_ARG
from gpu_pack import api, ctx  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pack(api, ref, port):
    return DevicePack(api, cases(ref or port))


def assert_points(pack, got, firsts):
    assert firsts == pack.point_firsts and got.size == pack.points.size
    for c, first in zip(pack.cases, firsts):
        mine = got[first:first + len(c.points)]
        for field in ("byte_off", "skip", "prev", "reserved", "table"):
            bad = np.flatnonzero([not np.array_equal(a[field], b[field]) for a, b in zip(mine, c.points)])
            assert bad.size == 0, (c.name, field, int(bad[0]), mine[int(bad[0])][field], c.points[int(bad[0])][field])


def plan_of(pack, staging):
    with_points = [c for c in pack.cases if len(c.points)]
    return packplan.plan([c.w * c.h * 4 for c in with_points], staging)


def test_points_equal_the_model(ctx, pack):
    got, firsts = ctx.build_seek_index(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, pack.intervals)
    assert_points(pack, got, firsts)
    assert ctx.seek_stats()[0] == 1 == len(plan_of(pack, 1 << 30))
    assert np.array_equal(pack.dev.cpu().numpy(), pack.host)


@pytest.mark.parametrize("staging", [1, 4200000, 8200000])
def test_sub_batches(api, pack, staging):
    c = api.Context(0)
    try:
        subs = plan_of(pack, staging)
        assert len(subs) > 1
        got, firsts = c.build_seek_index(pack.dev.data_ptr(), pack.offsets, pack.sizes, pack.descs, pack.intervals, staging_bytes=staging)
        assert_points(pack, got, firsts)
        assert c.seek_stats()[0] == len(subs), (c.seek_stats(), subs)
    finally:
        c.close()


def test_one_image_and_an_image_without_points(ctx, pack):
    i = [c.name for c in pack.cases].index("no_point")
    got, firsts = ctx.build_seek_index(pack.dev.data_ptr(), pack.offsets[i:i + 1], pack.sizes[i:i + 1], pack.descs[i:i + 1], pack.intervals[i:i + 1])
    assert got.size == 0 and firsts == [0] and ctx.seek_stats()[0] == 0
    j = [c.name for c in pack.cases].index("all_ff")
    got, _ = ctx.build_seek_index(pack.dev.data_ptr(), [pack.offsets[j]], [pack.sizes[j]], [pack.descs[j]], [pack.intervals[j]])
    assert np.array_equal(got, pack.cases[j].points)
    # another interval for the same stream: the points of that interval
    c = pack.cases[0]
    got, _ = ctx.build_seek_index(pack.dev.data_ptr(), [pack.offsets[0]], [pack.sizes[0]], [pack.descs[0]], [7])
    assert np.array_equal(got, si.points(c.stream, c.w, c.h, 7, c.full[4])) and got.size == 13


def test_rejections_on_a_live_context(api, ctx, pack):
    lib = api.load_library()
    n = len(pack.cases)
    out = (api.QoimiSeekPoint * pack.points.size)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    before = bytes(out)

    def call(sizes=pack.sizes, descs=pack.descs, ks=pack.intervals, n_=n, points=out):
        return lib.qoimi_build_seek_index(ctx._h, pack.dev.data_ptr(), (ctypes.c_size_t * n)(*pack.offsets), (ctypes.c_int * n)(*sizes), (api.QoiDesc * n)(*descs),
                                          n_, (ctypes.c_uint * n)(*ks), points, 0, None)

    assert call(sizes=[21] + pack.sizes[1:]) == E_ARG and "22" in api.last_error()
    assert call(descs=[api.QoiDesc(96, 96, 5, 0)] + pack.descs[1:]) == E_ARG
    assert call(ks=[1] + pack.intervals[1:]) == E_ARG and "128" in api.last_error()       # 1 * 96 < 128
    assert call(ks=[0] + pack.intervals[1:]) == E_ARG
    assert call(n_=0) == E_ARG and call(points=None) == E_ARG
    assert bytes(out) == before
