"""The fold of a tap index on the device over its whole accepted range (-m gpu), and without a GPU the conditions that keep that from passing
vacuously.  warp_fold_position (qoi_warp_border_core.h) brings a far index into [-P, 2P) with a quotient estimate in double precision and
finishes with a conditional add or subtract; on the host it is walked as g++ compiles it, on the device it is clang's code for gfx950 with
its own division expansion and contraction rules.  tests/warp_fold_cases.py builds the sweep: source images that hold their own pixel index,
items of 16 x 1 or 1 x 16 output pixels whose first tap is k0 = q * P + r - 8 - for n in 1, 2, 3, 5, 7 and 16387 (P = 1 and 2, where the
quotient is largest, up to 32774), every border, q from 0 to the largest the API accepts (near 2**39 / P) in both directions and r on and
beside the multiple of P and the mirror point; the 16 pixels of an item are lanes of one wavefront, and for q = -1 and q = 2 they lie on
either side of the branch.  The whole NEAREST sweep is ONE call of qoimi_decode_warped with guard bytes between the items, at 4 channels and
at 3, and one of qoimi_decode_warped_tensors as int64 HW; the samplings that fold more than one tap - bilinear at a fraction of one half,
BICUBIC, SUPER2 with the border - run the same positions with q thinned to +-2, +-1000, +-(2**39 // P) (r and n are never thinned; the model
of sixteen taps an output pixel is what takes the time).  Every byte is compared with qoi_amd/warp.py: warp.  The same (k, n, border) run
through the host build in tests/test_warp_border_core_host.py, so a failure here and not there is the device's."""
import numpy as np
import pytest

import warp_fold_cases as W
from qoi_amd import tensors, warp
from qoi_amd.tensors import HW, I64
from qoi_amd.warp import BICUBIC, NEAREST, PLAIN, SUPER2
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu
_MODELS = {}


def model(D, it, och, mode=PLAIN):
    """the u8 result of one item by the definition: computed once, never changed; D the 4-channel pixels of the item's image"""
    key = (tuple(it), och, mode)
    if key not in _MODELS:
        _, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
        P = warp.warp(np.ascontiguousarray(D[..., :och]), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode)
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


# ------------------------------------------------------------------ without a GPU: what the sweep holds
def test_the_sweep_is_the_fold_and_holds_every_class():
    D = W.pixels()
    cases = W.sweep()
    assert len(cases) == 1773 and [len(W.sweep(s, True)) for s in W.SAMPLINGS_THINNED] == [865, 865, 865]
    assert len({tuple(D[i].reshape(-1, 4)[j]) for i in range(4) for j in range(D[i].shape[0] * D[i].shape[1])}) == 2 * W.WIDE + 36     # one-to-one
    classes = {b: dict.fromkeys(("inside", "outside", "P1", "P2", "far", "across -P", "across 2P", "on a multiple"), 0) for b in W.BORDERS}
    for it, first, (n, border, axis) in cases:
        assert np.array_equal(model(D[it[0]], it, 4), W.direct(D[it[0]], it, first)), it
        assert np.array_equal(model(D[it[0]], it, 3), W.direct(D[it[0]], it, first)[..., :3]), it
        if axis == 2:
            continue
        P, k0, c = W.period(n, border), first[axis], classes[border]
        assert -W.K_TOP < k0 and k0 + W.OUT < W.K_TOP
        c["inside"] += -P <= k0 and k0 + W.OUT <= 2 * P
        c["outside"] += k0 + W.OUT <= -P or k0 >= 2 * P
        c["P1"] += P == 1
        c["P2"] += P == 2
        c["far"] += abs(k0) // P >= (1 << 39) // P - 1               # the largest quotient of this period (above 2**38 only where P = 1)
        c["across -P"] += k0 < -P <= k0 + W.OUT - 1                  # two neighbouring output pixels on either side of the branch
        c["across 2P"] += k0 < 2 * P <= k0 + W.OUT - 1
        c["on a multiple"] += any((k0 + X) % P == 0 for X in range(1, W.OUT)) and abs(k0) > 2 * P
    assert classes[warp.REFLECT].pop("P1") == 0                              # (REFLECT has P = 2n: no period of 1)
    assert all(v > 0 for c in classes.values() for v in c.values()), classes
    assert max(abs(first[axis]) // W.period(n, border) for _, first, (n, border, axis) in cases if axis != 2) >= (1 << 39) - 16     # P = 1: the largest quotient
    # the thinned sweeps stand at the same positions, and their taps are the ones the docstring of the cases names
    for s in W.SAMPLINGS_THINNED:
        thin = W.sweep(s, True)
        assert {(f, k) for _, f, k in thin} <= {(f, k) for _, f, k in W.sweep(NEAREST, True)} and all(it[7] & ~warp.BORDERS == s for it, _, _ in thin)
    it, first, _ = W.sweep(0, True)[0]
    p = (it[8] * 1 + it[14]) - warp.ONE                                      # X = 0: U = 1
    assert p >> 17 == first[0] and p & (2 * warp.ONE - 1) == warp.ONE       # the first tap and a fraction of one half


# ------------------------------------------------------------------ on the device


@pytest.fixture(scope="module")
def pack(api, oracle):
    from gpu_pack import OraclePack
    p = OraclePack(api, oracle, W.SHAPES, W.pixels())
    assert all(np.array_equal(p.decoded(i, 4), D) and np.array_equal(p.decoded(i, 3), D[..., :3]) for i, D in enumerate(W.pixels()))
    return p


def guarded_offsets(items, och):
    """outputs behind 65 guard bytes with 1 to 3 guard bytes between neighbours"""
    offsets, at = [], 65
    for j, it in enumerate(items):
        offsets.append(at)
        at += it[5] * it[6] * och + 1 + j % 3
    return offsets


def assert_items(p, got, items, och, what):
    for j, it in enumerate(items):
        w = model(p.decoded(it[0], 4), it, och).reshape(-1)
        if not np.array_equal(got[j], w):
            k = int(np.argmax(got[j] != w)) // och
            raise AssertionError((what, och, "item", j, it, "output pixel", k, "is", got[j][k * och:(k + 1) * och].tolist(), "not", w[k * och:(k + 1) * och].tolist()))


@gpu
@pytest.mark.parametrize("channels", [4, 3])
def test_the_nearest_sweep_in_one_call(ctx, pack, channels):
    from gpu_calls import run_warp
    items = [it for it, _, _ in W.sweep()]
    got = run_warp(ctx, pack, channels, items, PLAIN, offsets=guarded_offsets(items, channels))
    assert ctx.warp_stats()[:2] == (1, 1)
    assert_items(pack, got, items, channels, "nearest")


@gpu
@pytest.mark.parametrize("sampling", W.SAMPLINGS_THINNED, ids=["bilinear", "bicubic", "super2"])
def test_the_samplings_that_fold_more_than_one_tap(ctx, pack, sampling):
    """the positions of the sweep, q thinned to +-2, +-1000, +-(2**39 // P): two taps and warp_fold_next across P; four taps, the first at
    k - 1; warp_border_axis from warp_super_pixel"""
    from gpu_calls import run_warp
    items = [it for it, _, _ in W.sweep(sampling, True)]
    assert all(it[7] & (NEAREST | BICUBIC | SUPER2) == sampling for it in items)
    for channels in (4, 3):
        got = run_warp(ctx, pack, channels, items, PLAIN, offsets=guarded_offsets(items, channels))
        assert ctx.warp_stats()[:2] == (1, 1)
        assert_items(pack, got, items, channels, sampling)


@gpu
def test_the_nearest_sweep_as_a_label_tensor(ctx, pack):
    """warp_border_tensor: the whole sweep as int64 HW in one call"""
    from gpu_calls import run_label_tensors as run_tensors
    items = [it for it, _, _ in W.sweep()]
    f = tensors.fmt(I64, HW)
    got = run_tensors(ctx, pack, "warp", 4, items, PLAIN, f)
    assert ctx.tensor_stats()[:2] == (1, 1)
    for j, it in enumerate(items):
        w = tensors.convert(model(pack.decoded(it[0], 4), it, 4), f).view(np.uint8).reshape(-1)
        assert got[j].size == w.size and np.array_equal(got[j], w), ("tensor", j, it, int(np.argmax(got[j] != w)) // 8)
