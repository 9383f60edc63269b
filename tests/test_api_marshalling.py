"""CPU-only, no library: what every ``Context`` method of qoi_amd/api.py hands its C function.

A stub stands in for the loaded library: every ``qoimi_*`` attribute records its arguments - each scalar, the bytes behind each pointer for
the length the call implies, None where a NULL is passed - and returns 0.  Every method is called once with small fixed inputs, then once
per variant of the inputs it reads (another spelling of the same values, a sequence one short, a malformed item, a negative offset); what
the C function would receive, what the method returns and what it raises are compared with tests/golden/api_marshalling.json, which was
recorded from the hand-written binding before its marshalling was consolidated.  ``python tests/test_api_marshalling.py`` records it again.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qoi_amd import api  # noqa: E402
from qoi_amd.seekindex import POINT_DTYPE  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_marshalling.json")
HANDLE = 0x5EED0
_BYREF = type(ctypes.byref(ctypes.c_int()))


def _memory(arg):
    """(address, bytes the object itself says it spans) of a pointer argument."""
    if isinstance(arg, _BYREF):
        arg = arg._obj
    if isinstance(arg, (ctypes.Array, ctypes.Structure, ctypes._SimpleCData)):
        return ctypes.addressof(arg), ctypes.sizeof(arg)
    assert isinstance(arg, ctypes._Pointer), arg
    return ctypes.cast(arg, ctypes.c_void_p).value, arg._arr.nbytes if hasattr(arg, "_arr") else ctypes.sizeof(arg._type_)


def _seen(arg, want):
    """An argument as the golden file states it: ints as they are, a pointer as "hex:" and the bytes behind it - as many as the golden
    entry `want` has, or (recording) as the object spans."""
    if arg is None or isinstance(arg, (bool, int)):
        return None if arg is None else int(arg)
    if isinstance(arg, ctypes._SimpleCData):
        return arg.value
    address, nbytes = _memory(arg)
    if isinstance(want, str) and want.startswith("hex:"):
        nbytes = (len(want) - 4) // 2
    return "hex:" + ctypes.string_at(address, nbytes).hex()


class StubLib:
    """Stands in for the loaded library: records every ``qoimi_*`` call and returns 0 (``qoimi_seek_points``: the count, so that the
    callers that size an index by it can go on)."""

    def __init__(self, want_calls):
        self.calls, self.want_calls = [], want_calls or []

    def __getattr__(self, name):
        if not name.startswith("qoimi_"):
            raise AttributeError(name)

        def call(*args):
            k = len(self.calls)
            want = self.want_calls[k][1] if k < len(self.want_calls) and len(self.want_calls[k][1]) == len(args) else [None] * len(args)
            self.calls.append([name, [_seen(a, w) for a, w in zip(args, want)]])
            if name == "qoimi_seek_points":
                desc, rows = args[0]._obj, args[1]
                return -1 if rows == 0 or rows * desc.width < 128 else -(-desc.height // rows) - 1
            return 0
        return call


def _plain(v):
    """A method's result as JSON."""
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "shape": list(v.shape), "hex": v.tobytes().hex()}
    if isinstance(v, (ctypes.Structure, ctypes.Array)):
        return "hex:" + bytes(v).hex()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v if v is None else int(v)


def _index(n):
    a = np.zeros(n, dtype=POINT_DTYPE)
    a["byte_off"], a["skip"], a["prev"] = np.arange(n) * 100 + 14, np.arange(n), 0xFF000000 + np.arange(n)
    a["table"] = np.arange(n * 64).reshape(n, 64)
    return a


def _ctypes_index(n):
    arr = (api.QoimiSeekPoint * n)()
    ctypes.memmove(arr, _index(n).ctypes.data, n * 272)
    return arr


class Inputs:
    """The fixed inputs of every call - three images, two items of every kind (a tuple and a structure) - with a variant's values in
    place of some; `used` collects what a call read, so that a method is run under the variants of its own inputs only."""

    def __init__(self, **over):
        self.used = set()
        self.values = dict(
            so=[0, 4096, 12288], sz=[1000, 2000, 300], po=[0, 16384, 65536], oo=[7, 256], ao=[1, 2, 3], bo=[30, 20, 10],
            descs=[api.QoiDesc(64, 48, 4, 0), api.QoiDesc(40, 30, 3, 1), api.QoiDesc(200, 16, 4, 0)],
            crops=[(0, 1, 2, 3, 4, 0), api.QoimiCrop(2, 5, 6, 7, 8, 3)],
            items=[(0, 0, 0, 32, 24, 16, 12, 0), api.QoimiResize(1, 2, 3, 20, 10, 5, 6, 1)],
            warps=[(0, 1, 2, 30, 20, 15, 10, 0, 65536, -3, -2 ** 31, 2 ** 31 - 1, 0x80FF00FF, 0, -2 ** 63, 2 ** 63 - 1),
                   api.QoimiWarp(2, 0, 0, 200, 16, 8, 8, 1, -65536, 0, 0, 65536, 7, 0, 1 << 40, -5)],
            tiles=[(0, 0, 0, 32, 32, 2), (1, 8, 8, 16, 16, 1, 3), api.QoimiTile(2, 0, 0, 200, 16, 4, 1, 0)],
            bands=[(0, 16, 16), api.QoimiBand(2, 0, 8, 0)],
            factors=2, k=16, points=_index(3), pf=[0, 2, 3], fmt=(2, 1, (0.5, 0.25, 2.0, 1.0), (0.0, -1.0, 1.0, 3.5)))
        self.values.update(over)

    def __getattr__(self, key):
        self.used.add(key)
        return self.values[key]


# name -> what to call; the scalars differ from one another, so that two of them swapped show
CALLS = {
    "encode_batch": lambda c, a: c.encode_batch(0x1000, 12288, a.descs[0], 5, 0x2000, 20000, 0x3000, 0x77),
    "encode_images": lambda c, a: c.encode_images(0x1000, a.po, a.descs, 0x2000, a.so, 0x3000, 0x77),
    "encode_status": lambda c, a: c.encode_status(0x77),
    "encode_suspect_calls": lambda c, a: c.encode_suspect_calls(),
    "set_encode_small_call_order": lambda c, a: c.set_encode_small_call_order(True),
    "encode_retries": lambda c, a: c.encode_retries(),
    "decode_batch": lambda c, a: c.decode_batch(0x2000, 4096, a.sz, a.descs, 4, 0x1000, 16384, 0x77),
    "decode_batch_c_arrays": lambda c, a: c.decode_batch(0x2000, 100, (ctypes.c_int * 3)(*a.sz), (api.QoiDesc * 3)(*a.descs), 3, 0x1000, 16384),
    "decode_batch_long_stream": lambda c, a: c.decode_batch(0x2000, 1999, a.sz, a.descs, 4, 0x1000, 16384),
    "decode_images": lambda c, a: c.decode_images(0x2000, a.so, a.sz, a.descs, 4, 0x1000, a.po, 0x77),
    "pack_streams": lambda c, a: c.pack_streams(0x2000, 20000, 0x3000, 5, 64, 0x4000, 1 << 20, 0x5000, 0x77),
    "encode_packed": lambda c, a: c.encode_packed(0x1000, 12288, a.descs[0], 2, 64, 0x4000, 1 << 20, 0x5000, 0x3000, 1 << 16, 0x77),
    "encode_images_packed": lambda c, a: c.encode_images_packed(0x1000, a.po, a.descs, 64, 0x4000, 1 << 20, 0x5000, 0x3000, 1 << 16, 0x77),
    "encode_tiles": lambda c, a: c.encode_tiles(0x1000, a.po, a.descs, 3, a.tiles, 1, 64, 0x4000, 1 << 20, 0x5000, 0x3000, 1 << 16, 0x77),
    "read_descs": lambda c, a: c.read_descs(0x2000, a.so, a.sz, 0x77),
    "inspect_streams": lambda c, a: c.inspect_streams(0x2000, a.so, a.sz, 0x77),
    "compare_images": lambda c, a: c.compare_images(0x1000, a.ao, 3, 0x6000, a.bo, 4, a.descs, 0x77),
    "verify_images": lambda c, a: c.verify_images(0x1000, a.po, a.descs, 0x2000, a.so, a.sz, 1 << 16, 0x77),
    "decode_thumbnails": lambda c, a: c.decode_thumbnails(0x2000, a.so, a.sz, a.descs, 4, a.factors, 1, 0x7000, a.po, 1 << 16, 0x77),
    "decode_crops": lambda c, a: c.decode_crops(0x2000, a.so, a.sz, a.descs, 4, a.crops, 0x7000, a.oo, 1 << 16, 0x77),
    "decode_resized": lambda c, a: c.decode_resized(0x2000, a.so, a.sz, a.descs, 4, a.items, 1, 0x7000, a.oo, 1 << 16, 0x77),
    "decode_bilinear": lambda c, a: c.decode_bilinear(0x2000, a.so, a.sz, a.descs, 4, a.items, 1, 0x7000, a.oo, 1 << 16, 0x77),
    "decode_warped": lambda c, a: c.decode_warped(0x2000, a.so, a.sz, a.descs, 4, a.warps, 1, 0x7000, a.oo, 1 << 16, 0x77),
    "decode_tensors": lambda c, a: c.decode_tensors(0x2000, a.so, a.sz, a.descs, 4, a.items, 1, 0, a.fmt, 0x7000, a.oo, 1 << 16, 0x77),
    "decode_tensors_format_structure": lambda c, a: c.decode_tensors(0x2000, a.so, a.sz, a.descs, 3, a.items, 0, 1, api.tensor_format(a.fmt), 0x7000, a.oo),
    "decode_warped_tensors": lambda c, a: c.decode_warped_tensors(0x2000, a.so, a.sz, a.descs, 4, a.warps, 1, a.fmt, 0x7000, a.oo, 1 << 16, 0x77),
    "pixel_stats": lambda c, a: c.pixel_stats(0x2000, a.so, a.sz, a.descs, a.crops, 0x8000, 1 << 16, 0x77),
    "pixel_stats_no_histogram": lambda c, a: c.pixel_stats(0x2000, a.so, a.sz, a.descs, a.crops),
    "build_seek_index": lambda c, a: c.build_seek_index(0x2000, a.so, a.sz, a.descs, a.k, 1 << 16, 0x77),
    "seek_index_from_pixels": lambda c, a: c.seek_index_from_pixels(0x1000, a.po, 0x2000, a.so, a.sz, a.descs, a.k, 0x77),
    "make_band_streams": lambda c, a: c.make_band_streams(0x2000, a.so, a.sz, a.descs, a.k, a.points, a.pf, a.bands, 0x7000, a.oo, 0x77),
    "decode_crops_indexed": lambda c, a: c.decode_crops_indexed(0x2000, a.so, a.sz, a.descs, 4, a.crops, 0x7000, a.oo, a.k, a.points, a.pf, 1 << 16, 0x77),
    "decode_resized_indexed": lambda c, a: c.decode_resized_indexed(0x2000, a.so, a.sz, a.descs, 4, a.items, 1, 0x7000, a.oo, a.k, a.points, a.pf, 1 << 16, 0x77),
    "decode_bilinear_indexed": lambda c, a: c.decode_bilinear_indexed(0x2000, a.so, a.sz, a.descs, 4, a.items, 1, 0x7000, a.oo, a.k, a.points, a.pf, 1 << 16, 0x77),
    "decode_warped_indexed": lambda c, a: c.decode_warped_indexed(0x2000, a.so, a.sz, a.descs, 4, a.warps, 1, 0x7000, a.oo, a.k, a.points, a.pf, 1 << 16, 0x77),
    "pixel_stats_indexed": lambda c, a: c.pixel_stats_indexed(0x2000, a.so, a.sz, a.descs, a.crops, a.k, a.points, a.pf, 0x8000, 1 << 16, 0x77),
    "synth_frames": lambda c, a: c.synth_frames(1, 42, 7, 3, 64, 48, 0x1000, 12288, 0x77),
    "hash_streams": lambda c, a: c.hash_streams(0x2000, 20000, 0x3000, 5, 0x9000, 0x77),
    "set_profiling": lambda c, a: c.set_profiling(True),
    "get_profile": lambda c, a: c.get_profile(0x77),
    "workspace_bytes": lambda c, a: c.workspace_bytes(),
    "set_decode_record_cap": lambda c, a: c.set_decode_record_cap(1 << 20, True),
    "decode_stats": lambda c, a: c.decode_stats(),
    "close": lambda c, a: c.close(),
    # the module functions that marshal a descriptor and an item
    "encode_bound": lambda c, a: api.encode_bound(64, 48, 4),
    "thumbnail_size": lambda c, a: api.thumbnail_size(64, 48, 4, 3, 4),
    "thumbnail_size_wide": lambda c, a: api.thumbnail_size(64, 48, 4, 2 ** 32, 4),
    "crop_size": lambda c, a: api.crop_size(64, 48, 4, a.crops[1], 3),
    "crop_size_wide": lambda c, a: api.crop_size(2 ** 32, 48, 4, a.crops[1], 3),
    "tile_size": lambda c, a: api.tile_size(64, 48, 4, a.tiles[1], 3),
    "tile_size_wide": lambda c, a: api.tile_size(64, 48, 256, a.tiles[1]),
    "tile_pyramid": lambda c, a: api.tile_pyramid(64, 48, 4, 16, 8, 2),
    "tile_pyramid_wide": lambda c, a: api.tile_pyramid(64, 48, 4, 16, 2 ** 32, 2),
    "resize_size": lambda c, a: api.resize_size(64, 48, 4, a.items[1], 3),
    "resize_size_wide": lambda c, a: api.resize_size(64, -1, 4, a.items[1], 3),
    "bilinear_size": lambda c, a: api.bilinear_size(64, 48, 4, a.items[1], 3),
    "warp_size": lambda c, a: api.warp_size(64, 48, 4, a.warps[1], 3),
    "tensor_size": lambda c, a: api.tensor_size(64, 48, 4, a.items[1], 1, 3, a.fmt),
    "warp_tensor_size": lambda c, a: api.warp_tensor_size(64, 48, 4, a.warps[1], 3, a.fmt),
    "warp_orient": lambda c, a: api.warp_orient(64, 48, 4, (1, 2, 30, 20), 6),
    "warp_orient_wide": lambda c, a: api.warp_orient(64, 48, 4, (1, 2, 30, 2 ** 32), 6),
    "seek_points": lambda c, a: api.seek_points(64, 48, 4, 16),
    "seek_points_wide": lambda c, a: api.seek_points(64, 48, 4, -1),
    "band_plan": lambda c, a: api.band_plan(a.descs[0], 1000, a.k, a.points, 16, 16),
    "band_plan_wide": lambda c, a: api.band_plan(a.descs[0], 2 ** 31, a.k, a.points, 16, 16),
}
for _name in ("tile", "thumbnail", "crop", "resize", "bilinear", "warp", "tensor", "seek"):
    CALLS[_name + "_stats"] = lambda c, a, _name=_name: getattr(c, _name + "_stats")()
CALLS["pixel_stats_counters"] = lambda c, a: c.pixel_stats_counters()

_BAD_WARP = (0, 1, 2, 30, 20, 15, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0)
# name -> the inputs it replaces; a call is run under a variant when it reads one of them
VARIANTS = {
    "numpy_sequences": dict(so=np.array([0, 4096, 12288]), sz=np.array([1000, 2000, 300], dtype=np.int64), po=np.array([0, 16384, 65536], dtype=np.uint64),
                            oo=(7, 256), pf=np.array([0, 2, 3]), ao=(1, 2, 3), bo=np.array([30, 20, 10], dtype=np.uint32)),
    "interval_list": dict(k=[24, 16, 16]), "interval_numpy_int": dict(k=np.uint32(16)), "interval_short": dict(k=[16, 16]),
    "interval_rejected": dict(k=[16, 3, 16]), "interval_negative": dict(k=[16, -1, 16]),
    "factor_list": dict(factors=[1, 2, 64]), "factor_short": dict(factors=[1, 2]), "factor_wide": dict(factors=[1, 2 ** 32, 2]),
    "ctypes_index": dict(points=_ctypes_index(3)),
    "short_stream_offsets": dict(so=[0, 4096]), "short_sizes": dict(sz=[1000, 2000]), "short_descs": dict(descs=[api.QoiDesc(64, 48, 4, 0)] * 2),
    "short_pixel_offsets": dict(po=[0, 16384]), "short_output_offsets": dict(oo=[7]), "short_point_firsts": dict(pf=[0, 2]),
    "short_side_offsets": dict(ao=[1, 2]),
    "negative_stream_offset": dict(so=[0, -1, 12288]), "negative_pixel_offset": dict(po=[0, -16, 65536]), "negative_output_offset": dict(oo=[7, -1]),
    "negative_point_first": dict(pf=[0, -2, 3]), "size_past_int": dict(sz=[1000, 2 ** 31, 300]), "side_offset_past_size_t": dict(bo=[30, 2 ** 64, 10]),
    "item_too_short": dict(crops=[(0, 1, 2, 3, 4, 0), (0, 1, 2, 3, 4)], items=[(0, 0, 0, 32, 24, 16, 12, 0), (0, 0, 0, 32, 24, 16, 12)],
                           warps=[_BAD_WARP, _BAD_WARP[:15]], tiles=[(0, 0, 0, 32, 32, 2), (0, 0, 0, 32, 32)], bands=[(0, 16, 16), (0, 16)]),
    "item_too_long": dict(crops=[(0, 1, 2, 3, 4, 0, 0), (0, 1, 2, 3, 4, 0)], items=[(0, 0, 0, 32, 24, 16, 12, 0, 0), (0, 0, 0, 32, 24, 16, 12, 0)],
                          warps=[_BAD_WARP + (0,), _BAD_WARP], tiles=[(0, 0, 0, 32, 32, 2, 0, 0, 0), (0, 0, 0, 32, 32, 2)], bands=[(0, 16, 16, 0), (0, 16, 16)]),
    "item_field_wide": dict(crops=[(0, 1, 2, 3, 4, 0), (0, 1, 2, 3, 4, 2 ** 32)], items=[(0, 0, 0, 32, 24, 16, 12, 0), (0, 0, 0, 32, 24, 2 ** 32, 12, 0)],
                            warps=[_BAD_WARP, _BAD_WARP[:12] + (2 ** 32,) + _BAD_WARP[13:]], tiles=[(0, 0, 0, 32, 32, 2), (0, 0, 0, 32, 32, 2, 0, 2 ** 32)],
                            bands=[(0, 16, 16), (0, 16, 2 ** 32)]),
    "item_field_negative": dict(crops=[(0, 1, 2, 3, 4, 0), (0, -1, 2, 3, 4, 0)], items=[(0, 0, 0, 32, 24, 16, 12, 0), (0, 0, -1, 32, 24, 16, 12, 0)],
                                warps=[_BAD_WARP, (-1,) + _BAD_WARP[1:]], tiles=[(0, 0, 0, 32, 32, 2), (0, 0, 0, 32, -1, 2)], bands=[(0, 16, 16), (-1, 16, 16)]),
    "warp_int_field_wide": dict(warps=[_BAD_WARP, _BAD_WARP[:8] + (2 ** 31,) + _BAD_WARP[9:]]),
    "warp_int_field_low": dict(warps=[_BAD_WARP, _BAD_WARP[:11] + (-2 ** 31 - 1,) + _BAD_WARP[12:]]),
    "warp_long_field_wide": dict(warps=[_BAD_WARP, _BAD_WARP[:14] + (2 ** 63, 0)]),
    "warp_long_field_low": dict(warps=[_BAD_WARP, _BAD_WARP[:15] + (-2 ** 63 - 1,)]),
    "format_short_scale": dict(fmt=(2, 1, (0.5, 0.25, 2.0), (0.0, -1.0, 1.0, 3.5))), "format_dtype_wide": dict(fmt=(2 ** 32, 1, (1,) * 4, (0,) * 4)),
}


def record(name, over, want=None):
    """What the call `name` does under the inputs `over`: {"read": the inputs it read, "calls": what the stub saw, and "result" or "raises"}."""
    stub = StubLib((want or {}).get("calls"))
    ctx = api.Context.__new__(api.Context)
    ctx._lib, ctx._h, ctx.device = stub, ctypes.c_void_p(HANDLE), 0
    inputs = Inputs(**over)
    saved, api._lib = api._lib, stub                 # the module functions reach the library through load_library()
    try:
        out = {"result": _plain(CALLS[name](ctx, inputs))}
    except api.QoiError as e:
        out = {"raises": "QoiError: " + str(e)}
    except Exception as e:                           # whatever a conversion raises: its type is pinned, its wording is numpy's or ctypes' own
        out = {"raises": type(e).__name__}
    finally:
        api._lib = saved
        ctx._h = None
    return dict(read=sorted(inputs.used), calls=stub.calls, **out)


def record_all(name, golden=None):
    base = record(name, {}, golden and golden[""])
    out = {"": base}
    for variant, over in VARIANTS.items():
        if set(over) & set(base["read"]):
            out[variant] = record(name, over, golden and golden.get(variant))
    return out


_GOLDEN = json.load(open(GOLDEN)) if __name__ != "__main__" else {}


def test_every_context_method_is_called():
    public = {n for n, v in vars(api.Context).items() if callable(v) and not n.startswith("_")}
    assert public <= set(CALLS) and set(_GOLDEN) == set(CALLS), public - set(CALLS)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_marshalling(name):
    got = record_all(name, _GOLDEN[name])
    assert sorted(got) == sorted(_GOLDEN[name])
    for variant in got:
        assert got[variant] == _GOLDEN[name][variant], (name, variant)


if __name__ == "__main__":
    with open(GOLDEN, "w") as _f:                   # one line per call and variant
        _f.write("{\n" + ",\n".join(json.dumps(name) + ": {\n" + ",\n".join(
            "  " + json.dumps(v) + ": " + json.dumps(r, sort_keys=True) for v, r in record_all(name).items()) + "\n}" for name in sorted(CALLS)) + "\n}\n")
