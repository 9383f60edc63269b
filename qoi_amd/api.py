"""Python host side of the MI355X QOI path — a ctypes binding of libqoi_mi355x.so.

Mirrors the reference's interface for this path (phoboslab/qoi ``qoi.h``):

* :func:`qoi_encode` / :func:`qoi_decode` — same argument meaning and failure
  behaviour (``None`` where the C functions return ``NULL``) as ``qoi.h:278`` /
  ``qoi.h:289``; :class:`QoiDesc` is ``qoi_desc`` (``qoi.h:236-241``).
* :class:`Context` — the additive device-resident batch API (``qoimi_*``), taking
  raw device pointers (e.g. ``torch.Tensor.data_ptr()``) and a HIP stream handle.

There is no CPU fallback here: if the shared library or the GPU is missing the
calls raise / return ``None`` exactly as the C-ABI does.  torch is NOT imported by
this module; bench.py and the tests use it only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

QOI_SRGB = 0
QOI_LINEAR = 1

_HERE = os.path.dirname(os.path.abspath(__file__))
# (tests and measurement tools that want another build of the library - the test flavour, an experimental build - set this before
# the first call: tests/libsel.py; nothing in the environment changes it)
LIB_PATH = os.path.join(_HERE, "lib", "libqoi_mi355x.so")

EXPORTS = (
    # Part 1 — drop-in symbols (qoi.h:252,265,278,289)
    "qoi_encode", "qoi_decode", "qoi_write", "qoi_read",
    # Part 2 — additive
    "qoimi_ctx_create", "qoimi_ctx_destroy", "qoimi_last_error", "qoimi_encode_bound",
    "qoimi_encode_batch", "qoimi_encode_status", "qoimi_decode_batch", "qoimi_synth_frames",
    "qoimi_decode_stats", "qoimi_version", "qoimi_set_profiling", "qoimi_get_profile", "qoimi_kernel_name",
    "qoimi_encode_suspect_calls", "qoimi_encode_retries", "qoimi_set_encode_small_call_order", "qoimi_workspace_bytes", "qoimi_set_decode_record_cap", "qoimi_hash_streams", "qoimi_encode_images",
    "qoimi_decode_images", "qoimi_pack_streams", "qoimi_read_descs", "qoimi_inspect_streams",
    "qoimi_encode_packed", "qoimi_encode_images_packed",
    "qoimi_compare_images", "qoimi_verify_images",
    "qoimi_decode_thumbnails", "qoimi_thumbnail_size", "qoimi_thumbnail_stats",
    "qoimi_decode_crops", "qoimi_crop_size", "qoimi_crop_stats",
    "qoimi_decode_resized", "qoimi_resize_size", "qoimi_resize_stats",
    "qoimi_pixel_stats", "qoimi_pixel_stats_counters",
    "qoimi_seek_points", "qoimi_build_seek_index", "qoimi_band_plan", "qoimi_make_band_streams", "qoimi_decode_crops_indexed", "qoimi_seek_stats",
    "qoimi_seek_index_from_pixels", "qoimi_decode_resized_indexed", "qoimi_pixel_stats_indexed",
    "qoimi_decode_bilinear", "qoimi_bilinear_size", "qoimi_bilinear_stats", "qoimi_decode_bilinear_indexed",
    "qoimi_decode_warped", "qoimi_warp_size", "qoimi_warp_stats", "qoimi_warp_orient", "qoimi_decode_warped_indexed",
    "qoimi_decode_tensors", "qoimi_decode_warped_tensors", "qoimi_tensor_size", "qoimi_warp_tensor_size", "qoimi_tensor_stats",
    "qoimi_encode_tiles", "qoimi_tile_size", "qoimi_tile_pyramid", "qoimi_tile_stats",
)


class QoiDesc(ctypes.Structure):
    """``qoi_desc`` (qoi.h:236-241)."""
    _fields_ = [("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("channels", ctypes.c_ubyte), ("colorspace", ctypes.c_ubyte)]

    def __repr__(self):
        return f"QoiDesc({self.width}x{self.height}, channels={self.channels}, colorspace={self.colorspace})"


class StreamInfo(ctypes.Structure):
    """``qoimi_stream_info``: 64 bytes, the layout of ``streaminfo.INFO_DTYPE``."""
    _fields_ = [("pixels", ctypes.c_ulonglong), ("run_pixels", ctypes.c_ulonglong), ("ops", ctypes.c_uint * 6),
                ("repeat_index", ctypes.c_uint), ("walk_end", ctypes.c_uint), ("flags", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


class ImageDiff(ctypes.Structure):
    """``qoimi_image_diff``: 32 bytes, the layout of ``imagediff.DIFF_DTYPE``."""
    _fields_ = [("mismatched", ctypes.c_ulonglong), ("first", ctypes.c_ulonglong), ("want", ctypes.c_uint), ("got", ctypes.c_uint),
                ("flags", ctypes.c_uint), ("reserved", ctypes.c_uint)]


class QoimiCrop(ctypes.Structure):
    """``qoimi_crop``: 24 bytes - a rectangle of image ``image`` and how it is mirrored (``crops.FLIP_X`` / ``crops.FLIP_Y``)."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("flags", ctypes.c_uint)]


assert ctypes.sizeof(QoimiCrop) == 24 and [getattr(QoimiCrop, f).offset for f, _ in QoimiCrop._fields_] == [0, 4, 8, 12, 16, 20]


class QoimiTile(ctypes.Structure):
    """``qoimi_tile``: 32 bytes - a rectangle of image ``image``, the factor it is box-reduced by and how the result is mirrored
    (``tiles.FLIP_X`` / ``tiles.FLIP_Y``); ``reserved`` is 0."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("factor", ctypes.c_uint), ("flags", ctypes.c_uint), ("reserved", ctypes.c_uint)]


assert ctypes.sizeof(QoimiTile) == 32 and [getattr(QoimiTile, f).offset for f, _ in QoimiTile._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]


class QoimiResize(ctypes.Structure):
    """``qoimi_resize``: 32 bytes - a rectangle of image ``image``, the size it is resampled to and how the result is mirrored
    (``resize.FLIP_X`` / ``resize.FLIP_Y``)."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("out_width", ctypes.c_uint), ("out_height", ctypes.c_uint), ("flags", ctypes.c_uint)]


assert ctypes.sizeof(QoimiResize) == 32 and [getattr(QoimiResize, f).offset for f, _ in QoimiResize._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]


class QoimiWarp(ctypes.Structure):
    """``qoimi_warp``: 72 bytes - a rectangle of image ``image``, the size of the output, the inverse affine map from the output into the
    rectangle (``warp.py`` states it), the border (``warp.REPLICATE`` or ``fill``)."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("out_width", ctypes.c_uint), ("out_height", ctypes.c_uint), ("flags", ctypes.c_uint), ("a", ctypes.c_int), ("b", ctypes.c_int),
                ("d", ctypes.c_int), ("e", ctypes.c_int), ("fill", ctypes.c_uint), ("reserved", ctypes.c_uint), ("c", ctypes.c_longlong),
                ("f", ctypes.c_longlong)]


assert ctypes.sizeof(QoimiWarp) == 72 and [getattr(QoimiWarp, f).offset for f, _ in QoimiWarp._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64]


class QoimiTensorFormat(ctypes.Structure):
    """``qoimi_tensor_format``: 48 bytes - the element type (``tensors.U8`` / ``F16`` / ``BF16`` / ``F32``), the layout (``tensors.HWC`` /
    ``CHW``) and the scale and bias of each channel (``tensors.py`` states the result)."""
    _fields_ = [("dtype", ctypes.c_uint), ("layout", ctypes.c_uint), ("scale", ctypes.c_float * 4), ("bias", ctypes.c_float * 4),
                ("reserved", ctypes.c_uint * 2)]


assert ctypes.sizeof(QoimiTensorFormat) == 48 and [getattr(QoimiTensorFormat, f).offset for f, _ in QoimiTensorFormat._fields_] == [0, 4, 8, 24, 40]


class QoimiPixelStat(ctypes.Structure):
    """``qoimi_pixel_stat``: 128 bytes - what ``qoimi_pixel_stats`` says of one region (``pixelstats.stats`` states the fields)."""
    _fields_ = [("pixels", ctypes.c_ulonglong), ("sum", ctypes.c_ulonglong * 4), ("sum_sq", ctypes.c_ulonglong * 4), ("min", ctypes.c_ubyte * 4),
                ("max", ctypes.c_ubyte * 4), ("first", ctypes.c_uint), ("flags", ctypes.c_uint), ("opaque_pixels", ctypes.c_ulonglong),
                ("transparent_pixels", ctypes.c_ulonglong), ("grey_pixels", ctypes.c_ulonglong), ("reserved", ctypes.c_uint * 4)]


assert ctypes.sizeof(QoimiPixelStat) == 128 and [getattr(QoimiPixelStat, f).offset for f, _ in QoimiPixelStat._fields_] == [0, 8, 40, 72, 76, 80, 84, 88, 96, 104, 112]


class QoimiSeekPoint(ctypes.Structure):
    """``qoimi_seek_point``: 272 bytes, the layout of ``seekindex.POINT_DTYPE`` - the decoder's state at a row boundary."""
    _fields_ = [("byte_off", ctypes.c_uint), ("skip", ctypes.c_uint), ("prev", ctypes.c_uint), ("reserved", ctypes.c_uint), ("table", ctypes.c_uint * 64)]


class QoimiBand(ctypes.Structure):
    """``qoimi_band``: 16 bytes - rows [first_row, first_row + rows) of image ``image``; first_row is 0 or a seek row."""
    _fields_ = [("image", ctypes.c_uint), ("first_row", ctypes.c_uint), ("rows", ctypes.c_uint), ("reserved", ctypes.c_uint)]


class QoimiBandInfo(ctypes.Structure):
    """``qoimi_band_info``: 24 bytes - what a band stream will be: its size, its descriptor and the rows in front of the band's own."""
    _fields_ = [("size", ctypes.c_ulonglong), ("desc", QoiDesc), ("pad_rows", ctypes.c_uint)]


assert ctypes.sizeof(QoimiSeekPoint) == 272 and [getattr(QoimiSeekPoint, f).offset for f, _ in QoimiSeekPoint._fields_] == [0, 4, 8, 12, 16]
assert ctypes.sizeof(QoimiBand) == 16 and ctypes.sizeof(QoimiBandInfo) == 24 and (QoimiBandInfo.desc.offset, QoimiBandInfo.pad_rows.offset) == (8, 20)


class QoiError(RuntimeError):
    pass


_lib = None


def load_library() -> ctypes.CDLL:
    """Load libqoi_mi355x.so (built in-tree by ``__graft_entry__.build()``); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QoiError(f"{LIB_PATH} not built - run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.qoi_encode.restype = vp
    lib.qoi_encode.argtypes = [vp, ctypes.POINTER(QoiDesc), ctypes.POINTER(ci)]
    lib.qoi_decode.restype = vp
    lib.qoi_decode.argtypes = [vp, ci, ctypes.POINTER(QoiDesc), ci]
    lib.qoi_write.restype = ci
    lib.qoi_write.argtypes = [ctypes.c_char_p, vp, ctypes.POINTER(QoiDesc)]
    lib.qoi_read.restype = vp
    lib.qoi_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(QoiDesc), ci]
    lib.qoimi_ctx_create.restype = ci
    lib.qoimi_ctx_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.qoimi_ctx_destroy.restype = None
    lib.qoimi_ctx_destroy.argtypes = [vp]
    lib.qoimi_last_error.restype = ctypes.c_char_p
    lib.qoimi_last_error.argtypes = []
    lib.qoimi_version.restype = ctypes.c_char_p
    lib.qoimi_version.argtypes = []
    lib.qoimi_encode_bound.restype = sz
    lib.qoimi_encode_bound.argtypes = [ctypes.POINTER(QoiDesc)]
    lib.qoimi_encode_batch.restype = ci
    lib.qoimi_encode_batch.argtypes = [vp, vp, sz, ctypes.POINTER(QoiDesc), ci, vp, sz, vp, vp]
    lib.qoimi_encode_status.restype = ci
    lib.qoimi_encode_status.argtypes = [vp, vp]
    lib.qoimi_decode_batch.restype = ci
    lib.qoimi_decode_batch.argtypes = [vp, vp, sz, ctypes.POINTER(ci), ctypes.POINTER(QoiDesc), ci, ci, vp, sz, vp]
    lib.qoimi_synth_frames.restype = ci
    lib.qoimi_synth_frames.argtypes = [vp, ci, ctypes.c_uint, ctypes.c_uint, ci, ctypes.c_uint, ctypes.c_uint, vp, sz, vp]
    lib.qoimi_decode_stats.restype = None
    lib.qoimi_decode_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.qoimi_set_profiling.restype = ci
    lib.qoimi_set_profiling.argtypes = [vp, ci]
    lib.qoimi_get_profile.restype = ci
    lib.qoimi_get_profile.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong), ci]
    lib.qoimi_kernel_name.restype = ctypes.c_char_p
    lib.qoimi_kernel_name.argtypes = [ci]
    lib.qoimi_set_decode_record_cap.restype = ctypes.c_int
    lib.qoimi_set_decode_record_cap.argtypes = [vp, sz, ctypes.c_int]
    lib.qoimi_workspace_bytes.restype = None
    lib.qoimi_workspace_bytes.argtypes = [vp, ctypes.POINTER(sz)]
    lib.qoimi_encode_suspect_calls.restype = ctypes.c_longlong
    lib.qoimi_encode_suspect_calls.argtypes = [vp]
    lib.qoimi_set_encode_small_call_order.restype = ci
    lib.qoimi_set_encode_small_call_order.argtypes = [vp, ci]
    lib.qoimi_encode_retries.restype = ctypes.c_longlong
    lib.qoimi_encode_retries.argtypes = [vp]
    lib.qoimi_encode_images.restype = ci
    lib.qoimi_encode_images.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.POINTER(QoiDesc), ci, vp, ctypes.POINTER(sz), vp, vp]
    lib.qoimi_hash_streams.restype = ci
    lib.qoimi_hash_streams.argtypes = [vp, vp, sz, vp, ci, vp, vp]
    lib.qoimi_decode_images.restype = ci
    lib.qoimi_decode_images.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.POINTER(ci), ctypes.POINTER(QoiDesc), ci, ci, vp, ctypes.POINTER(sz), vp]
    lib.qoimi_pack_streams.restype = ci
    lib.qoimi_pack_streams.argtypes = [vp, vp, sz, vp, ci, ctypes.c_uint, vp, sz, vp, vp]
    lib.qoimi_read_descs.restype = ci
    lib.qoimi_read_descs.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.POINTER(ci), ci, ctypes.POINTER(QoiDesc), ctypes.POINTER(ci), vp]
    lib.qoimi_inspect_streams.restype = ci
    lib.qoimi_inspect_streams.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.POINTER(ci), ci, ctypes.POINTER(StreamInfo), ctypes.POINTER(ci), vp]
    ullp = ctypes.POINTER(ctypes.c_ulonglong)
    lib.qoimi_encode_packed.restype = ci
    lib.qoimi_encode_packed.argtypes = [vp, vp, sz, ctypes.POINTER(QoiDesc), ci, ctypes.c_uint, vp, sz, vp, vp, sz, ullp, ctypes.POINTER(ci), vp]
    lib.qoimi_encode_images_packed.restype = ci
    lib.qoimi_encode_images_packed.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.POINTER(QoiDesc), ci, ctypes.c_uint, vp, sz, vp, vp, sz, ullp, ctypes.POINTER(ci), vp]
    szp, dp = ctypes.POINTER(sz), ctypes.POINTER(QoiDesc)
    lib.qoimi_compare_images.restype = ci
    lib.qoimi_compare_images.argtypes = [vp, vp, szp, ci, vp, szp, ci, dp, ci, ctypes.POINTER(ImageDiff), ctypes.POINTER(ci), vp]
    lib.qoimi_verify_images.restype = ci
    lib.qoimi_verify_images.argtypes = [vp, vp, szp, dp, ci, vp, szp, ctypes.POINTER(ci), sz, ctypes.POINTER(ImageDiff), ctypes.POINTER(ci), vp]
    up = ctypes.POINTER(ctypes.c_uint)
    lib.qoimi_decode_thumbnails.restype = ci
    lib.qoimi_decode_thumbnails.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, up, ci, vp, szp, sz, vp]
    lib.qoimi_thumbnail_size.restype = sz
    lib.qoimi_thumbnail_size.argtypes = [dp, ctypes.c_uint, ci, up, up]
    lib.qoimi_thumbnail_stats.restype = None
    lib.qoimi_thumbnail_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    cp = ctypes.POINTER(QoimiCrop)
    lib.qoimi_decode_crops.restype = ci
    lib.qoimi_decode_crops.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, cp, ci, vp, szp, sz, vp]
    lib.qoimi_crop_size.restype = sz
    lib.qoimi_crop_size.argtypes = [dp, cp, ci]
    lib.qoimi_crop_stats.restype = None
    lib.qoimi_crop_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    tp = ctypes.POINTER(QoimiTile)
    lib.qoimi_encode_tiles.restype = ci
    lib.qoimi_encode_tiles.argtypes = [vp, vp, szp, dp, ci, ci, tp, ci, ci, ctypes.c_uint, vp, sz, vp, vp, sz, ullp, ctypes.POINTER(ci), dp, vp]
    lib.qoimi_tile_size.restype = sz
    lib.qoimi_tile_size.argtypes = [dp, tp, ci, up, up]
    lib.qoimi_tile_pyramid.restype = ci
    lib.qoimi_tile_pyramid.argtypes = [dp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, tp, ci]
    lib.qoimi_tile_stats.restype = None
    lib.qoimi_tile_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    rp = ctypes.POINTER(QoimiResize)
    lib.qoimi_decode_resized.restype = ci
    lib.qoimi_decode_resized.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, rp, ci, ci, vp, szp, sz, vp]
    lib.qoimi_resize_size.restype = sz
    lib.qoimi_resize_size.argtypes = [dp, rp, ci]
    lib.qoimi_resize_stats.restype = None
    lib.qoimi_resize_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.qoimi_pixel_stats.restype = ci
    lib.qoimi_pixel_stats.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, cp, ci, ctypes.POINTER(QoimiPixelStat), vp, sz, vp]
    lib.qoimi_pixel_stats_counters.restype = None
    lib.qoimi_pixel_stats_counters.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    pp, bp, ip = ctypes.POINTER(QoimiSeekPoint), ctypes.POINTER(QoimiBand), ctypes.POINTER(QoimiBandInfo)
    lib.qoimi_seek_points.restype = ci
    lib.qoimi_seek_points.argtypes = [dp, ctypes.c_uint]
    lib.qoimi_build_seek_index.restype = ci
    lib.qoimi_build_seek_index.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, up, pp, sz, vp]
    lib.qoimi_band_plan.restype = ci
    lib.qoimi_band_plan.argtypes = [dp, ci, ctypes.c_uint, pp, bp, ip]
    lib.qoimi_make_band_streams.restype = ci
    lib.qoimi_make_band_streams.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, up, pp, szp, bp, ci, vp, szp, ip, vp]
    lib.qoimi_decode_crops_indexed.restype = ci
    lib.qoimi_decode_crops_indexed.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, cp, ci, vp, szp, sz, vp, up, pp, szp]
    lib.qoimi_seek_stats.restype = None
    lib.qoimi_seek_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.qoimi_seek_index_from_pixels.restype = ci
    lib.qoimi_seek_index_from_pixels.argtypes = [vp, vp, szp, vp, szp, ctypes.POINTER(ci), dp, ci, up, pp, vp]
    lib.qoimi_decode_resized_indexed.restype = ci
    lib.qoimi_decode_resized_indexed.argtypes = lib.qoimi_decode_resized.argtypes + [up, pp, szp]
    lib.qoimi_decode_bilinear.restype = ci
    lib.qoimi_decode_bilinear.argtypes = lib.qoimi_decode_resized.argtypes
    lib.qoimi_bilinear_size.restype = sz
    lib.qoimi_bilinear_size.argtypes = [dp, rp, ci]
    lib.qoimi_bilinear_stats.restype = None
    lib.qoimi_bilinear_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.qoimi_decode_bilinear_indexed.restype = ci
    lib.qoimi_decode_bilinear_indexed.argtypes = lib.qoimi_decode_resized_indexed.argtypes
    wp = ctypes.POINTER(QoimiWarp)
    lib.qoimi_decode_warped.restype = ci
    lib.qoimi_decode_warped.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, wp, ci, ci, vp, szp, sz, vp]
    lib.qoimi_warp_size.restype = sz
    lib.qoimi_warp_size.argtypes = [dp, wp, ci]
    lib.qoimi_warp_stats.restype = None
    lib.qoimi_warp_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.qoimi_warp_orient.restype = ci
    lib.qoimi_warp_orient.argtypes = [dp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ci, wp]
    lib.qoimi_decode_warped_indexed.restype = ci
    lib.qoimi_decode_warped_indexed.argtypes = lib.qoimi_decode_warped.argtypes + [up, pp, szp]
    tp = ctypes.POINTER(QoimiTensorFormat)
    lib.qoimi_decode_tensors.restype = ci
    lib.qoimi_decode_tensors.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, rp, ci, ci, ci, tp, vp, szp, sz, vp]
    lib.qoimi_decode_warped_tensors.restype = ci
    lib.qoimi_decode_warped_tensors.argtypes = [vp, vp, szp, ctypes.POINTER(ci), dp, ci, ci, wp, ci, ci, tp, vp, szp, sz, vp]
    lib.qoimi_tensor_size.restype = sz
    lib.qoimi_tensor_size.argtypes = [dp, rp, ci, ci, tp]
    lib.qoimi_warp_tensor_size.restype = sz
    lib.qoimi_warp_tensor_size.argtypes = [dp, wp, ci, tp]
    lib.qoimi_tensor_stats.restype = None
    lib.qoimi_tensor_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.qoimi_pixel_stats_indexed.restype = ci
    lib.qoimi_pixel_stats_indexed.argtypes = lib.qoimi_pixel_stats.argtypes + [up, pp, szp]
    _lib = lib
    return lib


def _libc_free(p: int) -> None:
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    libc.free.restype = None
    libc.free(p)


def last_error() -> str:
    return load_library().qoimi_last_error().decode()


def encode_bound(width: int, height: int, channels: int) -> int:
    return int(load_library().qoimi_encode_bound(ctypes.byref(QoiDesc(width, height, channels, 0))))


def thumbnail_size(width: int, height: int, channels_in: int, factor: int, channels: int) -> Tuple[int, int, int]:
    """``qoimi_thumbnail_size`` for an image of width x height x channels_in: (bytes, tw, th) of its thumbnail at `factor` with `channels`
    (3 or 4) bytes per pixel; (0, 0, 0) where the C function returns 0."""
    if not (0 <= factor < 2 ** 32 and 0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0, 0, 0
    tw, th = ctypes.c_uint(0), ctypes.c_uint(0)
    n = int(load_library().qoimi_thumbnail_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), factor, channels, ctypes.byref(tw), ctypes.byref(th)))
    return n, tw.value, th.value


def _crop_array(crops):
    """crops as a ``QoimiCrop`` array: a sequence of such structures or of (image, x, y, width, height, flags) tuples; None if a field
    does not fit an unsigned int."""
    rows = [(c.image, c.x, c.y, c.width, c.height, c.flags) if isinstance(c, QoimiCrop) else tuple(int(v) for v in c) for c in crops]
    if any(len(r) != 6 or any(not 0 <= v < 2 ** 32 for v in r) for r in rows):
        return None
    return (QoimiCrop * len(rows))(*[QoimiCrop(*r) for r in rows])


def crop_size(width: int, height: int, channels_in: int, crop, channels: int) -> int:
    """``qoimi_crop_size`` for an image of width x height x channels_in: the bytes of the output of `crop` (a ``QoimiCrop`` or an (image, x, y,
    width, height, flags) tuple) with `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    arr = _crop_array([crop])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0
    return int(load_library().qoimi_crop_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, channels))


def _tile_array(tiles):
    """tiles as a ``QoimiTile`` array: a sequence of such structures or of (image, x, y, width, height, factor[, flags[, reserved]]) tuples;
    None if a tuple has another length or a field does not fit an unsigned int."""
    rows = [tuple(getattr(t, f) for f, _ in QoimiTile._fields_) if isinstance(t, QoimiTile) else tuple(int(v) for v in t) for t in tiles]
    if any(not 6 <= len(r) <= 8 or any(not 0 <= v < 2 ** 32 for v in r) for r in rows):
        return None
    return (QoimiTile * len(rows))(*[QoimiTile(*r) for r in rows])


def tile_size(width: int, height: int, channels_in: int, tile, channels: int = 0):
    """``qoimi_tile_size`` for an image of width x height x channels_in: (bytes, tw, th) of the pixels of `tile` (a ``QoimiTile`` or an
    (image, x, y, width, height, factor[, flags[, reserved]]) tuple) at `channels` (0: channels_in) bytes per pixel; (0, 0, 0) where the C
    function returns 0."""
    arr = _tile_array([tile])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0, 0, 0
    tw, th = ctypes.c_uint(0), ctypes.c_uint(0)
    n = int(load_library().qoimi_tile_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, channels, ctypes.byref(tw), ctypes.byref(th)))
    return n, tw.value, th.value


def tile_pyramid(width: int, height: int, channels_in: int, tile_w: int, tile_h: int, levels: int):
    """``qoimi_tile_pyramid``: the tiles of a pyramid of `levels` levels over one image as a list of ``QoimiTile`` (image 0), in the order
    level, row, column; ``tiles.pyramid`` states them.  Raises ``QoiError`` where the C function returns QOIMI_E_ARG."""
    ok = all(0 <= int(v) < 2 ** 32 for v in (width, height, tile_w, tile_h, levels)) and 0 <= channels_in < 256
    lib = load_library()
    desc = QoiDesc(width, height, channels_in, 0) if ok else QoiDesc(0, 0, 0, 0)
    n = lib.qoimi_tile_pyramid(ctypes.byref(desc), tile_w if ok else 0, tile_h if ok else 0, levels if ok else 0, None, 0)
    if n < 0:
        raise QoiError("qoimi_tile_pyramid: " + last_error())
    arr = (QoimiTile * n)()
    if lib.qoimi_tile_pyramid(ctypes.byref(desc), tile_w, tile_h, levels, arr, n) != n:
        raise QoiError("qoimi_tile_pyramid: " + last_error())
    return list(arr)


def _resize_array(items):
    """items as a ``QoimiResize`` array: a sequence of such structures or of (image, x, y, width, height, out_width, out_height, flags)
    tuples; None if a field does not fit an unsigned int."""
    rows = [(r.image, r.x, r.y, r.width, r.height, r.out_width, r.out_height, r.flags) if isinstance(r, QoimiResize) else tuple(int(v) for v in r)
            for r in items]
    if any(len(r) != 8 or any(not 0 <= v < 2 ** 32 for v in r) for r in rows):
        return None
    return (QoimiResize * len(rows))(*[QoimiResize(*r) for r in rows])


def resize_size(width: int, height: int, channels_in: int, item, channels: int) -> int:
    """``qoimi_resize_size`` for an image of width x height x channels_in: the bytes of the output of `item` (a ``QoimiResize`` or an (image,
    x, y, width, height, out_width, out_height, flags) tuple) with `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    arr = _resize_array([item])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0
    return int(load_library().qoimi_resize_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, channels))


def bilinear_size(width: int, height: int, channels_in: int, item, channels: int) -> int:
    """``qoimi_bilinear_size`` for an image of width x height x channels_in: the bytes of the output of `item` (as for ``resize_size``) with
    `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    arr = _resize_array([item])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0
    return int(load_library().qoimi_bilinear_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, channels))


_WARP_UNSIGNED = (0, 1, 2, 3, 4, 5, 6, 7, 12, 13)          # of the sixteen fields of a qoimi_warp: unsigned int; 8..11: int; 14, 15: long long


def _warp_array(items):
    """items as a ``QoimiWarp`` array: a sequence of such structures or of the sixteen-field tuples of ``warp.fields``; None if a field does
    not fit its type."""
    names = [f for f, _ in QoimiWarp._fields_]
    rows = [tuple(int(getattr(r, f)) for f in names) if isinstance(r, QoimiWarp) else tuple(int(v) for v in r) for r in items]
    for r in rows:
        if len(r) != 16 or any(not 0 <= r[k] < 2 ** 32 for k in _WARP_UNSIGNED) or any(not -2 ** 31 <= r[k] < 2 ** 31 for k in (8, 9, 10, 11)) or \
                any(not -2 ** 63 <= r[k] < 2 ** 63 for k in (14, 15)):
            return None
    return (QoimiWarp * len(rows))(*[QoimiWarp(*r) for r in rows])


def warp_size(width: int, height: int, channels_in: int, item, channels: int) -> int:
    """``qoimi_warp_size`` for an image of width x height x channels_in: the bytes of the output of `item` (a ``QoimiWarp`` or the tuple of
    ``warp.fields``) with `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    arr = _warp_array([item])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0
    return int(load_library().qoimi_warp_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, channels))


def tensor_format(f) -> "QoimiTensorFormat":
    """f as a ``QoimiTensorFormat``: such a structure, or the (dtype, layout, scale[4], bias[4]) of ``tensors.fmt``."""
    if isinstance(f, QoimiTensorFormat):
        return f
    dtype, layout, scale, bias = f
    if not (0 <= int(dtype) < 2 ** 32 and 0 <= int(layout) < 2 ** 32 and len(scale) == 4 and len(bias) == 4):
        raise QoiError("tensor_format: (dtype, layout, scale[4], bias[4])")
    return QoimiTensorFormat(int(dtype), int(layout), (ctypes.c_float * 4)(*[float(v) for v in scale]), (ctypes.c_float * 4)(*[float(v) for v in bias]))


def tensor_size(width: int, height: int, channels_in: int, item, filter: int, channels: int, f) -> int:
    """``qoimi_tensor_size`` for an image of width x height x channels_in: the bytes of the output of `item` (as for ``resize_size``) under
    `filter` (``tensors.FILTER_AREA`` / ``FILTER_BILINEAR``) with `channels` (3 or 4) elements per pixel in the format f; 0 where the C
    function returns 0."""
    arr = _resize_array([item])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0
    return int(load_library().qoimi_tensor_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, filter, channels, ctypes.byref(tensor_format(f))))


def warp_tensor_size(width: int, height: int, channels_in: int, item, channels: int, f) -> int:
    """``qoimi_warp_tensor_size``: as ``tensor_size`` for an item of ``decode_warped_tensors`` (a ``QoimiWarp`` or the tuple of ``warp.fields``)."""
    arr = _warp_array([item])
    if arr is None or not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256):
        return 0
    return int(load_library().qoimi_warp_tensor_size(ctypes.byref(QoiDesc(width, height, channels_in, 0)), arr, channels, ctypes.byref(tensor_format(f))))


def warp_orient(width: int, height: int, channels_in: int, rect, orientation: int) -> Optional["QoimiWarp"]:
    """``qoimi_warp_orient`` for an image of width x height x channels_in: the item (image 0) that shows rect (x, y, width, height) in the
    EXIF orientation 1..8; None where the C function returns an error."""
    if not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256 and all(0 <= int(v) < 2 ** 32 for v in rect) and
            -2 ** 31 <= orientation < 2 ** 31):
        return None
    out = QoimiWarp()
    x, y, w, h = (int(v) for v in rect)
    rc = load_library().qoimi_warp_orient(ctypes.byref(QoiDesc(width, height, channels_in, 0)), x, y, w, h, orientation, ctypes.byref(out))
    return out if rc == 0 else None


def seek_points(width: int, height: int, channels_in: int, interval_rows: int) -> int:
    """``qoimi_seek_points`` for an image of width x height x channels_in: ceil(height / interval_rows) - 1, or -1 where the C function
    returns -1 (a rejected descriptor, interval_rows == 0, interval_rows * width < 128)."""
    if not (0 <= width < 2 ** 32 and 0 <= height < 2 ** 32 and 0 <= channels_in < 256 and 0 <= interval_rows < 2 ** 32):
        return -1
    return int(load_library().qoimi_seek_points(ctypes.byref(QoiDesc(width, height, channels_in, 0)), interval_rows))


def _point_array(points):
    """An index as a ``QoimiSeekPoint`` array and its length: such an array, or a numpy array of ``seekindex.POINT_DTYPE`` (copied)."""
    if isinstance(points, ctypes.Array):
        return points, len(points)
    from .seekindex import POINT_DTYPE
    a = np.ascontiguousarray(points, dtype=POINT_DTYPE).reshape(-1)
    arr = (QoimiSeekPoint * max(a.size, 1))()
    ctypes.memmove(arr, a.ctypes.data, a.nbytes)
    return arr, a.size


def band_plan(desc: QoiDesc, size: int, interval_rows: int, points, first_row: int, rows: int) -> Optional[QoimiBandInfo]:
    """``qoimi_band_plan``: what the band stream of rows [first_row, first_row + rows) of an image will be, from the image's points (a
    ``QoimiSeekPoint`` array or a numpy array of ``seekindex.POINT_DTYPE``) alone; None where the C function returns QOIMI_E_ARG."""
    if not all(0 <= int(v) < 2 ** 32 for v in (interval_rows, first_row, rows)) or not -2 ** 31 <= int(size) < 2 ** 31:
        return None
    arr, _ = _point_array(points)
    out = QoimiBandInfo()
    rc = load_library().qoimi_band_plan(ctypes.byref(desc), int(size), int(interval_rows), arr, ctypes.byref(QoimiBand(0, int(first_row), int(rows), 0)), ctypes.byref(out))
    return out if rc == 0 else None


# ----------------------------------------------------------------------------------
# drop-in functions on host memory
# ----------------------------------------------------------------------------------
def qoi_encode(data, desc: QoiDesc) -> Optional[bytes]:
    """``qoi_encode`` (qoi.h:278): raw RGB/RGBA bytes + desc -> QOI stream, ``None`` on failure."""
    lib = load_library()
    arr = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray))
                               else np.asarray(data, dtype=np.uint8))
    # the C function cannot know how long `data` is (qoi.h:278 trusts width*height*channels); this wrapper can: a short
    # buffer would make the copy engine read past the allocation
    if _desc_plausible(desc) and arr.size < desc.width * desc.height * desc.channels:
        return None
    n = ctypes.c_int(0)
    p = lib.qoi_encode(arr.ctypes.data, ctypes.byref(desc), ctypes.byref(n))
    if not p:
        return None
    try:
        return ctypes.string_at(p, n.value)
    finally:
        _libc_free(p)


def _desc_plausible(desc: QoiDesc) -> bool:
    """qoi.h:364-372's rules - only where they hold does width*height*channels say how many bytes the codec will read."""
    return (desc.width > 0 and desc.height > 0 and desc.channels in (3, 4) and desc.colorspace <= 1
            and desc.height < 400000000 // desc.width)


def qoi_decode(data: bytes, channels: int = 0, size: Optional[int] = None
               ) -> Tuple[Optional[np.ndarray], QoiDesc]:
    """``qoi_decode`` (qoi.h:289): QOI stream -> (pixels uint8[w*h*channels] or ``None``, desc)."""
    lib = load_library()
    buf = (ctypes.c_ubyte * max(len(data), 1)).from_buffer_copy(bytes(data).ljust(1, b"\0"))
    desc = QoiDesc()
    p = lib.qoi_decode(ctypes.addressof(buf), len(data) if size is None else size, ctypes.byref(desc), channels)
    if not p:
        return None, desc
    try:
        och = channels if channels else desc.channels
        return np.frombuffer(ctypes.string_at(p, desc.width * desc.height * och), dtype=np.uint8).copy(), desc
    finally:
        _libc_free(p)


def qoi_write(filename: str, data, desc: QoiDesc) -> int:
    """``qoi_write`` (qoi.h:252): returns bytes written, 0 on failure."""
    arr = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    if _desc_plausible(desc) and arr.size < desc.width * desc.height * desc.channels:
        return 0                                     # short pixel buffer: as a failed qoi_write (qoi.h:259-263)
    return int(load_library().qoi_write(filename.encode(), arr.ctypes.data, ctypes.byref(desc)))


def qoi_read(filename: str, channels: int = 0) -> Tuple[Optional[np.ndarray], QoiDesc]:
    """``qoi_read`` (qoi.h:265)."""
    lib = load_library()
    desc = QoiDesc()
    p = lib.qoi_read(filename.encode(), ctypes.byref(desc), channels)
    if not p:
        return None, desc
    try:
        och = channels if channels else desc.channels
        return np.frombuffer(ctypes.string_at(p, desc.width * desc.height * och), dtype=np.uint8).copy(), desc
    finally:
        _libc_free(p)


# ----------------------------------------------------------------------------------
# device-resident batch API
# ----------------------------------------------------------------------------------
class Context:
    """One GPU + workspace (``qoimi_ctx``).  Pointers are raw device addresses (ints)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.qoimi_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise QoiError(f"qoimi_ctx_create({device}) failed ({rc}): {last_error()}")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.qoimi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise QoiError(f"{what} failed ({rc}): {last_error()}")

    def encode_batch(self, d_pixels: int, pixel_stride: int, desc: QoiDesc, n_images: int,
                     d_streams: int, stream_stride: int, d_stream_len: int, stream: int = 0) -> None:
        self._check(self._lib.qoimi_encode_batch(self._h, d_pixels, pixel_stride, ctypes.byref(desc), n_images,
                                                 d_streams, stream_stride, d_stream_len, stream), "qoimi_encode_batch")

    def encode_images(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], d_streams: int,
                      stream_offsets: Sequence[int], d_stream_len: int, stream: int = 0) -> None:
        """Images of different shapes / channel counts in one call (``qoimi_encode_images``)."""
        n = len(descs)
        if len(pixel_offsets) != n or len(stream_offsets) != n:
            raise QoiError("encode_images: one pixel offset and one stream offset per descriptor")
        po = (ctypes.c_size_t * n)(*[int(x) for x in pixel_offsets])
        so = (ctypes.c_size_t * n)(*[int(x) for x in stream_offsets])
        self._check(self._lib.qoimi_encode_images(self._h, d_pixels, po, (QoiDesc * n)(*descs), n, d_streams, so, d_stream_len, stream), "qoimi_encode_images")

    def encode_status(self, stream: int = 0) -> None:
        self._check(self._lib.qoimi_encode_status(self._h, stream), "qoimi_encode_status")

    def encode_suspect_calls(self) -> int:
        """Encode calls of this context made with the exchange probe since the last passed LDS-order check when a repeat failed (0: never)."""
        return int(self._lib.qoimi_encode_suspect_calls(self._h))

    def set_encode_small_call_order(self, by_workgroup_index: bool) -> None:
        """Calls of fewer than 8 images: units by ticket (default, safe on a shared device) or by workgroup index (4 us less per 4K
        frame; then ``encode_status`` must be called before the streams are read)."""
        self._check(self._lib.qoimi_set_encode_small_call_order(self._h, 1 if by_workgroup_index else 0), "qoimi_set_encode_small_call_order")

    def encode_retries(self) -> int:
        """Calls ``encode_status`` encoded again order-free because a placement wait had given up (0: never)."""
        return int(self._lib.qoimi_encode_retries(self._h))

    def decode_batch(self, d_streams: int, stream_stride: int, sizes: Sequence[int], descs: Sequence[QoiDesc],
                     channels: int, d_pixels: int, pixel_stride: int, stream: int = 0) -> None:
        n = len(sizes)
        if len(descs) != n:
            raise QoiError(f"decode_batch: {n} sizes but {len(descs)} descriptors")
        if isinstance(sizes, ctypes.Array) and isinstance(descs, ctypes.Array):
            c_sizes, c_descs = sizes, descs               # the caller's own C arrays (int[n], qoi_desc[n]): handed through as they are
        else:
            if n > 1 and any(int(sz) > stream_stride for sz in sizes):
                raise QoiError("decode_batch: a stream is longer than stream_stride")
            c_sizes = (ctypes.c_int * n)(*[int(s) for s in sizes])
            c_descs = (QoiDesc * n)(*descs)
        self._check(self._lib.qoimi_decode_batch(self._h, d_streams, stream_stride, c_sizes, c_descs, n, channels,
                                                 d_pixels, pixel_stride, stream), "qoimi_decode_batch")

    def decode_images(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc],
                      channels: int, d_pixels: int, pixel_offsets: Sequence[int], stream: int = 0) -> None:
        """Streams and images at per-image byte offsets, any order (``qoimi_decode_images``): image i is written tightly packed."""
        n = len(sizes)
        if len(descs) != n or len(stream_offsets) != n or len(pixel_offsets) != n:
            raise QoiError("decode_images: one stream offset, size, descriptor and pixel offset per image")
        so = (ctypes.c_size_t * n)(*[int(x) for x in stream_offsets])
        po = (ctypes.c_size_t * n)(*[int(x) for x in pixel_offsets])
        self._check(self._lib.qoimi_decode_images(self._h, d_streams, so, (ctypes.c_int * n)(*[int(x) for x in sizes]), (QoiDesc * n)(*descs),
                                                  n, channels, d_pixels, po, stream), "qoimi_decode_images")

    def pack_streams(self, d_streams: int, stream_stride: int, d_stream_len: int, n_streams: int, align: int,
                     d_packed: int, packed_capacity: int, d_packed_off: int, stream: int = 0) -> None:
        """Strided streams -> back to back at d_packed; d_packed_off: device uint64[n_streams + 1] (``qoimi_pack_streams``, asynchronous)."""
        self._check(self._lib.qoimi_pack_streams(self._h, d_streams, stream_stride, d_stream_len, n_streams, align,
                                                 d_packed, packed_capacity, d_packed_off, stream), "qoimi_pack_streams")

    def encode_packed(self, d_pixels: int, pixel_stride: int, desc: QoiDesc, n_images: int, align: int, d_packed: int, packed_capacity: int,
                      d_packed_off: int, d_stream_len: int, staging_bytes: int = 0, stream: int = 0):
        """Pixels -> pack in one call through bounded staging (``qoimi_encode_packed``, synchronous): (offsets uint64[n + 1], sizes
        int32[n]) as numpy arrays - offsets[:n] and sizes are what ``read_descs`` / ``decode_images`` / ``inspect_streams`` take,
        offsets[n] the bytes the pack needs (larger than packed_capacity: the streams that did not fit wholly are absent)."""
        off, sizes = np.zeros(n_images + 1, dtype=np.uint64), np.zeros(n_images, dtype=np.intc)
        self._check(self._lib.qoimi_encode_packed(self._h, d_pixels, pixel_stride, ctypes.byref(desc), n_images, align, d_packed, packed_capacity,
                                                  d_packed_off, d_stream_len, staging_bytes, off.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                                                  sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), stream), "qoimi_encode_packed")
        return off, sizes

    def encode_images_packed(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], align: int, d_packed: int,
                             packed_capacity: int, d_packed_off: int, d_stream_len: int, staging_bytes: int = 0, stream: int = 0):
        """The same for images of different shapes / channel counts (``qoimi_encode_images_packed``)."""
        n = len(descs)
        if len(pixel_offsets) != n:
            raise QoiError("encode_images_packed: one pixel offset per descriptor")
        po = (ctypes.c_size_t * n)(*[int(x) for x in pixel_offsets])
        off, sizes = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.intc)
        self._check(self._lib.qoimi_encode_images_packed(self._h, d_pixels, po, (QoiDesc * n)(*descs), n, align, d_packed, packed_capacity,
                                                         d_packed_off, d_stream_len, staging_bytes, off.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                                                         sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), stream), "qoimi_encode_images_packed")
        return off, sizes

    def encode_tiles(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], channels: int, tiles, mode: int, align: int,
                     d_packed: int, packed_capacity: int, d_packed_off: int, d_stream_len: int, staging_bytes: int = 0, stream: int = 0):
        """Tiles and pyramid levels of device images -> pack in one call through bounded staging (``qoimi_encode_tiles``, synchronous):
        (offsets uint64[n + 1], sizes int32[n], tile descriptors) - what ``decode_images`` and the gather calls take to serve the pack.
        tiles: ``QoimiTile`` structures or (image, x, y, width, height, factor[, flags]) tuples; mode: ``tiles.PLAIN`` /
        ``tiles.ALPHA_WEIGHTED``; channels 0: every tile keeps its image's channel count; ``qoi_amd/tiles.py: tile`` states the pixels."""
        n_images = len(descs)
        if len(pixel_offsets) != n_images:
            raise QoiError("encode_tiles: one pixel offset per descriptor")
        arr = _tile_array(tiles)
        if arr is None:
            raise QoiError("encode_tiles: a tile is (image, x, y, width, height, factor[, flags[, reserved]]) of unsigned 32-bit values")
        n = len(arr)
        po = (ctypes.c_size_t * max(n_images, 1))(*[int(x) for x in pixel_offsets])
        off, sizes = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.intc)
        tds = (QoiDesc * max(n, 1))()
        self._check(self._lib.qoimi_encode_tiles(self._h, d_pixels, po, (QoiDesc * max(n_images, 1))(*descs), n_images, channels, arr, n, mode, align,
                                                 d_packed, packed_capacity, d_packed_off, d_stream_len, staging_bytes,
                                                 off.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                 tds, stream), "qoimi_encode_tiles")
        return off, sizes, list(tds)[:n]

    def tile_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``encode_tiles`` call: (sub-batches, launches of the gather kernel, bytes of staging planned, images referenced)."""
        return self._four_counters(self._lib.qoimi_tile_stats)

    def read_descs(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], stream: int = 0):
        """The headers of the streams of a pack: (descs, first_bad) - first_bad is None when every stream passes the rules of
        qoi.h:497-521, else the lowest failing index (``qoimi_read_descs`` then returns QOIMI_E_ARG; the descriptors are filled anyway)."""
        n = len(sizes)
        if len(stream_offsets) != n:
            raise QoiError("read_descs: one stream offset per size")
        so = (ctypes.c_size_t * n)(*[int(x) for x in stream_offsets])
        descs = (QoiDesc * n)()
        bad = ctypes.c_int(-1)
        rc = self._lib.qoimi_read_descs(self._h, d_streams, so, (ctypes.c_int * n)(*[int(x) for x in sizes]), n, descs, ctypes.byref(bad), stream)
        if rc != 0 and bad.value < 0:
            self._check(rc, "qoimi_read_descs")
        return list(descs), (bad.value if bad.value >= 0 else None)

    def inspect_streams(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], stream: int = 0):
        """Chunk statistics and strict checks of the streams of a pack (``qoimi_inspect_streams``): (infos, first_flagged) - infos is a
        numpy array of ``streaminfo.INFO_DTYPE``, first_flagged the lowest index with flags != 0 or None."""
        from .streaminfo import INFO_DTYPE
        n = len(sizes)
        if len(stream_offsets) != n:
            raise QoiError("inspect_streams: one stream offset per size")
        so = np.ascontiguousarray(stream_offsets, dtype=np.uintp)
        sz = np.ascontiguousarray(sizes, dtype=np.intc)
        infos = np.zeros(n, dtype=INFO_DTYPE)
        first = ctypes.c_int(-1)
        self._check(self._lib.qoimi_inspect_streams(self._h, d_streams, so.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                                    sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n,
                                                    infos.ctypes.data_as(ctypes.POINTER(StreamInfo)), ctypes.byref(first), stream), "qoimi_inspect_streams")
        return infos, (first.value if first.value >= 0 else None)

    def compare_images(self, d_a: int, a_offsets: Sequence[int], a_channels: int, d_b: int, b_offsets: Sequence[int], b_channels: int,
                       descs: Sequence[QoiDesc], stream: int = 0):
        """Two sets of device images, pixel by pixel (``qoimi_compare_images``): (diffs, first_diff) - diffs is a numpy array of
        ``imagediff.DIFF_DTYPE``, first_diff the lowest index with flags != 0 or -1, as the C call gives it.  a_channels / b_channels: bytes per pixel of a side,
        0 for each image's ``descs[i].channels``."""
        from .imagediff import DIFF_DTYPE
        n = len(descs)
        if len(a_offsets) != n or len(b_offsets) != n:
            raise QoiError("compare_images: one offset per side and descriptor")
        ao = np.ascontiguousarray(a_offsets, dtype=np.uintp)
        bo = np.ascontiguousarray(b_offsets, dtype=np.uintp)
        diffs = np.zeros(n, dtype=DIFF_DTYPE)
        first = ctypes.c_int(-1)
        szp = ctypes.POINTER(ctypes.c_size_t)
        self._check(self._lib.qoimi_compare_images(self._h, d_a, ao.ctypes.data_as(szp), a_channels, d_b, bo.ctypes.data_as(szp), b_channels,
                                                   (QoiDesc * n)(*descs), n, diffs.ctypes.data_as(ctypes.POINTER(ImageDiff)),
                                                   ctypes.byref(first), stream), "qoimi_compare_images")
        return diffs, first.value

    def verify_images(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], d_streams: int,
                      stream_offsets: Sequence[int], sizes: Sequence[int], staging_bytes: int = 0, stream: int = 0):
        """Do the streams decode back to exactly these pixels (``qoimi_verify_images``, synchronous, through bounded staging)?
        (diffs, first_diff) as ``compare_images`` gives them; a stream whose header does not match its descriptor is flagged
        ``imagediff.DIFF_HEADER`` and not decoded."""
        from .imagediff import DIFF_DTYPE
        n = len(descs)
        if len(pixel_offsets) != n or len(stream_offsets) != n or len(sizes) != n:
            raise QoiError("verify_images: one pixel offset, stream offset and size per descriptor")
        po = np.ascontiguousarray(pixel_offsets, dtype=np.uintp)
        so = np.ascontiguousarray(stream_offsets, dtype=np.uintp)
        sz = np.ascontiguousarray(sizes, dtype=np.intc)
        diffs = np.zeros(n, dtype=DIFF_DTYPE)
        first = ctypes.c_int(-1)
        szp = ctypes.POINTER(ctypes.c_size_t)
        self._check(self._lib.qoimi_verify_images(self._h, d_pixels, po.ctypes.data_as(szp), (QoiDesc * n)(*descs), n, d_streams,
                                                  so.ctypes.data_as(szp), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), staging_bytes,
                                                  diffs.ctypes.data_as(ctypes.POINTER(ImageDiff)), ctypes.byref(first), stream),
                    "qoimi_verify_images")
        return diffs, first.value

    def decode_thumbnails(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                          factors, mode: int, d_thumbs: int, thumb_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Every image of a pack at 1/f of its size (``qoimi_decode_thumbnails``, synchronous, through bounded staging): thumbnail i is
        written tightly packed at d_thumbs + thumb_offsets[i].  factors: one int for all images or one per image, each 1..64;
        mode: ``thumbs.PLAIN`` or ``thumbs.ALPHA_WEIGHTED``; ``qoi_amd/thumbs.py: thumbnail`` states the result."""
        n = len(sizes)
        if isinstance(factors, (int, np.integer)):
            factors = [int(factors)] * n
        if len(descs) != n or len(stream_offsets) != n or len(thumb_offsets) != n or len(factors) != n:
            raise QoiError("decode_thumbnails: one stream offset, size, descriptor, factor and thumbnail offset per image")
        if any(not 0 <= int(f) < 2 ** 32 for f in factors):
            raise QoiError("decode_thumbnails: a factor outside 1..64")
        n, ds, _, (so, sz, to), keep = self._gather_args("decode_thumbnails", stream_offsets, sizes, descs, thumb_offsets)
        fs = np.ascontiguousarray(factors, dtype=np.uintc)
        self._check(self._lib.qoimi_decode_thumbnails(self._h, d_streams, so, sz, ds, n, channels, fs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), mode,
                                                      d_thumbs, to, staging_bytes, stream), "qoimi_decode_thumbnails")
        del keep

    def thumbnail_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_thumbnails`` call: (sub-batches decoded, launches of the reduction kernel, bytes of staging planned, 0)."""
        return self._four_counters(self._lib.qoimi_thumbnail_stats)

    def decode_crops(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                     crops, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Rectangles of a pack's images (``qoimi_decode_crops``, synchronous, through bounded staging): output j is written tightly packed at
        d_out + out_offsets[j].  crops: ``QoimiCrop`` structures or (image, x, y, width, height, flags) tuples, flags of ``crops.FLIP_X`` /
        ``crops.FLIP_Y``; an image no crop names is not decoded; ``qoi_amd/crops.py: crop`` states the result."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_crops", stream_offsets, sizes, descs, out_offsets, crops=crops)
        self._check(self._lib.qoimi_decode_crops(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), d_out, oo, staging_bytes, stream), "qoimi_decode_crops")
        del keep

    def crop_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_crops`` call: (sub-batches decoded, launches of the gather kernel, bytes of staging planned, images decoded)."""
        return self._four_counters(self._lib.qoimi_crop_stats)

    def decode_resized(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                       items, mode: int, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Rectangles of a pack's images resampled to fixed sizes (``qoimi_decode_resized``, synchronous, through bounded staging): output j
        is written tightly packed at d_out + out_offsets[j].  items: ``QoimiResize`` structures or (image, x, y, width, height, out_width,
        out_height, flags) tuples, flags of ``resize.FLIP_X`` / ``resize.FLIP_Y``; mode: ``resize.PLAIN`` or ``resize.ALPHA_WEIGHTED``; an image
        no item names is not decoded; ``qoi_amd/resize.py: resize`` states the result."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_resized", stream_offsets, sizes, descs, out_offsets, items=items)
        self._check(self._lib.qoimi_decode_resized(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, d_out, oo, staging_bytes, stream), "qoimi_decode_resized")
        del keep

    def resize_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_resized`` call: (sub-batches decoded, launches of the filter kernel, bytes of staging planned, images decoded)."""
        return self._four_counters(self._lib.qoimi_resize_stats)

    def _gather_args(self, what: str, stream_offsets, sizes, descs, out_offsets=None, items=None, crops=None, noun: str = "crop", warps=None):
        """What the gather calls and their indexed forms make of their sequences: (n, descriptor array, item array or None - of ``items``
        (``QoimiResize``), of ``warps`` (``QoimiWarp``) or of ``crops`` (``QoimiCrop``, called ``noun`` in messages) -, pointers (stream
        offsets, sizes, output offsets or None), arrays to keep alive)."""
        n = len(sizes)
        if len(descs) != n or len(stream_offsets) != n:
            raise QoiError(what + ": one stream offset, size and descriptor per image")
        given, noun = (items, "item") if items is not None else (warps, "item") if warps is not None else (crops, noun)
        if out_offsets is not None and given is not None and len(out_offsets) != len(given):
            raise QoiError(what + ": one output offset per " + noun)
        arr = None
        if warps is not None and items is None:
            arr = _warp_array(warps)
            if arr is None:
                raise QoiError(what + ": an item is not the sixteen fields of a qoimi_warp")
        elif given is not None:
            arr = _resize_array(items) if items is not None else _crop_array(crops)
            if arr is None:
                raise QoiError(what + (": an item is not eight" if items is not None else ": a " + noun + " is not six") + " unsigned 32-bit fields")
        so = np.ascontiguousarray(stream_offsets, dtype=np.uintp)
        sz = np.ascontiguousarray(sizes, dtype=np.intc)
        oo = np.ascontiguousarray(out_offsets, dtype=np.uintp) if out_offsets is not None else None
        szp = ctypes.POINTER(ctypes.c_size_t)
        return n, (QoiDesc * n)(*descs), arr, (so.ctypes.data_as(szp), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                               oo.ctypes.data_as(szp) if oo is not None else None), (so, sz, oo)

    def _four_counters(self, getter) -> Tuple[int, int, int, int]:
        """The four counters a ``qoimi_*_stats`` function writes for this context."""
        out = (ctypes.c_longlong * 4)()
        getter(self._h, out)
        return tuple(int(x) for x in out)

    def decode_bilinear(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                        items, mode: int, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_resized`` with the antialiased bilinear (triangle) filter (``qoimi_decode_bilinear``, synchronous, through bounded
        staging): the same items, modes, flips and outputs; a rectangle is reduced by at most 32 per axis and
        max(width, out_width) * max(height, out_height) stays below 2**30; ``qoi_amd/bilinear.py: bilinear`` states the result."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_bilinear", stream_offsets, sizes, descs, out_offsets, items=items)
        self._check(self._lib.qoimi_decode_bilinear(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, d_out, oo, staging_bytes, stream), "qoimi_decode_bilinear")
        del keep

    def bilinear_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_bilinear`` call: (sub-batches decoded, launches of the filter kernel, bytes of staging planned, images decoded)."""
        return self._four_counters(self._lib.qoimi_bilinear_stats)

    def decode_warped(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                      items, mode: int, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Rectangles of a pack's images sampled through an affine map with bilinear weights (``qoimi_decode_warped``, synchronous, through
        bounded staging): output j is written tightly packed at d_out + out_offsets[j].  items: ``QoimiWarp`` structures or the tuples of
        ``warp.fields`` (``warp.item`` makes one); mode: ``warp.PLAIN`` or ``warp.ALPHA_WEIGHTED``; an image no item names is not decoded;
        ``qoi_amd/warp.py: warp`` states the result."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_warped", stream_offsets, sizes, descs, out_offsets, warps=items)
        self._check(self._lib.qoimi_decode_warped(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, d_out, oo, staging_bytes, stream), "qoimi_decode_warped")
        del keep

    def warp_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_warped`` call: (sub-batches decoded, launches of the warp kernel, bytes of staging planned, images decoded)."""
        return self._four_counters(self._lib.qoimi_warp_stats)

    def decode_tensors(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                       items, filter: int, mode: int, f, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_resized`` (filter ``tensors.FILTER_AREA``) or ``decode_bilinear`` (``tensors.FILTER_BILINEAR``) with the outputs written
        as tensors (``qoimi_decode_tensors``, synchronous, through bounded staging): f is a ``QoimiTensorFormat`` or the tuple of
        ``tensors.fmt`` - u8, f16, bf16 or f32 elements, HWC or CHW, each channel scaled and shifted; every d_out + out_offsets[j] is a
        multiple of the element size; ``qoi_amd/tensors.py: tensors`` states the result."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_tensors", stream_offsets, sizes, descs, out_offsets, items=items)
        tf = tensor_format(f)
        self._check(self._lib.qoimi_decode_tensors(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), filter, mode, ctypes.byref(tf), d_out, oo, staging_bytes, stream),
                    "qoimi_decode_tensors")
        del keep

    def decode_warped_tensors(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                              items, mode: int, f, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_warped`` with the outputs written as tensors (``qoimi_decode_warped_tensors``): f and the outputs as for
        ``decode_tensors``; ``qoi_amd/tensors.py: warped_tensors`` states the result."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_warped_tensors", stream_offsets, sizes, descs, out_offsets, warps=items)
        tf = tensor_format(f)
        self._check(self._lib.qoimi_decode_warped_tensors(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, ctypes.byref(tf), d_out, oo, staging_bytes, stream),
                    "qoimi_decode_warped_tensors")
        del keep

    def tensor_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_tensors`` or ``decode_warped_tensors`` call: (sub-batches decoded, launches of the tensor kernel, bytes of
        staging planned, images decoded)."""
        return self._four_counters(self._lib.qoimi_tensor_stats)

    def pixel_stats(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], regions,
                    d_hist: int = 0, staging_bytes: int = 0, stream: int = 0) -> List[QoimiPixelStat]:
        """Pixel statistics of rectangles of a pack's images (``qoimi_pixel_stats``, synchronous, through bounded staging): one
        ``QoimiPixelStat`` per region.  regions: ``QoimiCrop`` structures or (image, x, y, width, height, flags) tuples; d_hist: 0, or device
        memory of 4096 bytes per region that receives uint32[n_regions][4][256]; an image no region names is not decoded;
        ``qoi_amd/pixelstats.py: stats`` states the result."""
        n, ds, arr, (so, sz, _), keep = self._gather_args("pixel_stats", stream_offsets, sizes, descs, crops=regions, noun="region")
        out = (QoimiPixelStat * max(len(arr), 1))()
        self._check(self._lib.qoimi_pixel_stats(self._h, d_streams, so, sz, ds, n, arr, len(arr), out, d_hist or None, staging_bytes, stream), "qoimi_pixel_stats")
        del keep
        return list(out)[:len(arr)]

    def pixel_stats_counters(self) -> Tuple[int, int, int, int]:
        """Of the last ``pixel_stats`` call: (sub-batches decoded, launches of the reduction kernel, bytes of staging planned, images decoded)."""
        return self._four_counters(self._lib.qoimi_pixel_stats_counters)

    def build_seek_index(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc],
                         interval_rows, staging_bytes: int = 0, stream: int = 0):
        """The seek points of every image of a pack (``qoimi_build_seek_index``, synchronous: one inspect plus one full decode): (points,
        point_firsts) - points a numpy array of ``seekindex.POINT_DTYPE``, the images' points back to back, image i's from point_firsts[i]
        on.  interval_rows: one int for all images or one per image, each with interval_rows * width >= 128; ``qoi_amd/seekindex.py:
        points`` states the result."""
        from .seekindex import POINT_DTYPE
        n = len(sizes)
        if isinstance(interval_rows, (int, np.integer)):
            interval_rows = [int(interval_rows)] * n
        if len(descs) != n or len(stream_offsets) != n or len(interval_rows) != n:
            raise QoiError("build_seek_index: one stream offset, size, descriptor and interval per image")
        counts = [seek_points(d.width, d.height, d.channels, int(k)) for d, k in zip(descs, interval_rows)]
        if any(k < 0 for k in counts):
            raise QoiError("build_seek_index: a rejected descriptor or interval_rows * width < 128")
        firsts = [int(x) for x in np.cumsum([0] + counts[:-1])]
        points = np.zeros(sum(counts), dtype=POINT_DTYPE)
        room = points if points.size else np.zeros(1, dtype=POINT_DTYPE)
        so = np.ascontiguousarray(stream_offsets, dtype=np.uintp)
        sz = np.ascontiguousarray(sizes, dtype=np.intc)
        ks = np.ascontiguousarray(interval_rows, dtype=np.uintc)
        self._check(self._lib.qoimi_build_seek_index(self._h, d_streams, so.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                     (QoiDesc * n)(*descs), n, ks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                                     room.ctypes.data_as(ctypes.POINTER(QoimiSeekPoint)), staging_bytes, stream), "qoimi_build_seek_index")
        return points, firsts

    def make_band_streams(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], interval_rows,
                          points, point_firsts: Sequence[int], bands, d_out: int, out_offsets: Sequence[int], stream: int = 0) -> List[QoimiBandInfo]:
        """Band streams written on the device (``qoimi_make_band_streams``, synchronous): band stream j at d_out + out_offsets[j]; returns
        one ``QoimiBandInfo`` per band.  bands: ``QoimiBand`` structures or (image, first_row, rows) tuples; points, point_firsts: as
        ``build_seek_index`` returns them; ``qoi_amd/seekindex.py: band_stream`` states the result."""
        n = len(sizes)
        if isinstance(interval_rows, (int, np.integer)):
            interval_rows = [int(interval_rows)] * n
        if len(descs) != n or len(stream_offsets) != n or len(interval_rows) != n or len(point_firsts) != n:
            raise QoiError("make_band_streams: one stream offset, size, descriptor, interval and first point per image")
        if len(out_offsets) != len(bands):
            raise QoiError("make_band_streams: one output offset per band")
        rows = [(b.image, b.first_row, b.rows) if isinstance(b, QoimiBand) else tuple(int(v) for v in b) for b in bands]
        if any(len(r) != 3 or any(not 0 <= v < 2 ** 32 for v in r) for r in rows):
            raise QoiError("make_band_streams: a band is not three unsigned 32-bit fields")
        arr = (QoimiBand * max(len(rows), 1))(*[QoimiBand(r[0], r[1], r[2], 0) for r in rows])
        pts, _ = _point_array(points)
        infos = (QoimiBandInfo * max(len(rows), 1))()
        so = np.ascontiguousarray(stream_offsets, dtype=np.uintp)
        oo = np.ascontiguousarray(out_offsets, dtype=np.uintp)
        pf = np.ascontiguousarray(point_firsts, dtype=np.uintp)
        sz = np.ascontiguousarray(sizes, dtype=np.intc)
        ks = np.ascontiguousarray(interval_rows, dtype=np.uintc)
        szp = ctypes.POINTER(ctypes.c_size_t)
        self._check(self._lib.qoimi_make_band_streams(self._h, d_streams, so.ctypes.data_as(szp), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), (QoiDesc * n)(*descs), n,
                                                      ks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), pts, pf.ctypes.data_as(szp), arr, len(rows), d_out,
                                                      oo.ctypes.data_as(szp), infos, stream), "qoimi_make_band_streams")
        return list(infos)[:len(rows)]

    def decode_crops_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                             crops, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                             staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_crops`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost crop
        (``qoimi_decode_crops_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``crop_stats`` then holds the counters of the inner call over the band streams."""
        n = len(sizes)
        if isinstance(interval_rows, (int, np.integer)):
            interval_rows = [int(interval_rows)] * n
        if len(descs) != n or len(stream_offsets) != n or len(interval_rows) != n or len(point_firsts) != n:
            raise QoiError("decode_crops_indexed: one stream offset, size, descriptor, interval and first point per image")
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_crops_indexed", stream_offsets, sizes, descs, out_offsets, crops=crops)
        index, keep_index = self._index_args("decode_crops_indexed", n, interval_rows, points, point_firsts)
        self._check(self._lib.qoimi_decode_crops_indexed(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), d_out, oo, staging_bytes, stream, *index),
                    "qoimi_decode_crops_indexed")
        del keep, keep_index

    def seek_index_from_pixels(self, d_pixels: int, pixel_offsets: Sequence[int], d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int],
                               descs: Sequence[QoiDesc], interval_rows, stream: int = 0):
        """``build_seek_index`` for whoever holds the pixels the pack was encoded from (``qoimi_seek_index_from_pixels``, synchronous: one
        inspect and two kernels over the pixels, no decode, no staging): image i is width * height * channels bytes at d_pixels +
        pixel_offsets[i], any byte offset.  Returns (points, point_firsts) as ``build_seek_index`` does; that stream i decodes to those
        pixels is not checked (``verify_images`` does that); ``qoi_amd/seekindex.py: points_from_pixels`` states the result."""
        from .seekindex import POINT_DTYPE
        n = len(sizes)
        if isinstance(interval_rows, (int, np.integer)):
            interval_rows = [int(interval_rows)] * n
        if len(descs) != n or len(stream_offsets) != n or len(interval_rows) != n or len(pixel_offsets) != n:
            raise QoiError("seek_index_from_pixels: one pixel offset, stream offset, size, descriptor and interval per image")
        counts = [seek_points(d.width, d.height, d.channels, int(k)) for d, k in zip(descs, interval_rows)]
        if any(k < 0 for k in counts):
            raise QoiError("seek_index_from_pixels: a rejected descriptor or interval_rows * width < 128")
        firsts = [int(x) for x in np.cumsum([0] + counts[:-1])]
        points = np.zeros(sum(counts), dtype=POINT_DTYPE)
        room = points if points.size else np.zeros(1, dtype=POINT_DTYPE)
        po = np.ascontiguousarray(pixel_offsets, dtype=np.uintp)
        so = np.ascontiguousarray(stream_offsets, dtype=np.uintp)
        sz = np.ascontiguousarray(sizes, dtype=np.intc)
        ks = np.ascontiguousarray(interval_rows, dtype=np.uintc)
        szp = ctypes.POINTER(ctypes.c_size_t)
        self._check(self._lib.qoimi_seek_index_from_pixels(self._h, d_pixels, po.ctypes.data_as(szp), d_streams, so.ctypes.data_as(szp),
                                                           sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), (QoiDesc * n)(*descs), n,
                                                           ks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), room.ctypes.data_as(ctypes.POINTER(QoimiSeekPoint)),
                                                           stream), "qoimi_seek_index_from_pixels")
        return points, firsts

    def _index_args(self, what: str, n: int, interval_rows, points, point_firsts):
        """(interval_rows, points, point_firsts) as the three trailing arguments of an indexed call; the arrays are kept alive by the tuple."""
        if isinstance(interval_rows, (int, np.integer)):
            interval_rows = [int(interval_rows)] * n
        if len(interval_rows) != n or len(point_firsts) != n:
            raise QoiError(what + ": one interval and first point per image")
        pts, _ = _point_array(points)
        pf = np.ascontiguousarray(point_firsts, dtype=np.uintp)
        ks = np.ascontiguousarray(interval_rows, dtype=np.uintc)
        return (ks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), pts, pf.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))), (ks, pts, pf)

    def decode_resized_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                               items, mode: int, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                               staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_resized`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost source
        rectangle (``qoimi_decode_resized_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``resize_stats`` then holds the counters of the inner call over the band streams."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_resized_indexed", stream_offsets, sizes, descs, out_offsets, items=items)
        index, keep_index = self._index_args("decode_resized_indexed", n, interval_rows, points, point_firsts)
        self._check(self._lib.qoimi_decode_resized_indexed(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, d_out, oo, staging_bytes, stream, *index),
                    "qoimi_decode_resized_indexed")
        del keep, keep_index

    def decode_bilinear_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                                items, mode: int, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                                staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_bilinear`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost source
        rectangle (``qoimi_decode_bilinear_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``bilinear_stats`` then holds the counters of the inner call over the band streams."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_bilinear_indexed", stream_offsets, sizes, descs, out_offsets, items=items)
        index, keep_index = self._index_args("decode_bilinear_indexed", n, interval_rows, points, point_firsts)
        self._check(self._lib.qoimi_decode_bilinear_indexed(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, d_out, oo, staging_bytes, stream, *index),
                    "qoimi_decode_bilinear_indexed")
        del keep, keep_index

    def decode_warped_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                              items, mode: int, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                              staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_warped`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost source
        rectangle (``qoimi_decode_warped_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``warp_stats`` then holds the counters of the inner call over the band streams."""
        n, ds, arr, (so, sz, oo), keep = self._gather_args("decode_warped_indexed", stream_offsets, sizes, descs, out_offsets, warps=items)
        index, keep_index = self._index_args("decode_warped_indexed", n, interval_rows, points, point_firsts)
        self._check(self._lib.qoimi_decode_warped_indexed(self._h, d_streams, so, sz, ds, n, channels, arr, len(arr), mode, d_out, oo, staging_bytes, stream, *index),
                    "qoimi_decode_warped_indexed")
        del keep, keep_index

    def pixel_stats_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], regions,
                            interval_rows, points, point_firsts: Sequence[int], d_hist: int = 0, staging_bytes: int = 0,
                            stream: int = 0) -> List[QoimiPixelStat]:
        """``pixel_stats`` field for field, decoding every referenced image only from the last seek row at or above its topmost region
        (``qoimi_pixel_stats_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``pixel_stats_counters`` then holds the counters of the inner call over the band streams."""
        n, ds, arr, (so, sz, _), keep = self._gather_args("pixel_stats_indexed", stream_offsets, sizes, descs, crops=regions, noun="region")
        index, keep_index = self._index_args("pixel_stats_indexed", n, interval_rows, points, point_firsts)
        out = (QoimiPixelStat * max(len(arr), 1))()
        self._check(self._lib.qoimi_pixel_stats_indexed(self._h, d_streams, so, sz, ds, n, arr, len(arr), out, d_hist or None, staging_bytes, stream, *index),
                    "qoimi_pixel_stats_indexed")
        del keep, keep_index
        return list(out)[:len(arr)]

    def seek_stats(self) -> Tuple[int, int, int, int]:
        """(sub-batches decoded by the last ``build_seek_index``; of the last ``make_band_streams`` / indexed call: band streams
        assembled, bytes of the band arena planned, stream bytes copied)."""
        return self._four_counters(self._lib.qoimi_seek_stats)

    def synth_frames(self, kind: int, seed: int, first_frame: int, n_frames: int, width: int, height: int,
                     d_pixels: int, pixel_stride: int, stream: int = 0) -> None:
        self._check(self._lib.qoimi_synth_frames(self._h, kind, seed, first_frame, n_frames, width, height,
                                                 d_pixels, pixel_stride, stream), "qoimi_synth_frames")

    def hash_streams(self, d_streams: int, stream_stride: int, d_stream_len: int, n_streams: int, d_hash: int, stream: int = 0) -> None:
        """64-bit content hash of every stream into the device array d_hash (uint64[n_streams]); synth.stream_hash64 is the same function."""
        self._check(self._lib.qoimi_hash_streams(self._h, d_streams, stream_stride, d_stream_len, n_streams, d_hash, stream), "qoimi_hash_streams")

    def set_profiling(self, on: bool) -> None:
        self._check(self._lib.qoimi_set_profiling(self._h, 1 if on else 0), "qoimi_set_profiling")

    def get_profile(self, stream: int = 0) -> dict:
        """kernel name -> (accumulated ms, launches) since profiling was enabled (syncs stream)."""
        ms = (ctypes.c_double * 64)()
        calls = (ctypes.c_longlong * 64)()
        n = min(64, self._lib.qoimi_get_profile(self._h, stream, ms, calls, 64))
        return {self._lib.qoimi_kernel_name(i).decode(): (ms[i], calls[i]) for i in range(1, n)}

    def workspace_bytes(self) -> dict:
        """Device bytes the context's arenas hold: encode workspace (with the staging of ``encode_packed`` and ``encode_tiles``), decode workspace (with the tables of ``inspect_streams`` and ``compare_images`` and the staging of ``verify_images`` / ``decode_thumbnails`` / ``decode_crops`` / ``decode_resized`` / ``decode_bilinear`` / ``pixel_stats``, the tables of ``build_seek_index`` / ``seek_index_from_pixels`` and the band arena of the indexed calls), staging of the host-pointer entry points."""
        out = (ctypes.c_size_t * 3)()
        self._lib.qoimi_workspace_bytes(self._h, out)
        return {"encode": int(out[0]), "decode": int(out[1]), "staging": int(out[2])}

    def set_decode_record_cap(self, nbytes: int, release: bool = False) -> None:
        """Caps the chunk-record arena of decode calls (larger calls run as sub-batches of whole images); release=True frees the arena grown so far."""
        self._check(self._lib.qoimi_set_decode_record_cap(self._h, int(nbytes), 1 if release else 0), "qoimi_set_decode_record_cap")

    def decode_stats(self) -> dict:
        out = (ctypes.c_longlong * 4)()
        self._lib.qoimi_decode_stats(self._h, out)
        return {"rounds": out[0], "redo_segments": out[1], "segments": out[2], "sync_fallback_segments": out[3]}
